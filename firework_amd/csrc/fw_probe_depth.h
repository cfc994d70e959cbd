// fw_probe_depth.h — what the host runtime (fw_runtime.cpp) and the probe-visibility kernels (fw_probe_depth.hip) share.  A header of its
// own, so that the translation units of fw_kernels.hip, fw_build.hip, fw_temporal.hip, fw_camera_models.hip, fw_probes.hip,
// fw_lightmap.hip and fw_probe_lookup.hip read exactly what they read before.
#pragma once
#include "fw_probe_lookup.h"

namespace fw {

// The depth maps of a probe grid as the lookup kernels need them (include/firework_hip.h has the statement): the checked fw_probe_depth's
// resolution, the moments and the caller's normal bias.
struct DProbeVis {
    const float *moments;       // device memory: n_probes x R x R x 2 floats, 4-byte aligned
    double bias;                // normal_bias >= 0, world units
    uint32_t R;                 // 4, 8, 16 or 32
};

// sums[p][b][a].xyz += float(A), float(B), float(W) of one round's rays and hits of n probes: rays n x D x 6 floats, hits n x D records
// of 48 B (16-byte aligned), sums n x R x R x 4 floats (16-byte aligned; .w is left alone), all device memory; one launch on `stream`.
// n x D < 2^31 and n x R x R < 2^31 (the runtime checks both).
void launch_probe_depth(hipStream_t stream, uint32_t n, uint32_t directions, uint32_t R, uint32_t sharpness_log2, float max_distance,
                        const float *rays, const void *hits, float *sums);

// launch_probe_irradiance and launch_probe_shade (fw_probe_lookup.h) with the visibility weight: the same arguments, and the depth maps.
void launch_probe_irradiance_vis(hipStream_t stream, const DProbeGrid &g, const DProbeVis &v, const float *sh, uint32_t n, const float *positions,
                                 const float *normals, uint32_t stride_floats, float *irradiance);
void launch_probe_shade_vis(hipStream_t stream, const DProbeGrid &g, const DProbeVis &v, const float *sh, uint32_t n, const float *aov, float gamma,
                            uint8_t *rgb8, float *gamma_rgb, float *linear_rgb);

} // namespace fw
