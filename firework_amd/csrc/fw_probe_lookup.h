// fw_probe_lookup.h — what the host runtime (fw_runtime.cpp) and the probe-lookup kernels (fw_probe_lookup.hip, and through
// fw_probe_corners.h fw_probe_radiance.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// A probe grid as the kernels need it (include/firework_hip.h has the statement): the checked fw_probe_grid and what the host derives
// from it once, in double and in the statement's order.
struct DProbeGrid {
    double lo[3];
    double span[3];             // hi - lo
    double step[3];             // (hi - lo) / (counts - 1); 0 on a flat axis
    double mid[3];              // 0.5 (lo + hi): where a flat axis' probes are
    uint32_t counts[3];
    uint32_t wrap;              // FW_PROBE_WRAP
};

// The depth maps of a probe grid as the lookup kernels need them (include/firework_hip.h has the statement): the checked fw_probe_depth's
// resolution, the moments and the caller's normal bias.
struct DProbeVis {
    const float *moments;       // device memory: n_probes x R x R x 2 floats, 4-byte aligned
    double bias;                // normal_bias >= 0, world units
    uint32_t R;                 // 4, 8, 16 or 32
};

// irradiance[i] = the lookup at (positions[i stride], normals[i stride]) for n points, 3 floats each; sh: n_probes x 27 floats.  v: the
// depth maps of the visibility weight, or NULL for none; placement: n_probes x 4 floats of moved and classified probes, or NULL for
// none.  All device memory, every array 4-byte aligned; one launch on `stream`.
void launch_probe_irradiance(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const float *sh, const float *placement, uint32_t n,
                             const float *positions, const float *normals, uint32_t stride_floats, float *irradiance);

// The shade step of fw_probe_shade over n pixels with the same lookup: aov n x 12 floats (16-byte aligned), the outputs n x 3 each, any
// of them NULL.
void launch_probe_shade(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const float *sh, const float *placement, uint32_t n,
                        const float *aov, float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb);

} // namespace fw
