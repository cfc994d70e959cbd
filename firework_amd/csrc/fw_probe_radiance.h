// fw_probe_radiance.h — what the host runtime (fw_runtime.cpp) and the probe-radiance kernels (fw_probe_radiance.hip) share (DESIGN.md
// §9v).
#pragma once
#include "fw_probe_lookup.h"    // DProbeGrid, DProbeVis

namespace fw {

// A checked fw_probe_radiance as the kernels need it (include/firework_hip.h has the statement): level l has resolution R >> l, and the
// pyramid of one probe has `texels` = sum_l (R >> l)^2 texels of 16 B.
struct DProbeRadiance {
    uint32_t R;                 // 4, 8, 16 or 32
    uint32_t k;                 // sharpness_log2, 0..8
    uint32_t levels;            // 1..4, R >> (levels - 1) >= 4
    uint32_t texels;            // M
    double rho[4];              // the levels' roughness, widened; entries >= levels are 0
};

// sums[p][b][a] += float(A_r), float(A_g), float(A_b), float(W) of one round's rays and rendered accum of n probes: rays n x D x 6 floats,
// accum n x D x 4 floats (16-byte aligned), sums n x R x R x 4 floats (16-byte aligned), all device memory; one launch on `stream`.
// n x D < 2^31 and n x R x R < 2^31 (the runtime checks both).
void launch_probe_radiance_reduce(hipStream_t stream, uint32_t n, uint32_t directions, const DProbeRadiance &pr, uint32_t samples, const float *rays,
                                  const float *accum, float *sums);

// maps (n x M x 4 floats, 16-byte aligned) from sums (n x R x R x 4 floats, 16-byte aligned): level 0 divided, the levels above it
// prefiltered from level 0.  Device memory; one launch on `stream`.  n x M < 2^31.
void launch_probe_radiance_prefilter(hipStream_t stream, int n_cus, uint32_t n, const DProbeRadiance &pr, const float *sums, float *maps);

// The radiance lookup: out (n x 3 floats) for n points (positions and normals at `stride_floats`, dirs n x 3 and roughness n, packed).
// v NULL: no visibility weight; placement NULL: every record is (0, 0, 0, 1).
void launch_probe_radiance_lookup(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const DProbeRadiance &pr, const float *maps,
                                  const float *placement, uint32_t n, const float *positions, const float *normals, uint32_t stride_floats,
                                  const float *dirs, const float *roughness, float *radiance);

// The glossy probe shade of n pixels: aov n x 12 floats and spec n x 4 floats (both 16-byte aligned), view three floats per pixel at
// `view_stride` floats.  v and placement as above.
void launch_probe_shade_glossy(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const DProbeRadiance &pr, const float *sh,
                               const float *maps, const float *placement, uint32_t n, const float *aov, const float *spec, const float *view,
                               uint32_t view_stride, float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb);

} // namespace fw
