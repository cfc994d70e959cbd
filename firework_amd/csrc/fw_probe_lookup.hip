// fw_probe_lookup.hip — the kernels that read a baked probe grid back as irradiance, for gfx950, in all their forms: plain, with the
// visibility weight of the depth maps, and over placed probes (include/firework_hip.h has the statement, DESIGN.md §9q, §9s and §9u the
// design).
//
//   k_probe_irradiance<PLACED, DEPTH>   one lane per point: 12 B of position and 12 B of normal at the caller's stride, the cell and the (up
//                                       to) eight corner weights in float64, then corner by corner the nine (r, g, b) triples of that
//                                       probe (108 B, 4-byte aligned; hipcc merges them into six 16-byte loads and one of 12 B) folded
//                                       with B_k = A_k Y_k(n) into three float64 sums; writes 12 B.  DEPTH: per corner the lane fetches
//                                       four texels (mu, mu2: 8 B each, two 16-byte rows) of that probe's depth map, bilinearly.  PLACED:
//                                       per corner the lane reads 16 B of placement; an inactive corner reads nothing else.
//   k_probe_shade<PLACED, DEPTH>        one lane per pixel: fw_render_aovs' 48-byte record as three 16-byte loads, the same lookup at
//                                       (position, normal), then out = albedo (coverage E / pi + (1 - coverage)) in float32 and
//                                       resolve_pixel's three outputs.
//
// The lookup itself is fw_probe_corners.h's, which says where the forms differ; the float32 tail is fw_shared.h's.  Corner-major: beside
// the nine B_k a lane holds eight weights and three sums, never the 27 interpolated coefficients.  Neighbouring points share a cell, so a
// wave's 8 x 108 B of coefficients are a few cache lines.  No LDS, no atomics, no barrier, no inline assembly: every output is one
// lane's, a pure function of the inputs.
#include "fw_probe_corners.h"

namespace fw {
namespace {

constexpr int PL_BLOCK = 256;

template <bool PLACED, bool DEPTH>
__global__ __launch_bounds__(PL_BLOCK) void k_probe_irradiance(DProbeGrid G, DProbeVis V, ShLookupConst K, const float *__restrict__ sh,
                                                               const float *__restrict__ placement, uint32_t n,
                                                               const float *__restrict__ positions, const float *__restrict__ normals,
                                                               uint32_t stride, float *__restrict__ out) {
    const uint32_t q = blockIdx.x * PL_BLOCK + threadIdx.x;                           // one point per lane: the grid covers n
    if (q < n) {
        const float *pp = positions + (size_t)q * stride, *nn = normals + (size_t)q * stride;
        if (PLACED) __builtin_assume(placement != nullptr);                            // the launch picks PLACED by it: no test per corner
        Corners C;
        double E[3];
        float r = 0.f, g = 0.f, b = 0.f;
        if (corner_weights<PLACED, DEPTH>(G, V, placement, pp[0], pp[1], pp[2], nn[0], nn[1], nn[2], C)) {
            corners_sh(G, C, K, sh, E);
            r = (float)E[0]; g = (float)E[1]; b = (float)E[2];
        }
        float *o = out + (size_t)q * 3u;
        o[0] = r; o[1] = g; o[2] = b;
    }
}

template <bool PLACED, bool DEPTH>
__global__ __launch_bounds__(PL_BLOCK) void k_probe_shade(DProbeGrid G, DProbeVis V, ShLookupConst K, const float *__restrict__ sh,
                                                          const float *__restrict__ placement, uint32_t n, const float4 *__restrict__ aov,
                                                          float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    const uint32_t p = blockIdx.x * PL_BLOCK + threadIdx.x;                           // one pixel per lane: the grid covers n
    if (p < n) {
        const float4 a = aov[3 * (size_t)p], nd = aov[3 * (size_t)p + 1], xa = aov[3 * (size_t)p + 2];
        if (PLACED) __builtin_assume(placement != nullptr);                            // as above
        Corners C;
        const bool ok = corner_weights<PLACED, DEPTH>(G, V, placement, xa.x, xa.y, xa.z, nd.x, nd.y, nd.z, C);
        shade_diffuse(G, C, ok, K, sh, a, gamma, p, rgb8, gamma_rgb, linear_rgb);
    }
}

uint32_t lookup_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + PL_BLOCK - 1) / PL_BLOCK); }      // n > 0; at most 2^24 blocks
const DProbeVis NO_VIS{nullptr, 0.0, 0u};

} // namespace

// Both launches pick the instantiation by what is given: placement picks PLACED, v picks DEPTH.
void launch_probe_irradiance(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const float *sh, const float *placement, uint32_t n,
                             const float *positions, const float *normals, uint32_t stride_floats, float *irradiance) {
    auto *k = placement ? (v ? k_probe_irradiance<true, true> : k_probe_irradiance<true, false>)
                        : (v ? k_probe_irradiance<false, true> : k_probe_irradiance<false, false>);
    hipLaunchKernelGGL(k, dim3(lookup_blocks(n)), dim3(PL_BLOCK), 0, stream, g, v ? *v : NO_VIS, sh_lookup_const(), sh, placement, n, positions,
                       normals, stride_floats, irradiance);
}

void launch_probe_shade(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const float *sh, const float *placement, uint32_t n,
                        const float *aov, float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    auto *k = placement ? (v ? k_probe_shade<true, true> : k_probe_shade<true, false>)
                        : (v ? k_probe_shade<false, true> : k_probe_shade<false, false>);
    hipLaunchKernelGGL(k, dim3(lookup_blocks(n)), dim3(PL_BLOCK), 0, stream, g, v ? *v : NO_VIS, sh_lookup_const(), sh, placement, n,
                       (const float4 *)aov, gamma, rgb8, gamma_rgb, linear_rgb);
}

} // namespace fw
