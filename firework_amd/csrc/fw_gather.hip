// fw_gather.hip — the final gather's reduction for gfx950: the radiance that each gather ray brought back, from its surface record
// (k_hit_surface, fw_kernels.hip), the probe lookup at its hit and optionally the delta lights' irradiance there, summed per receiver
// (include/firework_hip.h has the statement, DESIGN.md §9z the design).
//
//   k_gather_reduce   k_ao_reduce's geometry and order: G = the smallest power of two >= min(D, 64) lanes per point, 64 / G points per
//                     wave.  Lane l of a group takes the entries j = l, l + G, ... in ascending order — consecutive lanes read consecutive
//                     64 B records (two whole float4 of each: albedo + kind, emitted), 12 B irradiances and 32 B direct records — into four
//                     float64 sums (L.rgb, sky); an xor butterfly over the distances G/2 .. 1 leaves the same bits in every lane of the
//                     group; lane 0 rounds (pi / D) x L and (1 / D) x sky to float32 once and adds them to the point's running sums.
//   k_gather_resolve  one lane per point: sums / rounds.
//
// No atomics, no LDS, no inline assembly: the kernel streams its inputs once and is bound by that.  A point's result depends on no other
// point and not on the launch geometry; two runs are bit-equal.
//
// Numerics: -ffp-contract=off, so + and * round as written and in the order of api.gather_reduce / api.gather_resolve.
#include "fw_gather.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int GA_BLOCK = 256;
constexpr int GA_WAVES = GA_BLOCK / 64;

__global__ __launch_bounds__(GA_BLOCK) void k_gather_reduce(uint32_t first, uint32_t n, uint32_t directions, uint32_t group,
                                                            const uint32_t *__restrict__ ids, const float4 *__restrict__ surface,
                                                            const float *__restrict__ irradiance, const float *__restrict__ direct,
                                                            float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * GA_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * GA_WAVES;
    const uint32_t per = 64u / group, l = lane & (group - 1u), sub = lane / group;
    const double inv_pi = 1.0 / 3.141592653589793;
    const double scale_l = 3.141592653589793 / (double)directions, scale_s = 1.0 / (double)directions;
    for (uint32_t base = wave * per; base < n; base += n_waves * per) {                   // wave-uniform: every lane reaches the shuffles
        const uint32_t q = base + sub;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (q < n) {
            const size_t e0 = (size_t)q * directions;                                    // < 2^31
            for (uint32_t j = l; j < directions; j += group) {
                const size_t e = e0 + j;
                const float4 a = surface[4 * e], em = surface[4 * e + 3];
                const float kind = a.w;
                if (kind == -2.f) continue;                                               // not traced: contributes nothing
                double lr, lg, lb;
                if (kind == -1.f || kind == 3.f) {                                        // the environment, an emitter
                    lr = (double)em.x; lg = (double)em.y; lb = (double)em.z;
                    if (kind == -1.f) s3 = s3 + 1.0;
                } else {
                    const float *E = irradiance + 3 * e;
                    const float ex = E[0], ey = E[1], ez = E[2];
                    double tr = ex > 0.f ? (double)ex : 0.0, tg = ey > 0.f ? (double)ey : 0.0, tb = ez > 0.f ? (double)ez : 0.0;
                    if (direct) { const float *Ed = direct + 8 * e; tr = tr + (double)Ed[0]; tg = tg + (double)Ed[1]; tb = tb + (double)Ed[2]; }
                    lr = ((double)a.x * tr) * inv_pi; lg = ((double)a.y * tg) * inv_pi; lb = ((double)a.z * tb) * inv_pi;
                }
                s0 = s0 + lr; s1 = s1 + lg; s2 = s2 + lb;
            }
        }
        for (uint32_t m = group >> 1; m >= 1u; m >>= 1) {
            s0 = s0 + __shfl_xor(s0, (int)m, 64); s1 = s1 + __shfl_xor(s1, (int)m, 64);
            s2 = s2 + __shfl_xor(s2, (int)m, 64); s3 = s3 + __shfl_xor(s3, (int)m, 64);
        }
        if (q < n && l == 0u) {
            const uint32_t id = ids ? ids[(size_t)first + q] : first + q;
            float *s = sums + (size_t)id * 4u;
            s[0] = s[0] + (float)(scale_l * s0); s[1] = s[1] + (float)(scale_l * s1); s[2] = s[2] + (float)(scale_l * s2);
            s[3] = s[3] + (float)(scale_s * s3);
        }
    }
}

__global__ __launch_bounds__(GA_BLOCK) void k_gather_resolve(uint32_t n, double rounds, const uint32_t *__restrict__ ids,
                                                             const float4 *__restrict__ sums, float4 *__restrict__ out) {
    for (uint32_t q = blockIdx.x * GA_BLOCK + threadIdx.x; q < n; q += gridDim.x * GA_BLOCK) {
        const uint32_t id = ids ? ids[q] : q;
        const float4 s = sums[id];
        out[id] = make_float4((float)((double)s.x / rounds), (float)((double)s.y / rounds), (float)((double)s.z / rounds),
                              (float)((double)s.w / rounds));
    }
}

} // namespace

void launch_gather_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t directions, const uint32_t *ids, const float *surface,
                          const float *irradiance, const float *direct, float *sums) {
    uint32_t group = 1;
    while (group < std::min<uint32_t>(directions, 64u)) group <<= 1;
    const uint32_t per_block = GA_WAVES * (64u / group);
    hipLaunchKernelGGL(k_gather_reduce, dim3(grid_for(n, per_block, n_cus, 32u)), dim3(GA_BLOCK), 0, stream, first, n, directions, group, ids,
                       (const float4 *)surface, irradiance, direct, sums);
}

void launch_gather_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out) {
    hipLaunchKernelGGL(k_gather_resolve, dim3(grid_for(n, GA_BLOCK, 256, 32u)), dim3(GA_BLOCK), 0, stream, n, rounds, ids, (const float4 *)sums,
                       (float4 *)out);
}

} // namespace fw
