// fw_ao.hip — ambient occlusion and bent normals for gfx950: hemisphere rays around surface points wherever they lie, and the reduction
// of their traced hits into occlusion and a mean unoccluded direction (include/firework_hip.h has the statement, DESIGN.md §9t the
// design).
//
//   k_ao_rays      k_lm_rays (fw_lightmap.hip) with the texel's record replaced by a point read in place: one lane per entry (point q,
//                  direction j), id = ids ? ids[first + q] : first + q, position and normal three floats each at id x stride.  The
//                  (round, id) shift, the cosine-weighted Fibonacci direction in float64 in the frame of Duff et al. 2017 around the
//                  float32 normal made unit again in float64, one rounding to float32; 24 B per entry through LDS: six dword stores per
//                  lane at consecutive addresses.  A point with a non-finite component or a zero normal gets D all-zero rays.
//   k_ao_reduce    k_lm_reduce's geometry: G = the smallest power of two >= min(D, 64) lanes per point, 64 / G points per wave.  Lane l
//                  of a group takes the entries j = l, l + G, ... in ascending order (consecutive lanes read consecutive 24 B rays and
//                  48 B hits) into four float64 sums (Bx, By, Bz, O), an xor butterfly over the distances G/2 .. 1 leaves the same bits
//                  in every lane of the group, lane 0 rounds (1 / D) x each to float32 once and adds it to the point's running sums.
//   k_ao_resolve   one lane per point: (bent.xyz, ao) from the running sums.
//
// No atomics, no inline assembly; k_ao_rays alone uses LDS (1536 B) and a barrier.  A point's result depends on no other point and not
// on the launch geometry; two runs are bit-equal.
//
// What it has in common with fw_lightmap.hip (the jitter draw, the lattice, the frame, grid_for) is fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.ao_rays / api.ao_reduce / api.ao_resolve; sin, cos
// and sqrt are the device library's float64 functions.
#include "fw_ao.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int AO_BLOCK = 256;
constexpr int AO_WAVES = AO_BLOCK / 64;
constexpr int AR_BLOCK = 64;

__global__ __launch_bounds__(AR_BLOCK) void k_ao_rays(DAoRays R, uint32_t n_entries, float *__restrict__ out) {
    __shared__ float tr[6 * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (n_entries + 63u) / 64u;                                    // n_entries < 2^31
    const double Dd = (double)R.directions;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t id0 = c * 64u;
        const uint32_t cnt = min(64u, n_entries - id0);
        if (lane < cnt) {
            const uint32_t i = id0 + lane;
            const uint32_t q = i / R.directions, j = i - q * R.directions;
            const uint32_t id = R.pts.ids ? R.pts.ids[(size_t)R.first + q] : R.first + q;
            double xi_u = 0.5, xi_v = 0.5;
            if (R.jitter) { const Jitter xi = jitter_pair(R.seed32, R.round, id); xi_u = xi.u; xi_v = xi.v; }
            const float *pp = R.pts.positions + (size_t)id * R.pts.stride, *pn = R.pts.normals + (size_t)id * R.pts.stride;
            const float px = pp[0], py = pp[1], pz = pp[2], fx = pn[0], fy = pn[1], fz = pn[2];
            const CosineDir cd = cosine_dir(j, Dd, xi_u, xi_v, fx, fy, fz);
            const bool usable = finite_f(px) && finite_f(py) && finite_f(pz) && finite_f(fx) && finite_f(fy) && finite_f(fz) && cd.rl2 > 0.0;
            float *d = tr + lane * 6u;
            if (!usable) { d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = 0.f; d[5] = 0.f; }
            else {
                if (R.bias == 0.f) { d[0] = px; d[1] = py; d[2] = pz; }
                else {
                    const double bd = (double)R.bias;
                    d[0] = (float)((double)px + bd * cd.nx); d[1] = (float)((double)py + bd * cd.ny); d[2] = (float)((double)pz + bd * cd.nz);
                }
                d[3] = (float)cd.dx; d[4] = (float)cd.dy; d[5] = (float)cd.dz;
            }
        }
        __syncthreads();
        float *dst = out + (size_t)id0 * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * 64u + lane; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(AO_BLOCK) void k_ao_reduce(uint32_t first, uint32_t n, uint32_t directions, uint32_t group, uint32_t falloff,
                                                        double radius, const uint32_t *__restrict__ ids, const float *__restrict__ rays,
                                                        const uint32_t *__restrict__ hits, float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * AO_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * AO_WAVES;
    const uint32_t per = 64u / group, l = lane & (group - 1u), sub = lane / group;
    const double scale = 1.0 / (double)directions;
    for (uint32_t base = wave * per; base < n; base += n_waves * per) {                   // wave-uniform: every lane reaches the shuffles
        const uint32_t q = base + sub;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (q < n) {
            const size_t e0 = (size_t)q * directions;                                    // < 2^31
            for (uint32_t j = l; j < directions; j += group) {
                const float *r = rays + (e0 + j) * 6u + 3u;
                const uint32_t *h = hits + (e0 + j) * 12u;
                const float fx = r[0], fy = r[1], fz = r[2];
                if (fx == 0.f && fy == 0.f && fz == 0.f) continue;                        // a zero ray contributes nothing
                const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
                const double dist = (double)__uint_as_float(h[0]) * sqrt((dx * dx + dy * dy) + dz * dz);
                double o = 0.0;
                if (!(h[10] == 0xFFFFFFFFu || dist >= radius)) o = falloff ? 1.0 - dist / radius : 1.0;
                const double w = 1.0 - o;
                s0 = s0 + w * dx; s1 = s1 + w * dy; s2 = s2 + w * dz; s3 = s3 + o;
            }
        }
        for (uint32_t m = group >> 1; m >= 1u; m >>= 1) {
            s0 = s0 + __shfl_xor(s0, (int)m, 64); s1 = s1 + __shfl_xor(s1, (int)m, 64);
            s2 = s2 + __shfl_xor(s2, (int)m, 64); s3 = s3 + __shfl_xor(s3, (int)m, 64);
        }
        if (q < n && l == 0u) {
            const uint32_t id = ids ? ids[(size_t)first + q] : first + q;
            float *s = sums + (size_t)id * 4u;
            s[0] = s[0] + (float)(scale * s0); s[1] = s[1] + (float)(scale * s1); s[2] = s[2] + (float)(scale * s2);
            s[3] = s[3] + (float)(scale * s3);
        }
    }
}

__global__ __launch_bounds__(AO_BLOCK) void k_ao_resolve(uint32_t n, double rounds, const uint32_t *__restrict__ ids,
                                                         const float4 *__restrict__ sums, float4 *__restrict__ out) {
    for (uint32_t q = blockIdx.x * AO_BLOCK + threadIdx.x; q < n; q += gridDim.x * AO_BLOCK) {
        const uint32_t id = ids ? ids[q] : q;
        const float4 s = sums[id];
        const double bx = (double)s.x, by = (double)s.y, bz = (double)s.z;
        const double len = sqrt((bx * bx + by * by) + bz * bz);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (len > 0.0 && len <= 1.7976931348623157e308) o = make_float4((float)(bx / len), (float)(by / len), (float)(bz / len), 0.f);
        o.w = (float)fmin(1.0, fmax(0.0, 1.0 - (double)s.w / rounds));
        out[id] = o;
    }
}

} // namespace

void launch_ao_rays(hipStream_t stream, int n_cus, const DAoRays &r, uint32_t n, float *out) {
    const uint32_t n_entries = n * r.directions;                              // < 2^31
    hipLaunchKernelGGL(k_ao_rays, dim3(grid_for(n_entries, 64u, n_cus, 128u)), dim3(AR_BLOCK), 0, stream, r, n_entries, out);
}

void launch_ao_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t directions, uint32_t falloff, float radius,
                      const uint32_t *ids, const float *rays, const void *hits, float *sums) {
    uint32_t group = 1;
    while (group < std::min<uint32_t>(directions, 64u)) group <<= 1;
    const uint32_t per_block = AO_WAVES * (64u / group);
    hipLaunchKernelGGL(k_ao_reduce, dim3(grid_for(n, per_block, n_cus, 32u)), dim3(AO_BLOCK), 0, stream, first, n, directions, group, falloff,
                       (double)radius, ids, rays, (const uint32_t *)hits, sums);
}

void launch_ao_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out) {
    hipLaunchKernelGGL(k_ao_resolve, dim3(grid_for(n, AO_BLOCK, 256, 32u)), dim3(AO_BLOCK), 0, stream, n, rounds, ids, (const float4 *)sums,
                       (float4 *)out);
}

} // namespace fw
