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
// A file of its own, last on the link line: the code objects of the other files stay byte for byte what they were.  What it needs of
// fw_lightmap.hip (hash32, the lattice, the frame) is restated here: the same bits.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.ao_rays / api.ao_reduce / api.ao_resolve; sin, cos
// and sqrt are the device library's float64 functions.
#include "fw_ao.h"
#include <algorithm>
#include <cmath>

namespace fw {
namespace {

constexpr int AO_BLOCK = 256;
constexpr int AO_WAVES = AO_BLOCK / 64;
constexpr int AR_BLOCK = 64;

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.40282347e+38f; }   // false for NaN and +-inf

__global__ __launch_bounds__(AR_BLOCK) void k_ao_rays(DAoRays R, uint32_t n_entries, float *__restrict__ out) {
    __shared__ float tr[6 * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (n_entries + 63u) / 64u;                                    // n_entries < 2^31
    const double PI = 3.141592653589793, G = 0.6180339887498949;                        // G = (sqrt(5) - 1) / 2
    const double Dd = (double)R.directions;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t id0 = c * 64u;
        const uint32_t cnt = min(64u, n_entries - id0);
        if (lane < cnt) {
            const uint32_t i = id0 + lane;
            const uint32_t q = i / R.directions, j = i - q * R.directions;
            const uint32_t id = R.pts.ids ? R.pts.ids[(size_t)R.first + q] : R.first + q;
            double xi_u = 0.5, xi_v = 0.5;
            if (R.jitter) {
                const uint32_t key = hash32(R.seed32 ^ hash32(R.round + 0x9E3779B9u));
                xi_u = (double)(hash32(hash32(2u * id) ^ key) >> 8) * 0x1p-24;
                xi_v = (double)(hash32(hash32(2u * id + 1u) ^ key) >> 8) * 0x1p-24;
            }
            const float *pp = R.pts.positions + (size_t)id * R.pts.stride, *pn = R.pts.normals + (size_t)id * R.pts.stride;
            const float px = pp[0], py = pp[1], pz = pp[2], fx = pn[0], fy = pn[1], fz = pn[2];
            const double u = ((double)j + xi_u) / Dd;
            const double r = sqrt(u);
            const double cz = sqrt(fmax(0.0, 1.0 - u));
            const double t = (double)j * G + xi_v;
            const double phi = (2.0 * PI) * (t - floor(t));
            const double lx = r * cos(phi), ly = r * sin(phi);
            // the float32 normal made unit again in float64: the frame is then orthonormal to float64 and d unit to one float32 rounding
            const double rx = (double)fx, ry = (double)fy, rz = (double)fz;
            const double rl2 = (rx * rx + ry * ry) + rz * rz;
            const double rl = sqrt(rl2);
            const double nx = rx / rl, ny = ry / rl, nz = rz / rl;
            const double s = copysign(1.0, nz);
            const double a = -1.0 / (s + nz);
            const double b = (nx * ny) * a;
            const double tx = 1.0 + (s * (nx * nx)) * a, ty = s * b, tz = -s * nx;
            const double bx = b, by = s + (ny * ny) * a, bz = -ny;
            const bool usable = finite_f(px) && finite_f(py) && finite_f(pz) && finite_f(fx) && finite_f(fy) && finite_f(fz) && rl2 > 0.0;
            float *d = tr + lane * 6u;
            if (!usable) { d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = 0.f; d[5] = 0.f; }
            else {
                if (R.bias == 0.f) { d[0] = px; d[1] = py; d[2] = pz; }
                else {
                    const double bd = (double)R.bias;
                    d[0] = (float)((double)px + bd * nx); d[1] = (float)((double)py + bd * ny); d[2] = (float)((double)pz + bd * nz);
                }
                d[3] = (float)((lx * tx + ly * bx) + cz * nx);
                d[4] = (float)((lx * ty + ly * by) + cz * ny);
                d[5] = (float)((lx * tz + ly * bz) + cz * nz);
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

inline uint32_t grid_for(uint64_t items, uint32_t per_block, int n_cus, uint32_t per_cu) {
    const uint64_t want = (items + per_block - 1u) / per_block;
    return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(want, (uint64_t)std::max(1, n_cus) * per_cu));
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
