// fw_emitters.hip — the direct light of every emitting primitive of a scene at surface points for gfx950: S shadow rays per point and
// round, each towards an entry picked in proportion to area x power through a CDF, and the reduction of the traced hits and their surface
// records into irradiance and a visible share per point (include/firework_hip.h has the statement, DESIGN.md §9zc the design).
//
//   k_emitters_rays     one lane per entry e = q S + s, 256 entries per block and chunk.  A coarse CDF — every K-th value, K =
//                       ceil(N / 1024), the whole CDF where N <= 1024 — is staged in LDS once per block (at most 8 KiB): the pick's
//                       first ten steps are a binary search there, the remaining ones a binary search over the at most K values of the
//                       coarse interval in global memory, which neighbouring lanes (ascending xi within a point) share.  The picked
//                       record (64 B, four float4) is gathered from global memory: the pick decides it.  The point's unit normal and
//                       origin are recomputed by every lane of the point, as k_area_rays does.  24 B per entry go out through LDS, six
//                       dword stores per lane at consecutive addresses; the weight and the pick are one dword per lane each.
//   k_emitters_reduce   k_area_reduce's geometry over the S entries of a point: G = the smallest power of two >= min(S, 64) lanes per
//                       point, 64 / G points per wave, lane l takes the entries l, l + G, ... ascending into four float64 sums, an xor
//                       butterfly over G/2 .. 1, lane 0 rounds once and adds.
//
// No atomics, no inline assembly; k_emitters_rays alone uses LDS (14 KiB) and barriers.  Every index is formed from q < n and s < S; both
// searches stay inside [0, N) because the CDF's last value is 1 and xi < 1 (the host checks the CDF before any launch); the reduction
// reads codes only below n_entries.  A point's result depends on no other point and not on the launch geometry; two runs are bit-equal.
//
// The sphere's and the rectangle's arithmetic is k_area_rays' own, restated here so that fw_area.hip's code object stays as it was.
// jitter_pair, finite_f and grid_for are fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.emitters_rays / api.emitters_reduce; sqrt, sin, cos
// and floor are the device library's float64 functions.
#include "fw_emitters.h"
#include "fw_shared.h"
#include <cstdlib>

namespace fw {
namespace {

constexpr int EL_BLOCK = 256;                    // k_emitters_rays: entries per chunk = lanes per block
constexpr int EL_COARSE = 1024;                  // coarse CDF values in LDS
constexpr int ED_BLOCK = 256;
constexpr int ED_WAVES = ED_BLOCK / 64;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// COARSE: the search starts in the LDS table; without it (the A/B build's alternative under FIREWORK_EMITTERS_PLAIN_SEARCH; DESIGN.md §9zc has both measured) it is one binary
// search over the whole CDF in global memory
template <bool COARSE>
__global__ __launch_bounds__(EL_BLOCK) void k_emitters_rays(DEmittersRays R, uint32_t n_rays, float *__restrict__ out, float *__restrict__ weights,
                                                            uint32_t *__restrict__ picks) {
    __shared__ double coarse[EL_COARSE];
    __shared__ float tr[6 * EL_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint32_t N = R.n_entries, S = R.samples;
    const uint32_t n_chunks = (n_rays + (uint32_t)EL_BLOCK - 1u) / (uint32_t)EL_BLOCK;        // n_rays < 2^31
    const uint32_t K = (N + (uint32_t)EL_COARSE - 1u) / (uint32_t)EL_COARSE;                  // >= 1; N <= 2^24: K <= 2^14
    const uint32_t C = (N + K - 1u) / K;                                                      // 1 <= C <= 1024 coarse intervals
    const double PI = 3.141592653589793, G = 0.6180339887498949, Sd = (double)S, U1MAX = 1.0 - 1.1102230246251565e-16;    // 1 - 2^-53
    if (COARSE) {
        for (uint32_t j = t; j < C; j += EL_BLOCK) coarse[j] = R.cdf[min((j + 1u) * K, N) - 1u];   // the last value of interval j; index < N
        __syncthreads();
    }
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t e0 = c * (uint32_t)EL_BLOCK;
        const uint32_t cnt = min((uint32_t)EL_BLOCK, n_rays - e0);
        if (t < cnt) {
            const uint32_t e = e0 + t;
            const uint32_t q = e / S, s = e - q * S;                                          // q < n
            const uint32_t id = R.pts.ids ? R.pts.ids[(size_t)R.first + q] : R.first + q;
            double xi_u = 0.5, xi_v = 0.5;
            if (R.jitter) { const Jitter xj = jitter_pair(R.seed32, R.round, id); xi_u = xj.u; xi_v = xj.v; }
            const float *pp = R.pts.positions + (size_t)id * R.pts.stride, *pn = R.pts.normals + (size_t)id * R.pts.stride;
            const float px = pp[0], py = pp[1], pz = pp[2], fx = pn[0], fy = pn[1], fz = pn[2];
            const double rx = (double)fx, ry = (double)fy, rz = (double)fz;
            const double rl2 = (rx * rx + ry * ry) + rz * rz;
            const double rl = sqrt(rl2);
            const double nx = rx / rl, ny = ry / rl, nz = rz / rl;
            const bool usable = finite_f(px) && finite_f(py) && finite_f(pz) && finite_f(fx) && finite_f(fy) && finite_f(fz) && rl2 > 0.0;
            double ox = (double)px, oy = (double)py, oz = (double)pz;
            if (R.bias != 0.f) { const double bd = (double)R.bias; ox = ox + bd * nx; oy = oy + bd * ny; oz = oz + bd * nz; }
            const double a1 = ((double)s + xi_u) / Sd, a2 = (double)s * G + xi_v;
            const double xi = a1 - floor(a1), u2 = a2 - floor(a2);
            // the pick: the first index with cdf[index] > xi.  coarse[C - 1] = cdf[N - 1] = 1 > xi, so both searches have an answer
            uint32_t lo_i = 0, hi_i = COARSE ? C - 1u : N - 1u;
            if (COARSE) while (lo_i < hi_i) { const uint32_t mid = (lo_i + hi_i) >> 1; if (coarse[mid] > xi) hi_i = mid; else lo_i = mid + 1u; }
            uint32_t i = lo_i;
            if (!COARSE || K > 1u) {
                if (COARSE) { lo_i = i * K; hi_i = min(lo_i + K, N) - 1u; }                                   // cdf[hi_i] = coarse[i] > xi; lo_i <= hi_i < N
                while (lo_i < hi_i) { const uint32_t mid = (lo_i + hi_i) >> 1; if (R.cdf[mid] > xi) hi_i = mid; else lo_i = mid + 1u; }
                i = lo_i;
            }
            const double c_lo = i ? R.cdf[i - 1u] : 0.0;
            const double p = R.cdf[i] - c_lo;
            const double u1 = fmin((xi - c_lo) / p, U1MAX);
            const float4 r0 = R.records[4u * (size_t)i], r1 = R.records[4u * (size_t)i + 1u], r2 = R.records[4u * (size_t)i + 2u],
                         r3 = R.records[4u * (size_t)i + 3u];
            double dx, dy, dz, g;
            bool live = usable;
            if (r0.y == 0.f) {                                                        // a sphere: (centre, radius) in r0.zw r1.xy
                const double vx = (double)r0.z - ox, vy = (double)r0.w - oy, vz = (double)r1.x - oz;
                const double d2v = dot3(vx, vy, vz, vx, vy, vz);
                const double rr = (double)r1.y, rr2 = rr * rr;
                live = live && d2v > rr2;
                const double s2 = rr2 / d2v, cmax = sqrt(1.0 - s2), omc = s2 / (1.0 + cmax);
                const double om = u1 * omc, ct = 1.0 - om, st = sqrt(fmax(om * (2.0 - om), 0.0));
                const double phi = (2.0 * PI) * u2;
                const double lx = st * cos(phi), ly = st * sin(phi);
                const double dist = sqrt(d2v);
                const double wx = vx / dist, wy = vy / dist, wz = vz / dist;
                const double sg = copysign(1.0, wz);
                const double a = -1.0 / (sg + wz);
                const double b = (wx * wy) * a;
                const double tx = 1.0 + (sg * (wx * wx)) * a, ty = sg * b, tz = -sg * wx;
                const double bx = b, by = sg + (wy * wy) * a, bz = -wy;
                const double ex = (lx * tx + ly * bx) + ct * wx, ey = (lx * ty + ly * by) + ct * wy, ez = (lx * tz + ly * bz) + ct * wz;
                const double bb = dot3(ex, ey, ez, vx, vy, vz);
                const double tt = bb - sqrt(fmax(bb * bb - (d2v - rr2), 0.0));
                dx = tt * ex; dy = tt * ey; dz = tt * ez;
                const double dl = sqrt(dot3(dx, dy, dz, dx, dy, dz));
                const double cr = dot3(nx, ny, nz, dx / dl, dy / dl, dz / dl);
                live = live && cr > 0.0;
                g = (cr * (2.0 * PI)) * omc;
            } else {                                                                  // a flat entry: a point, its normal n_l and its area A
                const double g0x = (double)r0.z, g0y = (double)r0.w, g0z = (double)r1.x;      // the first three of the 12 geometry floats
                const double g1x = (double)r1.y, g1y = (double)r1.z, g1z = (double)r1.w;
                const double g2x = (double)r2.x, g2y = (double)r2.y, g2z = (double)r2.z;
                double lnx, lny, lnz, A, nlen;
                if (r0.y == 9.f) {                                                    // a disk: centre, x axis, z axis, then r, r_in, phi_max
                    const double r_o = (double)r2.w, r_i = (double)r3.x, pm = (double)r3.y;
                    const double ro2 = r_o * r_o, ri2 = r_i * r_i;
                    const double rr = sqrt(ri2 + u1 * (ro2 - ri2));
                    const double phi = u2 * pm;
                    const double ca = rr * cos(phi), sa = rr * sin(phi);
                    dx = ((g0x + ca * g1x) + sa * g2x) - ox; dy = ((g0y + ca * g1y) + sa * g2y) - oy; dz = ((g0z + ca * g1z) + sa * g2z) - oz;
                    lnx = g1y * g2z - g1z * g2y; lny = g1z * g2x - g1x * g2z; lnz = g1x * g2y - g1y * g2x;
                    nlen = sqrt(dot3(lnx, lny, lnz, lnx, lny, lnz));
                    A = (0.5 * pm) * (ro2 - ri2);
                } else if (r0.y == 5.f) {                                             // a triangle: v0, v1, v2
                    const double e1x = g1x - g0x, e1y = g1y - g0y, e1z = g1z - g0z;
                    const double e2x = g2x - g0x, e2y = g2y - g0y, e2z = g2z - g0z;
                    const double sq = sqrt(u1);
                    const double b0 = 1.0 - sq, b1 = sq * (1.0 - u2), b2 = sq * u2;
                    dx = ((b0 * g0x + b1 * g1x) + b2 * g2x) - ox; dy = ((b0 * g0y + b1 * g1y) + b2 * g2y) - oy; dz = ((b0 * g0z + b1 * g1z) + b2 * g2z) - oz;
                    lnx = e1y * e2z - e1z * e2y; lny = e1z * e2x - e1x * e2z; lnz = e1x * e2y - e1y * e2x;
                    nlen = sqrt(dot3(lnx, lny, lnz, lnx, lny, lnz));
                    A = nlen / 2.0;
                } else {                                                              // a rectangle or a Rect3d face: corners c0 .. c3
                    const double e1x = g1x - g0x, e1y = g1y - g0y, e1z = g1z - g0z;
                    const double e2x = (double)r2.w - g0x, e2y = (double)r3.x - g0y, e2z = (double)r3.y - g0z;
                    dx = ((g0x + u1 * e1x) + u2 * e2x) - ox; dy = ((g0y + u1 * e1y) + u2 * e2y) - oy; dz = ((g0z + u1 * e1z) + u2 * e2z) - oz;
                    lnx = e1y * e2z - e1z * e2y; lny = e1z * e2x - e1x * e2z; lnz = e1x * e2y - e1y * e2x;
                    nlen = sqrt(dot3(lnx, lny, lnz, lnx, lny, lnz));
                    A = nlen;
                }
                const double d2 = dot3(dx, dy, dz, dx, dy, dz);
                const double dl = sqrt(d2);
                const double wx = dx / dl, wy = dy / dl, wz = dz / dl;
                const double cr = dot3(nx, ny, nz, wx, wy, wz);
                const double cl = fabs(dot3(lnx, lny, lnz, wx, wy, wz) / nlen);
                live = live && cr > 0.0 && A > 0.0 && nlen > 0.0;
                g = ((cr * cl) * A) / d2;
            }
            const double gw = g / p;
            const float o0 = (float)ox, o1 = (float)oy, o2 = (float)oz, d0 = (float)dx, d1 = (float)dy, d2f = (float)dz, gf = (float)gw;
            live = live && finite_d(gw) && gf > 0.f && finite_f(gf) && finite_f(o0) && finite_f(o1) && finite_f(o2) && finite_f(d0) && finite_f(d1)
                   && finite_f(d2f) && !(d0 == 0.f && d1 == 0.f && d2f == 0.f);
            float *d = tr + t * 6u;
            if (!live) { d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = 0.f; d[5] = 0.f; }
            else { d[0] = o0; d[1] = o1; d[2] = o2; d[3] = d0; d[4] = d1; d[5] = d2f; }
            weights[e] = live ? gf : 0.f;
            picks[e] = live ? i : 0xffffffffu;
        }
        __syncthreads();
        float *dst = out + (size_t)e0 * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * (uint32_t)EL_BLOCK + t; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(ED_BLOCK) void k_emitters_reduce(uint32_t first, uint32_t n, uint32_t samples, uint32_t group, uint32_t n_entries,
                                                              const uint32_t *__restrict__ ids, const uint32_t *__restrict__ codes,
                                                              const uint32_t *__restrict__ picks, const float *__restrict__ weights,
                                                              const uint32_t *__restrict__ hits, const float4 *__restrict__ surface,
                                                              float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * ED_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * ED_WAVES;
    const uint32_t per = 64u / group, l = lane & (group - 1u), sub = lane / group;
    const uint32_t M = samples;
    const double scale = 1.0 / (double)samples;
    for (uint32_t base = wave * per; base < n; base += n_waves * per) {                   // wave-uniform: every lane reaches the shuffles
        const uint32_t q = base + sub;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (q < n) {
            const size_t e0 = (size_t)q * M;                                             // < 2^31
            for (uint32_t m = l; m < M; m += group) {
                const size_t e = e0 + m;
                const float w = weights[e];
                const uint32_t pick = picks[e];
                const uint32_t hobj = hits[e * 12u + 10u], hprim = hits[e * 12u + 11u];
                const float4 a = surface[4 * e], em = surface[4 * e + 3];
                if (!(w > 0.f) || pick >= n_entries || a.w != 3.f) continue;
                if (hobj != codes[2u * (size_t)pick] || hprim != codes[2u * (size_t)pick + 1u]) continue;      // the ray did not reach its entry
                const double wd = (double)w;
                s0 = s0 + (double)em.x * wd; s1 = s1 + (double)em.y * wd; s2 = s2 + (double)em.z * wd; s3 = s3 + 1.0;
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

} // namespace

void launch_emitters_rays(hipStream_t stream, int n_cus, const DEmittersRays &r, uint32_t n, float *rays, float *weights, uint32_t *picks) {
    const uint32_t n_rays = n * r.samples;                                    // < 2^31
#if FW_AB
    static const bool plain = getenv("FIREWORK_EMITTERS_PLAIN_SEARCH") != nullptr;
    if (plain) {
        hipLaunchKernelGGL(k_emitters_rays<false>, dim3(grid_for(n_rays, EL_BLOCK, n_cus, 32u)), dim3(EL_BLOCK), 0, stream, r, n_rays, rays, weights, picks);
        return;
    }
#endif
    hipLaunchKernelGGL(k_emitters_rays<true>, dim3(grid_for(n_rays, EL_BLOCK, n_cus, 32u)), dim3(EL_BLOCK), 0, stream, r, n_rays, rays, weights, picks);
}

void launch_emitters_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t samples, const uint32_t *ids, const uint32_t *codes,
                            uint32_t n_entries, const uint32_t *picks, const float *weights, const void *hits, const float *surface, float *sums) {
    uint32_t group = 1;
    while (group < std::min<uint32_t>(samples, 64u)) group <<= 1;
    const uint32_t per_block = ED_WAVES * (64u / group);
    hipLaunchKernelGGL(k_emitters_reduce, dim3(grid_for(n, per_block, n_cus, 32u)), dim3(ED_BLOCK), 0, stream, first, n, samples, group, n_entries, ids,
                       codes, picks, weights, (const uint32_t *)hits, (const float4 *)surface, sums);
}

} // namespace fw
