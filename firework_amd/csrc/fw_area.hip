// fw_area.hip — the direct light of sphere and rectangle emitters at surface points for gfx950: S shadow rays per (point, light) towards
// points drawn on the light as the receiver sees it, the reduction of the traced hits and their surface records into irradiance and a
// visible share per point, and the mask that takes the sampled lights out of a final gather's records (include/firework_hip.h has the
// statement, DESIGN.md §9zb the design).
//
//   k_area_rays     one lane per entry e = (q Ln + i) S + s, 256 entries per block and chunk.  The light records (64 B, four float4) are
//                   staged in LDS in tiles of at most 256: with Ln <= 256 the whole list once per block, slot i = light i; with more,
//                   per chunk the at most 256 records its entries need, slot t = the light of flat index e0 / S + t (flat = q Ln + i).
//                   The point's unit normal and origin are recomputed by every lane of the point, as k_direct_rays does and for its
//                   reasons.  24 B per entry go out through LDS, six dword stores per lane at consecutive addresses; the weight is one
//                   dword per lane at consecutive addresses as it is.
//   k_area_reduce   k_ao_reduce's geometry over the M = Ln S entries of a point: G = the smallest power of two >= min(M, 64) lanes per
//                   point, 64 / G points per wave.  Lane l of a group takes the entries m = l, l + G, ... in ascending order — consecutive
//                   lanes read consecutive weights, the object words of consecutive 48 B hits and two float4 of consecutive 64 B records
//                   — into four float64 sums (E.rgb, V); an xor butterfly over the distances G/2 .. 1 leaves the same bits in every lane
//                   of the group; lane 0 rounds (1 / S) x E and (1 / M) x V to float32 once and adds them to the point's running sums.
//   k_area_resolve  one lane per point: sums / rounds.
//   k_area_mask     one lane per record: kind 3 and the hit's object among the ascending light objects (binary search) -> (-2, zeros).
//
// No atomics, no inline assembly; k_area_rays alone uses LDS (22 KiB) and barriers.  Every index is formed from q < n, i < Ln and s < S;
// the binary search stays inside [0, n_objects); no load depends on the content of a record otherwise.  A point's result depends on no
// other point and not on the launch geometry; two runs are bit-equal.
//
// jitter_pair, finite_f and grid_for are fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.area_rays / api.area_reduce / api.area_resolve; sqrt,
// sin, cos and floor are the device library's float64 functions.
#include "fw_area.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int AL_BLOCK = 256;                    // k_area_rays: entries per chunk = lanes per block
constexpr int AL_TILE = 256;                     // light records per LDS tile
constexpr int AD_BLOCK = 256;
constexpr int AD_WAVES = AD_BLOCK / 64;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

__global__ __launch_bounds__(AL_BLOCK) void k_area_rays(DAreaRays R, uint32_t n_entries, float *__restrict__ out, float *__restrict__ weights) {
    __shared__ float4 lrec[4 * AL_TILE];
    __shared__ float tr[6 * AL_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint32_t Ln = R.n_lights, S = R.samples;
    const uint32_t n_chunks = (n_entries + (uint32_t)AL_BLOCK - 1u) / (uint32_t)AL_BLOCK;     // n_entries < 2^31
    const bool whole = Ln <= (uint32_t)AL_TILE;
    const double PI = 3.141592653589793, G = 0.6180339887498949, Sd = (double)S;
    if (whole) for (uint32_t f = t; f < 4u * Ln; f += AL_BLOCK) lrec[f] = R.lights[f];
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t e0 = c * (uint32_t)AL_BLOCK;
        const uint32_t cnt = min((uint32_t)AL_BLOCK, n_entries - e0);
        const uint32_t f0 = e0 / S;                                                   // the flat (point, light) index of the chunk's first entry
        if (!whole) {                                                                 // slot s = the light of flat index f0 + s
            for (uint32_t f = t; f < 4u * AL_TILE; f += AL_BLOCK) {
                const uint32_t s = f >> 2, w = f & 3u;
                lrec[f] = R.lights[4u * ((f0 + s) % Ln) + w];                         // (f0 + s) % Ln < Ln
            }
        }
        __syncthreads();
        if (t < cnt) {
            const uint32_t e = e0 + t;
            const uint32_t fl = e / S, s = e - fl * S;                                // fl - f0 <= 255
            const uint32_t q = fl / Ln, i = fl - q * Ln;                              // q < n, i < Ln
            const uint32_t id = R.pts.ids ? R.pts.ids[(size_t)R.first + q] : R.first + q;
            double xi_u = 0.5, xi_v = 0.5;
            if (R.jitter) { const Jitter xi = jitter_pair(R.seed32, R.round, id * Ln + i); xi_u = xi.u; xi_v = xi.v; }
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
            const double u1 = a1 - floor(a1), u2 = a2 - floor(a2);
            const uint32_t slot = whole ? i : fl - f0;
            const float4 r0 = lrec[4u * slot], r1 = lrec[4u * slot + 1u], r2 = lrec[4u * slot + 2u], r3 = lrec[4u * slot + 3u];
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
            } else {                                                                  // a rectangle: corners c0 .. c3 in r0.zw r1 r2 r3.xy
                const double c0x = (double)r0.z, c0y = (double)r0.w, c0z = (double)r1.x;
                const double e1x = (double)r1.y - c0x, e1y = (double)r1.z - c0y, e1z = (double)r1.w - c0z;
                const double e2x = (double)r2.w - c0x, e2y = (double)r3.x - c0y, e2z = (double)r3.y - c0z;
                dx = ((c0x + u1 * e1x) + u2 * e2x) - ox; dy = ((c0y + u1 * e1y) + u2 * e2y) - oy; dz = ((c0z + u1 * e1z) + u2 * e2z) - oz;
                const double lnx = e1y * e2z - e1z * e2y, lny = e1z * e2x - e1x * e2z, lnz = e1x * e2y - e1y * e2x;
                const double A = sqrt(dot3(lnx, lny, lnz, lnx, lny, lnz));
                const double d2 = dot3(dx, dy, dz, dx, dy, dz);
                const double dl = sqrt(d2);
                const double wx = dx / dl, wy = dy / dl, wz = dz / dl;
                const double cr = dot3(nx, ny, nz, wx, wy, wz);
                const double cl = fabs(dot3(lnx, lny, lnz, wx, wy, wz) / A);
                live = live && cr > 0.0 && A > 0.0;
                g = ((cr * cl) * A) / d2;
            }
            const float o0 = (float)ox, o1 = (float)oy, o2 = (float)oz, d0 = (float)dx, d1 = (float)dy, d2f = (float)dz, gf = (float)g;
            live = live && finite_d(g) && gf > 0.f && finite_f(gf) && finite_f(o0) && finite_f(o1) && finite_f(o2) && finite_f(d0) && finite_f(d1)
                   && finite_f(d2f) && !(d0 == 0.f && d1 == 0.f && d2f == 0.f);
            float *d = tr + t * 6u;
            if (!live) { d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = 0.f; d[5] = 0.f; }
            else { d[0] = o0; d[1] = o1; d[2] = o2; d[3] = d0; d[4] = d1; d[5] = d2f; }
            weights[e] = live ? gf : 0.f;
        }
        __syncthreads();
        float *dst = out + (size_t)e0 * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * (uint32_t)AL_BLOCK + t; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(AD_BLOCK) void k_area_reduce(uint32_t first, uint32_t n, uint32_t n_lights, uint32_t samples, uint32_t group,
                                                          const uint32_t *__restrict__ ids, const uint32_t *__restrict__ objects,
                                                          const float *__restrict__ weights, const uint32_t *__restrict__ hits,
                                                          const float4 *__restrict__ surface, float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * AD_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * AD_WAVES;
    const uint32_t per = 64u / group, l = lane & (group - 1u), sub = lane / group;
    const uint32_t M = n_lights * samples;                                                // < 2^31
    const double scale_e = 1.0 / (double)samples, scale_v = 1.0 / (double)M;
    for (uint32_t base = wave * per; base < n; base += n_waves * per) {                   // wave-uniform: every lane reaches the shuffles
        const uint32_t q = base + sub;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (q < n) {
            const size_t e0 = (size_t)q * M;                                             // < 2^31
            for (uint32_t m = l; m < M; m += group) {
                const size_t e = e0 + m;
                const float w = weights[e];
                const uint32_t hobj = hits[e * 12u + 10u];
                const float4 a = surface[4 * e], em = surface[4 * e + 3];
                const uint32_t lobj = objects[m / samples];                               // m / samples < Ln
                if (!(w > 0.f) || hobj != lobj || a.w != 3.f) continue;                   // the ray did not reach its light
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
            s[0] = s[0] + (float)(scale_e * s0); s[1] = s[1] + (float)(scale_e * s1); s[2] = s[2] + (float)(scale_e * s2);
            s[3] = s[3] + (float)(scale_v * s3);
        }
    }
}

__global__ __launch_bounds__(AD_BLOCK) void k_area_resolve(uint32_t n, double rounds, const uint32_t *__restrict__ ids,
                                                           const float4 *__restrict__ sums, float4 *__restrict__ out) {
    for (uint32_t q = blockIdx.x * AD_BLOCK + threadIdx.x; q < n; q += gridDim.x * AD_BLOCK) {
        const uint32_t id = ids ? ids[q] : q;
        const float4 s = sums[id];
        out[id] = make_float4((float)((double)s.x / rounds), (float)((double)s.y / rounds), (float)((double)s.z / rounds),
                              (float)((double)s.w / rounds));
    }
}

__global__ __launch_bounds__(AD_BLOCK) void k_area_mask(uint32_t n, const uint32_t *__restrict__ objects, uint32_t n_objects,
                                                        const uint32_t *__restrict__ hits, float4 *__restrict__ surface) {
    for (uint32_t e = blockIdx.x * AD_BLOCK + threadIdx.x; e < n; e += gridDim.x * AD_BLOCK) {
        if (surface[4 * (size_t)e].w != 3.f) continue;
        const uint32_t obj = hits[(size_t)e * 12u + 10u];
        uint32_t lo = 0, hi = n_objects;                                                  // the first index with objects[index] >= obj, in [0, n_objects]
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (objects[mid] < obj) lo = mid + 1u; else hi = mid; }
        if (lo == n_objects || objects[lo] != obj) continue;
        float4 *r = surface + 4 * (size_t)e;
        r[0] = make_float4(0.f, 0.f, 0.f, -2.f);
        r[1] = make_float4(0.f, 0.f, 0.f, 0.f); r[2] = make_float4(0.f, 0.f, 0.f, 0.f); r[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

} // namespace

void launch_area_rays(hipStream_t stream, int n_cus, const DAreaRays &r, uint32_t n, float *rays, float *weights) {
    const uint32_t n_entries = n * r.n_lights * r.samples;                    // < 2^31
    hipLaunchKernelGGL(k_area_rays, dim3(grid_for(n_entries, AL_BLOCK, n_cus, 32u)), dim3(AL_BLOCK), 0, stream, r, n_entries, rays, weights);
}

void launch_area_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t n_lights, uint32_t samples, const uint32_t *ids,
                        const uint32_t *objects, const float *weights, const void *hits, const float *surface, float *sums) {
    uint32_t group = 1;
    while (group < std::min<uint32_t>(n_lights * samples, 64u)) group <<= 1;
    const uint32_t per_block = AD_WAVES * (64u / group);
    hipLaunchKernelGGL(k_area_reduce, dim3(grid_for(n, per_block, n_cus, 32u)), dim3(AD_BLOCK), 0, stream, first, n, n_lights, samples, group, ids,
                       objects, weights, (const uint32_t *)hits, (const float4 *)surface, sums);
}

void launch_area_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out) {
    hipLaunchKernelGGL(k_area_resolve, dim3(grid_for(n, AD_BLOCK, 256, 32u)), dim3(AD_BLOCK), 0, stream, n, rounds, ids, (const float4 *)sums,
                       (float4 *)out);
}

void launch_area_mask(hipStream_t stream, int n_cus, uint32_t n, const uint32_t *objects, uint32_t n_objects, const void *hits, float *surface) {
    hipLaunchKernelGGL(k_area_mask, dim3(grid_for(n, AD_BLOCK, n_cus, 32u)), dim3(AD_BLOCK), 0, stream, n, objects, n_objects, (const uint32_t *)hits,
                       (float4 *)surface);
}

} // namespace fw
