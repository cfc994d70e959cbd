// fw_direct.hip — the direct light of point, spot and directional lights at surface points for gfx950: one shadow ray per (point, light),
// and the reduction of the traced hits into irradiance, a visible-light count and a GGX highlight per point (include/firework_hip.h has
// the statement, DESIGN.md §9w the design).
//
//   k_direct_rays     one lane per entry (point q, light i), entry = q Ln + i, 256 entries per block and chunk.  The light records (48 B)
//                     are staged in LDS in tiles of at most 256: with Ln <= 256 the whole list once per block, slot i = light i; with more,
//                     per chunk the 256 records its entries need, slot t = the light of entry chunk + t.  The point's unit normal and
//                     origin are recomputed by every lane of the point rather than shared through LDS: the lanes of a point read the same
//                     three + three floats (one cache line, broadcast), one sqrt and three divisions in float64 are a small part of what an
//                     entry costs, and a shared copy would need a per-chunk pass over a varying number of points (256 / Ln + 2) and a
//                     barrier more.  24 B per entry go out through LDS: six dword stores per lane at consecutive addresses.
//   k_direct_reduce   k_ao_reduce's geometry: G = the smallest power of two >= min(Ln, 64) lanes per point, 64 / G points per wave.  Lane l
//                     of a group takes the lights i = l, l + G, ... in ascending order (consecutive lanes read consecutive 24 B rays, 48 B
//                     light records and the t and object words of consecutive 48 B hits) into seven float64 sums (E.rgb, N, S.rgb), an xor
//                     butterfly over the distances G/2 .. 1 leaves the same bits in every lane of the group, lane 0 rounds each to float32
//                     once and adds it to the point's running sums.  Of a hit only t and object are read, as k_ao_reduce reads them.
//   k_direct_resolve  one lane per point: the running sums divided by the number of rounds.
//
// No atomics, no inline assembly; k_direct_rays alone uses LDS (18 KiB) and barriers.  Every index is formed from q < n and i < Ln; no load
// depends on the content of a record.  A point's result depends on no other point and not on the launch geometry; two runs are bit-equal.
//
// finite_f and grid_for are fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.direct_rays / api.direct_reduce / api.direct_resolve;
// sqrt is the device library's float64 function.
#include "fw_direct.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int DR_BLOCK = 256;                    // k_direct_rays: entries per chunk = lanes per block
constexpr int DR_TILE = 256;                     // light records per LDS tile
constexpr int DD_BLOCK = 256;
constexpr int DD_WAVES = DD_BLOCK / 64;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// A point as both kernels see it: usable, its unit normal nh (negated towards the eye with face_view), its view and spec
struct Point {
    double px, py, pz, nx, ny, nz, vx, vy, vz;
    float f0x, f0y, f0z, rho;
    bool usable, has_view;
};
__device__ __forceinline__ Point load_point(const DDirectPoints &P, uint32_t id, uint32_t face_view) {
    Point pt;
    const float *pp = P.positions + (size_t)id * P.stride, *pn = P.normals + (size_t)id * P.stride;
    const float px = pp[0], py = pp[1], pz = pp[2], fx = pn[0], fy = pn[1], fz = pn[2];
    const double rx = (double)fx, ry = (double)fy, rz = (double)fz;
    const double rl2 = (rx * rx + ry * ry) + rz * rz;
    const double rl = sqrt(rl2);
    pt.px = (double)px; pt.py = (double)py; pt.pz = (double)pz;
    pt.nx = rx / rl; pt.ny = ry / rl; pt.nz = rz / rl;
    pt.usable = finite_f(px) && finite_f(py) && finite_f(pz) && finite_f(fx) && finite_f(fy) && finite_f(fz) && rl2 > 0.0;
    pt.has_view = P.view != nullptr;
    pt.vx = pt.vy = pt.vz = 0.0;
    if (pt.has_view) {
        const float *pv = P.view + (size_t)id * P.view_stride;
        pt.vx = (double)pv[0]; pt.vy = (double)pv[1]; pt.vz = (double)pv[2];
        if (face_view && dot3(pt.nx, pt.ny, pt.nz, pt.vx, pt.vy, pt.vz) > 0.0) { pt.nx = -pt.nx; pt.ny = -pt.ny; pt.nz = -pt.nz; }
    }
    pt.f0x = pt.f0y = pt.f0z = pt.rho = 0.f;
    if (P.spec) { const float4 s = P.spec[id]; pt.f0x = s.x; pt.f0y = s.y; pt.f0z = s.z; pt.rho = s.w; }
    return pt;
}

// §9l's spot factor of the cosine c = -(w . axis): full inside cos_inner, none outside cos_outer, a smoothstep between
__device__ __forceinline__ double spot_factor(double c, double ci, double co) {
    if (ci > co) { const double t = fmin(fmax((c - co) / (ci - co), 0.0), 1.0); return (t * t) * (3.0 - 2.0 * t); }
    return c >= co ? 1.0 : 0.0;
}

__global__ __launch_bounds__(DR_BLOCK) void k_direct_rays(DDirect R, uint32_t n_entries, float *__restrict__ out) {
    __shared__ float4 lrec[3 * DR_TILE];
    __shared__ float tr[6 * DR_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint32_t Ln = R.n_lights;
    const uint32_t n_chunks = (n_entries + (uint32_t)DR_BLOCK - 1u) / (uint32_t)DR_BLOCK;     // n_entries < 2^31
    const bool whole = Ln <= (uint32_t)DR_TILE;
    if (whole) for (uint32_t f = t; f < 3u * Ln; f += DR_BLOCK) lrec[f] = R.lights[f];
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t e0 = c * (uint32_t)DR_BLOCK;
        const uint32_t cnt = min((uint32_t)DR_BLOCK, n_entries - e0);
        if (!whole) {                                                                 // slot s = the light of entry e0 + s
            const uint32_t i0 = e0 % Ln;
            for (uint32_t f = t; f < 3u * DR_TILE; f += DR_BLOCK) {
                const uint32_t s = f / 3u, w = f - 3u * s;
                lrec[f] = R.lights[3u * ((i0 + s) % Ln) + w];                         // (i0 + s) % Ln < Ln
            }
        }
        __syncthreads();
        if (t < cnt) {
            const uint32_t e = e0 + t;
            const uint32_t q = e / Ln, i = e - q * Ln;                                // q < n, i < Ln
            const uint32_t id = R.pts.ids ? R.pts.ids[(size_t)R.first + q] : R.first + q;
            const Point pt = load_point(R.pts, id, R.face_view);
            const uint32_t slot = whole ? i : t;
            const float4 r0 = lrec[3u * slot], r1 = lrec[3u * slot + 1u], r2 = lrec[3u * slot + 2u];
            const uint32_t kind = __float_as_uint(r0.w);
            double ox = pt.px, oy = pt.py, oz = pt.pz;
            if (R.bias != 0.f) { const double bd = (double)R.bias; ox = pt.px + bd * pt.nx; oy = pt.py + bd * pt.ny; oz = pt.pz + bd * pt.nz; }
            double dx, dy, dz;
            if (kind == 2u) { dx = -(double)r1.x; dy = -(double)r1.y; dz = -(double)r1.z; }
            else { dx = (double)r0.x - ox; dy = (double)r0.y - oy; dz = (double)r0.z - oz; }
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const double dl = sqrt(d2);
            const double wx = dx / dl, wy = dy / dl, wz = dz / dl;
            const double cn = dot3(pt.nx, pt.ny, pt.nz, wx, wy, wz);
            double s = 1.0;
            if (kind == 1u) s = spot_factor(-dot3(wx, wy, wz, (double)r1.x, (double)r1.y, (double)r1.z), (double)r1.w, (double)r2.w);
            const float o0 = (float)ox, o1 = (float)oy, o2 = (float)oz, d0 = (float)dx, d1 = (float)dy, d2f = (float)dz;
            const bool lit = pt.usable && !(R.pts.spec && pt.rho < 0.f) && !(r2.x == 0.f && r2.y == 0.f && r2.z == 0.f) && d2 > 0.0 && finite_d(d2)
                             && cn > 0.0 && s != 0.0 && finite_f(o0) && finite_f(o1) && finite_f(o2) && finite_f(d0) && finite_f(d1) && finite_f(d2f)
                             && !(d0 == 0.f && d1 == 0.f && d2f == 0.f);
            float *d = tr + t * 6u;
            if (!lit) { d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = 0.f; d[5] = 0.f; }
            else { d[0] = o0; d[1] = o1; d[2] = o2; d[3] = d0; d[4] = d1; d[5] = d2f; }
        }
        __syncthreads();
        float *dst = out + (size_t)e0 * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * (uint32_t)DR_BLOCK + t; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DD_BLOCK) void k_direct_reduce(DDirect R, uint32_t n, uint32_t group, const float *__restrict__ rays,
                                                            const uint32_t *__restrict__ hits, float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * DD_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * DD_WAVES;
    const uint32_t per = 64u / group, l = lane & (group - 1u), sub = lane / group;
    const uint32_t Ln = R.n_lights;
    const double PI = 3.141592653589793;
    for (uint32_t base = wave * per; base < n; base += n_waves * per) {                   // wave-uniform: every lane reaches the shuffles
        const uint32_t q = base + sub;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6 = 0.0;
        uint32_t id = 0;
        if (q < n) {
            id = R.pts.ids ? R.pts.ids[(size_t)R.first + q] : R.first + q;
            const Point pt = load_point(R.pts, id, R.face_view);
            const bool glossy = pt.rho > 0.f;
            // the eye's side of a glossy point: wo = -view / |view|, its cosine, Smith's Lambda of it
            double wox = 0.0, woy = 0.0, woz = 0.0, co = 0.0, lo = 0.0, al2 = 0.0;
            if (glossy) {
                const double ul = sqrt(dot3(pt.vx, pt.vy, pt.vz, pt.vx, pt.vy, pt.vz));
                wox = -(pt.vx / ul); woy = -(pt.vy / ul); woz = -(pt.vz / ul);
                co = dot3(pt.nx, pt.ny, pt.nz, wox, woy, woz);
                const double al = (double)(pt.rho * pt.rho);
                al2 = al * al;
                const double tx = wox - co * pt.nx, ty = woy - co * pt.ny, tz = woz - co * pt.nz;
                lo = 0.5 * (sqrt(1.0 + al2 * (dot3(tx, ty, tz, tx, ty, tz) / (co * co))) - 1.0);
            }
            const bool takes = pt.usable && !(pt.rho < 0.f) && (!glossy || (pt.has_view && co > 0.0));
            const size_t e0 = (size_t)q * Ln;                                            // < 2^31
            for (uint32_t i = l; i < Ln; i += group) {
                const float *r = rays + (e0 + i) * 6u + 3u;
                const uint32_t *h = hits + (e0 + i) * 12u;
                const float4 r0 = R.lights[3u * i], r1 = R.lights[3u * i + 1u], r2 = R.lights[3u * i + 2u];
                const float fx = r[0], fy = r[1], fz = r[2];
                const float ht = __uint_as_float(h[0]);
                const uint32_t hobj = h[10];
                if ((fx == 0.f && fy == 0.f && fz == 0.f) || !takes) continue;             // a zero ray contributes nothing
                const uint32_t kind = __float_as_uint(r0.w);
                const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!finite_d(d2)) continue;
                const double dl = sqrt(d2);
                const double wx = dx / dl, wy = dy / dl, wz = dz / dl;
                const double cn = dot3(pt.nx, pt.ny, pt.nz, wx, wy, wz);
                if (!(cn > 0.0)) continue;
                const bool vis = hobj == 0xFFFFFFFFu || (kind != 2u && ht >= 1.0f);
                if (!vis) continue;
                a3 = a3 + 1.0;
                double Lx = (double)r2.x, Ly = (double)r2.y, Lz = (double)r2.z;
                if (kind != 2u) {
                    double s = 1.0;
                    if (kind == 1u) s = spot_factor(-dot3(wx, wy, wz, (double)r1.x, (double)r1.y, (double)r1.z), (double)r1.w, (double)r2.w);
                    Lx = (Lx * s) / d2; Ly = (Ly * s) / d2; Lz = (Lz * s) / d2;
                }
                if (!glossy) {
                    const double g = R.lobe ? 2.0 * ((cn * cn) * cn) : cn;
                    a0 = a0 + Lx * g; a1 = a1 + Ly * g; a2 = a2 + Lz * g;
                } else {
                    // §9m's f cos = F D G2 / (4 wo.n) around nh, without a tangent frame: tangential parts as x - (x . nh) nh
                    const double hx0 = wox + wx, hy0 = woy + wy, hz0 = woz + wz;
                    const double hl = sqrt(dot3(hx0, hy0, hz0, hx0, hy0, hz0));
                    const double hx = hx0 / hl, hy = hy0 / hl, hz = hz0 / hl;
                    const double hn = dot3(pt.nx, pt.ny, pt.nz, hx, hy, hz), oh = dot3(wox, woy, woz, hx, hy, hz);
                    const double tx = hx - hn * pt.nx, ty = hy - hn * pt.ny, tz = hz - hn * pt.nz;
                    const double sd = dot3(tx, ty, tz, tx, ty, tz) + al2 * (hn * hn);
                    const double D = al2 / (PI * (sd * sd));
                    const double ux = wx - cn * pt.nx, uy = wy - cn * pt.ny, uz = wz - cn * pt.nz;
                    const double li = 0.5 * (sqrt(1.0 + al2 * (dot3(ux, uy, uz, ux, uy, uz) / (cn * cn))) - 1.0);
                    const double gg = (D / (4.0 * co)) / ((1.0 + lo) + li);
                    const double m = 1.0 - oh, m2 = m * m, m5 = (m2 * m2) * m;
                    const double f0x = (double)pt.f0x, f0y = (double)pt.f0y, f0z = (double)pt.f0z;
                    a4 = a4 + Lx * ((f0x + (1.0 - f0x) * m5) * gg);
                    a5 = a5 + Ly * ((f0y + (1.0 - f0y) * m5) * gg);
                    a6 = a6 + Lz * ((f0z + (1.0 - f0z) * m5) * gg);
                }
            }
        }
        for (uint32_t m = group >> 1; m >= 1u; m >>= 1) {
            a0 = a0 + __shfl_xor(a0, (int)m, 64); a1 = a1 + __shfl_xor(a1, (int)m, 64); a2 = a2 + __shfl_xor(a2, (int)m, 64);
            a3 = a3 + __shfl_xor(a3, (int)m, 64); a4 = a4 + __shfl_xor(a4, (int)m, 64); a5 = a5 + __shfl_xor(a5, (int)m, 64);
            a6 = a6 + __shfl_xor(a6, (int)m, 64);
        }
        if (q < n && l == 0u) {
            float *s = sums + (size_t)id * 8u;
            s[0] = s[0] + (float)a0; s[1] = s[1] + (float)a1; s[2] = s[2] + (float)a2; s[3] = s[3] + (float)a3;
            s[4] = s[4] + (float)a4; s[5] = s[5] + (float)a5; s[6] = s[6] + (float)a6;
        }
    }
}

__global__ __launch_bounds__(DD_BLOCK) void k_direct_resolve(uint32_t n, double rounds, const uint32_t *__restrict__ ids,
                                                             const float4 *__restrict__ sums, float4 *__restrict__ out) {
    for (uint32_t q = blockIdx.x * DD_BLOCK + threadIdx.x; q < n; q += gridDim.x * DD_BLOCK) {
        const uint32_t id = ids ? ids[q] : q;
        const float4 a = sums[2u * (size_t)id], b = sums[2u * (size_t)id + 1u];
        out[2u * (size_t)id] = make_float4((float)((double)a.x / rounds), (float)((double)a.y / rounds), (float)((double)a.z / rounds),
                                           (float)((double)a.w / rounds));
        out[2u * (size_t)id + 1u] = make_float4((float)((double)b.x / rounds), (float)((double)b.y / rounds), (float)((double)b.z / rounds), 0.f);
    }
}

} // namespace

void launch_direct_rays(hipStream_t stream, int n_cus, const DDirect &d, uint32_t n, float *out) {
    const uint32_t n_entries = n * d.n_lights;                                // < 2^31
    hipLaunchKernelGGL(k_direct_rays, dim3(grid_for(n_entries, DR_BLOCK, n_cus, 32u)), dim3(DR_BLOCK), 0, stream, d, n_entries, out);
}

void launch_direct_reduce(hipStream_t stream, int n_cus, const DDirect &d, uint32_t n, const float *rays, const void *hits, float *sums) {
    uint32_t group = 1;
    while (group < std::min<uint32_t>(d.n_lights, 64u)) group <<= 1;
    const uint32_t per_block = DD_WAVES * (64u / group);
    hipLaunchKernelGGL(k_direct_reduce, dim3(grid_for(n, per_block, n_cus, 32u)), dim3(DD_BLOCK), 0, stream, d, n, group, rays,
                       (const uint32_t *)hits, sums);
}

void launch_direct_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out) {
    hipLaunchKernelGGL(k_direct_resolve, dim3(grid_for(n, DD_BLOCK, 256, 32u)), dim3(DD_BLOCK), 0, stream, n, rounds, ids, (const float4 *)sums,
                       (float4 *)out);
}

} // namespace fw
