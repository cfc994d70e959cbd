// fw_probe_place.hip — probe relocation and classification for gfx950: the survey of a probe's traced rays, the step that moves a probe
// out of geometry and marks it active or inactive, and the two lookup kernels that honour the result (include/firework_hip.h has the
// statement, DESIGN.md §9u the design).
//
//   k_probe_survey             one wave per probe, as k_probe_project.  Lane l walks the rays j = l, l + 64, ... in ascending order: 12 B of
//                              direction, and of the 48-byte hit 4 B of t, 12 B of normal and 4 B of object.  It keeps the nearest back
//                              face and the nearest front face as (dist, j) with strict <, and three counters, all in registers.  The 64
//                              lanes are joined by six __shfl_xor steps that take the lexicographic minimum of (dist, j) and add the
//                              counters; the loop over probes is wave-uniform, so every lane reaches every shuffle.  Lane 0 re-reads the
//                              two winning directions and writes the record as three 16-byte stores.  The minimum and the sums of
//                              integers do not depend on the order they are taken in: the result is a pure function of the inputs.
//   k_probe_relocate_step      one lane per probe: 48 B of survey and 16 B of placement in, 16 B (or, without a move, 4 B) out.
//   k_probe_irradiance_placed  k_probe_irradiance_vis over moved probes, one lane per point, templated on whether depth maps are given.
//                              Per corner the lane reads 16 B of placement; an inactive corner reads nothing else.
//   k_probe_shade_placed       k_probe_shade_vis with the same lookup.
//
// No LDS, no atomics, no barrier, no inline assembly.  Every sh, placement and moments index is formed from a clamped cell index and
// texel indices clamped to [0, R - 2] plus 0 or 1, so no load leaves the arrays wherever the point lies.
//
// A file of its own, last on the link line: the code objects of the other files stay byte for byte what they were.  What it needs of
// fw_probe_lookup.hip and fw_probe_depth.hip (the SH constants, the cell, depth_fetch, fdiv, resolve_pixel) is restated here, operation
// for operation: the same bits.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.probe_survey, api.probe_relocate_step and
// api.probe_lookup_placed; floor, min, max and fabs are exact; sqrt is the device library's float64 function.
#include "fw_probe_place.h"
#include "fw_libm.h"
#include <algorithm>
#include <cmath>

namespace fw {
namespace {

constexpr int PS_WAVES = 4;                     // waves per workgroup of k_probe_survey
constexpr int PM_BLOCK = 256;                   // k_probe_relocate_step
constexpr int PP_BLOCK = 256;                   // the placed lookups
constexpr uint32_t NO_RAY = 0xFFFFFFFFu;        // no hit of a class yet: above every j (D <= 2^20)

// the nearer of (d, j) and (od, oj): the smaller distance, at equal distance the lower index
__device__ __forceinline__ void take_nearer(double &d, uint32_t &j, double od, uint32_t oj) {
    if (od < d || (od == d && oj < j)) { d = od; j = oj; }
}

__global__ __launch_bounds__(PS_WAVES * 64) void k_probe_survey(uint32_t n_probes, uint32_t directions, const float *__restrict__ rays,
                                                                const uint32_t *__restrict__ hits, float4 *__restrict__ survey) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * PS_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * PS_WAVES;
    const double INF = __builtin_huge_val();
    for (uint32_t p = wave; p < n_probes; p += n_waves) {                             // wave-uniform
        const size_t base = (size_t)p * directions;                                   // < 2^31
        double bd = INF, fd = INF;
        uint32_t bj = NO_RAY, fj = NO_RAY, nb = 0u, nf = 0u, nm = 0u;
        for (uint32_t j = lane; j < directions; j += 64u) {
            const float *r = rays + (base + j) * 6u + 3u;
            const uint32_t *h = hits + (base + j) * 12u;
            const float fx = r[0], fy = r[1], fz = r[2];
            if (fx == 0.f && fy == 0.f && fz == 0.f) continue;                        // a ray that was never asked for
            if (h[10] == 0xFFFFFFFFu) { nm++; continue; }
            const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
            const double dist = (double)__uint_as_float(h[0]) * sqrt((dx * dx + dy * dy) + dz * dz);
            const double nx = (double)__uint_as_float(h[4]), ny = (double)__uint_as_float(h[5]), nz = (double)__uint_as_float(h[6]);
            if (((nx * dx + ny * dy) + nz * dz) > 0.0) {
                nb++;
                if (dist < bd) { bd = dist; bj = j; }
            } else {
                nf++;
                if (dist < fd) { fd = dist; fj = j; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double obd = __shfl_xor(bd, m, 64), ofd = __shfl_xor(fd, m, 64);
            const uint32_t obj = __shfl_xor(bj, m, 64), ofj = __shfl_xor(fj, m, 64);
            take_nearer(bd, bj, obd, obj);
            take_nearer(fd, fj, ofd, ofj);
            nb += __shfl_xor(nb, m, 64);
            nf += __shfl_xor(nf, m, 64);
            nm += __shfl_xor(nm, m, 64);
        }
        if (lane == 0u) {
            float4 b = make_float4(0.f, 0.f, 0.f, (float)INF), f = b;
            if (bj != NO_RAY) { const float *r = rays + (base + bj) * 6u + 3u; b = make_float4(r[0], r[1], r[2], (float)bd); }
            if (fj != NO_RAY) { const float *r = rays + (base + fj) * 6u + 3u; f = make_float4(r[0], r[1], r[2], (float)fd); }
            float4 *s = survey + (size_t)p * 3u;
            s[0] = b; s[1] = f; s[2] = make_float4((float)nb, (float)nf, (float)nm, 0.f);
        }
    }
}

__global__ __launch_bounds__(PM_BLOCK) void k_probe_relocate_step(DRelocate L, uint32_t n_probes, uint32_t directions,
                                                                  const float4 *__restrict__ survey, float4 *__restrict__ placement, int move) {
    const uint32_t p = blockIdx.x * PM_BLOCK + threadIdx.x;                           // one probe per lane: the grid covers n_probes
    if (p >= n_probes) return;
    const float4 b = survey[(size_t)p * 3u], f = survey[(size_t)p * 3u + 1u], c = survey[(size_t)p * 3u + 2u];
    const bool inside = (double)c.x > L.back_fraction * (double)directions;
    const float a = inside ? 0.f : 1.f;
    if (!move) { ((float *)(placement + p))[3] = a; return; }
    const float4 o = placement[p];
    const double od[3] = {(double)o.x, (double)o.y, (double)o.z};
    double cand[3] = {od[0], od[1], od[2]};
    if (inside) {
        const double dx = (double)b.x, dy = (double)b.y, dz = (double)b.z;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        const double s = (double)b.w + 0.5 * L.min_front;
        cand[0] = od[0] + (dx / len) * s; cand[1] = od[1] + (dy / len) * s; cand[2] = od[2] + (dz / len) * s;
    } else if (c.y > 0.f && (double)f.w < L.min_front) {
        const double dx = (double)f.x, dy = (double)f.y, dz = (double)f.z;
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        const double s = L.min_front - (double)f.w;
        cand[0] = od[0] - (dx / len) * s; cand[1] = od[1] - (dy / len) * s; cand[2] = od[2] - (dz / len) * s;
    }
    const float cx = (float)cand[0], cy = (float)cand[1], cz = (float)cand[2];
    // rejected, not clamped; a candidate that is not a number is rejected too
    const bool ok = fabs((double)cx) <= L.max_offset[0] && fabs((double)cy) <= L.max_offset[1] && fabs((double)cz) <= L.max_offset[2];
    placement[p] = ok ? make_float4(cx, cy, cz, a) : make_float4(o.x, o.y, o.z, a);
}

// the constants of fw_probe_lookup.hip's LookupConst, restated
struct PlaceConst { double y0, c1, c2, c6, c8, a0, a1, a2; };

__device__ __forceinline__ double sgn1(double v) { return v >= 0.0 ? 1.0 : -1.0; }      // sgn(0) = +1
__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.40282347e+38f; }   // false for NaN and +-inf

// fw_probe_depth.hip's depth_fetch, restated
__device__ __forceinline__ void depth_fetch(const float *__restrict__ m, uint32_t R, double x, double y, double z, double &mu, double &mu2) {
    const double s1 = (fabs(x) + fabs(y)) + fabs(z);
    double ox = x / s1, oy = y / s1;
    if (z < 0.0) {
        const double fx = (1.0 - fabs(oy)) * sgn1(ox), fy = (1.0 - fabs(ox)) * sgn1(oy);
        ox = fx; oy = fy;
    }
    const double Rd = (double)R, top = Rd - 1.0;
    const double su = fmin(fmax(((ox + 1.0) * 0.5) * Rd - 0.5, 0.0), top), sv = fmin(fmax(((oy + 1.0) * 0.5) * Rd - 0.5, 0.0), top);
    const double iu = fmin(floor(su), top - 1.0), jv = fmin(floor(sv), top - 1.0);       // in [0, R - 2] whatever su and sv are
    const double fu = su - iu, fv = sv - jv;
    const float *__restrict__ r0 = m + ((size_t)((uint32_t)jv * R + (uint32_t)iu)) * 2u;
    const float *__restrict__ r1 = r0 + (size_t)R * 2u;
    const double gu = 1.0 - fu, gv = 1.0 - fv;
    mu = (((double)r0[0] * gu + (double)r0[2] * fu) * gv) + (((double)r1[0] * gu + (double)r1[2] * fu) * fv);
    mu2 = (((double)r0[1] * gu + (double)r0[3] * fu) * gv) + (((double)r1[1] * gu + (double)r1[3] * fu) * fv);
}

// The lookup of fw_probe_lookup.hip (DEPTH false) or fw_probe_depth.hip (DEPTH true) over placed probes: a corner's probe stands at
// P + o, a corner with a == 0 is skipped, and the remaining weights are always divided by their sum.  E[c] in float64 before its one
// rounding; false (and E untouched) for a point that the statement answers with zeros.
template <bool DEPTH>
__device__ __forceinline__ bool probe_lookup_placed(const DProbeGrid &G, const DProbeVis &V, const PlaceConst &K, const float *__restrict__ sh,
                                                    const float *__restrict__ placement, float pxf, float pyf, float pzf, float nxf, float nyf,
                                                    float nzf, double E[3]) {
    if (!(finite_f(pxf) && finite_f(pyf) && finite_f(pzf) && finite_f(nxf) && finite_f(nyf) && finite_f(nzf))) return false;
    const double p[3] = {(double)pxf, (double)pyf, (double)pzf};
    const double nx = (double)nxf, ny = (double)nyf, nz = (double)nzf;
    const double nl2 = (nx * nx + ny * ny) + nz * nz;
    if (!(nl2 > 0.0)) return false;
    const double nl = sqrt(nl2);
    const double x = nx / nl, y = ny / nl, z = nz / nl;
    double q[3] = {p[0], p[1], p[2]};
    if (DEPTH) { q[0] = p[0] + V.bias * x; q[1] = p[1] + V.bias * y; q[2] = p[2] + V.bias * z; }

    // the cell: the nominal grid's
    uint32_t i[3];
    double f[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        i[k] = 0u; f[k] = 0.0;
        if (G.counts[k] > 1u) {
            const double cm1 = (double)(G.counts[k] - 1u);
            double s = ((p[k] - G.lo[k]) / G.span[k]) * cm1;
            s = fmin(fmax(s, 0.0), cm1);
            const double fl = fmin(floor(s), cm1 - 1.0);
            i[k] = (uint32_t)fl;
            f[k] = s - fl;
        }
    }
    const bool two[3] = {G.counts[0] > 1u, G.counts[1] > 1u, G.counts[2] > 1u};      // wave-uniform: a flat axis has one corner
    const size_t map_floats = DEPTH ? (size_t)V.R * V.R * 2u : 0u;

    // the corner weights, corner d = 4 dz + 2 dy + dx
    double w[8];
    uint32_t active = 0u;
    double wsum = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        w[d] = 0.0;
        if ((dx == 0 || two[0]) && (dy == 0 || two[1]) && (dz == 0 || two[2])) {
            const uint32_t probe = ((i[2] + (uint32_t)dz) * G.counts[1] + (i[1] + (uint32_t)dy)) * G.counts[0] + (i[0] + (uint32_t)dx);   // < 2^31
            const float *__restrict__ pl = placement + (size_t)probe * 4u;
            if (pl[3] == 0.f) continue;                                                // inactive: nothing of this probe is read
            active |= 1u << d;
            const double wx = dx ? f[0] : 1.0 - f[0], wy = dy ? f[1] : 1.0 - f[1], wz = dz ? f[2] : 1.0 - f[2];
            const int dd[3] = {dx, dy, dz};
            double P[3];
#pragma unroll
            for (int k = 0; k < 3; k++) P[k] = (two[k] ? G.lo[k] + (double)(i[k] + (uint32_t)dd[k]) * G.step[k] : G.mid[k]) + (double)pl[k];
            double fac = 1.0;
            if (G.wrap) {
                const double r[3] = {P[0] - p[0], P[1] - p[1], P[2] - p[2]};
                const double rl2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                fac = 1.2;
                if (rl2 > 0.0) {
                    const double rl = sqrt(rl2);
                    const double dot = (x * (r[0] / rl) + y * (r[1] / rl)) + z * (r[2] / rl);
                    const double h = 0.5 * (dot + 1.0);
                    fac = h * h + 0.2;
                }
            }
            double wd = (wx * wy) * wz;
            if (DEPTH) {
                // the visibility of this probe from the biased point
                const double rv[3] = {q[0] - P[0], q[1] - P[1], q[2] - P[2]};
                const double dist = sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2]);
                double v = 1.0;
                if (dist != 0.0) {
                    double mu, mu2;
                    depth_fetch(V.moments + (size_t)probe * map_floats, V.R, rv[0] / dist, rv[1] / dist, rv[2] / dist, mu, mu2);
                    if (!(dist <= mu)) {
                        const double var = fabs(mu * mu - mu2);
                        const double t = dist - mu;
                        const double c = var / (var + t * t);
                        v = (c * c) * c;
                    }
                }
                double g = fmax(1e-6, fac * v);
                if (g < 0.2) g = (g * (g * g)) * 25.0;
                wd = wd * g;
            } else if (G.wrap) {
                wd = wd * fac;
            }
            wsum = wsum + wd;
            w[d] = wd;
        }
    }
    if (wsum == 0.0) return false;                                                     // no active corner, or none with a weight

    const double B[9] = {K.a0 * K.y0,           K.a1 * (K.c1 * y),       K.a1 * (K.c1 * z),
                         K.a1 * (K.c1 * x),     K.a2 * ((K.c2 * x) * y), K.a2 * ((K.c2 * y) * z),
                         K.a2 * (K.c6 * (3.0 * (z * z) - 1.0)), K.a2 * ((K.c2 * x) * z), K.a2 * (K.c8 * (x * x - y * y))};
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        if (active & (1u << d)) {
            const uint32_t probe = ((i[2] + (uint32_t)dz) * G.counts[1] + (i[1] + (uint32_t)dy)) * G.counts[0] + (i[0] + (uint32_t)dx);   // < 2^31
            const float *__restrict__ s = sh + (size_t)probe * 27u;
            double c0 = B[0] * (double)s[0], c1 = B[0] * (double)s[1], c2 = B[0] * (double)s[2];
#pragma unroll
            for (int k = 1; k < 9; k++) {
                c0 = c0 + B[k] * (double)s[3 * k];
                c1 = c1 + B[k] * (double)s[3 * k + 1];
                c2 = c2 + B[k] * (double)s[3 * k + 2];
            }
            const double wd = w[d] / wsum;
            e0 = e0 + wd * c0; e1 = e1 + wd * c1; e2 = e2 + wd * c2;
        }
    }
    E[0] = e0; E[1] = e1; E[2] = e2;
    return true;
}

template <bool DEPTH>
__global__ __launch_bounds__(PP_BLOCK) void k_probe_irradiance_placed(DProbeGrid G, DProbeVis V, PlaceConst K, const float *__restrict__ sh,
                                                                      const float *__restrict__ placement, uint32_t n,
                                                                      const float *__restrict__ positions, const float *__restrict__ normals,
                                                                      uint32_t stride, float *__restrict__ out) {
    const uint32_t q = blockIdx.x * PP_BLOCK + threadIdx.x;                           // one point per lane: the grid covers n
    if (q < n) {
        const float *pp = positions + (size_t)q * stride, *nn = normals + (size_t)q * stride;
        double E[3];
        float r = 0.f, g = 0.f, b = 0.f;
        if (probe_lookup_placed<DEPTH>(G, V, K, sh, placement, pp[0], pp[1], pp[2], nn[0], nn[1], nn[2], E)) { r = (float)E[0]; g = (float)E[1]; b = (float)E[2]; }
        float *o = out + (size_t)q * 3u;
        o[0] = r; o[1] = g; o[2] = b;
    }
}

// fw_kernels.hip's fdiv and resolve_pixel, as fw_probe_lookup.hip restates them: the same bits
__device__ __forceinline__ float fdiv(float a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    r = fmaf(fmaf(-b, r, 1.0f), r, r);
    float q = a * r;
    q = fmaf(fmaf(-b, q, a), r, q);
    q = fmaf(fmaf(-b, q, a), r, q);
    return __builtin_amdgcn_div_fixupf(q, b, a);
}
__device__ __forceinline__ uint8_t sat_u8(float f) { if (!(f > 0.f)) return 0; if (f >= 255.f) return 255; return (uint8_t)f; }
__device__ __forceinline__ float clamp01(float x) { return (x != x) ? x : (x < 0.f ? 0.f : (x > 1.f ? 1.f : x)); }
__device__ __forceinline__ void resolve_pixel(float cr, float cg, float cb, float spp, float gamma, uint32_t p, uint8_t *rgb8, float *gamma_rgb,
                                              float *linear_rgb) {
    const float tr = fdiv(cr, spp), tg = fdiv(cg, spp), tb = fdiv(cb, spp);
    const float ig = fdiv(1.f, gamma);
    const float gr = clamp01(fwlm::powf_glibc(tr, ig)), gg = clamp01(fwlm::powf_glibc(tg, ig)), gb = clamp01(fwlm::powf_glibc(tb, ig));
    if (linear_rgb) { linear_rgb[3 * (size_t)p] = tr; linear_rgb[3 * (size_t)p + 1] = tg; linear_rgb[3 * (size_t)p + 2] = tb; }
    if (gamma_rgb) { gamma_rgb[3 * (size_t)p] = gr; gamma_rgb[3 * (size_t)p + 1] = gg; gamma_rgb[3 * (size_t)p + 2] = gb; }
    if (rgb8) { rgb8[3 * (size_t)p] = sat_u8(gr * 255.99f); rgb8[3 * (size_t)p + 1] = sat_u8(gg * 255.99f); rgb8[3 * (size_t)p + 2] = sat_u8(gb * 255.99f); }
}

template <bool DEPTH>
__global__ __launch_bounds__(PP_BLOCK) void k_probe_shade_placed(DProbeGrid G, DProbeVis V, PlaceConst K, const float *__restrict__ sh,
                                                                 const float *__restrict__ placement, uint32_t n, const float4 *__restrict__ aov,
                                                                 float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    const float inv_pi = (float)(1.0 / 3.141592653589793);
    const uint32_t p = blockIdx.x * PP_BLOCK + threadIdx.x;                           // one pixel per lane: the grid covers n
    if (p < n) {
        const float4 a = aov[3 * (size_t)p], nd = aov[3 * (size_t)p + 1], xa = aov[3 * (size_t)p + 2];
        double E[3];
        float er = 0.f, eg = 0.f, eb = 0.f;
        if (probe_lookup_placed<DEPTH>(G, V, K, sh, placement, xa.x, xa.y, xa.z, nd.x, nd.y, nd.z, E)) { er = (float)E[0]; eg = (float)E[1]; eb = (float)E[2]; }
        er = er > 0.f ? er : 0.f; eg = eg > 0.f ? eg : 0.f; eb = eb > 0.f ? eb : 0.f;
        const float v = a.w, rest = 1.f - v;
        resolve_pixel(a.x * (v * (er * inv_pi) + rest), a.y * (v * (eg * inv_pi) + rest), a.z * (v * (eb * inv_pi) + rest), 1.0f, gamma, p, rgb8,
                      gamma_rgb, linear_rgb);
    }
}

PlaceConst place_const() {
    const double PI = 3.141592653589793;
    return PlaceConst{0.5 * std::sqrt(1.0 / PI), std::sqrt(3.0 / (4.0 * PI)), 0.5 * std::sqrt(15.0 / PI), 0.25 * std::sqrt(5.0 / PI),
                      0.25 * std::sqrt(15.0 / PI), PI, 2.0 * PI / 3.0, PI / 4.0};
}
uint32_t place_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + PP_BLOCK - 1) / PP_BLOCK); }      // n > 0; at most 2^24 blocks

} // namespace

void launch_probe_survey(hipStream_t stream, int n_cus, uint32_t n, uint32_t directions, const float *rays, const void *hits, float *survey) {
    const uint32_t want = (n + PS_WAVES - 1u) / PS_WAVES;
    const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>(want, (uint32_t)std::max(1, n_cus) * 32u));
    hipLaunchKernelGGL(k_probe_survey, dim3(blocks), dim3(PS_WAVES * 64), 0, stream, n, directions, rays, (const uint32_t *)hits, (float4 *)survey);
}

void launch_probe_relocate_step(hipStream_t stream, const DRelocate &rl, uint32_t n, uint32_t directions, const float *survey, float *placement,
                                int move) {
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PM_BLOCK - 1) / PM_BLOCK);
    hipLaunchKernelGGL(k_probe_relocate_step, dim3(blocks), dim3(PM_BLOCK), 0, stream, rl, n, directions, (const float4 *)survey, (float4 *)placement,
                       move);
}

void launch_probe_irradiance_placed(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const float *sh, const float *placement, uint32_t n,
                                    const float *positions, const float *normals, uint32_t stride_floats, float *irradiance) {
    if (v) hipLaunchKernelGGL(k_probe_irradiance_placed<true>, dim3(place_blocks(n)), dim3(PP_BLOCK), 0, stream, g, *v, place_const(), sh, placement, n,
                              positions, normals, stride_floats, irradiance);
    else hipLaunchKernelGGL(k_probe_irradiance_placed<false>, dim3(place_blocks(n)), dim3(PP_BLOCK), 0, stream, g, DProbeVis{nullptr, 0.0, 0u},
                            place_const(), sh, placement, n, positions, normals, stride_floats, irradiance);
}

void launch_probe_shade_placed(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const float *sh, const float *placement, uint32_t n,
                               const float *aov, float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    if (v) hipLaunchKernelGGL(k_probe_shade_placed<true>, dim3(place_blocks(n)), dim3(PP_BLOCK), 0, stream, g, *v, place_const(), sh, placement, n,
                              (const float4 *)aov, gamma, rgb8, gamma_rgb, linear_rgb);
    else hipLaunchKernelGGL(k_probe_shade_placed<false>, dim3(place_blocks(n)), dim3(PP_BLOCK), 0, stream, g, DProbeVis{nullptr, 0.0, 0u},
                            place_const(), sh, placement, n, (const float4 *)aov, gamma, rgb8, gamma_rgb, linear_rgb);
}

} // namespace fw
