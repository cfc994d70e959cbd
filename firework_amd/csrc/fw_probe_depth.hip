// fw_probe_depth.hip — probe visibility for gfx950: the reduction of traced distances into per-probe depth moments, and the two lookup
// kernels that weight a probe by them (include/firework_hip.h has the statement, DESIGN.md §9s the design).
//
//   k_probe_depth           one workgroup of 256 lanes per probe.  256 directions at a time, lane l turns ray and hit c0 + l (12 B of
//                           direction, 4 B of t and 4 B of object) into (d.xyz, dist) in float64 and stages the 32 B in LDS; after the
//                           barrier every lane walks the staged chunk in ascending j for its texels t = lane, lane + 256, ... (at most
//                           four, R = 32).  All lanes read the same LDS address at once: a broadcast, no bank conflict.  A texel's three
//                           float64 accumulators stay in registers across the chunks; at the end each is rounded to float32 once and
//                           added to the texel's running sums with one float32 addition (.w is neither read nor written).  A texel is
//                           one lane's and its sum is sequential in j, so the result is a pure function of the inputs: no atomics, and
//                           no dependence on the launch geometry.  With R = 4 only 16 lanes of a workgroup have a texel; that is accepted
//                           (the trace beside it is the cost of a bake).
//   k_probe_irradiance_vis  k_probe_irradiance (fw_probe_lookup.hip) with the visibility weight: one lane per point.  Per corner the
//                           lane fetches four texels (mu, mu2: 8 B each, two 16-byte rows) of that probe's map, bilinearly.
//   k_probe_shade_vis       k_probe_shade with the same lookup.
//
// The lookup kernels use no LDS, no atomics and no barrier.  Every moments index is formed from a clamped cell index (as in
// fw_probe_lookup.hip) and texel indices clamped to [0, R - 2] plus 0 or 1, so no load leaves the arrays wherever the point lies.  No
// inline assembly anywhere.
//
// A file of its own, last on the link line: the code objects of the other files stay byte for byte what they were.  What it needs of
// fw_probe_lookup.hip (the SH constants, the cell) and of fw_kernels.hip (fdiv, resolve_pixel) is restated here: the same bits.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.probe_depth_reduce / api.probe_lookup_vis; floor, min,
// max and fabs are exact; sqrt is the device library's float64 function.
#include "fw_probe_depth.h"
#include "fw_libm.h"
#include <algorithm>
#include <cmath>

namespace fw {
namespace {

constexpr int PD_BLOCK = 256;
constexpr int PD_MAXT = 4;                      // texels per lane at R = 32
constexpr int PV_BLOCK = 256;

__device__ __forceinline__ double sgn1(double v) { return v >= 0.0 ? 1.0 : -1.0; }      // sgn(0) = +1

// the unit direction of texel t = b R + a of an R x R octahedral map
__device__ __forceinline__ void texel_dir(uint32_t t, uint32_t R, double T[3]) {
    const uint32_t b = t / R, a = t - b * R;
    const double Rd = (double)R;
    const double ex = (((double)a + 0.5) * 2.0) / Rd - 1.0, ey = (((double)b + 0.5) * 2.0) / Rd - 1.0;
    const double z = (1.0 - fabs(ex)) - fabs(ey);
    double x = ex, y = ey;
    if (z < 0.0) { x = (1.0 - fabs(ey)) * sgn1(ex); y = (1.0 - fabs(ex)) * sgn1(ey); }
    const double l = sqrt((x * x + y * y) + z * z);
    T[0] = x / l; T[1] = y / l; T[2] = z / l;
}

__global__ __launch_bounds__(PD_BLOCK) void k_probe_depth(uint32_t n_probes, uint32_t directions, uint32_t R, uint32_t k, double r_max,
                                                          const float *__restrict__ rays, const uint32_t *__restrict__ hits,
                                                          float *__restrict__ sums) {
    __shared__ double st[PD_BLOCK * 4];                                                 // (dx, dy, dz, dist) of the staged directions
    const uint32_t lane = threadIdx.x;
    const uint32_t n_tex = R * R;
    const uint32_t nq = (n_tex + PD_BLOCK - 1u) / PD_BLOCK;                             // wave-uniform: 1, or 4 at R = 32
    double T[PD_MAXT][3];
#pragma unroll
    for (int q = 0; q < PD_MAXT; q++) {
        T[q][0] = T[q][1] = T[q][2] = 0.0;
        const uint32_t t = lane + (uint32_t)q * PD_BLOCK;
        if (t < n_tex) texel_dir(t, R, T[q]);
    }
    for (uint32_t p = blockIdx.x; p < n_probes; p += gridDim.x) {
        const size_t base = (size_t)p * directions;                                    // < 2^31
        double A[PD_MAXT], B[PD_MAXT], W[PD_MAXT];
#pragma unroll
        for (int q = 0; q < PD_MAXT; q++) { A[q] = 0.0; B[q] = 0.0; W[q] = 0.0; }
        for (uint32_t c0 = 0; c0 < directions; c0 += PD_BLOCK) {
            const uint32_t cnt = min((uint32_t)PD_BLOCK, directions - c0);
            if (lane < cnt) {
                const size_t e = base + c0 + lane;
                const float *r = rays + e * 6u + 3u;
                const uint32_t *h = hits + e * 12u;
                const double dx = (double)r[0], dy = (double)r[1], dz = (double)r[2];
                double dist = r_max;
                if (h[10] != 0xFFFFFFFFu) dist = fmin((double)__uint_as_float(h[0]) * sqrt((dx * dx + dy * dy) + dz * dz), r_max);
                double *s = st + lane * 4u;
                s[0] = dx; s[1] = dy; s[2] = dz; s[3] = dist;
            }
            __syncthreads();
            for (uint32_t j = 0; j < cnt; j++) {
                const double dx = st[j * 4u], dy = st[j * 4u + 1u], dz = st[j * 4u + 2u], dist = st[j * 4u + 3u];
#pragma unroll
                for (int q = 0; q < PD_MAXT; q++) {
                    if ((uint32_t)q < nq && lane + (uint32_t)q * PD_BLOCK < n_tex) {
                        double w = fmax(0.0, (T[q][0] * dx + T[q][1] * dy) + T[q][2] * dz);
                        for (uint32_t s = 0; s < k; s++) w = w * w;
                        const double wd = w * dist;
                        A[q] = A[q] + wd;
                        B[q] = B[q] + wd * dist;
                        W[q] = W[q] + w;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < PD_MAXT; q++) {
            const uint32_t t = lane + (uint32_t)q * PD_BLOCK;
            if (t < n_tex) {
                float *s = sums + ((size_t)p * n_tex + t) * 4u;                         // < 2^33 floats
                s[0] = s[0] + (float)A[q]; s[1] = s[1] + (float)B[q]; s[2] = s[2] + (float)W[q];
            }
        }
    }
}

// the constants of fw_probe_lookup.hip's LookupConst, restated
struct VisConst { double y0, c1, c2, c6, c8, a0, a1, a2; };

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.40282347e+38f; }   // false for NaN and +-inf

// (mu, mu2) of one probe's map `m` (R x R x 2 floats) along the unit direction (x, y, z): bilinear over the four texel centres, edges
// clamped
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

// fw_probe_lookup.hip's probe_lookup with the visibility weight of include/firework_hip.h: E[c] in float64 before its one rounding; false
// (and E untouched) for a point that the statement answers with zeros.
__device__ __forceinline__ bool probe_lookup_vis(const DProbeGrid &G, const DProbeVis &V, const VisConst &K, const float *__restrict__ sh,
                                                 float pxf, float pyf, float pzf, float nxf, float nyf, float nzf, double E[3]) {
    if (!(finite_f(pxf) && finite_f(pyf) && finite_f(pzf) && finite_f(nxf) && finite_f(nyf) && finite_f(nzf))) return false;
    const double p[3] = {(double)pxf, (double)pyf, (double)pzf};
    const double nx = (double)nxf, ny = (double)nyf, nz = (double)nzf;
    const double nl2 = (nx * nx + ny * ny) + nz * nz;
    if (!(nl2 > 0.0)) return false;
    const double nl = sqrt(nl2);
    const double x = nx / nl, y = ny / nl, z = nz / nl;
    const double q[3] = {p[0] + V.bias * x, p[1] + V.bias * y, p[2] + V.bias * z};

    // the cell
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
    const size_t map_floats = (size_t)V.R * V.R * 2u;

    // the corner weights, corner d = 4 dz + 2 dy + dx
    double w[8];
    double wsum = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        w[d] = 0.0;
        if ((dx == 0 || two[0]) && (dy == 0 || two[1]) && (dz == 0 || two[2])) {
            const double wx = dx ? f[0] : 1.0 - f[0], wy = dy ? f[1] : 1.0 - f[1], wz = dz ? f[2] : 1.0 - f[2];
            const int dd[3] = {dx, dy, dz};
            double P[3];
#pragma unroll
            for (int k = 0; k < 3; k++) P[k] = two[k] ? G.lo[k] + (double)(i[k] + (uint32_t)dd[k]) * G.step[k] : G.mid[k];
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
            // the visibility of this probe from the biased point
            const double rv[3] = {q[0] - P[0], q[1] - P[1], q[2] - P[2]};
            const double dist = sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2]);
            double v = 1.0;
            if (dist != 0.0) {
                const uint32_t probe = ((i[2] + (uint32_t)dz) * G.counts[1] + (i[1] + (uint32_t)dy)) * G.counts[0] + (i[0] + (uint32_t)dx);
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
            const double wd = ((wx * wy) * wz) * g;
            wsum = wsum + wd;
            w[d] = wd;
        }
    }

    const double B[9] = {K.a0 * K.y0,           K.a1 * (K.c1 * y),       K.a1 * (K.c1 * z),
                         K.a1 * (K.c1 * x),     K.a2 * ((K.c2 * x) * y), K.a2 * ((K.c2 * y) * z),
                         K.a2 * (K.c6 * (3.0 * (z * z) - 1.0)), K.a2 * ((K.c2 * x) * z), K.a2 * (K.c8 * (x * x - y * y))};
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        if ((dx == 0 || two[0]) && (dy == 0 || two[1]) && (dz == 0 || two[2])) {
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

__global__ __launch_bounds__(PV_BLOCK) void k_probe_irradiance_vis(DProbeGrid G, DProbeVis V, VisConst K, const float *__restrict__ sh, uint32_t n,
                                                                   const float *__restrict__ positions, const float *__restrict__ normals,
                                                                   uint32_t stride, float *__restrict__ out) {
    const uint32_t q = blockIdx.x * PV_BLOCK + threadIdx.x;                           // one point per lane: the grid covers n
    if (q < n) {
        const float *pp = positions + (size_t)q * stride, *nn = normals + (size_t)q * stride;
        double E[3];
        float r = 0.f, g = 0.f, b = 0.f;
        if (probe_lookup_vis(G, V, K, sh, pp[0], pp[1], pp[2], nn[0], nn[1], nn[2], E)) { r = (float)E[0]; g = (float)E[1]; b = (float)E[2]; }
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

__global__ __launch_bounds__(PV_BLOCK) void k_probe_shade_vis(DProbeGrid G, DProbeVis V, VisConst K, const float *__restrict__ sh, uint32_t n,
                                                              const float4 *__restrict__ aov, float gamma, uint8_t *rgb8, float *gamma_rgb,
                                                              float *linear_rgb) {
    const float inv_pi = (float)(1.0 / 3.141592653589793);
    const uint32_t p = blockIdx.x * PV_BLOCK + threadIdx.x;                           // one pixel per lane: the grid covers n
    if (p < n) {
        const float4 a = aov[3 * (size_t)p], nd = aov[3 * (size_t)p + 1], xa = aov[3 * (size_t)p + 2];
        double E[3];
        float er = 0.f, eg = 0.f, eb = 0.f;
        if (probe_lookup_vis(G, V, K, sh, xa.x, xa.y, xa.z, nd.x, nd.y, nd.z, E)) { er = (float)E[0]; eg = (float)E[1]; eb = (float)E[2]; }
        er = er > 0.f ? er : 0.f; eg = eg > 0.f ? eg : 0.f; eb = eb > 0.f ? eb : 0.f;
        const float v = a.w, rest = 1.f - v;
        resolve_pixel(a.x * (v * (er * inv_pi) + rest), a.y * (v * (eg * inv_pi) + rest), a.z * (v * (eb * inv_pi) + rest), 1.0f, gamma, p, rgb8,
                      gamma_rgb, linear_rgb);
    }
}

VisConst vis_const() {
    const double PI = 3.141592653589793;
    return VisConst{0.5 * std::sqrt(1.0 / PI), std::sqrt(3.0 / (4.0 * PI)), 0.5 * std::sqrt(15.0 / PI), 0.25 * std::sqrt(5.0 / PI),
                    0.25 * std::sqrt(15.0 / PI), PI, 2.0 * PI / 3.0, PI / 4.0};
}
uint32_t vis_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + PV_BLOCK - 1) / PV_BLOCK); }        // n > 0; at most 2^24 blocks

} // namespace

void launch_probe_depth(hipStream_t stream, uint32_t n, uint32_t directions, uint32_t R, uint32_t sharpness_log2, float max_distance,
                        const float *rays, const void *hits, float *sums) {
    hipLaunchKernelGGL(k_probe_depth, dim3(n), dim3(PD_BLOCK), 0, stream, n, directions, R, sharpness_log2, (double)max_distance, rays,
                       (const uint32_t *)hits, sums);                                   // n < 2^27: one workgroup per probe
}

void launch_probe_irradiance_vis(hipStream_t stream, const DProbeGrid &g, const DProbeVis &v, const float *sh, uint32_t n, const float *positions,
                                 const float *normals, uint32_t stride_floats, float *irradiance) {
    hipLaunchKernelGGL(k_probe_irradiance_vis, dim3(vis_blocks(n)), dim3(PV_BLOCK), 0, stream, g, v, vis_const(), sh, n, positions, normals,
                       stride_floats, irradiance);
}

void launch_probe_shade_vis(hipStream_t stream, const DProbeGrid &g, const DProbeVis &v, const float *sh, uint32_t n, const float *aov, float gamma,
                            uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    hipLaunchKernelGGL(k_probe_shade_vis, dim3(vis_blocks(n)), dim3(PV_BLOCK), 0, stream, g, v, vis_const(), sh, n, (const float4 *)aov, gamma,
                       rgb8, gamma_rgb, linear_rgb);
}

} // namespace fw
