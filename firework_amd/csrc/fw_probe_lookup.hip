// fw_probe_lookup.hip — the two kernels that read a baked probe grid back, for gfx950 (include/firework_hip.h has the statement,
// DESIGN.md §9q the design).
//
//   k_probe_irradiance   one lane per point: 12 B of position and 12 B of normal at the caller's stride, the cell and the (up to) eight
//                        corner weights in float64, then corner by corner the nine (r, g, b) triples of that probe (108 B, 4-byte
//                        aligned; hipcc merges them into six 16-byte loads and one of 12 B) folded with B_k = A_k Y_k(n) into three
//                        float64 sums; writes 12 B.
//   k_probe_shade        one lane per pixel: fw_render_aovs' 48-byte record as three 16-byte loads, the same lookup at (position, normal),
//                        then out = albedo (coverage E / pi + (1 - coverage)) in float32 and resolve_pixel's three outputs.
//
// Both share probe_lookup() below.  Corner-major: beside the nine B_k a lane holds eight weights and three sums, never the 27
// interpolated coefficients.  Neighbouring points share a cell, so a wave's 8 x 108 B of coefficients are a few cache lines.  No LDS,
// no atomics, no barrier, no inline assembly: every output is one lane's, a pure function of the inputs.  Every probe index is formed
// from a cell index clamped to [0, counts - 2] plus 0 or 1, so no load leaves sh whatever the point is.
//
// A file of its own, after the others on the link line: the code objects of fw_kernels.hip, fw_build.hip, fw_temporal.hip,
// fw_camera_models.hip, fw_probes.hip and fw_lightmap.hip stay byte for byte what they were.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.probe_lookup; floor, min and max are exact; sqrt is
// the device library's float64 function.  The float32 tail of the shade step is fw_kernels.hip's resolve_pixel restated (the same bits).
#include "fw_probe_lookup.h"
#include "fw_libm.h"
#include <algorithm>
#include <cmath>

namespace fw {
namespace {

constexpr int PL_BLOCK = 256;

// the constants of the real orthonormal SH basis up to l = 2 (fw_probes.hip's) and the cosine lobe's band factors, formed in double on
// the host
struct LookupConst { double y0, c1, c2, c6, c8, a0, a1, a2; };

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.40282347e+38f; }   // false for NaN and +-inf

// The lookup of include/firework_hip.h at one point: E[c] in float64 before its one rounding; false (and E untouched) for a point that
// the statement answers with zeros.
__device__ __forceinline__ bool probe_lookup(const DProbeGrid &G, const LookupConst &K, const float *__restrict__ sh, float pxf, float pyf,
                                             float pzf, float nxf, float nyf, float nzf, double E[3]) {
    if (!(finite_f(pxf) && finite_f(pyf) && finite_f(pzf) && finite_f(nxf) && finite_f(nyf) && finite_f(nzf))) return false;
    const double p[3] = {(double)pxf, (double)pyf, (double)pzf};
    const double nx = (double)nxf, ny = (double)nyf, nz = (double)nzf;
    const double nl2 = (nx * nx + ny * ny) + nz * nz;
    if (!(nl2 > 0.0)) return false;
    const double nl = sqrt(nl2);
    const double x = nx / nl, y = ny / nl, z = nz / nl;

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

    // the corner weights, corner d = 4 dz + 2 dy + dx
    double w[8];
    double wsum = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        w[d] = 0.0;
        if ((dx == 0 || two[0]) && (dy == 0 || two[1]) && (dz == 0 || two[2])) {
            const double wx = dx ? f[0] : 1.0 - f[0], wy = dy ? f[1] : 1.0 - f[1], wz = dz ? f[2] : 1.0 - f[2];
            double wd = (wx * wy) * wz;
            if (G.wrap) {
                const int dd[3] = {dx, dy, dz};
                double r[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double pk = two[k] ? G.lo[k] + (double)(i[k] + (uint32_t)dd[k]) * G.step[k] : G.mid[k];
                    r[k] = pk - p[k];
                }
                const double rl2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                double fac = 1.2;
                if (rl2 > 0.0) {
                    const double rl = sqrt(rl2);
                    const double dot = (x * (r[0] / rl) + y * (r[1] / rl)) + z * (r[2] / rl);
                    const double h = 0.5 * (dot + 1.0);
                    fac = h * h + 0.2;
                }
                wd = wd * fac;
                wsum = wsum + wd;
            }
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
            const double wd = G.wrap ? w[d] / wsum : w[d];
            e0 = e0 + wd * c0; e1 = e1 + wd * c1; e2 = e2 + wd * c2;
        }
    }
    E[0] = e0; E[1] = e1; E[2] = e2;
    return true;
}

__global__ __launch_bounds__(PL_BLOCK) void k_probe_irradiance(DProbeGrid G, LookupConst K, const float *__restrict__ sh, uint32_t n,
                                                               const float *__restrict__ positions, const float *__restrict__ normals,
                                                               uint32_t stride, float *__restrict__ out) {
    const uint32_t q = blockIdx.x * PL_BLOCK + threadIdx.x;                           // one point per lane: the grid covers n
    if (q < n) {
        const float *pp = positions + (size_t)q * stride, *nn = normals + (size_t)q * stride;
        double E[3];
        float r = 0.f, g = 0.f, b = 0.f;
        if (probe_lookup(G, K, sh, pp[0], pp[1], pp[2], nn[0], nn[1], nn[2], E)) { r = (float)E[0]; g = (float)E[1]; b = (float)E[2]; }
        float *o = out + (size_t)q * 3u;
        o[0] = r; o[1] = g; o[2] = b;
    }
}

// fw_kernels.hip's fdiv (see there for why), as fw_temporal.hip restates it, and its resolve_pixel: the same bits
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

__global__ __launch_bounds__(PL_BLOCK) void k_probe_shade(DProbeGrid G, LookupConst K, const float *__restrict__ sh, uint32_t n,
                                                          const float4 *__restrict__ aov, float gamma, uint8_t *rgb8, float *gamma_rgb,
                                                          float *linear_rgb) {
    const float inv_pi = (float)(1.0 / 3.141592653589793);
    const uint32_t p = blockIdx.x * PL_BLOCK + threadIdx.x;                           // one pixel per lane: the grid covers n
    if (p < n) {
        const float4 a = aov[3 * (size_t)p], nd = aov[3 * (size_t)p + 1], xa = aov[3 * (size_t)p + 2];
        double E[3];
        float er = 0.f, eg = 0.f, eb = 0.f;
        if (probe_lookup(G, K, sh, xa.x, xa.y, xa.z, nd.x, nd.y, nd.z, E)) { er = (float)E[0]; eg = (float)E[1]; eb = (float)E[2]; }
        er = er > 0.f ? er : 0.f; eg = eg > 0.f ? eg : 0.f; eb = eb > 0.f ? eb : 0.f;
        const float v = a.w, rest = 1.f - v;
        resolve_pixel(a.x * (v * (er * inv_pi) + rest), a.y * (v * (eg * inv_pi) + rest), a.z * (v * (eb * inv_pi) + rest), 1.0f, gamma, p, rgb8,
                      gamma_rgb, linear_rgb);
    }
}

LookupConst lookup_const() {
    const double PI = 3.141592653589793;
    return LookupConst{0.5 * std::sqrt(1.0 / PI), std::sqrt(3.0 / (4.0 * PI)), 0.5 * std::sqrt(15.0 / PI), 0.25 * std::sqrt(5.0 / PI),
                       0.25 * std::sqrt(15.0 / PI), PI, 2.0 * PI / 3.0, PI / 4.0};
}
uint32_t lookup_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + PL_BLOCK - 1) / PL_BLOCK); }      // n > 0; at most 2^24 blocks

} // namespace

void launch_probe_irradiance(hipStream_t stream, const DProbeGrid &g, const float *sh, uint32_t n, const float *positions,
                             const float *normals, uint32_t stride_floats, float *irradiance) {
    hipLaunchKernelGGL(k_probe_irradiance, dim3(lookup_blocks(n)), dim3(PL_BLOCK), 0, stream, g, lookup_const(), sh, n, positions, normals,
                       stride_floats, irradiance);
}

void launch_probe_shade(hipStream_t stream, const DProbeGrid &g, const float *sh, uint32_t n, const float *aov, float gamma,
                        uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    hipLaunchKernelGGL(k_probe_shade, dim3(lookup_blocks(n)), dim3(PL_BLOCK), 0, stream, g, lookup_const(), sh, n, (const float4 *)aov, gamma,
                       rgb8, gamma_rgb, linear_rgb);
}

} // namespace fw
