// fw_shared.h — the small device helpers that the baker and probe kernel files share, one copy each: fw_probes.hip, fw_lightmap.hip,
// fw_ao.hip, fw_direct.hip, fw_camera_models.hip, fw_temporal.hip and the four probe files include it.  fw_kernels.hip and fw_build.hip
// do not: their fdiv and resolve_pixel have another shape (a shared reciprocal, a float4 pixel), which is why everything here has
// internal linkage and nothing of it is in fw_device.h.
//
// Numerics: -ffp-contract=off, so + - * / round as written; floor, min, max and fabs are exact; sqrt, sin and cos are the device
// library's float64 functions.  Every function is one statement of include/firework_hip.h, operation for operation: do not reassociate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include "fw_libm.h"

namespace fw {
namespace {

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.40282347e+38f; }   // false for NaN and +-inf
__device__ __forceinline__ double sgn1(double v) { return v >= 0.0 ? 1.0 : -1.0; }      // sgn(0) = +1

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
// the two shifts in [0, 1) that item `id` (2 id + 1 < 2^32) draws in round `round` of seed `seed32`
struct Jitter { double u, v; };
__device__ __forceinline__ Jitter jitter_pair(uint32_t seed32, uint32_t round, uint32_t id) {
    const uint32_t key = hash32(seed32 ^ hash32(round + 0x9E3779B9u));
    return Jitter{(double)(hash32(hash32(2u * id) ^ key) >> 8) * 0x1p-24, (double)(hash32(hash32(2u * id + 1u) ^ key) >> 8) * 0x1p-24};
}

// Direction j of Dd cosine-weighted Fibonacci directions, shifted by (xi_u, xi_v), in the frame of Duff et al. 2017 around the float32 normal
// (fx, fy, fz) made unit again in float64 (the frame is then orthonormal to float64 and d unit to one float32 rounding).  n: that unit
// normal and rl2 its squared length before, d: the direction before its rounding.
struct CosineDir { double nx, ny, nz, dx, dy, dz, rl2; };
__device__ __forceinline__ CosineDir cosine_dir(uint32_t j, double Dd, double xi_u, double xi_v, float fx, float fy, float fz) {
    const double PI = 3.141592653589793, G = 0.6180339887498949;                        // G = (sqrt(5) - 1) / 2
    const double u = ((double)j + xi_u) / Dd;
    const double r = sqrt(u);
    const double cz = sqrt(fmax(0.0, 1.0 - u));
    const double t = (double)j * G + xi_v;
    const double phi = (2.0 * PI) * (t - floor(t));
    const double lx = r * cos(phi), ly = r * sin(phi);
    const double rx = (double)fx, ry = (double)fy, rz = (double)fz;
    const double rl2 = (rx * rx + ry * ry) + rz * rz;
    const double rl = sqrt(rl2);
    const double nx = rx / rl, ny = ry / rl, nz = rz / rl;
    const double s = copysign(1.0, nz);
    const double a = -1.0 / (s + nz);
    const double b = (nx * ny) * a;
    const double tx = 1.0 + (s * (nx * nx)) * a, ty = s * b, tz = -s * nx;
    const double bx = b, by = s + (ny * ny) * a, bz = -ny;
    return CosineDir{nx, ny, nz, (lx * tx + ly * bx) + cz * nx, (lx * ty + ly * by) + cz * ny, (lx * tz + ly * bz) + cz * nz, rl2};
}

// texel t = b R + a of an R x R octahedral map: its centre on the octahedron (x, y, z) and that point's length
__device__ __forceinline__ double texel_point(uint32_t t, uint32_t R, double &x, double &y, double &z) {
    const uint32_t b = t / R, a = t - b * R;
    const double Rd = (double)R;
    const double ex = (((double)a + 0.5) * 2.0) / Rd - 1.0, ey = (((double)b + 0.5) * 2.0) / Rd - 1.0;
    z = (1.0 - fabs(ex)) - fabs(ey);
    x = ex; y = ey;
    if (z < 0.0) { x = (1.0 - fabs(ey)) * sgn1(ex); y = (1.0 - fabs(ex)) * sgn1(ey); }
    return sqrt((x * x + y * y) + z * z);
}
// the unit direction of that texel
__device__ __forceinline__ void texel_dir(uint32_t t, uint32_t R, double T[3]) {
    double x, y, z;
    const double l = texel_point(t, R, x, y, z);
    T[0] = x / l; T[1] = y / l; T[2] = z / l;
}

// where a unit direction falls in an R x R octahedral map: the first texel (column iu, row jv, both in [0, R - 2] whatever the
// direction is) of the four that a bilinear fetch reads, and the fractions
__device__ __forceinline__ void octa_cell(uint32_t R, double x, double y, double z, uint32_t &iu, uint32_t &jv, double &fu, double &fv) {
    const double s1 = (fabs(x) + fabs(y)) + fabs(z);
    double ox = x / s1, oy = y / s1;
    if (z < 0.0) {
        const double fx = (1.0 - fabs(oy)) * sgn1(ox), fy = (1.0 - fabs(ox)) * sgn1(oy);
        ox = fx; oy = fy;
    }
    const double Rd = (double)R, top = Rd - 1.0;
    const double su = fmin(fmax(((ox + 1.0) * 0.5) * Rd - 0.5, 0.0), top), sv = fmin(fmax(((oy + 1.0) * 0.5) * Rd - 0.5, 0.0), top);
    const double i = fmin(floor(su), top - 1.0), j = fmin(floor(sv), top - 1.0);         // fmin and fmax drop a NaN: still in [0, R - 2]
    fu = su - i; fv = sv - j;
    iu = (uint32_t)i; jv = (uint32_t)j;
}

// (mu, mu2) of one probe's depth map `m` (R x R x 2 floats) along the unit direction (x, y, z): bilinear over the four texel centres,
// edges clamped
__device__ __forceinline__ void depth_fetch(const float *__restrict__ m, uint32_t R, double x, double y, double z, double &mu, double &mu2) {
    uint32_t iu, jv;
    double fu, fv;
    octa_cell(R, x, y, z, iu, jv, fu, fv);
    const float *__restrict__ r0 = m + ((size_t)(jv * R + iu)) * 2u;
    const float *__restrict__ r1 = r0 + (size_t)R * 2u;
    const double gu = 1.0 - fu, gv = 1.0 - fv;
    mu = (((double)r0[0] * gu + (double)r0[2] * fu) * gv) + (((double)r1[0] * gu + (double)r1[2] * fu) * fv);
    mu2 = (((double)r0[1] * gu + (double)r0[3] * fu) * gv) + (((double)r1[1] * gu + (double)r1[3] * fu) * fv);
}

// The float32 tail of the shades.  fdiv is fw_kernels.hip's (see there for why) with the reciprocal formed in place: the compiler's
// Newton chain without the scaling steps, v_div_fixup for the IEEE special cases; resolve_pixel is fw_kernels.hip's over three floats.
// The bits are the same.
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

// the constants of the real orthonormal SH basis up to l = 2 (fw_probes.hip's) and the cosine lobe's band factors, formed in double on
// the host
struct ShLookupConst { double y0, c1, c2, c6, c8, a0, a1, a2; };
inline ShLookupConst sh_lookup_const() {
    const double PI = 3.141592653589793;
    return ShLookupConst{0.5 * std::sqrt(1.0 / PI), std::sqrt(3.0 / (4.0 * PI)), 0.5 * std::sqrt(15.0 / PI), 0.25 * std::sqrt(5.0 / PI),
                         0.25 * std::sqrt(15.0 / PI), PI, 2.0 * PI / 3.0, PI / 4.0};
}

// blocks for `items` at `per_block` each, at most per_cu per compute unit and at least one
inline uint32_t grid_for(uint64_t items, uint32_t per_block, int n_cus, uint32_t per_cu) {
    const uint64_t want = (items + per_block - 1u) / per_block;
    return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(want, (uint64_t)std::max(1, n_cus) * per_cu));
}

} // namespace
} // namespace fw
