// fw_probe_radiance_fetch.h — the device side of the radiance lookup (include/firework_hip.h, "Lookup" under the probe radiance maps;
// DESIGN.md §9v), one copy for the files that read radiance maps: fw_probe_radiance.hip (k_probe_radiance_lookup, k_probe_shade_glossy)
// and fw_ggx_table.hip (k_probe_split_shade), and the pixel of those two shades, shade_glossy_pixel, stated once over its specular term.
// Internal linkage, as everything in fw_shared.h and fw_probe_corners.h.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.probe_radiance_lookup: do not reassociate.
#pragma once
#include "fw_probe_radiance.h"
#include "fw_probe_corners.h"

namespace fw {
namespace {

// the rgb of one level (R x R texels of 16 B at `m`) along the unit direction (x, y, z): bilinear, edges clamped; the flags are not read
__device__ __forceinline__ void radiance_fetch(const float4 *__restrict__ m, uint32_t R, double x, double y, double z, double c[3]) {
    uint32_t iu, jv;
    double fu, fv;
    octa_cell(R, x, y, z, iu, jv, fu, fv);
    const float4 *__restrict__ r0 = m + (size_t)(jv * R + iu);
    const float4 *__restrict__ r1 = r0 + R;
    const float4 t00 = r0[0], t10 = r0[1], t01 = r1[0], t11 = r1[1];
    const double gu = 1.0 - fu, gv = 1.0 - fv;
    c[0] = (((double)t00.x * gu + (double)t10.x * fu) * gv) + (((double)t01.x * gu + (double)t11.x * fu) * fv);
    c[1] = (((double)t00.y * gu + (double)t10.y * fu) * gv) + (((double)t01.y * gu + (double)t11.y * fu) * fv);
    c[2] = (((double)t00.z * gu + (double)t10.z * fu) * gv) + (((double)t01.z * gu + (double)t11.z * fu) * fv);
}

// the radiance sum over those corners along (dx, dy, dz), which need not be a unit vector, at roughness `rough`: E[c] in float64 before
// its one rounding; false for a direction or a roughness the statement answers with zeros
__device__ __forceinline__ bool corners_radiance(const DProbeGrid &G, const Corners &C, const DProbeRadiance &pr, const float4 *__restrict__ maps, double dx, double dy,
                                                 double dz, double rough, double E[3]) {
    const double dl2 = (dx * dx + dy * dy) + dz * dz;
    if (!(dl2 > 0.0) || !(dl2 <= 1.79769313486231570e+308) || !(fabs(rough) <= 1.79769313486231570e+308)) return false;
    const double dl = sqrt(dl2);
    const double rx = dx / dl, ry = dy / dl, rz = dz / dl;
    // the level pair and the blend
    const uint32_t L = pr.levels;
    const double top = L == 1u ? pr.rho[0] : (L == 2u ? pr.rho[1] : (L == 3u ? pr.rho[2] : pr.rho[3]));
    const double rho = fmin(fmax(rough, pr.rho[0]), top);
    uint32_t l = 0u;
    double lo = pr.rho[0], hi = pr.rho[1];
    if (L > 2u && pr.rho[1] <= rho) { l = 1u; lo = pr.rho[1]; hi = pr.rho[2]; }
    if (L > 3u && pr.rho[2] <= rho) { l = 2u; lo = pr.rho[2]; hi = pr.rho[3]; }
    const bool pair = L > 1u;
    const double t = pair ? (rho - lo) / (hi - lo) : 0.0;
    const double t1 = 1.0 - t;
    const uint32_t R = pr.R;
    const uint32_t off0 = l == 0u ? 0u : (l == 1u ? R * R : R * R + (R >> 1) * (R >> 1));
    const uint32_t Rl = R >> l, Rn = Rl >> 1;
    const uint32_t off1 = off0 + Rl * Rl;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        if (C.active & (1u << d)) {
            const float4 *__restrict__ m = maps + (size_t)corner_probe(G, C.cell, d) * pr.texels;      // n_probes x M < 2^31 texels
            double c[3];
            radiance_fetch(m + off0, Rl, rx, ry, rz, c);
            if (pair) {
                double n[3];
                radiance_fetch(m + off1, Rn, rx, ry, rz, n);
                c[0] = c[0] * t1 + n[0] * t; c[1] = c[1] * t1 + n[1] * t; c[2] = c[2] * t1 + n[2] * t;
            }
            const double wd = C.w[d] / C.wsum;
            e0 = e0 + wd * c[0]; e1 = e1 + wd * c[1]; e2 = e2 + wd * c[2];
        }
    }
    E[0] = e0; E[1] = e1; E[2] = e2;
    return true;
}

// One pixel p of the glossy probe shades (k_probe_shade_glossy, k_probe_split_shade): fw_probe_shade_placed's arithmetic where the
// pixel's roughness is not > 0; elsewhere v (s Ls) + (1 - v) albedo, with Ls the radiance of the maps along the mirrored view direction,
// clamped at zero, and s the specular term that the caller supplies: term(cos, sp, s0, s1, s2) gets the cosine between the normal and
// the direction to the eye, clamped to [0, 1], as a double, and the pixel's spec record (F0.rgb, rho).  Where the view or the normal is
// unusable Ls is zero and the term is asked at Term::UNSEEN.
template <bool DEPTH, class Term>
__device__ __forceinline__ void shade_glossy_pixel(const DProbeGrid &G, const DProbeVis &V, const DProbeRadiance &pr, const ShLookupConst &K,
                                                   const float *__restrict__ sh, const float4 *__restrict__ maps, const float *__restrict__ placement,
                                                   uint32_t p, const float4 *__restrict__ aov, const float4 *__restrict__ spec,
                                                   const float *__restrict__ view, uint32_t view_stride, float gamma, uint8_t *rgb8, float *gamma_rgb,
                                                   float *linear_rgb, const Term &term) {
    const float4 a = aov[3 * (size_t)p], nd = aov[3 * (size_t)p + 1], xa = aov[3 * (size_t)p + 2];
    const float4 sp = spec[p];
    Corners C;
    const bool ok = corner_weights<true, DEPTH>(G, V, placement, xa.x, xa.y, xa.z, nd.x, nd.y, nd.z, C);
    const float v = a.w, rest = 1.f - v;
    if (!(sp.w > 0.f)) {                                                               // diffuse: fw_probe_shade_placed's arithmetic
        shade_diffuse(G, C, ok, K, sh, a, gamma, p, rgb8, gamma_rgb, linear_rgb);
        return;
    }
    const float *vw = view + (size_t)p * view_stride;
    const float vxf = vw[0], vyf = vw[1], vzf = vw[2];
    float l0 = 0.f, l1 = 0.f, l2 = 0.f;
    double cost = Term::UNSEEN;
    if (finite_f(vxf) && finite_f(vyf) && finite_f(vzf)) {
        const double vx = (double)vxf, vy = (double)vyf, vz = (double)vzf;
        const double vl2 = (vx * vx + vy * vy) + vz * vz;
        if (vl2 > 0.0 && C.usable) {
            const double vl = sqrt(vl2);
            const double ux = vx / vl, uy = vy / vl, uz = vz / vl;
            const double c = (C.x * ux + C.y * uy) + C.z * uz;
            const double c2 = 2.0 * c;
            const float rx = (float)(ux - c2 * C.x), ry = (float)(uy - c2 * C.y), rz = (float)(uz - c2 * C.z);
            cost = fmin(1.0, fmax(0.0, -c));
            double E[3];
            if (ok && finite_f(sp.w) && corners_radiance(G, C, pr, maps, (double)rx, (double)ry, (double)rz, (double)sp.w, E)) {
                l0 = (float)E[0]; l1 = (float)E[1]; l2 = (float)E[2];
            }
        }
    }
    l0 = fmaxf(l0, 0.f); l1 = fmaxf(l1, 0.f); l2 = fmaxf(l2, 0.f);
    float s0, s1, s2;
    term(cost, sp, s0, s1, s2);
    resolve_pixel(v * (s0 * l0) + rest * a.x, v * (s1 * l1) + rest * a.y, v * (s2 * l2) + rest * a.z, 1.0f, gamma, p, rgb8, gamma_rgb, linear_rgb);
}

} // namespace
} // namespace fw
