// fw_probe_corners.h — the probe-grid lookup of include/firework_hip.h on the device, stated once.  fw_probe_lookup.hip
// (the irradiance and shade kernels in all their forms) and fw_probe_radiance.hip (the radiance lookup and the glossy shade) include it.
//
//   corner_weights<PLACED, DEPTH>   the point checks and the unit normal, the cell, and corner by corner the probe index, the placement
//                                   record and its skip, the trilinear weight, the wrap factor, the visibility weight and the sum
//   corners_sh                      the SH sum over the active corners
//   shade_diffuse                   the float32 tail of the diffuse probe shades
//
// The forms of the statement differ in three places only:
//   placement       PLACED reads a probe's record where `placement` is given (NULL: every probe active where it stands), adds the offset
//                   to the probe's position and skips a corner whose a == 0.  !PLACED compiles neither the loads nor the additions.
//   normalisation   the plain form (!PLACED, !DEPTH) divides by the weight sum only under wrap: without it the trilinear weights are
//                   used as they are and no sum is formed.  Every other form always divides (Corners::norm).
//   zero sum        PLACED answers a zero weight sum with zeros.  The plain and visibility forms have no such exit: every corner of the
//                   cell takes part, the trilinear weights are >= 0 with one of them >= 1/8, the wrap factor is >= 0.2 and the crushed
//                   visibility factor >= 25e-18, so for finite input the sum is > 0; a NaN sum (a NaN in the depth maps) goes through the
//                   division in every form, as `wsum == 0.0` is false for it.
//
// Everything is float64 under -ffp-contract=off: + - * / round as written and in the order of api.probe_lookup / _vis / _placed; floor,
// min, max and fabs are exact; sqrt is the device library's float64 function.  Every probe index is formed from a cell index clamped to
// [0, counts - 2] plus 0 or 1, so no load leaves sh, placement or the maps whatever the point is.
#pragma once
#include "fw_probe_lookup.h"
#include "fw_shared.h"

namespace fw {
namespace {

// what a lookup keeps of its point: the unit normal, the cell, the weights of the cell's active corners and their sum
struct Corners {
    double x, y, z;             // the unit normal
    double w[8], wsum;
    uint32_t cell[3], active;   // corner d = 4 dz + 2 dy + dx is probe corner_probe(G, cell, d); bit d of active: it takes part
    bool usable;                // the position and the normal are finite and the normal is not zero
    bool norm;                  // the weights are divided by wsum
};

// the probe at corner d of the cell `i`: below n_probes < 2^31, as i[k] <= counts[k] - 2 on an axis with two corners and 0 on a flat one
__device__ __forceinline__ uint32_t corner_probe(const DProbeGrid &G, const uint32_t i[3], int d) {
    const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
    return ((i[2] + (uint32_t)dz) * G.counts[1] + (i[1] + (uint32_t)dy)) * G.counts[0] + (i[0] + (uint32_t)dx);
}

// false for a point that the statement answers with zeros: one that is not usable, or (PLACED) one whose weights sum to zero
template <bool PLACED, bool DEPTH>
__device__ __forceinline__ bool corner_weights(const DProbeGrid &G, const DProbeVis &V, const float *__restrict__ placement, float pxf, float pyf,
                                               float pzf, float nxf, float nyf, float nzf, Corners &C) {
    C.usable = false;
    if (!(finite_f(pxf) && finite_f(pyf) && finite_f(pzf) && finite_f(nxf) && finite_f(nyf) && finite_f(nzf))) return false;
    const double p[3] = {(double)pxf, (double)pyf, (double)pzf};
    const double nx = (double)nxf, ny = (double)nyf, nz = (double)nzf;
    const double nl2 = (nx * nx + ny * ny) + nz * nz;
    if (!(nl2 > 0.0)) return false;
    const double nl = sqrt(nl2);
    const double x = nx / nl, y = ny / nl, z = nz / nl;
    C.x = x; C.y = y; C.z = z;
    C.usable = true;
    C.norm = PLACED || DEPTH || G.wrap;
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
    C.cell[0] = i[0]; C.cell[1] = i[1]; C.cell[2] = i[2];
    const bool two[3] = {G.counts[0] > 1u, G.counts[1] > 1u, G.counts[2] > 1u};      // wave-uniform: a flat axis has one corner
    const size_t map_floats = DEPTH ? (size_t)V.R * V.R * 2u : 0u;

    // the corner weights, corner d = 4 dz + 2 dy + dx
    uint32_t active = 0u;
    double wsum = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        C.w[d] = 0.0;
        if ((dx == 0 || two[0]) && (dy == 0 || two[1]) && (dz == 0 || two[2])) {
            const uint32_t probe = corner_probe(G, i, d);
            // this probe's record, if there is one.  Its offset is read where it is added, not here: kept in registers across the
            // weights it costs the placed kernels a wave per SIMD
            const float *__restrict__ pl = (PLACED && placement) ? placement + (size_t)probe * 4u : nullptr;
            if (pl && pl[3] == 0.f) continue;                                          // inactive: nothing else of this probe is read
            active |= 1u << d;
            const double wx = dx ? f[0] : 1.0 - f[0], wy = dy ? f[1] : 1.0 - f[1], wz = dz ? f[2] : 1.0 - f[2];
            double wd = (wx * wy) * wz;
            if (DEPTH || G.wrap) {
                const int dd[3] = {dx, dy, dz};
                double off[3] = {0.0, 0.0, 0.0};
                if (pl) { off[0] = (double)pl[0]; off[1] = (double)pl[1]; off[2] = (double)pl[2]; }
                double P[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    P[k] = two[k] ? G.lo[k] + (double)(i[k] + (uint32_t)dd[k]) * G.step[k] : G.mid[k];
                    if (PLACED) P[k] = P[k] + off[k];
                }
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
                } else {
                    wd = wd * fac;
                }
            }
            if (PLACED || DEPTH || G.wrap) wsum = wsum + wd;
            C.w[d] = wd;
        }
    }
    C.active = active;
    C.wsum = wsum;
    return !(PLACED && wsum == 0.0);                                                   // PLACED: no active corner, or none with a weight
}

// the SH sum of the statement over those corners: E[c] in float64 before its one rounding
__device__ __forceinline__ void corners_sh(const DProbeGrid &G, const Corners &C, const ShLookupConst &K, const float *__restrict__ sh, double E[3]) {
    const double x = C.x, y = C.y, z = C.z;
    const double B[9] = {K.a0 * K.y0,           K.a1 * (K.c1 * y),       K.a1 * (K.c1 * z),
                         K.a1 * (K.c1 * x),     K.a2 * ((K.c2 * x) * y), K.a2 * ((K.c2 * y) * z),
                         K.a2 * (K.c6 * (3.0 * (z * z) - 1.0)), K.a2 * ((K.c2 * x) * z), K.a2 * (K.c8 * (x * x - y * y))};
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        if (C.active & (1u << d)) {
            const float *__restrict__ s = sh + (size_t)corner_probe(G, C.cell, d) * 27u;
            double c0 = B[0] * (double)s[0], c1 = B[0] * (double)s[1], c2 = B[0] * (double)s[2];
#pragma unroll
            for (int k = 1; k < 9; k++) {
                c0 = c0 + B[k] * (double)s[3 * k];
                c1 = c1 + B[k] * (double)s[3 * k + 1];
                c2 = c2 + B[k] * (double)s[3 * k + 2];
            }
            const double wd = C.norm ? C.w[d] / C.wsum : C.w[d];
            e0 = e0 + wd * c0; e1 = e1 + wd * c1; e2 = e2 + wd * c2;
        }
    }
    E[0] = e0; E[1] = e1; E[2] = e2;
}

// the diffuse shade of pixel p: out = albedo (coverage E / pi + (1 - coverage)) in float32 from the aov record's first float4 `a` and the
// lookup's E (zeros where `ok` is false), then resolve_pixel's three outputs
__device__ __forceinline__ void shade_diffuse(const DProbeGrid &G, const Corners &C, bool ok, const ShLookupConst &K, const float *__restrict__ sh, float4 a, float gamma,
                                              uint32_t p, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    const float inv_pi = (float)(1.0 / 3.141592653589793);
    double E[3];
    float er = 0.f, eg = 0.f, eb = 0.f;
    if (ok) { corners_sh(G, C, K, sh, E); er = (float)E[0]; eg = (float)E[1]; eb = (float)E[2]; }
    er = er > 0.f ? er : 0.f; eg = eg > 0.f ? eg : 0.f; eb = eb > 0.f ? eb : 0.f;
    const float v = a.w, rest = 1.f - v;
    resolve_pixel(a.x * (v * (er * inv_pi) + rest), a.y * (v * (eg * inv_pi) + rest), a.z * (v * (eb * inv_pi) + rest), 1.0f, gamma, p, rgb8,
                  gamma_rgb, linear_rgb);
}

} // namespace
} // namespace fw
