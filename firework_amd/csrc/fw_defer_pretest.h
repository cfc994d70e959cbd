// fw_defer_pretest.h — the conservative slab pre-test of the box-list scan (k_extend_linear_defer), and the one it replaced.
//
// A deferred object is a plain Rect3d; the exact test (hit_rect3d in the object's frame) decides its hits, run from the object's list.
// The pre-test only picks the rays that go on the list: it must say "maybe" for every ray the exact test could accept with a t in
// (TMIN, best_t), and may say it for any other.  tools/defer_pretest_check.cpp proves that on the host, over 1e8+ rays, for both forms.
//
// The old form (pretest_sub, still what closest_hit's segment-0 cull does in line) moved each of the six planes by the margin
//     m = eps + mc,   mc = 1e-4 (max|lo| + max|hi|) + 1e-6   (wave-uniform: the box),   eps = 1e-4 (|o.x| + |o.y| + |o.z|)   (per ray)
// and computed t = ((plane -+ m) - o) * (1/d) with three approximate reciprocals of its own: 44 and 47 vector instructions per box.
//
// The new form (pretest_fma) keeps the geometry and moves the work:
//   host      the box as centre c and half extent h, h already grown by 1.01 mc and rounded outwards (make_cull_box): the kernel does no
//             arithmetic on wave-uniform values.
//   per ray   oi = o * inv (inv: the reciprocals the in-line rectangles already made), eps = 1.01e-4 |o|_1, and `odd` (below).
//   per axis  tc = fma(c, inv, -oi)                 the centre plane's distance: ONE fma, c from an SGPR
//             he = h + eps                          the per-ray margin, added to the half extent, not to each plane
//             near = fma(-he, |inv|, tc),  far = fma(he, |inv|, tc)      |inv| is a source modifier: near <= far with no min/max pair
//   per box   tn = max3(near), tf = min3(far);  reject iff  min(tf, best_t) < max(tn, 0) (1 - 1e-4) - 1e-4   and the ray is not odd
// 18 vector instructions per box and 9 per ray: 45 for two boxes, and no v_rcp_f32 (profiles/defer_pretest_isa.txt).
//
// Margin.  With exact arithmetic the form is the slab test of the box grown by 1.01 (mc + eps_old) on every side.  Rounding: oi, tc and
// near/far are each rounded once, he once, so a computed plane distance differs from the exact (plane - o) * inv by at most
//     |t_fma - t_exact| <= 2^-24 (|o inv| + |tc| + |near|) + 2^-24 he |inv| <= 3 * 2^-24 (|c| + |o| + he) |inv|,
// i.e. it is the exact distance of a plane displaced by at most 3 * 2^-24 (|c| + |o_axis| + he) = 1.8e-7 (...).  With S = max|lo| + max|hi|
// both |c| and h are <= S, so the displacement is below 1.8e-7 (2.0002 S + 1.0001 |o_axis|) + 2e-13, and the extra hundredth of the margin
// alone is 1e-6 (S + |o|_1) + 1e-8: more than twice that, at every coordinate scale (the bound is homogeneous: nothing in it depends on
// whether the box sits at 1 or at 3e4, the largest offset tests/coord_scenes.py uses, as long as nothing overflows — see `odd`; the
// additive 1e-6 only matters for boxes smaller than 1e-2, where it dominates).  So the new test admits every ray the slab test of the
// box grown by the OLD margin admits when evaluated exactly.  The reciprocal's own error (inv = (1/d)(1 + rho), |rho| <= 2^-22 after
// make_rcp's Newton step) scales every t of an axis alike; across axes it moves tn against tf by 2^-21 relative, which the 1e-4 relative
// slack of the comparison covers, as it did for the 1-ulp v_rcp_f32 of the old form.
//
// Odd rays.  Two things the slabs cannot decide, both for rays with a direction component that is 0, denormal, below 2^-40, infinite or
// NaN.  (1) The exact test ACCEPTS t = 0/0 — a ray in a face's plane with a zero direction component — whatever the other two
// coordinates say, so such a ray has to be listed even if another axis separates it from the box (the old form missed these).
// (2) fma(c, inv, -oi) is a difference of two products: with |inv| near 2^126 each overflows on its own and the difference is an
// infinity of the wrong sign or a NaN, where the old (plane - o) * inv gave a correctly signed infinity.  For these components inv is
// huge or a NaN (make_rcp's Newton step turns rcp's inf or 0 into one), so  odd = !(|inv.x| + |inv.y| + |inv.z| < 2^40)  — a sum, which
// keeps NaNs — lists the ray whatever the slabs say: two adds and a compare per ray, the OR is the scalar unit's.  Below the threshold
// no product overflows for coordinates up to 2^88, and the margin argument above holds.  One ray in 1e12 is odd by its direction alone.
//
// NaN elsewhere.  fminf / fmaxf (v_min / v_max / v_min3 / v_max3 in IEEE mode) return the operand that is not a NaN, whichever position it
// holds, so an axis whose near / far are NaN simply drops out of tn / tf: the test gets weaker, never stronger.  A NaN or infinite origin
// makes eps, he and every near / far a NaN: tn = tf = NaN, max(tn, 0) = 0 and min(tf, best_t) = best_t > 0: maybe.  A NaN best_t (rect.rs
// accepts t = 0/0, see hit_rect) drops out the same way.  The final comparison is written !(a < b), true for a NaN on either side.
//
// Compiles as plain C++ (host: the runtime's make_cull_box, the checker under tools/) and as HIP device code.  Only compiler builtins that
// exist on both sides; no device intrinsic.
#pragma once

#if defined(__HIPCC__)
#define FW_PT __host__ __device__ __forceinline__
#else
#define FW_PT static inline
#endif

namespace fwpt {

constexpr float MARGIN_REL = 1e-4f, MARGIN_ABS = 1e-6f;      // the old form's margin, kept by pretest_sub
constexpr float GROW = 1.01f;                                // the fma form's: that much more, which covers its own rounding (above)
constexpr float EPS_REL = 1.01e-4f;                          // GROW * MARGIN_REL, per ray
constexpr float T_REL = 1.f - 1e-4f, T_ABS = 1e-4f;          // slack of the comparison, both forms

FW_PT float max3abs(const float v[3]) { return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])), __builtin_fabsf(v[2])); }
// the constant part of the margin of the box [lo, hi]
FW_PT float box_margin(const float lo[3], const float hi[3]) { return MARGIN_REL * (max3abs(lo) + max3abs(hi)) + MARGIN_ABS; }

// ---- the old form: per-plane subtractions, approximate reciprocals ainv of its own, the margin rebuilt from lo / hi per ray ----
FW_PT bool pretest_sub(const float lo[3], const float hi[3], const float o[3], const float ainv[3], float best_t) {
    const float eps = MARGIN_REL * (__builtin_fabsf(o[0]) + __builtin_fabsf(o[1]) + __builtin_fabsf(o[2]));
    const float m = eps + MARGIN_REL * (max3abs(lo) + max3abs(hi)) + MARGIN_ABS;
    float t0 = (lo[0] - m - o[0]) * ainv[0], t1 = (hi[0] + m - o[0]) * ainv[0];
    float tn = __builtin_fminf(t0, t1), tf = __builtin_fmaxf(t0, t1);
    t0 = (lo[1] - m - o[1]) * ainv[1]; t1 = (hi[1] + m - o[1]) * ainv[1];
    tn = __builtin_fmaxf(tn, __builtin_fminf(t0, t1)); tf = __builtin_fminf(tf, __builtin_fmaxf(t0, t1));
    t0 = (lo[2] - m - o[2]) * ainv[2]; t1 = (hi[2] + m - o[2]) * ainv[2];
    tn = __builtin_fmaxf(tn, __builtin_fminf(t0, t1)); tf = __builtin_fminf(tf, __builtin_fmaxf(t0, t1));
    return !(tf < tn * T_REL - T_ABS) && !(tf < 0.f) && !(tn * T_REL - T_ABS > best_t);
}

// ---- the new form ----
struct CullBox { float c[3], h[3]; };       // centre and grown half extent: [c - h, c + h] encloses [lo - GROW mc, hi + GROW mc]
// host side (double arithmetic, rounded outwards); lo / hi in either order per axis
FW_PT CullBox make_cull_box(const float lo_in[3], const float hi_in[3]) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = __builtin_fminf(lo_in[a], hi_in[a]); hi[a] = __builtin_fmaxf(lo_in[a], hi_in[a]); }
    const double m = (double)GROW * (double)box_margin(lo, hi);
    CullBox b;
    for (int a = 0; a < 3; a++) {
        const double l = (double)lo[a] - m, u = (double)hi[a] + m;
        const float c = (float)(0.5 * (l + u));
        const double need = __builtin_fmax(u - (double)c, (double)c - l);      // what the rounded centre has to reach on either side
        float h = (float)need;
        if ((double)h < need) h = __builtin_nextafterf(h, __builtin_inff());
        b.c[a] = c; b.h[a] = h;
    }
    return b;
}

struct RayTerms { float inv[3], oi[3], eps; bool odd; };
constexpr float INV_MAX = 0x1p40f;
// inv: reciprocals of the direction's components, a relative error of 2^-22 allowed; NaN (or huge) for a component that is 0, denormal, inf or NaN
FW_PT RayTerms ray_terms(float ox, float oy, float oz, float ix, float iy, float iz) {
    RayTerms r;
    r.inv[0] = ix; r.inv[1] = iy; r.inv[2] = iz;
    r.oi[0] = ox * ix; r.oi[1] = oy * iy; r.oi[2] = oz * iz;
    r.eps = EPS_REL * (__builtin_fabsf(ox) + __builtin_fabsf(oy) + __builtin_fabsf(oz));
    r.odd = !(__builtin_fabsf(ix) + __builtin_fabsf(iy) + __builtin_fabsf(iz) < INV_MAX);      // list this ray whatever the slabs say
    return r;
}
FW_PT bool pretest_fma(const RayTerms &r, float cx, float cy, float cz, float hx, float hy, float hz, float best_t) {
    const float tcx = __builtin_fmaf(cx, r.inv[0], -r.oi[0]), tcy = __builtin_fmaf(cy, r.inv[1], -r.oi[1]), tcz = __builtin_fmaf(cz, r.inv[2], -r.oi[2]);
    const float hex = hx + r.eps, hey = hy + r.eps, hez = hz + r.eps;
    const float ax = __builtin_fabsf(r.inv[0]), ay = __builtin_fabsf(r.inv[1]), az = __builtin_fabsf(r.inv[2]);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(-hex, ax, tcx), __builtin_fmaf(-hey, ay, tcy)), __builtin_fmaf(-hez, az, tcz));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaf(hex, ax, tcx), __builtin_fmaf(hey, ay, tcy)), __builtin_fmaf(hez, az, tcz));
    const float lo_t = __builtin_fmaf(__builtin_fmaxf(tn, 0.f), T_REL, -T_ABS);
    return (bool)((int)r.odd | (int)!(__builtin_fminf(tf, best_t) < lo_t));      // (| not ||: nothing here is worth a branch around it)
}

}  // namespace fwpt
