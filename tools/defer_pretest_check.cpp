// defer_pretest_check — host proof that the box-list scan's pre-test (firework_amd/csrc/fw_defer_pretest.h) is conservative.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -mfma -pthread -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o tools/defer_pretest_check.bin tools/defer_pretest_check.cpp && tools/defer_pretest_check.bin [rays, default 1.2e8]
//
// For every ray and box: when the exact test — hit_rect3d on the ray taken into the object's frame, restated below from fw_kernels.hip
// operation for operation (host division is the correctly rounded quotient fdiv produces) — accepts the ray with t in (TMIN, best_t], the
// new pre-test must have said "maybe".  One violation fails the run (exit 1).  The boxes a scene hands the kernel are made the way the
// runtime makes them: the eight rotated corners' float min / max plus the position, then fwpt::make_cull_box.
// Rays: cornell-like ones (origins in and on the room, best_t = the room's own hit), and adversarial ones: origins on the box's faces,
// edges and corners, origins 1e3 .. 1e5 box sizes away aimed at faces, edges and corners, direction components of 0, +-tiny, denormal,
// inf and NaN, and best_t at, just above and just below the true hit.
// Also printed: how many candidates old and new form admit on the cornell-like rays (each is a list run's lane), and how often the OLD
// form rejected a ray the exact test accepts (it could: t = 0/0 is accepted by rect.rs whatever the other coordinates say).
#include "../firework_amd/csrc/fw_defer_pretest.h"

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

namespace {

struct V3 { float x, y, z; };
struct Ray { V3 o, d; };
inline float comp(const V3 &v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
constexpr float TMIN = 0.001f, TMAX = 2e9f;

// objects/rect.rs:47-73 as hit_rect<AX, false> computes it: rejects on `x < lo || x > hi`, so a NaN passes
template <int AX>
bool hit_rect(float a_min, float a_max, float b_min, float b_max, float k, const Ray &r, float tmin, float tmax, float &t_out) {
    constexpr int A1 = (AX == 2) ? 1 : 0, A2 = (AX == 0) ? 1 : 2, OT = (AX == 0) ? 2 : (AX == 1 ? 1 : 0);
    const float t = (k - comp(r.o, OT)) / comp(r.d, OT);
    const float pa = comp(r.o, A1) + t * comp(r.d, A1), pb = comp(r.o, A2) + t * comp(r.d, A2);
    t_out = t;
    return !(t < tmin || t > tmax) && !(pa < a_min || pa > a_max) && !(pb < b_min || pb > b_max);
}
// objects/rect3d.rs:18-100 as hit_rect3d_t<false>: faces +z, -z, +y, -y, +x, -x, narrowing, a later face wins a tie
bool hit_rect3d(const float p[3], const float s[3], const Ray &r, float tmin, float tmax, float &t_out) {
    const float px = p[0], py = p[1], pz = p[2], sx = s[0], sy = s[1], sz = s[2];
    float closest = tmax, t; bool any = false, h;
    h = hit_rect<0>(px, px + sx, py, py + sy, pz + sz, r, tmin, closest, t); if (h) { closest = t; any = true; }
    h = hit_rect<0>(px, px + sx, py, py + sy, pz, r, tmin, closest, t);      if (h) { closest = t; any = true; }
    h = hit_rect<1>(px, px + sx, pz, pz + sz, py + sy, r, tmin, closest, t); if (h) { closest = t; any = true; }
    h = hit_rect<1>(px, px + sx, pz, pz + sz, py, r, tmin, closest, t);      if (h) { closest = t; any = true; }
    h = hit_rect<2>(py, py + sy, pz, pz + sz, px + sx, r, tmin, closest, t); if (h) { closest = t; any = true; }
    h = hit_rect<2>(py, py + sy, pz, pz + sz, px, r, tmin, closest, t);      if (h) { closest = t; any = true; }
    t_out = closest;
    return any;
}

struct BoxCase {
    const char *name;
    float R[3][3], pos[3], p[3], s[3];
    bool rotated;
    float lo[3], hi[3];          // the world box the runtime stores (obj_cull, first half)
    fwpt::CullBox cb;            // ... and what it stores behind it
    float size;                  // largest extent
};
V3 rot_fwd(const BoxCase &b, V3 v) {
    return {b.R[0][0] * v.x + b.R[0][1] * v.y + b.R[0][2] * v.z, b.R[1][0] * v.x + b.R[1][1] * v.y + b.R[1][2] * v.z,
            b.R[2][0] * v.x + b.R[2][1] * v.y + b.R[2][2] * v.z};
}
V3 rot_inv(const BoxCase &b, V3 v) {
    return {b.R[0][0] * v.x + b.R[1][0] * v.y + b.R[2][0] * v.z, b.R[0][1] * v.x + b.R[1][1] * v.y + b.R[2][1] * v.z,
            b.R[0][2] * v.x + b.R[1][2] * v.y + b.R[2][2] * v.z};
}
Ray to_object_space(const BoxCase &b, const Ray &r) {
    const V3 q{r.o.x - b.pos[0], r.o.y - b.pos[1], r.o.z - b.pos[2]};
    if (b.rotated) return Ray{rot_inv(b, q), rot_inv(b, r.d)};
    return Ray{q, r.d};
}
V3 to_world(const BoxCase &b, V3 v) {
    const V3 w = b.rotated ? rot_fwd(b, v) : v;
    return {w.x + b.pos[0], w.y + b.pos[1], w.z + b.pos[2]};
}
// rotation by `ay` about y, then `ax` about x, then `az` about z (double, rounded once per entry)
BoxCase make_box(const char *name, double ay, double ax, double az, float px, float py, float pz, float sx, float sy, float sz, float opx = 0.f, float opy = 0.f,
                 float opz = 0.f) {
    BoxCase b{};
    b.name = name;
    const double cy = std::cos(ay), sy_ = std::sin(ay), cx = std::cos(ax), sx_ = std::sin(ax), cz = std::cos(az), sz_ = std::sin(az);
    const double Ry[3][3] = {{cy, 0, sy_}, {0, 1, 0}, {-sy_, 0, cy}}, Rx[3][3] = {{1, 0, 0}, {0, cx, -sx_}, {0, sx_, cx}}, Rz[3][3] = {{cz, -sz_, 0}, {sz_, cz, 0}, {0, 0, 1}};
    double T[3][3] = {}, M[3][3] = {};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) T[i][j] += Rx[i][k] * Ry[k][j];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) M[i][j] += Rz[i][k] * T[k][j];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) b.R[i][j] = (float)M[i][j];
    b.pos[0] = px; b.pos[1] = py; b.pos[2] = pz;
    b.p[0] = opx; b.p[1] = opy; b.p[2] = opz; b.s[0] = sx; b.s[1] = sy; b.s[2] = sz;
    b.rotated = 0.5f * ((b.R[0][0] + b.R[1][1] + b.R[2][2]) - 1.f) < 0.999f;          // scene.rs:180-185
    float mn[3] = {b.p[0], b.p[1], b.p[2]}, mx[3] = {b.p[0] + sx, b.p[1] + sy, b.p[2] + sz};
    if (b.rotated) {                                                                    // scene.rs:188-203: float corners
        const float omn[3] = {mn[0], mn[1], mn[2]}, omx[3] = {mx[0], mx[1], mx[2]};
        for (int a = 0; a < 3; a++) { mn[a] = 10e9f; mx[a] = -10e9f; }
        for (int i = 0; i < 8; i++) {
            const V3 c = rot_fwd(b, V3{(i & 1) ? omx[0] : omn[0], (i & 2) ? omx[1] : omn[1], (i & 4) ? omx[2] : omn[2]});
            mn[0] = std::fmin(c.x, mn[0]); mn[1] = std::fmin(c.y, mn[1]); mn[2] = std::fmin(c.z, mn[2]);
            mx[0] = std::fmax(c.x, mx[0]); mx[1] = std::fmax(c.y, mx[1]); mx[2] = std::fmax(c.z, mx[2]);
        }
    }
    for (int a = 0; a < 3; a++) { b.lo[a] = mn[a] + b.pos[a]; b.hi[a] = mx[a] + b.pos[a]; }
    b.cb = fwpt::make_cull_box(b.lo, b.hi);
    b.size = std::fmax(sx, std::fmax(sy, sz));
    return b;
}

struct Rng {
    uint64_t s;
    uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    float u() { return (float)(next() >> 40) * (1.f / 16777216.f); }               // [0, 1)
    float sym() { return 2.f * u() - 1.f; }
    uint32_t below(uint32_t n) { return (uint32_t)(next() >> 33) % n; }
    V3 unit() {
        for (;;) { const V3 v{sym(), sym(), sym()}; const float l = v.x * v.x + v.y * v.y + v.z * v.z; if (l > 1e-4f && l <= 1.f) { const float q = 1.f / std::sqrt(l); return {v.x * q, v.y * q, v.z * q}; } }
    }
};
float ulps(float x, int n) {
    if (!(std::fabs(x) < std::numeric_limits<float>::infinity()) || x == 0.f) return x;
    uint32_t u; std::memcpy(&u, &x, 4); u += (uint32_t)n; float y; std::memcpy(&y, &u, 4);
    return std::isfinite(y) ? y : x;
}
// make_rcp(b).r as the device computes it: v_rcp_f32 (1 ulp: the rounded quotient moved by up to an ulp), then one Newton step
float device_rcp(float b, Rng &g, bool loose) {
    float r = ulps(1.0f / b, (int)g.below(3) - 1);
    r = __builtin_fmaf(__builtin_fmaf(-b, r, 1.0f), r, r);
    return loose ? ulps(r, (int)g.below(5) - 2) : r;            // ... and up to the 2^-22 the header's argument allows
}

struct Counts {
    uint64_t rays = 0, exact_hits = 0, violations = 0, old_holes = 0, flagged = 0;
    uint64_t cornell_tests = 0, cand_old = 0, cand_new = 0, cand_exact = 0;
};

void report(const BoxCase &b, const Ray &r, float best_t, float t, const fwpt::RayTerms &rt) {
    std::fprintf(stderr, "VIOLATION box %s: o = (%a, %a, %a) d = (%a, %a, %a) best_t = %a: exact t = %a, inv = (%a, %a, %a)\n", b.name, r.o.x, r.o.y, r.o.z, r.d.x,
                 r.d.y, r.d.z, best_t, t, rt.inv[0], rt.inv[1], rt.inv[2]);
}

// one ray against one box; `cornell`: counted in the candidate statistics
void check(const BoxCase &b, const Ray &r, float best_t, Rng &g, Counts &c, bool cornell) {
    const float ainv[3] = {ulps(1.0f / r.d.x, (int)g.below(3) - 1), ulps(1.0f / r.d.y, (int)g.below(3) - 1), ulps(1.0f / r.d.z, (int)g.below(3) - 1)};
    const bool loose = !cornell && g.below(2);
    const fwpt::RayTerms rt = fwpt::ray_terms(r.o.x, r.o.y, r.o.z, device_rcp(r.d.x, g, loose), device_rcp(r.d.y, g, loose), device_rcp(r.d.z, g, loose));
    const float o[3] = {r.o.x, r.o.y, r.o.z};
    const bool m_new = fwpt::pretest_fma(rt, b.cb.c[0], b.cb.c[1], b.cb.c[2], b.cb.h[0], b.cb.h[1], b.cb.h[2], best_t);
    const bool m_old = fwpt::pretest_sub(b.lo, b.hi, o, ainv, best_t);
    float t;
    const bool hit = hit_rect3d(b.p, b.s, to_object_space(b, r), TMIN, best_t, t);
    c.rays++;
    c.flagged += rt.odd;
    if (hit) {
        c.exact_hits++;
        if (!m_new) { if (c.violations++ < 8) report(b, r, best_t, t, rt); }
        if (!m_old) c.old_holes++;
    }
    if (cornell) { c.cornell_tests++; c.cand_old += m_old; c.cand_new += m_new; c.cand_exact += hit; }
}

// a point on the box's surface in its own frame: on a face, an edge or a corner
V3 surface_point(const BoxCase &b, Rng &g, int kind) {
    float q[3];
    for (int a = 0; a < 3; a++) q[a] = b.p[a] + b.s[a] * g.u();
    const int fixed = kind == 0 ? 1 : (kind == 1 ? 2 : 3);        // face: one coordinate on a plane; edge: two; corner: three
    const int first = (int)g.below(3);
    for (int i = 0; i < fixed; i++) { const int a = (first + i) % 3; q[a] = g.below(2) ? b.p[a] + b.s[a] : b.p[a]; }
    return {q[0], q[1], q[2]};
}
float odd_component(Rng &g) {
    static const float v[] = {0.f, -0.f, 1e-30f, -1e-30f, 1e-20f, -1e-20f, 1e-10f, -1e-10f, 1e-42f, -1e-42f, 1.17549435e-38f, 1e-7f, -1e-7f,
                              std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    return v[g.below(sizeof v / sizeof v[0])];
}

void adversarial(const BoxCase &b, Rng &g, Counts &c) {
    const int mode = (int)g.below(8);
    Ray r;
    const V3 target = to_world(b, surface_point(b, g, (int)g.below(3)));
    if (mode <= 1) {                       // from the surface: any direction, or along a face / an edge (object-frame axis directions)
        r.o = target;
        if (mode == 0) r.d = g.unit();
        else { V3 e{0, 0, 0}; const int a = (int)g.below(3); (a == 0 ? e.x : a == 1 ? e.y : e.z) = g.below(2) ? 1.f : -1.f; if (g.below(2)) (a == 0 ? e.y : a == 1 ? e.z : e.x) = g.sym(); r.d = b.rotated ? rot_fwd(b, e) : e; }
    } else if (mode <= 3) {                // from far away, aimed at a face, edge or corner point (or a hair beside it)
        const float dist = b.size * std::pow(10.f, 3.f + 2.f * g.u());
        const V3 u = g.unit();
        r.o = {target.x + dist * u.x, target.y + dist * u.y, target.z + dist * u.z};
        V3 aim = target;
        if (mode == 3) { const float j = b.size * 1e-6f; aim = {aim.x + j * g.sym(), aim.y + j * g.sym(), aim.z + j * g.sym()}; }
        const V3 d{aim.x - r.o.x, aim.y - r.o.y, aim.z - r.o.z};
        const float l = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
        r.d = g.below(2) ? V3{d.x / l, d.y / l, d.z / l} : d;                       // (camera rays are not normalised either)
    } else if (mode <= 5) {                // zero, tiny, infinite and NaN direction components, from the surface or from nearby
        r.o = target;
        if (mode == 5) { const float s = b.size * 2.f; r.o = {r.o.x + s * g.sym(), r.o.y + s * g.sym(), r.o.z + s * g.sym()}; }
        r.d = g.unit();
        const int n = 1 + (int)g.below(2), a0 = (int)g.below(3);
        for (int i = 0; i < n; i++) { const int a = (a0 + i) % 3; (a == 0 ? r.d.x : a == 1 ? r.d.y : r.d.z) = odd_component(g); }
        if (!b.rotated || g.below(2)) { /* as drawn: world axes */ } else r.d = rot_fwd(b, r.d);      // ... or the object's axes
    } else {                               // from nearby towards the box: best_t at, just above and just below the true hit (below)
        const float s = b.size * (0.1f + 3.f * g.u());
        const V3 u = g.unit();
        r.o = {target.x + s * u.x, target.y + s * u.y, target.z + s * u.z};
        const V3 inner = to_world(b, V3{b.p[0] + b.s[0] * g.u(), b.p[1] + b.s[1] * g.u(), b.p[2] + b.s[2] * g.u()});
        r.d = {inner.x - r.o.x, inner.y - r.o.y, inner.z - r.o.z};
        if (g.below(2)) { const float l = std::sqrt(r.d.x * r.d.x + r.d.y * r.d.y + r.d.z * r.d.z); r.d = {r.d.x / l, r.d.y / l, r.d.z / l}; }
    }
    if (g.below(16) == 0) (g.below(2) ? r.o.x : r.o.z) = std::numeric_limits<float>::quiet_NaN();
    float t;
    float best_t = TMAX;
    if (hit_rect3d(b.p, b.s, to_object_space(b, r), TMIN, TMAX, t)) {
        switch (g.below(5)) {
        case 0: best_t = t; break;                     // `t > t_max` rejects: t == best_t is accepted
        case 1: best_t = ulps(t, 1); break;
        case 2: best_t = ulps(t, -1); break;           // this face is out; a farther one never is nearer: usually a reject
        case 3: best_t = t * (1.f + 1e-4f); break;
        default: break;
        }
    } else if (g.below(4) == 0) best_t = b.size * 4.f * g.u();
    check(b, r, best_t, g, c, false);
}

// cornell: the room is [0, 555]^3 (open towards -z, where the camera stands); a ray starts on a wall, on a box or at the camera and
// best_t is where it leaves the room (what the six in-line rectangles give before the pre-tests run)
void cornell(const BoxCase *boxes, Rng &g, Counts &c) {
    Ray r;
    const uint32_t m = g.below(8);
    if (m == 0) { r.o = {278.f, 278.f, -800.f}; r.d = {555.f * g.u() - 278.f, 555.f * g.u() - 278.f, 800.f}; }
    else if (m <= 2) { r.o = to_world(boxes[m - 1], surface_point(boxes[m - 1], g, 0)); r.d = g.unit(); }
    else {
        float q[3] = {555.f * g.u(), 555.f * g.u(), 555.f * g.u()};
        const int a = (int)g.below(3); q[a] = (a == 2 || g.below(2)) ? 555.f : 0.f;
        r.o = {q[0], q[1], q[2]}; r.d = g.unit();
        const float into = a == 0 ? r.d.x : (a == 1 ? r.d.y : r.d.z);
        if ((q[a] == 0.f) != (into > 0.f)) r.d = {-r.d.x, -r.d.y, -r.d.z};          // leaves the wall into the room
    }
    float best_t = TMAX;
    const float o[3] = {r.o.x, r.o.y, r.o.z}, d[3] = {r.d.x, r.d.y, r.d.z};
    for (int a = 0; a < 3; a++)
        for (int side = 0; side < 2; side++) {
            if (a == 2 && side == 0) continue;
            const float t = ((side ? 555.f : 0.f) - o[a]) / d[a];
            if (t > TMIN && t < best_t) best_t = t;
        }
    check(boxes[0], r, best_t, g, c, true);
    check(boxes[1], r, best_t, g, c, true);
}

}  // namespace

int main(int argc, char **argv) {
    const uint64_t total = argc > 1 ? (uint64_t)std::strtod(argv[1], nullptr) : 120000000ull;
    const double rad = 3.14159265358979323846 / 180.0;
    std::vector<BoxCase> boxes = {
        make_box("cornell short", 18.0 * rad, 0, 0, 130.f, 0.f, 65.f, 165.f, 165.f, 165.f),
        make_box("cornell tall", -15.0 * rad, 0, 0, 265.f, 0.f, 295.f, 165.f, 330.f, 165.f),
        make_box("unrotated", 0, 0, 0, 0.5f, -0.2f, 3.f, 1.3f, 0.7f, 2.1f),
        make_box("unrotated, off its origin", 0, 0, 0, 100.f, 0.f, -40.f, 30.f, 20.f, 10.f, -15.f, -10.f, -5.f),
        make_box("rotated 45 about y", 45.0 * rad, 0, 0, 0.f, 0.f, 0.f, 2.f, 1.f, 2.f, -1.f, -0.5f, -1.f),
        make_box("at 1e4", 0.3, 0.5, -0.7, 1e4f, -1e4f, 1e4f, 1.f, 2.f, 0.5f),
        make_box("at 3e4, unrotated", 0, 0, 0, -3e4f, 3e4f, 16384.37f, 0.4f, 0.4f, 0.4f),
        make_box("tiny", 1.1, -0.4, 0.2, 0.01f, 0.02f, -0.01f, 1e-3f, 2e-3f, 1e-3f),
        make_box("flat slab", 0.2, 0, 0, -500.f, 10.f, 200.f, 1e3f, 1.f, 1e3f),
        make_box("2^12 scale", 0.6, 0.1, 0.9, 1e5f, 2e5f, -3e5f, 4096.f, 8192.f, 4096.f),
        make_box("2^-10 scale", 0.6, 0.1, 0.9, 1e-3f, 2e-3f, -3e-3f, 9.765625e-4f, 1.953125e-3f, 9.765625e-4f),
    };
    const unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<Counts> counts(n_threads);
    std::vector<std::thread> pool;
    for (unsigned th = 0; th < n_threads; th++)
        pool.emplace_back([&, th] {
            Rng g{0x1234567ull + 0x51ED270Bull * th};
            Counts &c = counts[th];
            const uint64_t share = total / n_threads + 1;
            // a third cornell-like (two box tests each), the rest adversarial, every box in turn
            while (c.rays < share) {
                if (g.below(3) == 0) cornell(boxes.data(), g, c);
                else adversarial(boxes[g.below((uint32_t)boxes.size())], g, c);
            }
        });
    for (auto &t : pool) t.join();
    Counts s;
    for (const Counts &c : counts) {
        s.rays += c.rays; s.exact_hits += c.exact_hits; s.violations += c.violations; s.old_holes += c.old_holes; s.flagged += c.flagged;
        s.cornell_tests += c.cornell_tests; s.cand_old += c.cand_old; s.cand_new += c.cand_new; s.cand_exact += c.cand_exact;
    }
    std::printf("ray-box tests            %llu on %zu boxes, %u threads\n", (unsigned long long)s.rays, boxes.size(), n_threads);
    std::printf("exact test accepted      %llu\n", (unsigned long long)s.exact_hits);
    std::printf("  new form said no       %llu   (must be 0)\n", (unsigned long long)s.violations);
    std::printf("  old form said no       %llu   (informative)\n", (unsigned long long)s.old_holes);
    std::printf("listed as odd            %llu\n", (unsigned long long)s.flagged);
    std::printf("cornell-like tests       %llu: exact hits %llu, candidates old %llu, new %llu (%+.4f %%)\n", (unsigned long long)s.cornell_tests,
                (unsigned long long)s.cand_exact, (unsigned long long)s.cand_old, (unsigned long long)s.cand_new,
                s.cand_old ? 100.0 * ((double)s.cand_new - (double)s.cand_old) / (double)s.cand_old : 0.0);
    bool ok = s.violations == 0 && s.rays >= total;
    if (s.cand_old && (double)s.cand_new > 1.02 * (double)s.cand_old) { std::printf("FAIL: the new form lists more than 2 %% more candidates\n"); ok = false; }
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
