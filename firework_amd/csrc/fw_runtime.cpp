// fw_runtime.cpp — host side of libfirework_hip.so: the C ABI of include/firework_hip.h.
//
//   fw_scene_create : `Scene -> SceneInternal` (reference src/scene.rs:111-135,279-292) flattened to the
//                     HBM layout of fw_device.h; TLAS/BLAS built with the reference's median split
//                     (src/bvh.rs:21-71) and stored in DFS order.
//   fw_render       : the wavefront loop that replaces the rayon pixel loop of src/render.rs:127-161:
//                     raygen -> 11 x (extend, shade+compact) -> accumulate, per batch of paths; resolve.
//
// No CPU rendering path exists here: without a HIP device every entry point fails with FW_ERR_NO_DEVICE.
#include "../../include/firework_hip.h"
#include "fw_device.h"
#include "fw_build.h"
#include "fw_temporal.h"
#include "fw_camera_models.h"
#include "fw_probes.h"
#include "fw_lightmap.h"
#include "fw_probe_lookup.h"
#include "fw_probe_depth.h"
#include "fw_ao.h"
#include "fw_probe_place.h"
#include "fw_probe_radiance.h"
#include "fw_direct.h"
#include "fw_sky.h"
#include "fw_ggx_table.h"
#include "fw_gather.h"
#include "fw_reflect.h"
#include "fw_area.h"
#include "fw_emitters.h"
#include "fw_defer_pretest.h"

#include <algorithm>
#include <atomic>
#include <exception>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace {

thread_local std::string g_last_error;

int fail(int status, const std::string &msg) { g_last_error = msg; return status; }

// ---- options: every runtime switch of the library.  The environment (FIREWORK_<NAME>) is read ONCE, when the library is loaded;
// fw_set_option changes one afterwards (tests, tools/).  Nothing on the render path calls getenv, and the product build carries
// no switch for a kernel it does not carry.
struct Options {
    bool bvh_median = false;      // BVH=median: walk the reference's own topology (parity / A-B mode)
    bool no_exact = false, exact_all = false;   // NO_EXACT: no literal walk at all; EXACT_ALL=1: every ray takes it (the renderer then IS bvh.rs:115-151)
    int exact_form = 0;           // EXACT_FORM=lane|wave
    bool no_defer = false, no_hit4 = false, no_hoist = false, no_lds_tables = false, no_lds_trees = false, no_lds_tris = false, no_short_rays = false,
         no_tile_order = false, no_zero_skip = false, dep_pixel_major = false, dep_slot_major = false, trace = false, no_chain = false,
         exact_product = false;   // EXACT_PRODUCT: textured scenes keep every scattering's attenuation and multiply back to front at deposit (render.rs:23-28's order)
    int streams = 0;              // STREAMS=n batches in flight (0: the library's choice)
    int graph = -1;               // GRAPH=0|1: a frame that repeats is replayed as one hipGraph (-1: frames of small batches, whose launches are short)
    int phase_lock = -1;          // PHASE_LOCK=0|1: the two batches in flight held in anti-phase, one's extend beside the other's shade (-1: where it pays: box-list scenes)
    int soft_shear_log2 = 5, exact_shear_log2 = 10; double exact_far_x = 256.0;   // SOFT_SHEAR_LOG2 (0: off), EXACT_SHEAR_LOG2, EXACT_FAR_X: the flag rules' thresholds (tools/flag_margin.py)
    double wide_node_cost = 0.0005;   // WIDE_NODE_COST: the constant a wide node costs in the collapse, in root areas (wide_convert)
    int wide = -1;                // WIDE=0|f32|q8: no wide nodes / force an encoding (-1: by size)
    int build = -1;               // BUILD=host|device: where a scene's trees are built (-1: by size, BUILD_MIN)
    int fuse_segments = -1;       // FUSE_SEGMENTS=0|1: a box-list batch's segments in one launch of k_segments_boxlist (-1: off — fused frames did not clear the 2 x spread bar over the unfused launches at the same queue count)
    long waves = 0;               // WAVES=n wave queues (0: the library's choice)
    long long paths_per_batch = 0;
    std::string dump_path;        // DUMP_PATH=file (tools/diverge.py)
#if FW_AB
    bool fused = false, tlas_refill_off = false, shade_list = false, no_shade_defer = false, stagger = false;
    int debug_wide_levels = 0;    // DEBUG_WIDE_LEVELS=n: undersized LDS stacks for the wide walks (the error word's test)
#endif
};
const char *const OPTION_NAMES[] = {"BVH", "NO_EXACT", "EXACT_ALL", "EXACT_FORM", "NO_DEFER", "NO_HIT4", "NO_HOIST", "NO_LDS_TABLES", "NO_LDS_TREES", "NO_LDS_TRIS",
                                    "NO_SHORT_RAYS", "NO_TILE_ORDER", "NO_ZERO_SKIP", "DEP_PIXEL_MAJOR", "DEP_SLOT_MAJOR", "NO_CHAIN", "EXACT_PRODUCT", "PHASE_LOCK", "FUSE_SEGMENTS", "GRAPH", "SOFT_SHEAR_LOG2", "EXACT_SHEAR_LOG2", "EXACT_FAR_X", "WIDE_NODE_COST", "TRACE", "STREAMS", "WIDE", "BUILD", "WAVES",
                                    "PATHS_PER_BATCH", "DUMP_PATH",
#if FW_AB
                                    "FUSED", "TLAS_REFILL", "SHADE_LIST", "NO_SHADE_DEFER", "STAGGER", "DEBUG_WIDE_LEVELS",
#endif
                                    nullptr};
bool option_apply(Options &o, const char *name, const char *v) {      // v == nullptr: back to the default
    const std::string n = name;
    auto on = [&] { return v != nullptr; };
    auto num = [&] { return v ? atoll(v) : 0ll; };
    if (n == "BVH") o.bvh_median = v && std::strcmp(v, "median") == 0;
    else if (n == "NO_EXACT") o.no_exact = on();
    else if (n == "EXACT_ALL") o.exact_all = num() != 0;
    else if (n == "EXACT_FORM") o.exact_form = v ? (std::strcmp(v, "lane") == 0 ? 1 : (std::strcmp(v, "wave") == 0 ? 2 : 0)) : 0;
    else if (n == "NO_DEFER") o.no_defer = on();
    else if (n == "NO_HIT4") o.no_hit4 = on();
    else if (n == "NO_HOIST") o.no_hoist = on();
    else if (n == "NO_LDS_TABLES") o.no_lds_tables = on();
    else if (n == "NO_LDS_TREES") o.no_lds_trees = on();
    else if (n == "NO_LDS_TRIS") o.no_lds_tris = on();
    else if (n == "NO_SHORT_RAYS") o.no_short_rays = on();
    else if (n == "NO_TILE_ORDER") o.no_tile_order = on();
    else if (n == "NO_ZERO_SKIP") o.no_zero_skip = on();
    else if (n == "DEP_PIXEL_MAJOR") o.dep_pixel_major = on();
    else if (n == "DEP_SLOT_MAJOR") o.dep_slot_major = on();
    else if (n == "NO_CHAIN") o.no_chain = on();
    else if (n == "EXACT_PRODUCT") o.exact_product = v && atoi(v) != 0;
    else if (n == "PHASE_LOCK") o.phase_lock = v ? (atoi(v) != 0 ? 1 : 0) : -1;
    else if (n == "FUSE_SEGMENTS") o.fuse_segments = v ? (atoi(v) != 0 ? 1 : 0) : -1;
    else if (n == "GRAPH") o.graph = v ? (atoi(v) != 0 ? 1 : 0) : -1;
    else if (n == "SOFT_SHEAR_LOG2") o.soft_shear_log2 = v ? (int)num() : 5;
    else if (n == "EXACT_SHEAR_LOG2") o.exact_shear_log2 = v ? (int)num() : 10;
    else if (n == "EXACT_FAR_X") o.exact_far_x = v ? atof(v) : 256.0;
    else if (n == "WIDE_NODE_COST") o.wide_node_cost = v ? atof(v) : 0.0005;
    else if (n == "TRACE") o.trace = on();
    else if (n == "STREAMS") o.streams = (int)std::max<long long>(0, num());
    else if (n == "WIDE") o.wide = !v ? -1 : (std::strcmp(v, "0") == 0 ? 0 : (std::strcmp(v, "f32") == 0 ? 1 : (std::strcmp(v, "q8") == 0 ? 2 : -1)));
    else if (n == "BUILD") {
        if (v && std::strcmp(v, "host") != 0 && std::strcmp(v, "device") != 0) return false;
        o.build = !v ? -1 : (std::strcmp(v, "device") == 0 ? 1 : 0);
    }
    else if (n == "WAVES") o.waves = (long)std::max<long long>(0, num());
    else if (n == "PATHS_PER_BATCH") o.paths_per_batch = std::max<long long>(0, num());
    else if (n == "DUMP_PATH") o.dump_path = v ? v : "";
#if FW_AB
    else if (n == "FUSED") o.fused = num() != 0;
    else if (n == "TLAS_REFILL") o.tlas_refill_off = v && atoi(v) == 0;
    else if (n == "SHADE_LIST") o.shade_list = on();
    else if (n == "NO_SHADE_DEFER") o.no_shade_defer = on();
    else if (n == "STAGGER") o.stagger = on();
    else if (n == "DEBUG_WIDE_LEVELS") o.debug_wide_levels = (int)std::max<long long>(0, num());
#endif
    else return false;
    return true;
}
Options options_from_env() {
    Options o;
    for (int k = 0; OPTION_NAMES[k]; k++) { const std::string e = std::string("FIREWORK_") + OPTION_NAMES[k]; if (const char *v = getenv(e.c_str())) option_apply(o, OPTION_NAMES[k], v); }
    return o;
}
std::mutex g_opt_mu;
Options g_opt = options_from_env();          // once, at load
Options options() { std::lock_guard<std::mutex> g(g_opt_mu); return g_opt; }

#define HIPCHK(expr)                                                                                           \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            char buf_[512];                                                                                    \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return fail(e_ == hipErrorOutOfMemory ? FW_ERR_OOM : FW_ERR_HIP, buf_);                            \
        }                                                                                                      \
    } while (0)

// The device checks of an entry point, made once its arguments are valid (the header documents where in each call's order).
// need_device: a HIP device is visible (their number in *n_out); use_device: and `device` names one, which becomes the current device.
int need_device(int *n_out = nullptr) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(FW_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)"); }
    if (n_out) *n_out = ndev;
    return FW_OK;
}
int use_device(int device) {
    int ndev = 0;
    if (int rc = need_device(&ndev)) return rc;
    if (device < 0 || device >= ndev) return fail(FW_ERR_BAD_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    return FW_OK;
}

// the 32-bit seed the kernels key their draws with: a 64-bit seed folded
inline uint32_t seed32_of(uint64_t seed) { return (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x9E3779B9u); }

// The stats of one more render_impl call of a chunked entry point, added to the call's total: the one place that knows which fields
// add and which take the latest value (the tree sizes, and `reserved`: the depths walked, bit 31 clear where no chunk runs as a frame
// graph).  ms_scene and ms_wall are the caller's own; what a caller's other kernels took and moved it adds after this.
void stats_add(fw_stats &total, const fw_stats &part) {
    total.samples += part.samples; total.rays += part.rays;
    for (int s = 0; s < FW_MAX_SEGMENTS; s++) total.rays_per_depth[s] += part.rays_per_depth[s];
    total.algorithmic_bytes += part.algorithmic_bytes;
    total.ms_render += part.ms_render; total.ms_raygen += part.ms_raygen; total.ms_extend += part.ms_extend; total.ms_shade += part.ms_shade;
    total.ms_accumulate += part.ms_accumulate; total.ms_d2h += part.ms_d2h;
    total.n_extend_launches += part.n_extend_launches; total.n_shade_launches += part.n_shade_launches; total.n_batches += part.n_batches;
    total.tlas_nodes = part.tlas_nodes; total.blas_nodes = part.blas_nodes; total.reserved = part.reserved;
    total.bytes_raygen += part.bytes_raygen; total.bytes_extend += part.bytes_extend; total.bytes_shade += part.bytes_shade;
    total.bytes_accumulate += part.bytes_accumulate;
    total.deposits += part.deposits; total.parked_rays += part.parked_rays;
}

// ---- host-side f32 vector math; same expressions as the reference (and -ffp-contract=off) ------------
struct V3 { float x, y, z; float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); } };
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float dot(V3 a, V3 b) { return std::fmaf(a.x, b.x, std::fmaf(a.y, b.y, a.z * b.z)); }
inline V3 cross(V3 a, V3 b) { return {std::fmaf(a.y, b.z, -a.z * b.y), std::fmaf(a.z, b.x, -a.x * b.z), std::fmaf(a.x, b.y, -a.y * b.x)}; }
inline V3 normalized(V3 a) { float m = std::sqrt(dot(a, a)); return {a.x / m, a.y / m, a.z / m}; }
inline V3 vmin(V3 a, V3 b) { return {std::fmin(a.x, b.x), std::fmin(a.y, b.y), std::fmin(a.z, b.z)}; }
inline V3 vmax(V3 a, V3 b) { return {std::fmax(a.x, b.x), std::fmax(a.y, b.y), std::fmax(a.z, b.z)}; }
inline V3 tov(const fw_vec3 &v) { return {v.x, v.y, v.z}; }

struct Box { V3 mn, mx; };
inline Box box_union(const Box &a, const Box &b) { return {vmin(a.mn, b.mn), vmax(a.mx, b.mx)}; }   // aabb.rs:52-57
inline V3 box_center(const Box &b) { return 0.5f * b.mn + 0.5f * b.mx; }                             // aabb.rs:59-61

inline float bits_f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// ultraviolet Rotor3::into_matrix; rows[i] = row i of rotation_mat
void rotor_rows(const fw_rotor3 &r, float rows[3][3]) {
    float s2 = r.s * r.s, bxy2 = r.xy * r.xy, bxz2 = r.xz * r.xz, byz2 = r.yz * r.yz;
    float s_bxy = r.s * r.xy, s_bxz = r.s * r.xz, s_byz = r.s * r.yz;
    float bxz_byz = r.xz * r.yz, bxy_byz = r.xy * r.yz, bxy_bxz = r.xy * r.xz;
    float c0[3] = {s2 - bxy2 - bxz2 + byz2, -2.f * (bxz_byz + s_bxy), 2.f * (bxy_byz - s_bxz)};
    float c1[3] = {2.f * (s_bxy - bxz_byz), s2 - bxy2 + bxz2 - byz2, -2.f * (s_byz + bxy_bxz)};
    float c2[3] = {2.f * (s_bxz + bxy_byz), 2.f * (s_byz - bxy_bxz), s2 + bxy2 - bxz2 - byz2};
    for (int i = 0; i < 3; i++) { rows[i][0] = c0[i]; rows[i][1] = c1[i]; rows[i][2] = c2[i]; }
}
inline V3 mat_mul(const float rows[3][3], V3 v) {   // Mat3 * Vec3: c0*x + c1*y + c2*z
    return {rows[0][0] * v.x + rows[0][1] * v.y + rows[0][2] * v.z,
            rows[1][0] * v.x + rows[1][1] * v.y + rows[1][2] * v.z,
            rows[2][0] * v.x + rows[2][1] * v.y + rows[2][2] * v.z};
}

// ---- K10: flat BVH builder reproducing bvh.rs:21-71 ---------------------------------------------------
struct FlatBvh {
    std::vector<float> nodes;   // 8 floats per node
    uint32_t depth = 0;
    uint32_t count() const { return (uint32_t)(nodes.size() / 8); }
};
struct NanError {};

// ---- parallel host builds (round 5).  The reference builds its trees inside its timed region (main.rs:40-44) on one thread; so did this
// library until round 4: 1.0 s for the median tree and 0.5 s for the SAH tree of a million triangles (profiles/r05_big_mesh.txt).  Both
// recursions are independent below a node, so a node with enough items hands its left subtree to another thread, which builds it into a
// tree of its own; the two are appended behind the node in depth-first order (child indices shifted) — the same nodes in the same order as
// the sequential build — and the big sorts and binning passes near the root are split over the threads that are still free.  A stable
// sort's result does not depend on how it was computed, box unions (fmin / fmax) and counts are exact: the trees are bit-identical.
struct BuildPool {
    std::atomic<int> free_threads;
    explicit BuildPool(int n) : free_threads(n) {}
    int take(int want) {      // up to `want` helper threads (possibly 0)
        int got = 0;
        while (got < want) { int f = free_threads.load(); if (f <= 0) break; if (free_threads.compare_exchange_weak(f, f - 1)) got++; }
        return got;
    }
    void give(int n) { free_threads.fetch_add(n); }
};
inline int host_build_threads() {
    static const int n = [] { const char *e = getenv("FIREWORK_BUILD_THREADS"); int v = e ? atoi(e) : (int)std::thread::hardware_concurrency(); return std::max(1, std::min(v, 64)); }();
    return n;
}
constexpr size_t PAR_SUBTREE_MIN = 4096, PAR_PASS_MIN = 1 << 15;     // items below which a subtree / a pass over the items stays on its thread

// f(begin, end, part) over [0, n) in `parts` contiguous parts, part 0 on the calling thread
template <class F> void par_parts(size_t n, int parts, F f) {
    if (parts <= 1) { f((size_t)0, n, 0); return; }
    std::vector<std::thread> th;
    th.reserve((size_t)parts - 1);
    for (int k = 1; k < parts; k++) th.emplace_back([&, k] { f(n * (size_t)k / (size_t)parts, n * (size_t)(k + 1) / (size_t)parts, k); });
    f((size_t)0, n / (size_t)parts, 0);
    for (auto &t : th) t.join();
}
// std::stable_sort's result by any route: sorted parts, merged pairwise (inplace_merge is stable)
template <class Cmp> void par_stable_sort(uint32_t *b, size_t n, Cmp cmp, BuildPool &pool) {
    int helpers = n >= PAR_PASS_MIN ? pool.take(15) : 0;
    int parts = 1; while (parts * 2 <= helpers + 1) parts *= 2;           // a power of two
    pool.give(helpers - (parts - 1)); helpers = parts - 1;
    if (parts == 1) { std::stable_sort(b, b + n, cmp); return; }
    auto cut = [&](int k) { return n * (size_t)k / (size_t)parts; };
    par_parts(n, parts, [&](size_t lo, size_t hi, int) { std::stable_sort(b + lo, b + hi, cmp); });
    for (int width = 1; width < parts; width *= 2) {
        const int pairs = parts / (2 * width);
        par_parts((size_t)pairs, pairs, [&](size_t lo, size_t hi, int) {
            for (size_t q = lo; q < hi; q++) std::inplace_merge(b + cut((int)q * 2 * width), b + cut((int)q * 2 * width + width), b + cut((int)(q + 1) * 2 * width), cmp);
        });
    }
    pool.give(helpers);
}
// appends tree `t` (root at its node 0) to `out`, child indices shifted; returns where its root went
inline uint32_t append_tree(FlatBvh &out, const FlatBvh &t) {
    const uint32_t off = out.count();
    out.nodes.insert(out.nodes.end(), t.nodes.begin(), t.nodes.end());
    for (uint32_t i = 0; i < t.count(); i++) {
        float *p = &out.nodes[(size_t)(off + i) * 8];
        uint32_t A; std::memcpy(&A, p + 3, 4);
        if ((A >> 30) == 0u) { A += off; std::memcpy(p + 3, &A, 4); }      // a Branch: its right child
    }
    out.depth = std::max(out.depth, t.depth);
    return off;
}
// build(left, into) and build(right, into): the left one on a helper thread into a tree of its own when the node is big enough and a thread is
// free, else both in place.  Returns the right child's index; lb / rb = the children's boxes.
template <class Build> uint32_t build_children(FlatBvh &out, size_t n, size_t half, BuildPool &pool, Build build, Box &lb, Box &rb) {
    if (n >= PAR_SUBTREE_MIN && pool.take(1) == 1) {
        FlatBvh L, R;
        std::exception_ptr ep;
        std::thread th([&] { try { build(L, (size_t)0, half, lb); } catch (...) { ep = std::current_exception(); } });
        try { build(R, half, n - half, rb); } catch (...) { th.join(); pool.give(1); throw; }
        th.join(); pool.give(1);
        if (ep) std::rethrow_exception(ep);
        append_tree(out, L);
        return append_tree(out, R);
    }
    build(out, (size_t)0, half, lb);                                    // left child = me + 1
    const uint32_t before = out.count();
    build(out, half, n - half, rb);
    return before;
}

struct Centers { std::vector<float> c[3]; };     // box_center per item and axis, computed once per build (the comparators read them millions of times)
inline Centers centers_of(const std::vector<Box> &boxes, BuildPool &pool) {
    Centers ce;
    const size_t n = boxes.size();
    for (int a = 0; a < 3; a++) ce.c[a].resize(n);
    const int helpers = n >= PAR_PASS_MIN ? pool.take(7) : 0;
    par_parts(n, helpers + 1, [&](size_t lo, size_t hi, int) { for (size_t i = lo; i < hi; i++) { const V3 c = box_center(boxes[i]); ce.c[0][i] = c.x; ce.c[1][i] = c.y; ce.c[2][i] = c.z; } });
    pool.give(helpers);
    return ce;
}

uint32_t bvh_build_rec(FlatBvh &out, const std::vector<Box> &boxes, const Centers &ce, uint32_t *idx, size_t n, uint32_t depth, Box &node_box, BuildPool &pool) {
    int axis = (int)(depth % 3);
    const float *key = ce.c[axis].data();
    for (size_t i = 0; i < n; i++) { float c = key[idx[i]]; if (c != c) throw NanError(); }
    // Rust's sort_by is stable; the sub-slice is re-sorted at every level (bvh.rs:29-35)
    par_stable_sort(idx, n, [key](uint32_t a, uint32_t b) { return key[a] < key[b]; }, pool);
    uint32_t me = out.count();
    out.nodes.resize(out.nodes.size() + 8);
    out.depth = std::max(out.depth, depth);
    uint32_t A, B = 0;
    if (n == 1) { node_box = boxes[idx[0]]; A = (fw::NODE_LEAF << 30) | idx[0]; }
    else if (n == 2) { node_box = box_union(boxes[idx[0]], boxes[idx[1]]); A = (fw::NODE_DOUBLE << 30) | idx[0]; B = idx[1]; }
    else {
        size_t half = n / 2;
        Box lb, rb;
        const uint32_t right = build_children(out, n, half, pool, [&](FlatBvh &into, size_t first, size_t count, Box &b) {
            bvh_build_rec(into, boxes, ce, idx + first, count, depth + 1, b, pool); }, lb, rb);
        node_box = box_union(lb, rb);
        A = right;
        B = (uint32_t)axis;     // split axis of this Branch (depth % 3): picks the near child during traversal
    }
    float *p = &out.nodes[(size_t)me * 8];
    p[0] = node_box.mn.x; p[1] = node_box.mn.y; p[2] = node_box.mn.z; p[3] = bits_f(A);
    p[4] = node_box.mx.x; p[5] = node_box.mx.y; p[6] = node_box.mx.z; p[7] = bits_f(B);
    return me;
}
Box bvh_build(FlatBvh &out, const std::vector<Box> &boxes, BuildPool *shared = nullptr) {
    std::vector<uint32_t> idx(boxes.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)i;
    BuildPool own(host_build_threads() - 1);
    BuildPool &pool = shared ? *shared : own;
    const Centers ce = centers_of(boxes, pool);
    Box root;
    bvh_build_rec(out, boxes, ce, idx.data(), idx.size(), 0, root, pool);
    return root;
}

// In-order rank of every item in the reference (median-split) tree: leaves appear left to right in DFS order.
std::vector<uint32_t> reference_ranks(const FlatBvh &ref, size_t n_items) {
    std::vector<uint32_t> rank(n_items, 0);
    uint32_t next = 0;
    for (uint32_t i = 0; i < ref.count(); i++) {
        uint32_t A, B; std::memcpy(&A, &ref.nodes[(size_t)i * 8 + 3], 4); std::memcpy(&B, &ref.nodes[(size_t)i * 8 + 7], 4);
        uint32_t kind = A >> 30;
        if (kind == fw::NODE_LEAF) rank[A & fw::NODE_MASK] = next++;
        else if (kind == fw::NODE_DOUBLE) { rank[A & fw::NODE_MASK] = next++; rank[B] = next++; }
    }
    return rank;
}

// The boxes of the WALKED trees are the items' own boxes grown by 2^-14 of their largest extent (round 4).  The walks only have to
// reach every item the reference's rule admits and the item test accepts (fw_kernels.hip: hit_aabb_entry; the rule itself is applied
// to every hit that counts: tri_gate_ok / obj_gate_ok).  A triangle test carries (max|d| / |d_kz|) ulps of the distance from the ray's
// origin to the triangle's far vertices — at most distance + extent — so a ray can "hit" a triangle it passes by that much: the part
// in proportion to the distance is what the walks' relaxed exit planes admit (2^-12), the part in proportion to the extent is this.
// How much: an item test's error SIDEWAYS, for a ray that runs along a face of the box, is not helped by relaxed exit planes and has to
// be in the box itself (part2 pixel 1049389, sample 106: a camera ray 17 units away grazes a sphere of radius 0.1 past the face of its
// own box, gpurun_out/r04j).  Every ray that is not on the exact list starts within far_r = 256 x the smallest item (DExact.far_r):
//   triangle: shear x 2^-24 x distance, shear < 2^10 (beyond: the exact list) -> 2^-14 far_r = 2^-6 of a typical triangle of the mesh;
//   sphere / cone / cylinder: the discriminant's rounding lets a ray that misses by 2^-24 L^2 / r still hit -> 2^-22 far_r^2 / size;
//   rectangles and boxes: their tests are exact in the plane; 2^-14 of the extent for the rounding of the slab test itself.
inline float box_extent(const Box &b) { const V3 e = b.mx - b.mn; return std::fmax(std::fabs(e.x), std::fmax(std::fabs(e.y), std::fabs(e.z))); }
inline Box grown_by(const Box &b, float g) {
    if (!(g > 0.f) || !std::isfinite(g)) return b;
    return Box{{b.mn.x - g, b.mn.y - g, b.mn.z - g}, {b.mx.x + g, b.mx.y + g, b.mx.z + g}};
}
inline Box grown(const Box &b) { return grown_by(b, std::ldexp(box_extent(b), -14)); }
// The walks' plane distances carry a rounding that scales with the COORDINATES, not with the box: fw_kernels.hip's wide_step computes
// fma(plane, 1/d, -o/d), and the rounding of -o/d moves the plane by up to 2^-24 |o|; a quantised node's (node origin - o) / d moves it
// by up to 2^-23 (|node origin| + |o|).  For small items far from the origin that passes the growth above (a triangle of 0.03 at
// x = 3e4: 2^-24 |o| = 1.8e-3, growth 2^-6 x 0.03 = 4.7e-4; tests/test_gpu_coordinates.py).  So a frame's walked boxes grow by at least
// 2^-21 M as well, M a bound on the coordinates, in that frame, of every point of the scene: for a ray whose origin lies within M
// (every ray that starts on the scene's geometry, and a camera inside the scene's range) that is 8x the fma form's rounding and 2x the
// quantised form's.  A camera farther out than the scene's own coordinates is not covered.  The world frame's M is the largest finite
// coordinate of the objects' boxes (for an object inside the far rule's cluster box: at most |far_c| + far_r, which bounds the origin of
// every unflagged ray that reaches it); a mesh's frame's M is reach_in_frames' bound (the scene mapped into it), at least its own box's.
inline float coord_max(const std::vector<Box> &bs) {
    float m = 0.f;
    for (const Box &b : bs)
        for (float c : {b.mn.x, b.mn.y, b.mn.z, b.mx.x, b.mx.y, b.mx.z})
            if (std::isfinite(c)) m = std::fmax(m, std::fabs(c));
    return m;
}

// item boxes := the box of the reference leaf node that holds the item (its own box for a Leaf, the union for a DoubleLeaf)
void leaf_node_boxes(const FlatBvh &ref, std::vector<Box> &boxes) {
    for (uint32_t i = 0; i < ref.count(); i++) {
        const float *nd = &ref.nodes[(size_t)i * 8];
        uint32_t A, B; std::memcpy(&A, nd + 3, 4); std::memcpy(&B, nd + 7, 4);
        if ((A >> 30) != fw::NODE_DOUBLE) continue;
        const Box nb{{nd[0], nd[1], nd[2]}, {nd[4], nd[5], nd[6]}};
        boxes[A & fw::NODE_MASK] = nb; boxes[B] = nb;
    }
}

// ---- traversal tree: binned-SAH top-down build, same node format (leaves of 1 or 2 items, DFS order).
// The reference's tree (bvh_build above) fixes WHICH hit wins ties (in-order rank); it does not have to be the
// tree that is walked.  SAH isolates large items near the root (part2's r=5000 fog sphere otherwise inflates
// every ancestor box along its spine) and splits on the axis that actually separates the items.
constexpr uint32_t SAH_MAX_DEPTH = 40;
inline float box_area(const Box &b) { V3 d = b.mx - b.mn; return 2.f * (d.x * d.y + d.y * d.z + d.z * d.x); }

uint32_t sah_build_rec(FlatBvh &out, const std::vector<Box> &boxes, const Centers &ce, uint32_t *idx, size_t n, uint32_t depth, Box &node_box, BuildPool &pool) {
    uint32_t me = out.count();
    out.nodes.resize(out.nodes.size() + 8);
    out.depth = std::max(out.depth, depth);
    uint32_t A, B = 0;
    if (n == 1) { node_box = boxes[idx[0]]; A = (fw::NODE_LEAF << 30) | idx[0]; }
    else if (n == 2) { node_box = box_union(boxes[idx[0]], boxes[idx[1]]); A = (fw::NODE_DOUBLE << 30) | idx[0]; B = idx[1]; }
    else {
        const Box EMPTY{{1e30f, 1e30f, 1e30f}, {-1e30f, -1e30f, -1e30f}};
        constexpr int NB = 16;
        // the passes over the node's items (the centroids' bounds, then the bins of the three axes) in parts on the free threads: unions
        // by fmin / fmax and counts are exact, so the merged bins are the sequential ones
        const int helpers = n >= PAR_PASS_MIN ? pool.take(15) : 0, parts = helpers + 1;
        Box cb = EMPTY;
        {
            std::vector<Box> pcb((size_t)parts, EMPTY);
            par_parts(n, parts, [&](size_t lo, size_t hi, int k) {
                Box b = EMPTY;
                for (size_t i = lo; i < hi; i++) { const uint32_t it = idx[i]; const V3 c{ce.c[0][it], ce.c[1][it], ce.c[2][it]}; b.mn = vmin(b.mn, c); b.mx = vmax(b.mx, c); }
                pcb[(size_t)k] = b; });
            for (const Box &b : pcb) { cb.mn = vmin(cb.mn, b.mn); cb.mx = vmax(cb.mx, b.mx); }
        }
        int best_axis = -1; size_t best_split = 0; float best_cost = 1e38f;
        if (depth < SAH_MAX_DEPTH) {
            struct Bins { Box bb[3][NB]; size_t bc[3][NB]; };
            std::vector<Bins> pb((size_t)parts);
            par_parts(n, parts, [&](size_t lo_i, size_t hi_i, int k) {
                Bins &bn = pb[(size_t)k];
                for (int axis = 0; axis < 3; axis++) for (int q = 0; q < NB; q++) { bn.bb[axis][q] = EMPTY; bn.bc[axis][q] = 0; }
                for (int axis = 0; axis < 3; axis++) {
                    const float lo = cb.mn[axis], ext = cb.mx[axis] - lo;
                    if (!(ext > 0.f)) continue;
                    const float *key = ce.c[axis].data();
                    for (size_t i = lo_i; i < hi_i; i++) {
                        const uint32_t it = idx[i];
                        const int q = std::min(NB - 1, std::max(0, (int)((key[it] - lo) / ext * NB)));
                        bn.bb[axis][q] = box_union(bn.bb[axis][q], boxes[it]); bn.bc[axis][q]++;
                    }
                } });
            for (int axis = 0; axis < 3; axis++) {
                float lo = cb.mn[axis], ext = cb.mx[axis] - lo;
                if (!(ext > 0.f)) continue;
                Box bb[NB]; size_t bc[NB];
                for (int k = 0; k < NB; k++) { bb[k] = EMPTY; bc[k] = 0; }
                for (const Bins &bn : pb) for (int k = 0; k < NB; k++) if (bn.bc[axis][k]) { bb[k] = box_union(bb[k], bn.bb[axis][k]); bc[k] += bn.bc[axis][k]; }
                float la[NB], ra[NB]; size_t lc[NB], rc[NB];
                Box acc = EMPTY; size_t cnt = 0;
                for (int k = 0; k < NB; k++) { if (bc[k]) acc = box_union(acc, bb[k]); cnt += bc[k]; la[k] = cnt ? box_area(acc) : 0.f; lc[k] = cnt; }
                acc = EMPTY; cnt = 0;
                for (int k = NB - 1; k >= 0; k--) { if (bc[k]) acc = box_union(acc, bb[k]); cnt += bc[k]; ra[k] = cnt ? box_area(acc) : 0.f; rc[k] = cnt; }
                for (int k = 0; k + 1 < NB; k++) {
                    if (lc[k] == 0 || rc[k + 1] == 0) continue;
                    float cost = la[k] * (float)lc[k] + ra[k + 1] * (float)rc[k + 1];
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_split = (size_t)k; }
                }
            }
        }
        pool.give(helpers);
        size_t half;
        int axis;
        if (best_axis >= 0) {
            axis = best_axis;
            float lo = cb.mn[axis], ext = cb.mx[axis] - lo;
            const float *key = ce.c[axis].data();
            auto mid = std::stable_partition(idx, idx + n, [&](uint32_t a) {
                int k = std::min(NB - 1, std::max(0, (int)((key[a] - lo) / ext * NB)));
                return (size_t)k <= best_split; });
            half = (size_t)(mid - idx);
        } else {   // all centroids coincide (or depth cap): median split keeps the tree balanced
            V3 e = cb.mx - cb.mn;
            axis = e.x >= e.y ? (e.x >= e.z ? 0 : 2) : (e.y >= e.z ? 1 : 2);
            const float *key = ce.c[axis].data();
            par_stable_sort(idx, n, [key](uint32_t a, uint32_t b) { return key[a] < key[b]; }, pool);
            half = n / 2;
        }
        if (half == 0 || half == n) half = n / 2;
        Box lb, rb;
        const uint32_t right = build_children(out, n, half, pool, [&](FlatBvh &into, size_t first, size_t count, Box &b) {
            sah_build_rec(into, boxes, ce, idx + first, count, depth + 1, b, pool); }, lb, rb);
        node_box = box_union(lb, rb);
        A = right;
        B = (uint32_t)axis;     // left child holds the smaller centroids along this axis
    }
    float *p = &out.nodes[(size_t)me * 8];
    p[0] = node_box.mn.x; p[1] = node_box.mn.y; p[2] = node_box.mn.z; p[3] = bits_f(A);
    p[4] = node_box.mx.x; p[5] = node_box.mx.y; p[6] = node_box.mx.z; p[7] = bits_f(B);
    return me;
}
void sah_build(FlatBvh &out, const std::vector<Box> &boxes, BuildPool *shared = nullptr) {
    std::vector<uint32_t> idx(boxes.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)i;
    BuildPool own(host_build_threads() - 1);
    BuildPool &pool = shared ? *shared : own;
    const Centers ce = centers_of(boxes, pool);
    Box root;
    sah_build_rec(out, boxes, ce, idx.data(), idx.size(), 0, root, pool);
}

// ---- where a tree is built.  fw_build.hip restates both builders on the device, level by level, with the same nodes as the result
// (tests/test_gpu_device_build.py); BUILD=host|device picks one, the default takes the device from BUILD_MIN items on: measured against 64
// host threads, the device loses at 20 k triangles (14 against 10 ms of scene creation) and wins from 200 k (50 against 80 ms; DESIGN.md §9.4,
// profiles/device_build.txt).  Every tree of a scene is built through build_tree.  device < 0: the host.  Errors come back as status codes.
constexpr size_t BUILD_MIN = 100000;
static_assert(sizeof(Box) == 24, "Box = 6 floats: fw::device_build_tree reads an array of them");
int build_tree(int device, fw::BuildTree kind, const std::vector<Box> &boxes, FlatBvh &out, BuildPool *pool, fw::DeviceBuildTimes *times) {
    const int where = options().build;
    if (device >= 0 && !boxes.empty() && (where == 1 || (where == -1 && boxes.size() >= BUILD_MIN))) {
        std::string msg;
        const int rc = fw::device_build_tree(device, kind, reinterpret_cast<const float *>(boxes.data()), (uint32_t)boxes.size(), out.nodes, out.depth, times, msg);
        return rc ? fail(rc, msg) : FW_OK;
    }
    if (kind == fw::BUILD_MEDIAN) {
        try { (void)bvh_build(out, boxes, pool); } catch (NanError &) { return fail(FW_ERR_NAN_BBOX, "Float comparison failed in BVH constructor"); }
    } else sah_build(out, boxes, pool);
    return FW_OK;
}

// ---- the tree as walked on the device: pair nodes (fw_device.h), converted from a FlatBvh.  A DoubleLeaf becomes a
// pair node over two single-item leaves, each with its own box.  `depth` = inner nodes on the longest root-to-leaf path
// = the most references a walk can have pushed.
struct PairBvh {
    std::vector<float> nodes;   // 16 floats per pair node
    uint32_t depth = 0;
    uint32_t count() const { return (uint32_t)(nodes.size() / 16); }
};
static uint32_t pair_convert_rec(const FlatBvh &src, uint32_t i, const std::vector<Box> &item_boxes, PairBvh &out, uint32_t base,
                                 uint32_t depth, Box &box) {
    const float *nd = &src.nodes[(size_t)i * 8];
    uint32_t A, B; std::memcpy(&A, nd + 3, 4); std::memcpy(&B, nd + 7, 4);
    const uint32_t kind = A >> 30;
    if (kind == fw::NODE_LEAF) { box = item_boxes[A & fw::NODE_MASK]; return fw::REF_LEAF | (A & fw::NODE_MASK); }
    const uint32_t me = out.count();
    out.nodes.resize(out.nodes.size() + 16, 0.f);
    out.depth = std::max(out.depth, depth + 1);
    uint32_t rl, rr; Box bl, br;
    if (kind == fw::NODE_DOUBLE) {
        rl = fw::REF_LEAF | (A & fw::NODE_MASK); bl = item_boxes[A & fw::NODE_MASK];
        rr = fw::REF_LEAF | B; br = item_boxes[B];
    } else {
        rl = pair_convert_rec(src, i + 1, item_boxes, out, base, depth + 1, bl);
        rr = pair_convert_rec(src, A & fw::NODE_MASK, item_boxes, out, base, depth + 1, br);
    }
    box = box_union(bl, br);       // (= the node's own box when `src` was built over item_boxes; the reference tree walked as it is — BVH=median — was built over the items' exact boxes)
    float *p = &out.nodes[(size_t)me * 16];
    p[0] = bl.mn.x; p[1] = bl.mn.y; p[2] = bl.mn.z; p[3] = bits_f(rl);
    p[4] = bl.mx.x; p[5] = bl.mx.y; p[6] = bl.mx.z; p[7] = bits_f(rr);
    p[8] = br.mn.x; p[9] = br.mn.y; p[10] = br.mn.z; p[12] = br.mx.x; p[13] = br.mx.y; p[14] = br.mx.z;
    return base + me;
}
// appends the converted tree to `out` (whose nodes already hold `base` = out.count() pair nodes of other trees) and returns its root reference
static uint32_t pair_convert(const FlatBvh &src, const std::vector<Box> &item_boxes, PairBvh &out) {
    Box root;
    PairBvh local;
    uint32_t base = out.count();
    uint32_t ref = pair_convert_rec(src, 0, item_boxes, local, base, 0, root);
    out.nodes.insert(out.nodes.end(), local.nodes.begin(), local.nodes.end());
    out.depth = std::max(out.depth, local.depth);
    return ref;
}
inline bool use_sah() { return !options().bvh_median; }

// ---- WIDE nodes (fw_device.h): the tree the LDS-resident walks step through since round 4 — four children per node, collapsed
// from the same binary tree the pair nodes come from (a child is opened, largest box first, until four are held; a DoubleLeaf
// opens into its two items with their own boxes).  One step decides four boxes for one stack operation and one trip round the
// walk's loop, and the tree has a third of the pair tree's nodes.  Two encodings of the same topology:
//   WIDE_F32 (112 B)  the children's boxes as they are, SoA by plane: the slab test is the pair walk's, an item is reached iff its
//                     own box passes aabb.rs:30-50 — bit for bit what the pair walk decides;
//   WIDE_Q8  (48 B)   boxes quantised to 8 bits per plane relative to the node (origin + q * 2^e per axis), rounded OUTWARD and
//                     checked here with the device's own dequantisation (one fma): a superset of the exact box under the same
//                     monotone slab arithmetic, so no item the exact boxes admit is ever culled.  For trees whose f32 nodes do
//                     not fit a CU's LDS (teapot.yml: 6 320 triangles = 236 KB as f32 nodes, 101 KB quantised).
struct WideBvh {
    std::vector<uint32_t> words;   // fw::WIDE_F32_DW or fw::WIDE_Q8_DW dwords per node
    int fmt = 0;
    uint32_t depth = 0;            // wide nodes on the longest root-to-leaf path
    uint32_t dw() const { return fmt == fw::WIDE_Q8 ? fw::WIDE_Q8_DW : fw::WIDE_F32_DW; }
    uint32_t count() const { return (uint32_t)(words.size() / dw()); }
};
struct WideChild { bool leaf; uint32_t id; Box box; };   // id: item, or node index in the BinTree
// The binary tree the wide nodes are collapsed from: the FlatBvh with a DoubleLeaf opened into a node over two single items, and the
// collapse chosen by dynamic programming over the surface-area cost (Ylitie, Karras, Laine 2017, section 4.1, for 4 slots): cost[k] =
// the cheapest way to hang the subtree into AT MOST k slots of a parent — as one wide node of its own (its box's area x the cost of
// a step, its children spread over four slots), or with its two children spread over the k slots directly.  Opening the child
// with the largest box until four are held (the first version) left a third of the slots empty: a node's small children stayed
// nodes of two leaves (suzanne: 458 nodes for 968 triangles, teapot 3 116 for 6 320: 150 KB quantised, too big for a CU's LDS).
struct BinNode { int left = -1, right = -1; uint32_t item = 0; Box box{}; float cost[5] = {0, 0, 0, 0, 0}; uint8_t split[5] = {0, 0, 0, 0, 0}; bool inherit[5] = {false, false, false, false, false}; };
constexpr float WIDE_COST_STEP = 1.0f, WIDE_COST_ITEM = 0.7f;     // one wide step (four boxes, a stack operation) against one item test
static int bin_build(const FlatBvh &src, uint32_t i, const std::vector<Box> &item_boxes, std::vector<BinNode> &t, float node_cost) {
    const float *nd = &src.nodes[(size_t)i * 8];
    uint32_t A, B; std::memcpy(&A, nd + 3, 4); std::memcpy(&B, nd + 7, 4);
    const uint32_t kind = A >> 30;
    auto leaf = [&](uint32_t item) { BinNode n; n.item = item; n.box = item_boxes[item]; const float c = box_area(n.box) * WIDE_COST_ITEM; for (int k = 1; k <= 4; k++) n.cost[k] = c; t.push_back(n); return (int)t.size() - 1; };
    if (kind == fw::NODE_LEAF) return leaf(A & fw::NODE_MASK);
    BinNode n;
    if (kind == fw::NODE_DOUBLE) { n.left = leaf(A & fw::NODE_MASK); n.right = leaf(B); }
    else { n.left = bin_build(src, i + 1, item_boxes, t, node_cost); n.right = bin_build(src, A & fw::NODE_MASK, item_boxes, t, node_cost); }
    const BinNode &l = t[n.left], &r = t[n.right];
    n.box = box_union(l.box, r.box);
    float dist[5] = {0, 0, 0, 0, 0};
    for (int k = 2; k <= 4; k++) {
        dist[k] = 3.0e38f;
        for (int j = 1; j < k; j++) { const float c = l.cost[j] + r.cost[k - j]; if (c < dist[k]) { dist[k] = c; n.split[k] = (uint8_t)j; } }
    }
    n.cost[1] = box_area(n.box) * WIDE_COST_STEP + node_cost + dist[4];
    for (int k = 2; k <= 4; k++) { n.inherit[k] = !(dist[k] < n.cost[k - 1]); n.cost[k] = n.inherit[k] ? n.cost[k - 1] : dist[k]; }
    t.push_back(n);
    return (int)t.size() - 1;
}
static void wide_place(const std::vector<BinNode> &t, int m, int k, std::vector<WideChild> &out);
static void wide_spread(const std::vector<BinNode> &t, int n, int k, std::vector<WideChild> &out) {     // n's two children over k slots
    const int j = t[n].split[k];
    wide_place(t, t[n].left, j, out);
    wide_place(t, t[n].right, k - j, out);
}
static void wide_place(const std::vector<BinNode> &t, int m, int k, std::vector<WideChild> &out) {      // subtree m into at most k slots
    if (t[m].left < 0) { out.push_back({true, t[m].item, t[m].box}); return; }
    while (k > 1 && t[m].inherit[k]) k--;
    if (k == 1) out.push_back({false, (uint32_t)m, t[m].box});
    else wide_spread(t, m, k, out);
}
inline uint32_t f_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
// one axis of a WIDE_Q8 node: exponent byte e (scale 2^(e-127)) and the children's quantised planes, rounded outward
static bool wide_quantise_axis(const float *lo, const float *hi, int n, float org, uint32_t &e_out, uint8_t *qlo, uint8_t *qhi) {
    float ext = 0.f;
    for (int c = 0; c < n; c++) { if (!(lo[c] >= org) || !(hi[c] >= lo[c]) || !std::isfinite(hi[c])) return false; ext = std::fmax(ext, hi[c] - org); }
    int e = 1;                                               // smallest scale with every plane <= 254 quanta from the origin (255 is kept for the rounding step)
    if (ext > 0.f) { int ex; std::frexp(ext / 254.f, &ex); e = std::max(1, std::min(254, ex + 127)); }
    if (org != 0.f) { int eo; std::frexp(std::fabs(org), &eo); e = std::max(e, std::min(254, eo + 127 - 22)); }   // a quantum the origin can see: 255 quanta must move it (a free slot's inverted box)
    for (; e <= 254; e++) {
        const float s = bits_f((uint32_t)e << 23);
        bool ok = true;
        for (int c = 0; c < n && ok; c++) {
            double ql = std::floor(((double)lo[c] - (double)org) / (double)s), qh = std::ceil(((double)hi[c] - (double)org) / (double)s);
            if (ql < 0) ql = 0;
            if (ql > 255 || qh > 255) { ok = false; break; }
            int a = (int)ql, b = (int)qh;
            while (a > 0 && std::fmaf((float)a, s, org) > lo[c]) a--;          // the device's own dequantisation: one fma
            while (b < 255 && std::fmaf((float)b, s, org) < hi[c]) b++;
            if (std::fmaf((float)a, s, org) > lo[c] || std::fmaf((float)b, s, org) < hi[c]) { ok = false; break; }
            qlo[c] = (uint8_t)a; qhi[c] = (uint8_t)b;
        }
        if (ok) { e_out = (uint32_t)e; return true; }
    }
    return false;
}
// returns the node's index in `out` (relative to `base` nodes of other trees already there), or 0xffffffff when the tree cannot be encoded
static uint32_t wide_build_rec(const std::vector<BinNode> &t, int bin, WideBvh &out, uint32_t base, uint32_t depth) {
    std::vector<WideChild> ch;
    wide_spread(t, bin, 4, ch);
    const uint32_t me = out.count(), dw = out.dw();
    out.words.resize(out.words.size() + dw, 0u);
    out.depth = std::max(out.depth, depth + 1);
    uint32_t refs[4];
    const int n = (int)ch.size();
    for (int c = 0; c < n; c++) {
        if (ch[c].leaf) { if (ch[c].id >= 0x7fffu) return 0xffffffffu; refs[c] = fw::W_LEAF | ch[c].id; }
        else {
            const uint32_t r = wide_build_rec(t, (int)ch[c].id, out, base, depth + 1);
            if (r == 0xffffffffu || base + r >= 0x8000u) return 0xffffffffu;
            refs[c] = base + r;
        }
    }
    for (int c = n; c < 4; c++) refs[c] = refs[0];           // a free slot repeats child 0 behind a box no finite ray can hit
    uint32_t *w = &out.words[(size_t)me * dw];
    if (out.fmt == fw::WIDE_F32) {                            // planes: lo.x[4] lo.y[4] lo.z[4] hi.x[4] hi.y[4] hi.z[4], then the refs
        const float INF = std::numeric_limits<float>::infinity();
        for (int c = 0; c < 4; c++) {
            const bool on = c < n;
            const Box &b = ch[on ? c : 0].box;
            w[0 + c] = f_bits(on ? b.mn.x : INF); w[4 + c] = f_bits(on ? b.mn.y : INF); w[8 + c] = f_bits(on ? b.mn.z : INF);
            w[12 + c] = f_bits(on ? b.mx.x : -INF); w[16 + c] = f_bits(on ? b.mx.y : -INF); w[20 + c] = f_bits(on ? b.mx.z : -INF);
        }
        w[24] = refs[0] | (refs[1] << 16); w[25] = refs[2] | (refs[3] << 16); w[26] = w[27] = 0u;
    } else {
        V3 org = ch[0].box.mn;
        for (int c = 1; c < n; c++) org = vmin(org, ch[c].box.mn);
        uint32_t e[3]; uint8_t ql[3][4], qh[3][4];
        for (int a = 0; a < 3; a++) {
            float lo[4], hi[4];
            for (int c = 0; c < n; c++) { lo[c] = ch[c].box.mn[a]; hi[c] = ch[c].box.mx[a]; }
            if (!wide_quantise_axis(lo, hi, n, org[a], e[a], ql[a], qh[a])) return 0xffffffffu;
            for (int c = n; c < 4; c++) { ql[a][c] = 255; qh[a][c] = 0; }
        }
        w[0] = f_bits(org.x); w[1] = f_bits(org.y); w[2] = f_bits(org.z); w[3] = e[0] | (e[1] << 8) | (e[2] << 16);
        for (int a = 0; a < 3; a++) {
            w[4 + a] = (uint32_t)ql[a][0] | ((uint32_t)ql[a][1] << 8) | ((uint32_t)ql[a][2] << 16) | ((uint32_t)ql[a][3] << 24);
            w[8 + a] = (uint32_t)qh[a][0] | ((uint32_t)qh[a][1] << 8) | ((uint32_t)qh[a][2] << 16) | ((uint32_t)qh[a][3] << 24);
        }
        w[7] = refs[0] | (refs[1] << 16); w[11] = refs[2] | (refs[3] << 16);
    }
    return me;
}
// appends the wide form of `src` to `out`; returns its root reference (a node, or W_LEAF | item for a one-item tree), 0xffffffff on failure
static uint32_t wide_convert(const FlatBvh &src, const std::vector<Box> &item_boxes, WideBvh &out) {
    uint32_t A; std::memcpy(&A, &src.nodes[3], 4);
    if ((A >> 30) == fw::NODE_LEAF) return (A & fw::NODE_MASK) < 0x7fffu ? (fw::W_LEAF | (A & fw::NODE_MASK)) : 0xffffffffu;
    if (item_boxes.size() >= 0x7fffu) return 0xffffffffu;          // 15-bit item references: not encodable (found only at the last leaf otherwise: 90 ms for a million triangles)
    WideBvh local; local.fmt = out.fmt;
    const uint32_t base = out.count();
    std::vector<BinNode> bin;
    bin.reserve(2 * item_boxes.size());
    // a node also costs LDS: a constant per node (WIDE_COST_NODE of the root's area) makes the collapse prefer full nodes where the
    // surface-area terms are indifferent (teapot: 2 453 -> FILL nodes, which is what lets sixteen waves' stacks fit beside them)
    const float *rn = &src.nodes[0];
    const float node_cost = (float)options().wide_node_cost * box_area(Box{{rn[0], rn[1], rn[2]}, {rn[4], rn[5], rn[6]}});
    const int root = bin_build(src, 0, item_boxes, bin, node_cost);
    const uint32_t r = wide_build_rec(bin, root, local, base, 0);
    if (r == 0xffffffffu) return r;
    out.words.insert(out.words.end(), local.words.begin(), local.words.end());
    out.depth = std::max(out.depth, local.depth);
    return base + r;
}
// Every invariant the walks rely on, checked on the finished tree (fw_selftest_wide_bvh; the CPU test suite runs it on the
// reference's meshes): each item is the leaf of exactly one slot, a child's box as the DEVICE decodes it contains the exact box,
// node references point forward, free slots cannot be hit.  Returns the number of violations.
static uint32_t wide_check(const WideBvh &t, uint32_t root, const std::vector<Box> &item_boxes, uint32_t stats[4]) {
    uint32_t bad = 0, leaves = 0, free_slots = 0;
    std::vector<uint32_t> seen(item_boxes.size(), 0);
    if (root & fw::W_LEAF) { stats[0] = 0; stats[1] = 1; stats[2] = 0; stats[3] = 0; return (root & 0x7fffu) == 0 && item_boxes.size() == 1 ? 0u : 1u; }
    struct Rec { uint32_t node; Box bound; bool has_bound; };
    std::vector<Rec> todo{{root, Box{}, false}};
    std::vector<uint32_t> visited(t.count(), 0);
    auto subtree_box = [&](auto &&self, uint32_t ref) -> Box {
        if (ref & fw::W_LEAF) return item_boxes[ref & 0x7fffu];
        const uint32_t *w = &t.words[(size_t)ref * t.dw()];
        const uint32_t r[4] = {(t.fmt == fw::WIDE_F32 ? w[24] : w[7]) & 0xffffu, (t.fmt == fw::WIDE_F32 ? w[24] : w[7]) >> 16,
                               (t.fmt == fw::WIDE_F32 ? w[25] : w[11]) & 0xffffu, (t.fmt == fw::WIDE_F32 ? w[25] : w[11]) >> 16};
        Box b = self(self, r[0]);
        for (int c = 1; c < 4; c++) if (r[c] != r[0]) b = box_union(b, self(self, r[c]));
        return b;
    };
    while (!todo.empty()) {
        const Rec rec = todo.back(); todo.pop_back();
        if (rec.node >= t.count() || visited[rec.node]++) { bad++; continue; }
        const uint32_t *w = &t.words[(size_t)rec.node * t.dw()];
        uint32_t r[4]; Box dec[4];
        if (t.fmt == fw::WIDE_F32) {
            r[0] = w[24] & 0xffffu; r[1] = w[24] >> 16; r[2] = w[25] & 0xffffu; r[3] = w[25] >> 16;
            for (int c = 0; c < 4; c++) dec[c] = Box{{bits_f(w[c]), bits_f(w[4 + c]), bits_f(w[8 + c])}, {bits_f(w[12 + c]), bits_f(w[16 + c]), bits_f(w[20 + c])}};
        } else {
            r[0] = w[7] & 0xffffu; r[1] = w[7] >> 16; r[2] = w[11] & 0xffffu; r[3] = w[11] >> 16;
            const float org[3] = {bits_f(w[0]), bits_f(w[1]), bits_f(w[2])};
            for (int c = 0; c < 4; c++) {
                float lo[3], hi[3];
                for (int a = 0; a < 3; a++) {
                    const float s = bits_f(((w[3] >> (8 * a)) & 0xffu) << 23);
                    lo[a] = std::fmaf((float)((w[4 + a] >> (8 * c)) & 0xffu), s, org[a]);
                    hi[a] = std::fmaf((float)((w[8 + a] >> (8 * c)) & 0xffu), s, org[a]);
                }
                dec[c] = Box{{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
            }
        }
        for (int c = 0; c < 4; c++) {
            const bool is_free = c > 0 && r[c] == r[0];
            if (is_free) { free_slots++; if (!(dec[c].mn.x > dec[c].mx.x && dec[c].mn.y > dec[c].mx.y && dec[c].mn.z > dec[c].mx.z)) bad++; continue; }
            const Box exact = subtree_box(subtree_box, r[c]);
            if (!(dec[c].mn.x <= exact.mn.x && dec[c].mn.y <= exact.mn.y && dec[c].mn.z <= exact.mn.z &&
                  dec[c].mx.x >= exact.mx.x && dec[c].mx.y >= exact.mx.y && dec[c].mx.z >= exact.mx.z)) bad++;
            if (t.fmt == fw::WIDE_F32 && (r[c] & fw::W_LEAF) && std::memcmp(&dec[c], &item_boxes[r[c] & 0x7fffu], sizeof(Box)) != 0) bad++;   // an item's own box, bit for bit
            if (r[c] & fw::W_LEAF) { const uint32_t it = r[c] & 0x7fffu; if (it >= seen.size() || seen[it]++) bad++; leaves++; }
            else { if (r[c] <= rec.node) bad++; todo.push_back({r[c], Box{}, false}); }
        }
    }
    for (uint32_t s : seen) if (s != 1) bad++;
    for (uint32_t v : visited) if (v != 1) bad++;
    stats[0] = t.count(); stats[1] = leaves; stats[2] = free_slots; stats[3] = t.depth;
    return bad;
}

// ---- device allocations owned by a scene / workspace ----------------------------------------------------
struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    int alloc(size_t n) {
        if (n <= bytes && p) return FW_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if (n == 0) return FW_OK;
        HIPCHK(hipMalloc(&p, n));
        bytes = n;
        return FW_OK;
    }
    int upload(const void *src, size_t n) {
        int rc = alloc(n ? n : 16);
        if (rc) return rc;
        if (n) {   // async copy + explicit wait: the blocking hipMemcpy of pageable memory showed 20-30 ms stalls
            HIPCHK(hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, nullptr));
            HIPCHK(hipStreamSynchronize(nullptr));
        }
        return FW_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};


// Per-device wavefront workspace: the path pools, accumulators and events.  It is the library's only global state
// (created lazily, kept until fw_release_workspace or process exit): a one-shot `Renderer::render(scene)` would
// otherwise hipMalloc/hipFree tens of GB per call, which costs from 8 ms to seconds (fresh pages are cleared).
// Optionally (FIREWORK_STREAMS=n) up to MAX_LANES batches are in flight on their own streams, each with its own
// path pool, so that one batch's k_extend (VALU-bound) overlaps another's k_shade (HBM-bound).  Results do not
// depend on n (batches are accumulated in order).  Default 1: the measured gain is ~3 %.
struct Workspace {
    static constexpr int MAX_LANES = 4;
    // exact_slots: the two slot lists of the exact walk (DExact.slots) + their counters behind them
    // A lane's buffers are slices of ONE device allocation per workspace (`arena`, laid out per call by render_impl): with a DevBuf
    // each, a call that needed other sizes than the last one — one batch in flight after two, no parked rays after some — freed
    // and allocated two dozen multi-GB buffers, 2 s in the caller's timed region (profiles/r03z_oneshot_trace.txt: the first
    // volume frame after suzanne).  The arena only grows, in steps of 1 GiB.
    struct Lane { void *ray_a[2] = {nullptr, nullptr}, *ray_b[2] = {nullptr, nullptr}, *state[2] = {nullptr, nullptr}, *hits = nullptr, *sample_rad = nullptr,
                       *wcount = nullptr, *park_a = nullptr, *park_b = nullptr, *park_m = nullptr, *pcount = nullptr, *dep_bits = nullptr, *exact_slots = nullptr, *atten = nullptr,
                       *rays = nullptr,   // fw_render_rays with host rays: the batch's rays, copied in through ray_host
                       // light sampling (fw::DShadow): the shadow queue (ray, pending + home, light object, hit record, counts), p_b of the two path queues, nee
                       *s_ray_a = nullptr, *s_ray_b = nullptr, *s_state = nullptr, *s_obj = nullptr, *s_hits = nullptr, *s_wcount = nullptr, *pb[2] = {nullptr, nullptr}, *nee = nullptr;
                  hipStream_t stream = nullptr;
                  std::vector<hipEvent_t> events; };
    DevBuf arena;
    std::mutex mu;                        // one fw_render at a time per device
    Lane lanes[MAX_LANES];
    DevBuf accum, totals, pixel_ids, out_rgb8, out_gamma, out_linear;
    DevBuf scene_cache;                   // the last destroyed scene's allocation, reused by the next fw_scene_create
    std::vector<hipEvent_t> events;       // [0] frame start, [1] frame stop, [2] fork, [3..] per-batch "accumulated" events
    hipEvent_t ev_d2h = nullptr;          // after the device -> host copies of the outputs
    // GRAPH: the launches of one frame between fork and join, captured the second time the same frame is asked for and replayed from then on.
    // `key` is a hash of every by-value kernel argument struct of the frame (camera, frame, queue, launch configuration, scene) and of
    // the buffers they do not name: anything that changes what a launch would be changes it, and a changed key is only ever a miss.
    struct FrameGraph { uint64_t key = 0, seen = 0; hipGraphExec_t exec = nullptr; hipStream_t origin = nullptr; bool broken = false; fw::DFrame fr_after{};
                        fw::KernelLog kernels{}; } fg;      // kernels: what the launchers recorded while `exec` was captured (a replay runs no launcher)
    fw::KernelLog kernels{};              // the walk and shade kernels the last call on this device launched (fw_debug_kernels); under mu
    std::vector<hipEvent_t> phase_events; // PHASE_LOCK: [lane-in-group][segment] "this batch's extend of the segment has finished"
    DevBuf tile_ids; uint32_t tile_w = 0, tile_h = 0;   // the library's own 16x16-tile pixel order of a (tile_w x tile_h) frame
    // fw_render_adaptive: whole-frame sums and squares, the two id lists the rounds alternate between, the survivor mask, per-block
    // counts (+ the survivor count behind them), its own start / stop events and a pinned word for the survivor count
    DevBuf ad_accum, ad_moments, ad_ids[2], ad_mask, ad_counts;
    hipEvent_t ad_ev[2] = {nullptr, nullptr};
    DevBuf view_ids, view_cams;           // fw_render_views: a view group's repeated pixel table and its cameras (rewritten by every call)
    // fw_render_rays: the key table, the error word of the invalid-ray check, the fixed rays of a host caller, and the pinned staging
    // host rays pass through (one slab per lane)
    DevBuf ray_keys, ray_err, ray_fixed;
    void *ray_host = nullptr; size_t ray_host_bytes = 0;
    uint32_t *ad_count_host = nullptr;
    void *staging = nullptr; size_t staging_bytes = 0;  // pinned host memory the scene blob is assembled in (k_upload reads it)
    void *host_out = nullptr; size_t host_out_bytes = 0; // pinned host memory the counters and output frames are copied into
    hipEvent_t ev_upload = nullptr;       // after the latest scene upload on this device: renders wait for it in stream order
    hipStream_t upload_stream = nullptr;  // the upload kernel's own non-blocking stream: a launch on the legacy NULL stream would
                                          // synchronise with every blocking stream of the process (torch's default stream included)
    bool inited = false;                  // init_device_locked has run on this device (fw_init, or the first call that needed the device)
    void release() {
        inited = false;
        if (ev_d2h) { (void)hipEventDestroy(ev_d2h); ev_d2h = nullptr; }
        if (fg.exec) { (void)hipGraphExecDestroy(fg.exec); fg.exec = nullptr; } if (fg.origin) { (void)hipStreamDestroy(fg.origin); fg.origin = nullptr; } fg.key = fg.seen = 0; fg.broken = false;
        if (ev_upload) { (void)hipEventSynchronize(ev_upload); (void)hipEventDestroy(ev_upload); ev_upload = nullptr; }
        if (upload_stream) { (void)hipStreamDestroy(upload_stream); upload_stream = nullptr; }
        if (staging) { (void)hipHostFree(staging); staging = nullptr; staging_bytes = 0; }
        if (host_out) { (void)hipHostFree(host_out); host_out = nullptr; host_out_bytes = 0; }
        tile_ids.release(); tile_w = tile_h = 0;
        for (DevBuf *b : {&ad_accum, &ad_moments, &ad_ids[0], &ad_ids[1], &ad_mask, &ad_counts, &view_ids, &view_cams, &ray_keys, &ray_err, &ray_fixed}) b->release();
        if (ray_host) { (void)hipHostFree(ray_host); ray_host = nullptr; ray_host_bytes = 0; }
        for (hipEvent_t &e : ad_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (ad_count_host) { (void)hipHostFree(ad_count_host); ad_count_host = nullptr; }
        for (DevBuf *b : {&accum, &totals, &pixel_ids, &out_rgb8, &out_gamma, &out_linear, &scene_cache, &arena}) b->release();
        for (Lane &l : lanes) {
            for (hipEvent_t e : l.events) (void)hipEventDestroy(e);
            l.events.clear();
            if (l.stream) (void)hipStreamDestroy(l.stream);
            l.stream = nullptr;
        }
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        events.clear();
        for (hipEvent_t e : phase_events) (void)hipEventDestroy(e);
        phase_events.clear();
    }
};
constexpr int MAX_DEVICES = 64;
Workspace *workspace_for(int device) {
    static Workspace *table[MAX_DEVICES] = {};
    static std::mutex table_mu;
    if (device < 0 || device >= MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> g(table_mu);
    if (!table[device]) table[device] = new (std::nothrow) Workspace();   // intentionally never deleted (process lifetime)
    return table[device];
}

// hipGetDeviceProperties costs up to ~25 ms per call: ask once per device
int device_cus(int device) {
    static int cu_cache[MAX_DEVICES] = {};
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (device < 0 || device >= MAX_DEVICES) return 256;
    if (cu_cache[device] == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) return -1;
        cu_cache[device] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return cu_cache[device];
}

// ---- initialisation (round 5: fw_init).  A process's first call pays for things that are no part of any frame: the HIP context, the
// device query, the load of this library's code objects (its first kernel launch), every kernel's first resolution, the pinned
// staging buffer, the streams — 150-180 ms of the 213 ms of a cold cornell frame (profiles/r03z_oneshot_trace.txt) — and, where a
// big frame follows, the path arena, whose hipMalloc takes 0.4 ms on a device whose memory is clean and 0.2-1.4 s where the driver
// has pages to clear (profiles/r04z_bench.json).  Round 4 did all of it in a static initialiser, so that merely loading the library
// created a context and took 64 GiB on LOCAL_RANK's device.  Now LOADING THE LIBRARY MAKES NO HIP CALL: the host calls
// fw_init(device, arena_bytes) where it wants the cost (the CLI and bench.py do, before their timed regions), and a host that never
// does gets the same initialisation — without an arena — from its first fw_scene_create / fw_render on that device.
// Caller holds ws->mu and has made `dev` current.
int init_device_locked(Workspace *ws, int dev) {
    if (ws->inited) return FW_OK;
    if (device_cus(dev) <= 0) return fail(FW_ERR_HIP, "hipGetDeviceProperties failed");
    if (!ws->staging) { HIPCHK(hipHostMalloc(&ws->staging, 1 << 20, hipHostMallocDefault)); ws->staging_bytes = 1 << 20; }
    if (!ws->upload_stream) HIPCHK(hipStreamCreateWithFlags(&ws->upload_stream, hipStreamNonBlocking));
    if (!ws->ev_upload) HIPCHK(hipEventCreateWithFlags(&ws->ev_upload, hipEventDisableTiming));
    for (int l = 0; l < 2; l++) if (!ws->lanes[l].stream) HIPCHK(hipStreamCreateWithFlags(&ws->lanes[l].stream, hipStreamNonBlocking));
    void *tmp = nullptr;
    HIPCHK(hipMalloc(&tmp, 256));
    std::memset(ws->staging, 0, 256);
    fw::launch_upload(ws->upload_stream, ws->staging, tmp, 256);          // any launch loads the code objects of the whole library on this device
    fw::preload_kernels();                                                // ... and every kernel's first launch resolves it: 60 ms of a first frame's enqueue (gpurun_out/r04j)
    (void)hipEventRecord(ws->ev_upload, ws->upload_stream);
    const hipError_t e = hipStreamSynchronize(ws->upload_stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(FW_ERR_HIP, std::string("first launch failed: ") + hipGetErrorString(e)); }
    (void)hipGetLastError();
    ws->inited = true;
    return FW_OK;
}
// The arena grows by allocating the new one FIRST and freeing the old one on a background thread: hipFree of a 35 GB arena took 2.4 s of
// the caller's time (gpurun_out/r04j/oneshot.txt) while the allocation itself is lazy.  Only when both do not fit is the old one freed
// in line.  Caller holds ws->mu; no render of this workspace is in flight (fw_render returns after its stream has drained).
int arena_reserve_locked(Workspace *ws, int dev, size_t want) {
    if (want <= ws->arena.bytes && ws->arena.p) return FW_OK;
    void *old_p = ws->arena.p;
    void *np = nullptr;
    hipError_t e = hipMalloc(&np, want);
    if (e != hipSuccess && old_p) {         // no room for both
        (void)hipGetLastError();
        (void)hipFree(old_p); old_p = nullptr; ws->arena.p = nullptr; ws->arena.bytes = 0;
        e = hipMalloc(&np, want);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); ws->arena.p = old_p; if (!old_p) ws->arena.bytes = 0; return fail(FW_ERR_OOM, "path arena allocation failed: " + std::to_string(want >> 20) + " MiB"); }
    ws->arena.p = np; ws->arena.bytes = want;
    if (old_p) std::thread([old_p, dev] { if (hipSetDevice(dev) == hipSuccess) (void)hipFree(old_p); }).detach();
    return FW_OK;
}
size_t default_arena_bytes(const Workspace *ws) {      // what fw_init(device, 0) reserves: every default-budget frame of the BASELINE configs fits (the largest needs 52 GB)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return std::min<size_t>((size_t)64 << 30, (free_b + ws->arena.bytes) / 3) & ~(((size_t)1 << 30) - 1);
}
// the pinned staging buffer holds at least `total` bytes and no upload still reads it.  Caller holds ws->mu.
int staging_reserve_locked(Workspace *ws, size_t total) {
    (void)hipEventSynchronize(ws->ev_upload);          // the previous upload has read the staging buffer (long done)
    if (ws->staging_bytes >= total) return FW_OK;
    if (ws->staging) (void)hipHostFree(ws->staging);
    ws->staging = nullptr; ws->staging_bytes = 0;
    const size_t want = std::max<size_t>(total + total / 4, 1 << 20);
    if (hipHostMalloc(&ws->staging, want, hipHostMallocDefault) != hipSuccess) return fail(FW_ERR_OOM, "pinned staging allocation failed");
    ws->staging_bytes = want;
    return FW_OK;
}

struct ShapeParams { float q3[4] = {0, 0, 0, 0}, q4[4] = {0, 0, 0, 0}; uint32_t kind = 0, flags = 0, aux0 = 0, aux1 = 0; Box box{};
                     uint32_t wroot_f32 = 0xffffffffu, wroot_q8 = 0xffffffffu;   // meshes: root reference of the wide tree in either encoding
                     uint32_t ref_root = 0xffffffffu, n_tris = 0;   // meshes: first node of the reference tree in Flattener::ref_blas
                     Box true_box{}; };   // OF_GATE shapes: a box that really encloses the geometry (object space)

// What fw_scene_create keeps on the host for fw_scene_update: the small fields of the description it was made from
// (to check a new one against: objects' shapes, the shapes, materials, textures and environment without the arrays they point to),
// the parameters of every shape an object uses (a mesh's: roots, triangle count, boxes — so that an update never flattens it again),
// each shape's largest coordinate (reach_in_frames) and the reach each mesh's walked trees were built with.
struct SceneKeep {
    std::vector<int32_t> obj_shape;
    std::vector<fw_shape> shapes;
    std::vector<fw_material> materials;
    std::vector<fw_texture> textures;
    fw_environment env{};
    std::vector<ShapeParams> sp;         // per shape index (those the objects use, media with their inner shape's)
    std::vector<float> ext, reach;       // per shape index
};

} // namespace

// ---- every emitter (FW_FLAG_ALL_EMITTERS): the entries of a description, object by object (scene_emitters) ----------------
// obj, shape kind, its entries [first, first + count); pre[k]: entry k's weight (area x power) — for a mesh the object's power, the areas of
// its triangles come from the device's copy of them (fw::launch_emitter_weights)
// shape, pos, rot, power: the object's shape index, placement (rotor_rows' rows) and emitter_power, which the world-space records of §9zc read
struct EmitterObj { uint32_t obj, kind, count; uint64_t first; float pre[6]; int32_t shape; float pos[3]; float rot[3][3]; double power; };

struct fw_scene {
    int device = 0;
    int n_cus = 256;
    fw::DScene d{};
    DevBuf data;   // every scene array in one allocation (sections 256-byte aligned)
    uint32_t tlas_nodes = 0, blas_nodes = 0, tlas_depth = 0, blas_depth = 0, n_mat = 0, n_tex = 0;
    uint32_t blas_pair_nodes = 0, tlas_pair_nodes = 0, max_tris = 0, n_tris = 0;
    uint32_t n_defer = 0;
    uint32_t chain_bits = 0;                // != 0: the scene's paths can carry their material ids instead of a running product (DFrame.chain_bits)
    int wblas_fmt = 0, wtlas_fmt = 0;       // fw::WIDE_*: the encoding of the wide trees uploaded with this scene (0: none)
    uint32_t wblas_nodes = 0, wtlas_nodes = 0, wblas_depth = 0, wtlas_depth = 0;
    bool has_expensive = false;   // some material is a dielectric or carries a non-constant texture, or the environment is an HDR map (k_shade's list)
    bool simple_shapes = false;   // every object is a sphere, an axis-aligned rect or a Rect3d (no medium, mesh, cone, cylinder, disk)
    bool simple_set = false;      // ... or a medium around a sphere (LaunchCfg.simple_set)
    bool simple_but_meshes = false;   // every object is a sphere, a rect, a Rect3d or a TriangleMesh (LaunchCfg.simple_but_meshes)
    bool hdr_env = false;
    fw::DExact ex{};              // flag rule of the exact walk (bits pointer is per render)
    uint32_t ref_tlas_depth = 0, ref_blas_depth = 0;
    SceneKeep keep;               // fw_scene_update's host copy of the description and the per-shape parameters
    DevBuf obj_data;              // the object-level sections once an update has written them (data's own copies are then unused)
    size_t blob_bytes = 0;        // bytes of the creation's upload
    double ms_objects = 0, ms_objects_dev = 0;   // the last object-level build: host wall time, device tree builds (FIREWORK_TRACE)
    DevBuf lights;                // the sampled lights' object indices (fw::DLights.obj; FW_FLAG_LIGHT_SAMPLING)
    uint32_t n_lights = 0;
    std::vector<float> light_recs;   // the same lights as fw_selftest_lights' records (fw_scene_area_lights), and their device copy (k_area_rays)
    DevBuf area_recs;
    bool ls_vertices = false;     // some material is Lambertian, Isotropic or Ggx: a vertex that samples lights can occur
    bool has_ggx = false;         // some material is a GgxMat: the frame launches the k_shade_gx kernels
    // the HDR map's sampling table (fw::DEnvDist: cdf_m, cdf_c, dens; FW_FLAG_ENV_SAMPLING), built on the device by the first
    // render that needs it and kept for the scene's life (fw_scene_update never changes the environment)
    DevBuf env_dist;
    int env_state = 0;            // 0: not built; 1: built, positive total weight (the map is a sampled light); 2: built, nothing to sample
    double env_build_ms = 0;
    // every emitter (FW_FLAG_ALL_EMITTERS): the entry list from the description; the table (fw::DEmitters: tab, ent, first)
    // built by the first render that needs it and kept for the scene's life (fw_scene_update moves objects, which changes no entry's weight)
    std::vector<EmitterObj> emit_objs;
    uint64_t n_entries = 0;
    DevBuf emitters;
    int emit_state = 0;           // 0: not built; 1: built, some entry of positive weight; 2: built, nothing to sample
    uint32_t emit_cols = 0;       // the table's columns (entries of positive weight)
    size_t emit_ent_off = 0, emit_first_off = 0;
    double emit_build_ms = 0;
    // every emitter at surface points (fw_scene_emitters, fw_bake_emitters, FW_GATHER_NO_EMITTERS): the entries' world-space
    // records, their (object, prim) codes, their CDF and the ascending objects that have entries, built by the first call that needs
    // them (es_state 0 -> 1) and again after every fw_scene_update, which resets es_state; es_dev: one allocation, records | cdf | codes | objects
    std::vector<float> es_rec;
    std::vector<uint32_t> es_codes, es_objs;
    std::vector<double> es_cdf;
    double es_total = 0;          // the weights' float64 sum: 0 = no emitters
    DevBuf es_dev;
    int es_state = 0;
    // point, spot and directional lights (fw_scene_set_lights): fw::DDeltaLights.rec, three float4 per light, in an allocation
    // of the scene's own that fw_scene_update leaves alone
    DevBuf dlights;
    uint32_t n_dlights = 0;
    ~fw_scene() {
        dlights.release();
        data.release();
        obj_data.release();
        lights.release();
        area_recs.release();
        env_dist.release();
        emitters.release();
        es_dev.release();
    }
};

// A bound on the coordinates of every point of the scene in the frame of each shape's objects (coord_max), from the description alone —
// the meshes' walked trees are built before the objects' world boxes exist.  A shape's points lie within E of its frame's origin, E its
// largest finite coordinate (a medium: its boundary's); an object's within |position| + E x (rotated: sqrt 3) in the world; a world point
// x within (|x| + |position|) x (rotated: sqrt 3) in an object's frame.  max-norms throughout.
static inline float finite_abs(float v) { return std::isfinite(v) ? std::fabs(v) : 0.f; }
static std::vector<float> shape_extents(const fw_scene_desc *d) {      // E per shape (the part of reach_in_frames that reads the vertices)
    auto fin = finite_abs;
    std::vector<float> ext(d->n_shapes, 0.f);
    for (uint32_t i = 0; i < d->n_shapes; i++) {
        const fw_shape &h = d->shapes[i];
        float m = 0.f;
        for (float v : {h.radius, h.height, h.inner_radius, h.a_min, h.a_max, h.b_min, h.b_max, h.k}) m = std::fmax(m, fin(v));
        for (float v : {h.pos.x + h.size.x, h.pos.y + h.size.y, h.pos.z + h.size.z, h.pos.x, h.pos.y, h.pos.z}) m = std::fmax(m, fin(v));
        if (h.kind == FW_SHAPE_TRIANGLE_MESH && h.verts)
            for (size_t k = 0; k < (size_t)h.n_verts * 3; k++) m = std::fmax(m, fin(h.verts[k]));
        ext[i] = m;
    }
    return ext;
}
static std::vector<float> reach_in_frames(const fw_scene_desc *d, const std::vector<float> &ext) {
    auto fin = finite_abs;
    std::vector<float> reach(d->n_shapes, 0.f);
    auto inner = [&](int32_t si) {
        const fw_shape &h = d->shapes[si];
        return (h.kind == FW_SHAPE_CONSTANT_MEDIUM && h.inner >= 0 && (uint32_t)h.inner < d->n_shapes) ? h.inner : si;
    };
    auto rotated = [](const fw_object &o) { return !(o.rotation.s == 1.f && o.rotation.xy == 0.f && o.rotation.xz == 0.f && o.rotation.yz == 0.f); };
    auto pos_max = [&](const fw_object &o) { return std::fmax(fin(o.position.x), std::fmax(fin(o.position.y), fin(o.position.z))); };
    float world = 0.f;
    for (uint32_t i = 0; i < d->n_objects; i++) {
        const fw_object &o = d->objects[i];
        if (o.shape < 0 || (uint32_t)o.shape >= d->n_shapes) continue;
        world = std::fmax(world, pos_max(o) + (rotated(o) ? 1.7321f : 1.f) * ext[inner(o.shape)]);
    }
    for (uint32_t i = 0; i < d->n_objects; i++) {
        const fw_object &o = d->objects[i];
        if (o.shape < 0 || (uint32_t)o.shape >= d->n_shapes) continue;
        const int32_t si = inner(o.shape);
        reach[si] = std::fmax(reach[si], (rotated(o) ? 1.7321f : 1.f) * (world + pos_max(o)));
    }
    return reach;
}

namespace {

struct Flattener {
    const fw_scene_desc *d;
    std::vector<float> tri, tri_attr;     // 12 floats per triangle each
    std::vector<float> tri_gate;          // 8 floats per triangle: the box of its leaf node in the REFERENCE tree of its mesh (own box, or a DoubleLeaf's union)
    std::vector<uint32_t> tri_rank;       // in-order rank of each triangle in the reference tree of its mesh
    bool any_attr = false;
    PairBvh blas;                 // all meshes' trees, as walked on the device
    std::vector<float> ref_blas;  // all meshes' REFERENCE trees (FlatBvh nodes, 8 floats each; child indices relative to the mesh's first node)
    uint32_t ref_blas_depth = 0;
    uint32_t blas_depth = 0, ref_blas_nodes = 0, max_tris = 0;
    WideBvh wblas_f32, wblas_q8;  // all meshes' trees as WIDE nodes, both encodings
    bool wide_ok[2] = {true, true};
    std::vector<ShapeParams> mesh_cache;  // per shape index: a TriangleMesh shape referenced by several objects (or by a medium
    std::vector<uint8_t> mesh_cached;     // and an object) is flattened and built once, every user shares its triangles and BLAS
    int device = -1;                      // where build_tree may build the meshes' trees
    std::vector<float> frame_reach;       // per shape: a bound on the coordinates of every point of the scene in the frame of its objects
                                          // (reach_in_frames; a mesh's walked boxes grow by 2^-21 of it, coord_max)
    float reach = 0.f;                    // frame_reach of the mesh being built
    fw::DeviceBuildTimes dev_times;       // the device builds' upload / kernel / copy-back times (FIREWORK_TRACE)
    double ms_gather = 0, ms_ref = 0, ms_gate = 0, ms_sah = 0, ms_pair = 0, ms_wide = 0;   // where mesh_params spends its time (FIREWORK_TRACE=1, tools/big_mesh.py)

    int check_material(int32_t m) const { return (m < 0 || (uint32_t)m >= d->n_materials) ? FW_ERR_BAD_ARG : FW_OK; }

    // object-space shape -> parameters + bounding box (Hitable::bounding_box of each shape)
    int shape_params(int32_t si, ShapeParams &sp, int nest) {
        if (si < 0 || (uint32_t)si >= d->n_shapes) return fail(FW_ERR_BAD_ARG, "shape index out of range");
        const fw_shape &s = d->shapes[si];
        if (s.kind != FW_SHAPE_CONSTANT_MEDIUM || nest > 0) { if (check_material(s.material)) return fail(FW_ERR_BAD_ARG, "material index out of range"); }
        sp.kind = (uint32_t)s.kind;
        switch (s.kind) {
        case FW_SHAPE_SPHERE:                                        // sphere.rs:62-64
            sp.q3[0] = s.radius;
            sp.box = {{-s.radius, -s.radius, -s.radius}, {s.radius, s.radius, s.radius}};
            // the reference builds the box as -Vec3::one()*r .. Vec3::one()*r: same values
            return FW_OK;
        case FW_SHAPE_XYRECT: case FW_SHAPE_XZRECT: case FW_SHAPE_YZRECT: {   // rect.rs:75-85
            sp.q3[0] = s.a_min; sp.q3[1] = s.a_max; sp.q3[2] = s.b_min; sp.q3[3] = s.b_max; sp.q4[0] = s.k;
            sp.q4[1] = (s.a_min <= s.a_max && s.b_min <= s.b_max) ? 0.f : 1.f;      // an interval with lo > hi admits nothing (hit_rect)
            if (s.flip_normal) sp.flags |= fw::OF_RECT_FLIP;
            int a1 = s.kind == FW_SHAPE_YZRECT ? 1 : 0, a2 = s.kind == FW_SHAPE_XYRECT ? 1 : 2, ot = s.kind == FW_SHAPE_XYRECT ? 2 : (s.kind == FW_SHAPE_XZRECT ? 1 : 0);
            float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
            mn[a1] = s.a_min; mn[a2] = s.b_min; mn[ot] = s.k - 0.01f;
            mx[a1] = s.a_max; mx[a2] = s.b_max; mx[ot] = s.k + 0.01f;
            sp.box = {{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}};
            if (sp.q4[1] != 0.f) {   // inverted box: like Disk, reachable under use_bvh only through the reference's leaf-node box
                sp.flags |= fw::OF_GATE;
                sp.true_box = {vmin(sp.box.mn, sp.box.mx), vmax(sp.box.mn, sp.box.mx)};
            }
            return FW_OK; }
        case FW_SHAPE_RECT3D:                                        // rect3d.rs:102-104
            sp.q3[0] = s.pos.x; sp.q3[1] = s.pos.y; sp.q3[2] = s.pos.z; sp.q3[3] = s.size.x; sp.q4[0] = s.size.y; sp.q4[1] = s.size.z;
            // a negative size turns some faces' bounds into lo > hi (hit_rect); pos + size is what the faces use (rect3d.rs:30-75)
            sp.q4[2] = (s.pos.x <= s.pos.x + s.size.x && s.pos.y <= s.pos.y + s.size.y && s.pos.z <= s.pos.z + s.size.z) ? 0.f : 1.f;
            sp.box = {tov(s.pos), tov(s.pos) + tov(s.size)};
            if (sp.q4[2] != 0.f) { sp.flags |= fw::OF_GATE; sp.true_box = {vmin(sp.box.mn, sp.box.mx), vmax(sp.box.mn, sp.box.mx)}; }   // as above
            return FW_OK;
        case FW_SHAPE_CONE: case FW_SHAPE_CYLINDER:                 // cone.rs:90-95, cylinder.rs:92-97
            sp.q3[0] = s.radius; sp.q3[1] = s.height; sp.q3[2] = s.phi_max;
            sp.box = {{-s.radius, 0.f, -s.radius}, {s.radius, s.height, s.radius}};
            return FW_OK;
        case FW_SHAPE_DISK:                                          // disk.rs:85-90 — degenerate box, kept as written
            sp.q3[0] = s.radius; sp.q3[2] = s.phi_max; sp.q3[3] = s.inner_radius;
            sp.box = {{-s.radius, 0.f, s.radius}, {-s.radius, 0.001f, s.radius}};
            sp.flags |= fw::OF_GATE;
            sp.true_box = {{-s.radius, -0.001f, -s.radius}, {s.radius, 0.001f, s.radius}};
            return FW_OK;
        case FW_SHAPE_TRIANGLE_MESH: {
            if (mesh_cached.empty()) { mesh_cached.assign(d->n_shapes, 0); mesh_cache.resize(d->n_shapes); }
            if (mesh_cached[si]) { sp = mesh_cache[si]; return FW_OK; }
            reach = (size_t)si < frame_reach.size() ? frame_reach[si] : 0.f;
            int rc = mesh_params(s, sp);
            if (rc == FW_OK) { mesh_cache[si] = sp; mesh_cached[si] = 1; }
            return rc; }
        case FW_SHAPE_CONSTANT_MEDIUM: {                             // volume.rs:84-86: bbox of the inner shape
            if (nest > 0) return fail(FW_ERR_UNSUPPORTED, "ConstantMedium nested in a ConstantMedium");
            ShapeParams in;
            int rc = shape_params(s.inner, in, nest + 1);
            if (rc) return rc;
            if (in.kind == FW_SHAPE_CONSTANT_MEDIUM) return fail(FW_ERR_UNSUPPORTED, "ConstantMedium nested in a ConstantMedium");
            if (check_material(s.material)) return fail(FW_ERR_BAD_ARG, "material index out of range");
            sp = in;
            sp.kind = FW_SHAPE_CONSTANT_MEDIUM | (in.kind << 16);   // inner kind travels in bits 16..23 until packing
            sp.q4[3] = s.density;
            return FW_OK; }
        default: return fail(FW_ERR_BAD_ARG, "unknown shape kind");
        }
    }

    // mesh.rs:21-30,221-242: gather triangles, build the mesh's own BVH (always, even with use_bvh=false)
    int mesh_params(const fw_shape &s, ShapeParams &sp) {
        if (!s.verts || !s.indices || s.n_indices % 3) return fail(FW_ERR_BAD_ARG, "TriangleMesh needs verts and 3*k indices");
        if (s.n_indices == 0) return fail(FW_ERR_EMPTY_SCENE, "TriangleMesh with no triangles (reference: unbounded recursion in bvh.rs:29-70)");
        uint32_t n_tris = s.n_indices / 3, tri_base = (uint32_t)(tri.size() / 12);
        max_tris = std::max(max_tris, n_tris);
        if ((uint64_t)tri_base + n_tris > fw::NODE_MASK) return fail(FW_ERR_UNSUPPORTED, "too many triangles");
        bool attr = s.normals || s.uvs;
        auto tm = std::chrono::steady_clock::now();
        auto lap = [&](double &acc) { const auto t = std::chrono::steady_clock::now(); acc += std::chrono::duration<double, std::milli>(t - tm).count(); tm = t; };
        std::vector<Box> boxes(n_tris);
        tri.resize(tri.size() + (size_t)n_tris * 12);
        if (attr) any_attr = true;
        tri_attr.resize(tri.size(), 0.f);
        BuildPool pool(host_build_threads() - 1);
        std::atomic<bool> bad_index{false};
        {
            const int helpers = n_tris >= PAR_PASS_MIN ? pool.take(15) : 0;
            par_parts(n_tris, helpers + 1, [&](size_t t_lo, size_t t_hi, int) {
                for (size_t t = t_lo; t < t_hi; t++) {
                    V3 p[3];
                    for (int k = 0; k < 3; k++) {
                        uint32_t vi = s.indices[3 * t + k];
                        if (vi >= s.n_verts) { bad_index = true; return; }
                        p[k] = {s.verts[3 * vi], s.verts[3 * vi + 1], s.verts[3 * vi + 2]};
                        float *o = &tri[(size_t)(tri_base + t) * 12 + 4 * k];
                        o[0] = p[k].x; o[1] = p[k].y; o[2] = p[k].z;
                        o[3] = s.uvs ? s.uvs[2 * vi] : (k == 1 ? 1.f : 0.f);        // default uvs (0,0),(1,0),(0,1) mesh.rs:107
                        float *a = &tri_attr[(size_t)(tri_base + t) * 12 + 4 * k];
                        if (s.normals) { a[0] = s.normals[3 * vi]; a[1] = s.normals[3 * vi + 1]; a[2] = s.normals[3 * vi + 2]; }
                        a[3] = s.uvs ? s.uvs[2 * vi + 1] : (k == 2 ? 1.f : 0.f);
                    }
                    Box b{vmin(p[0], p[1]), vmax(p[0], p[1])};               // from_two_points(p0,p1).expand_to_point(p2)
                    b = {vmin(b.mn, p[2]), vmax(b.mx, p[2])};
                    V3 size = b.mx - b.mn;
                    if (std::fabs(size.x) < 0.001f) { b.mn.x -= 0.001f; b.mx.x += 0.001f; }
                    if (std::fabs(size.y) < 0.001f) { b.mn.y -= 0.001f; b.mx.y += 0.001f; }
                    if (std::fabs(size.z) < 0.001f) { b.mn.z -= 0.001f; b.mx.z += 0.001f; }
                    boxes[t] = b;
                } });
            pool.give(helpers);
        }
        if (bad_index) return fail(FW_ERR_BAD_ARG, "vertex index out of range");
        lap(ms_gather);
        // Round 5: the reference tree and the walked tree are built at the same time, each in parallel below its big nodes (BuildPool: one budget
        // of host threads for both), and the three forms of the walked tree — pair nodes, wide f32, wide q8 — are converted side by side.
        FlatBvh local, walked;
        int ref_rc = FW_OK;
        std::string ref_msg;
        std::exception_ptr ref_error;
        const bool two = n_tris >= PAR_SUBTREE_MIN && pool.take(1) == 1;
        auto build_reference = [&] {
            try { if ((ref_rc = build_tree(device, fw::BUILD_MEDIAN, boxes, local, &pool, &dev_times)) != FW_OK) ref_msg = g_last_error; }
            catch (...) { ref_error = std::current_exception(); } };
        std::thread ref_thread;
        if (two) ref_thread = std::thread(build_reference); else build_reference();
        // the mesh's own box = the reference root's: the union of every triangle's box (fmin / fmax: the same in any order)
        Box all = boxes[0];
        for (const Box &b : boxes) all = box_union(all, b);
        sp.box = all;
        // the boxes of the walked trees (grown_by: 2^-6 of a typical triangle, at least 2^-14 of the triangle's own extent)
        std::vector<Box> wboxes = boxes;
        {
            const float typ = box_extent(sp.box) / std::sqrt((float)std::max(1u, n_tris)), gc = std::ldexp(std::fmax(coord_max({sp.box}), reach), -21);
            for (Box &b : wboxes) b = grown_by(b, std::fmax(std::fmax(std::ldexp(typ, -6), std::ldexp(box_extent(b), -14)), gc));
        }
        const bool sah = use_sah();
        std::exception_ptr sah_error;
        int sah_rc = FW_OK;
        std::string sah_msg;
        if (sah) { try { if ((sah_rc = build_tree(device, fw::BUILD_SAH, wboxes, walked, &pool, &dev_times)) != FW_OK) sah_msg = g_last_error; } catch (...) { sah_error = std::current_exception(); } }
        lap(ms_sah);
        if (two) { ref_thread.join(); pool.give(1); }
        if (ref_rc) return fail(ref_rc, ref_msg);
        if (ref_error) std::rethrow_exception(ref_error);
        if (sah_error) std::rethrow_exception(sah_error);
        if (sah_rc) return fail(sah_rc, sah_msg);
        {   // ties are resolved by the reference tree's in-order rank, whatever tree is traversed
            std::vector<uint32_t> rk = reference_ranks(local, n_tris);
            tri_rank.insert(tri_rank.end(), rk.begin(), rk.end());
        }
        ref_blas_nodes += local.count();
        sp.ref_root = (uint32_t)(ref_blas.size() / 8); sp.n_tris = n_tris;
        ref_blas.insert(ref_blas.end(), local.nodes.begin(), local.nodes.end());
        ref_blas_depth = std::max(ref_blas_depth, local.depth);
        lap(ms_ref);
        // Round 4: the reference tests a triangle iff the ray passes every box down to its LEAF NODE, i.e. iff it passes that node's box
        // (bvh.rs:44-52: a DoubleLeaf's two triangles sit behind the union; the ancestors' boxes are supersets under the monotone slab
        // arithmetic).  The walked trees keep the triangles' own, tight boxes — walking the unions costs 30 % (gpurun_out/r04d) — and
        // every hit that would become a ray's best is checked against this rule before it counts (fw_kernels.hip: tri_gate_ok):
        // tri_gate holds each triangle's reference leaf-node box.
        {
            std::vector<Box> gboxes = boxes;
            leaf_node_boxes(local, gboxes);
            tri_gate.resize(tri.size() / 12 * 8, 0.f);
            const int helpers = n_tris >= PAR_PASS_MIN ? pool.take(15) : 0;
            par_parts(n_tris, helpers + 1, [&](size_t t_lo, size_t t_hi, int) {
                for (size_t t = t_lo; t < t_hi; t++) {
                    float *g = &tri_gate[(size_t)(tri_base + t) * 8];
                    g[0] = gboxes[t].mn.x; g[1] = gboxes[t].mn.y; g[2] = gboxes[t].mn.z; g[4] = gboxes[t].mx.x; g[5] = gboxes[t].mx.y; g[6] = gboxes[t].mx.z;
                } });
            pool.give(helpers);
        }
        lap(ms_gate);
        const FlatBvh &wt = sah ? walked : local;      // BVH=median walks the reference's own topology (over the grown boxes)
        uint32_t root = 0, wr[2] = {0xffffffffu, 0xffffffffu};
        for (int f = 0; f < 2; f++) { WideBvh &wb = f == 0 ? wblas_f32 : wblas_q8; if (wb.fmt == 0) wb.fmt = f == 0 ? fw::WIDE_F32 : fw::WIDE_Q8; }
        {
            std::exception_ptr conv_error[3];
            auto convert = [&](int which) {
                try {
                    if (which == 0) { root = pair_convert(wt, wboxes, blas); blas_depth = blas.depth; }      // root reference into the shared BLAS array
                    else if (wide_ok[which - 1]) wr[which - 1] = wide_convert(wt, wboxes, which == 1 ? wblas_f32 : wblas_q8);   // the same tree as WIDE nodes, in both encodings (create_scene_impl keeps one, or none)
                } catch (...) { conv_error[which] = std::current_exception(); }
            };
            const int helpers = n_tris >= PAR_SUBTREE_MIN ? pool.take(2) : 0;
            std::vector<std::thread> th;
            for (int k = 0; k < helpers; k++) th.emplace_back(convert, k + 1);
            convert(0);
            for (int k = helpers; k < 2; k++) convert(k + 1);
            for (auto &t : th) t.join();
            pool.give(helpers);
            for (auto &e : conv_error) if (e) std::rethrow_exception(e);
        }
        lap(ms_pair);
        sp.aux0 = root; sp.aux1 = tri_base;
        for (int f = 0; f < 2; f++) {
            if (!wide_ok[f]) continue;
            if (wr[f] == 0xffffffffu) wide_ok[f] = false;
            (f == 0 ? sp.wroot_f32 : sp.wroot_q8) = wr[f];
        }
        lap(ms_wide);
        if (s.normals) sp.flags |= fw::OF_MESH_NORMALS;
        if (attr) sp.flags |= fw::OF_MESH_ATTR;
        return FW_OK;
    }
};

// ---- the object level: everything of a scene that depends on where its objects are — the object records (rotation rows,
// OF_ROTATED, OF_FLIP), the world / true / grown boxes, the reference's median TLAS with its ranks and gate boxes, the exact walk's rule
// (far rule, cluster box, rotated mesh frames), hoisting, and the walked TLAS in pair and wide form.  fw_scene_create and fw_scene_update
// both build it here from the per-shape parameters that creation computes once, so an update equals a creation by construction.
struct ObjectLevel {
    std::vector<float> objs, gate, cull, leafb, ref_tlas;
    std::vector<uint32_t> obj_rank, hoisted;
    PairBvh tlas_p;
    uint32_t tlas_root = 0, ref_tlas_nodes = 0, ref_tlas_depth = 0;
    WideBvh wtlas;
    uint32_t wtlas_root = 0xffffffffu;
    fw::DExact ex{};
    fw::DeviceBuildTimes dev_times;       // the TLAS builds on the device (from BUILD_MIN objects on)
};
inline size_t wide_lds_bytes(const WideBvh &t, uint32_t waves) { return (size_t)t.words.size() * 4 + (size_t)waves * (3 * t.depth + 2) * 128 + 4096; }

// sps: per shape index, the parameters of every shape an object uses.  has_mesh: the scene has triangles.  Errors: the median build's
// (FW_ERR_NAN_BBOX for a non-finite box).
int object_level(const fw_scene_desc *desc, int device, const Options &O, const std::vector<ShapeParams> &sps, bool has_mesh, ObjectLevel &L) {
    const uint32_t n_obj = desc->n_objects;
    std::vector<float> &objs = L.objs;
    objs.assign((size_t)n_obj * fw::OBJ_Q * 4, 0.f);
    std::vector<Box> world(n_obj), true_world(n_obj);
    std::vector<float> obj_size(n_obj, 0.f);       // the exact walk's far rule: extent of an object (a mesh: of a typical triangle)
    fw::DExact &ex = L.ex;
    for (uint32_t i = 0; i < n_obj; i++) {
        const fw_object &o = desc->objects[i];
        const ShapeParams &sp = sps[o.shape];
        float rows[3][3];
        rotor_rows(o.rotation, rows);
        uint32_t flags = sp.flags;
        float cos_trace = 0.5f * ((rows[0][0] + rows[1][1] + rows[2][2]) - 1.f);     // scene.rs:180-185
        if (cos_trace < 0.999f) flags |= fw::OF_ROTATED;
        auto to_world = [&](const Box &ob) {                                          // scene.rs:177-212
            Box rb = ob;
            if (cos_trace < 0.999f) {
                V3 mn = 10e9f * V3{1, 1, 1}, mx = -10e9f * V3{1, 1, 1};               // scene.rs:188-203
                for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) for (int c = 0; c < 2; c++) {
                    V3 corner{a == 0 ? ob.mn.x : ob.mx.x, b == 0 ? ob.mn.y : ob.mx.y, c == 0 ? ob.mn.z : ob.mx.z};
                    V3 np = mat_mul(rows, corner);
                    mx = {std::fmax(np.x, mx.x), std::fmax(np.y, mx.y), std::fmax(np.z, mx.z)};
                    mn = {std::fmin(np.x, mn.x), std::fmin(np.y, mn.y), std::fmin(np.z, mn.z)};
                }
                rb = {mn, mx};
            }
            return Box{rb.mn + tov(o.position), rb.mx + tov(o.position)};             // scene.rs:207-210
        };
        world[i] = to_world(sp.box);
        if (flags & fw::OF_GATE) true_world[i] = to_world(sp.true_box);
        {
            const Box &tb = (flags & fw::OF_GATE) ? sp.true_box : sp.box;
            const V3 e = tb.mx - tb.mn;
            obj_size[i] = std::fmax(std::fabs(e.x), std::fmax(std::fabs(e.y), std::fabs(e.z)));
            if (sp.ref_root != 0xffffffffu) {
                obj_size[i] /= std::sqrt((float)std::max(1u, sp.n_tris));
                if (cos_trace < 0.999f) {      // a rotated mesh: its frame is one the ill-direction test has to look at
                    bool known = false;
                    for (uint32_t f = 0; f < ex.n_frames && !known; f++) known = std::memcmp(ex.frames[f], rows, 36) == 0;
                    if (!known && ex.n_frames < 4) { std::memcpy(ex.frames[ex.n_frames], rows, 36); ex.n_frames++; }
                }
            }
        }
        if (o.flip_normals) flags |= fw::OF_FLIP;
        uint32_t kind = sp.kind & 0xffu, inner = (sp.kind >> 16) & 0xffu;
        int32_t material = desc->shapes[o.shape].material;
        float *q = &objs[(size_t)i * fw::OBJ_Q * 4];
        const float pos[3] = {o.position.x, o.position.y, o.position.z};
        if ((kind == FW_SHAPE_RECT3D && sp.q4[2] == 0.f) || kind == FW_SHAPE_TRIANGLE_MESH || kind == FW_SHAPE_CONE || kind == FW_SHAPE_CYLINDER) flags |= fw::OF_CULL0;
        q[0] = pos[0]; q[1] = pos[1]; q[2] = pos[2]; q[3] = bits_f(kind | (flags << 8) | (inner << 24));
        std::memcpy(q + 4, sp.q3, 16);
        std::memcpy(q + 8, sp.q4, 16);
        const uint32_t tail[3] = {(uint32_t)material, sp.aux0, sp.aux1};
        for (int r = 0; r < 3; r++) { q[12 + 4 * r] = rows[r][0]; q[13 + 4 * r] = rows[r][1]; q[14 + 4 * r] = rows[r][2]; q[15 + 4 * r] = bits_f(tail[r]); }
    }
    FlatBvh tlas;
    if (int brc = build_tree(device, fw::BUILD_MEDIAN, world, tlas, nullptr, &L.dev_times)) return brc;
    L.obj_rank = reference_ranks(tlas, n_obj);
    L.ref_tlas_nodes = tlas.count();
    L.ref_tlas = tlas.nodes;          // the reference's own tree: what k_extend_exact walks
    L.ref_tlas_depth = tlas.depth;
    {   // the exact walk's flag rule (fw_device.h DExact)
        if (has_mesh) ex.mode |= 1u;
        float min_size = 3.0e38f;
        for (uint32_t i = 0; i < n_obj; i++) if (obj_size[i] > 0.f) min_size = std::fmin(min_size, obj_size[i]);
        if (min_size < 3.0e38f) {
            Box cl{{3e38f, 3e38f, 3e38f}, {-3e38f, -3e38f, -3e38f}};
            for (uint32_t i = 0; i < n_obj; i++)
                if (obj_size[i] > 0.f && obj_size[i] <= 16.f * min_size) cl = box_union(cl, world[i].mn.x <= world[i].mx.x ? world[i] : Box{vmin(world[i].mn, world[i].mx), vmax(world[i].mn, world[i].mx)});
            const V3 c = box_center(cl), h = cl.mx - c;
            const float radius = std::fmax(h.x, std::fmax(h.y, h.z));
            ex.far_c[0] = c.x; ex.far_c[1] = c.y; ex.far_c[2] = c.z;
            ex.far_r = std::fmax((float)O.exact_far_x * min_size, 2.f * radius);  // noise / signal of a sphere's discriminant = 2^-23 (|o| / r)^2 = 2^-23 (2 |o| / size)^2: 1/2 at this distance
                                                                    // (128 x flagged every camera ray of teapot.rs, whose camera sits 16 units from triangles of 0.08)
            const float pad = 2.f * min_size + 1e-3f * radius;
            ex.box_lo[0] = cl.mn.x - pad; ex.box_lo[1] = cl.mn.y - pad; ex.box_lo[2] = cl.mn.z - pad;
            ex.box_hi[0] = cl.mx.x + pad; ex.box_hi[1] = cl.mx.y + pad; ex.box_hi[2] = cl.mx.z + pad;
            ex.mode |= 2u;                                          // used under use_bvh only (render_impl)
        }
        ex.shear = std::ldexp(1.f, -O.exact_shear_log2);
        if (O.no_exact) ex.mode = 0;
        if (O.exact_all) ex.mode |= 4u;   // every ray takes the exact walk (parity tool / tests)
    }
    // gate boxes: the box of each object's leaf node in the reference tree (own box for a Leaf, the union for a
    // DoubleLeaf).  In the reference an object is tested iff the ray hits that box (ancestors are supersets), which
    // matters for shapes whose own box does not enclose them (OF_GATE): they stay exactly as (in)visible as there.
    // Round 4: the reference tests an object iff the ray passes the box of its LEAF NODE in the reference tree (the union for a
    // DoubleLeaf: bvh.rs:44-52; the ancestors' boxes are supersets).  The walked trees keep the objects' own boxes (the unions cost
    // part2 26 %: gpurun_out/r04d); every object hit is checked against its reference leaf-node box (obj_gate) before it counts, and
    // a mesh before its rays are parked (fw_kernels.hip: obj_gate_ok).
    std::vector<float> &gate = L.gate;
    gate.assign((size_t)n_obj * 8, 0.f);
    std::vector<Box> build_boxes = world, own_boxes = world;
    for (uint32_t i = 0; i < tlas.count(); i++) {
        const float *nd = &tlas.nodes[(size_t)i * 8];
        uint32_t A, B; std::memcpy(&A, nd + 3, 4); std::memcpy(&B, nd + 7, 4);
        uint32_t kind = A >> 30;
        if (kind == 0) continue;
        uint32_t items[2] = {A & fw::NODE_MASK, B};
        for (uint32_t q = 0; q < (kind == fw::NODE_DOUBLE ? 2u : 1u); q++) {
            float *g = &gate[(size_t)items[q] * 8];
            g[0] = nd[0]; g[1] = nd[1]; g[2] = nd[2]; g[4] = nd[4]; g[5] = nd[5]; g[6] = nd[6];
            uint32_t kf; std::memcpy(&kf, &objs[(size_t)items[q] * fw::OBJ_Q * 4 + 3], 4);
            const Box node_box{{nd[0], nd[1], nd[2]}, {nd[4], nd[5], nd[6]}};
            // a gated object (its own box does not enclose it): the leaf node's box (so the gate test is reachable) united with bounds
            // that really enclose the geometry (so culling against the best t so far stays valid)
            if ((kf >> 8) & fw::OF_GATE) build_boxes[items[q]] = own_boxes[items[q]] = box_union(node_box, true_world[items[q]]);
        }
    }
    // the world frame's coordinates (coord_max): M over all the objects' boxes; an object inside the far rule's cluster box is reached
    // unflagged only by rays that start within far_r of far_c, so min(M, |far_c| + far_r) bounds their origins (a giant fog sphere's M
    // then grows only the objects outside the cluster)
    const float m_all = coord_max(build_boxes);
    float m_near = m_all;
    if (ex.mode & 2u)
        m_near = std::fmin(m_all, std::fmax(std::fabs(ex.far_c[0]), std::fmax(std::fabs(ex.far_c[1]), std::fabs(ex.far_c[2]))) + ex.far_r);
    for (uint32_t i = 0; i < n_obj; i++) {             // the walked trees' boxes (grown_by: what a walk must still reach)
        uint32_t kf; std::memcpy(&kf, &objs[(size_t)i * fw::OBJ_Q * 4 + 3], 4);
        const uint32_t kind = kf & 0xffu, inner = kf >> 24, shape = kind == FW_SHAPE_CONSTANT_MEDIUM ? inner : kind;
        const float ext = box_extent(build_boxes[i]);
        float g = std::ldexp(ext, -14);
        if (shape == FW_SHAPE_TRIANGLE_MESH) g = std::fmax(g, std::ldexp(obj_size[i], -5));                        // its triangles' boxes grew by 2^-6 of this, in the mesh's frame
        else if ((shape == FW_SHAPE_SPHERE || shape == FW_SHAPE_CONE || shape == FW_SHAPE_CYLINDER) && (ex.mode & 2u) && ext > 0.f)
            g = std::fmax(g, std::fmin(ext, std::ldexp(ex.far_r * ex.far_r / ext, -22)));
        const Box &b = build_boxes[i];
        const bool near = (ex.mode & 2u) && std::fmin(b.mn.x, b.mx.x) >= ex.box_lo[0] && std::fmin(b.mn.y, b.mx.y) >= ex.box_lo[1] && std::fmin(b.mn.z, b.mx.z) >= ex.box_lo[2]
                          && std::fmax(b.mn.x, b.mx.x) <= ex.box_hi[0] && std::fmax(b.mn.y, b.mx.y) <= ex.box_hi[1] && std::fmax(b.mn.z, b.mx.z) <= ex.box_hi[2];
        const float gc = std::ldexp(near ? std::fmax(m_near, coord_max({b})) : m_all, -21);
        build_boxes[i] = grown_by(build_boxes[i], std::fmax(g, gc));
    }
    auto pack_boxes = [&](const std::vector<Box> &bs) {
        std::vector<float> out((size_t)n_obj * 8, 0.f);
        for (uint32_t i = 0; i < n_obj; i++) {
            const Box &b = bs[i];
            float *c = &out[(size_t)i * 8];
            c[0] = b.mn.x; c[1] = b.mn.y; c[2] = b.mn.z; c[4] = b.mx.x; c[5] = b.mx.y; c[6] = b.mx.z;
        }
        return out;
    };
    L.cull = pack_boxes(own_boxes);       // enclosing world boxes of the objects themselves: the pre-tests of the linear scan (k_extend_linear*)
    {   // ... and behind them the same boxes as centre and grown half extent, for the box-list scan's fma pre-test (fw_defer_pretest.h)
        L.cull.resize((size_t)n_obj * 16, 0.f);
        for (uint32_t i = 0; i < n_obj; i++) {
            const float *b = &L.cull[(size_t)i * 8];
            const fwpt::CullBox cb = fwpt::make_cull_box(b, b + 4);
            float *c = &L.cull[((size_t)n_obj + i) * 8];
            for (int a = 0; a < 3; a++) { c[a] = cb.c[a]; c[4 + a] = cb.h[a]; }
        }
    }
    L.leafb = pack_boxes(build_boxes);    // the objects' boxes in the walked trees (k_extend_scan, hoisted_hits)
    // Hoisting: an object whose box covers most of the scene (part2's r = 5000 fog medium) is met by nearly every ray, so in
    // the tree its leaf is one more divergent leaf test per ray.  Scenes without meshes and too many objects for the scan keep
    // such objects out of the WALKED tree; the kernels test them for every ray before the walk, with a wave-uniform index
    // (hoisted_hits in fw_kernels.hip: same own-box test, same tie rule, so the same result as the leaf would give).
    std::vector<uint32_t> &hoisted = L.hoisted;
    if (use_sah() && n_obj > 8 && !has_mesh && !O.no_hoist) {
        Box root = build_boxes[0];
        for (const Box &b : build_boxes) root = box_union(root, b);
        const float ra = box_area(root);
        for (uint32_t i = 0; i < n_obj && hoisted.size() < 4; i++)
            if (box_area(build_boxes[i]) >= 0.5f * ra) hoisted.push_back(i);
        if (n_obj - hoisted.size() < 2) hoisted.clear();
    }
    if (use_sah()) {
        FlatBvh sah;
        if (hoisted.empty()) { if (int brc = build_tree(device, fw::BUILD_SAH, build_boxes, sah, nullptr, &L.dev_times)) return brc; }
        else {
            std::vector<Box> sub; std::vector<uint32_t> ids;
            for (uint32_t i = 0; i < n_obj; i++)
                if (std::find(hoisted.begin(), hoisted.end(), i) == hoisted.end()) { sub.push_back(build_boxes[i]); ids.push_back(i); }
            if (int brc = build_tree(device, fw::BUILD_SAH, sub, sah, nullptr, &L.dev_times)) return brc;
            for (uint32_t i = 0; i < sah.count(); i++) {      // leaf items: positions in `sub` -> object ids
                float *nd = &sah.nodes[(size_t)i * 8];
                uint32_t A, B; std::memcpy(&A, nd + 3, 4); std::memcpy(&B, nd + 7, 4);
                const uint32_t kind = A >> 30;
                if (kind == fw::NODE_LEAF) { A = (kind << 30) | ids[A & fw::NODE_MASK]; std::memcpy(nd + 3, &A, 4); }
                else if (kind == fw::NODE_DOUBLE) { A = (kind << 30) | ids[A & fw::NODE_MASK]; B = ids[B]; std::memcpy(nd + 3, &A, 4); std::memcpy(nd + 7, &B, 4); }
            }
        }
        tlas = std::move(sah);
    }
    L.tlas_root = pair_convert(tlas, build_boxes, L.tlas_p);
    // WIDE nodes (fw_device.h) for the LDS-resident walks, where they fit a CU's LDS next to the walks' stacks: f32 nodes first,
    // quantised ones for a BLAS too big for those.  Option WIDE=0: none (the pair-node kernels, A/B); =f32 / =q8 force an encoding.
    const bool wide_on = use_sah() && O.wide != 0;
    WideBvh &wtlas = L.wtlas; wtlas.fmt = fw::WIDE_F32;
    uint32_t &wtlas_root = L.wtlas_root;
    if (wide_on && !has_mesh && n_obj > 8) {
        wtlas_root = wide_convert(tlas, build_boxes, wtlas);     // (hoisted objects are not in `tlas`; its leaves hold object ids)
        if (wtlas_root == 0xffffffffu || wide_lds_bytes(wtlas, 8) > fw::LDS_TREE_LIMIT) { wtlas.words.clear(); wtlas_root = 0xffffffffu; }
    }
    return FW_OK;
}

// every scene field the object level sets.  dev: where its sections live on the device, in this order: objs, tlas_p, obj_rank, gate, cull,
// ref_tlas, leafb, wtlas (creation: in the scene's blob; an update: in sc->obj_data)
void apply_object_level(fw_scene *sc, const ObjectLevel &L, const uint8_t *const dev[8]) {
    fw::DScene &d = sc->d;
    d.obj = (const float4 *)dev[0]; d.tlas = (const float4 *)dev[1]; d.obj_rank = (const uint32_t *)dev[2]; d.obj_gate = (const float4 *)dev[3];
    d.obj_cull = (const float4 *)dev[4]; d.ref_tlas = (const float4 *)dev[5]; d.obj_leaf = (const float4 *)dev[6];
    d.wtlas = L.wtlas.words.empty() ? nullptr : (const uint32_t *)dev[7];
    d.wtlas_root = L.wtlas_root; d.tlas_root = L.tlas_root;
    d.n_hoisted = (uint32_t)L.hoisted.size();
    for (size_t i = 0; i < 4; i++) d.hoisted[i] = i < L.hoisted.size() ? L.hoisted[i] : 0u;
    sc->wtlas_fmt = L.wtlas.words.empty() ? fw::WIDE_NONE : fw::WIDE_F32;
    sc->wtlas_nodes = L.wtlas.count(); sc->wtlas_depth = L.wtlas.depth;
    sc->ex = L.ex; sc->ref_tlas_depth = L.ref_tlas_depth;
    sc->tlas_nodes = L.ref_tlas_nodes;    // reported: the reference topology (bvh.rs)
    sc->tlas_depth = L.tlas_p.depth; sc->tlas_pair_nodes = L.tlas_p.count();
}

// reach: the frame_reach to build the meshes' walked trees with (nullptr: reach_in_frames of desc; fw_scene_update passes what a rebuild needs)
// ---- light sampling -------------------------------------------------------------------------------------------------
// The sampled lights of a description: every object whose material is EmissiveMat and whose shape is a sphere or an axis-aligned
// rectangle, in object order, picked uniformly.  A record gives the geometry the walks intersect: a rectangle's four corners in the world,
// rotated only where the object's rotation is not near the identity (cos_trace < 0.999, scene.rs:242-253: the reference intersects it
// unrotated otherwise); a sphere's centre and radius.  fw_selftest_lights returns these records; the device keeps the object indices.
struct LightRec { uint32_t obj, kind; float pts[12]; float area, p_pick; };
static std::vector<LightRec> scene_lights(const fw_scene_desc *d) {
    std::vector<LightRec> out;
    for (uint32_t i = 0; i < d->n_objects; i++) {
        const fw_object &o = d->objects[i];
        if (o.shape < 0 || (uint32_t)o.shape >= d->n_shapes) continue;
        const fw_shape &s = d->shapes[o.shape];
        if (s.kind < FW_SHAPE_SPHERE || s.kind > FW_SHAPE_YZRECT) continue;
        if (s.material < 0 || (uint32_t)s.material >= d->n_materials || d->materials[s.material].kind != FW_MAT_EMISSIVE) continue;
        LightRec r{}; r.obj = i; r.kind = (uint32_t)s.kind;
        const V3 pos = tov(o.position);
        if (s.kind == FW_SHAPE_SPHERE) {
            r.pts[0] = pos.x; r.pts[1] = pos.y; r.pts[2] = pos.z; r.pts[3] = s.radius;
            r.area = 4.f * 3.14159265358979323846f * s.radius * s.radius;
        } else {
            float rows[3][3];
            rotor_rows(o.rotation, rows);
            const bool rotated = 0.5f * ((rows[0][0] + rows[1][1] + rows[2][2]) - 1.f) < 0.999f;     // fw::OF_ROTATED
            const float a[4] = {s.a_min, s.a_max, s.a_max, s.a_min}, b[4] = {s.b_min, s.b_min, s.b_max, s.b_max};
            for (int c = 0; c < 4; c++) {
                const V3 p = s.kind == FW_SHAPE_XYRECT ? V3{a[c], b[c], s.k} : (s.kind == FW_SHAPE_XZRECT ? V3{a[c], s.k, b[c]} : V3{s.k, a[c], b[c]});
                const V3 w = (rotated ? mat_mul(rows, p) : p) + pos;
                r.pts[3 * c] = w.x; r.pts[3 * c + 1] = w.y; r.pts[3 * c + 2] = w.z;
            }
            r.area = std::fabs((s.a_max - s.a_min) * (s.b_max - s.b_min));
        }
        out.push_back(r);
    }
    for (LightRec &r : out) r.p_pick = 1.f / (float)out.size();
    return out;
}
// a record as fw_selftest_lights and fw_scene_area_lights return it and k_area_rays reads it: FW_LIGHT_RECORD_FLOATS floats
static void light_record_floats(const LightRec &l, float *r) {
    r[0] = (float)l.obj; r[1] = (float)l.kind;
    std::memcpy(r + 2, l.pts, sizeof l.pts);
    r[14] = l.area; r[15] = l.p_pick;
}
// FW_FLAG_ALL_EMITTERS: an EmissiveMat's power, max(r, g, b) of a ConstantTexture with a negative or non-finite channel
// counted as 0, and 1 for any other texture
static double emitter_power(const fw_scene_desc *d, const fw_material &m) {
    if (m.texture < 0 || (uint32_t)m.texture >= d->n_textures || d->textures[m.texture].kind != FW_TEX_CONSTANT) return 1.0;
    const fw_vec3 c = d->textures[m.texture].color;
    auto ok = [](float v) { return (std::isfinite(v) && v > 0.f) ? (double)v : 0.0; };
    return std::max(ok(c.x), std::max(ok(c.y), ok(c.z)));
}
// the object-space areas of a shape's entries (not a mesh's): a sphere 4 pi r^2, a rectangle |da db|, a Rect3d's faces (+z -z +y -y +x -x),
// a disk phi_max (r^2 - r_in^2) / 2
static uint32_t emitter_areas(const fw_shape &s, double area[6]) {
    switch (s.kind) {
    case FW_SHAPE_SPHERE: area[0] = 4.0 * M_PI * (double)s.radius * s.radius; return 1;
    case FW_SHAPE_XYRECT: case FW_SHAPE_XZRECT: case FW_SHAPE_YZRECT: area[0] = std::fabs(((double)s.a_max - s.a_min) * ((double)s.b_max - s.b_min)); return 1;
    case FW_SHAPE_RECT3D: {
        const double xy = std::fabs((double)s.size.x * s.size.y), xz = std::fabs((double)s.size.x * s.size.z), yz = std::fabs((double)s.size.y * s.size.z);
        area[0] = area[1] = xy; area[2] = area[3] = xz; area[4] = area[5] = yz;
        return 6; }
    case FW_SHAPE_DISK: area[0] = 0.5 * (double)s.phi_max * ((double)s.radius * s.radius - (double)s.inner_radius * s.inner_radius); return 1;
    default: return 0;
    }
}
// a weight as the table takes it: negative and non-finite weights count as 0 (never picked)
static inline double emitter_weight(double w) { return (std::isfinite(w) && w > 0.0) ? w : 0.0; }
static std::vector<EmitterObj> scene_emitters(const fw_scene_desc *d, uint64_t &n_entries) {
    std::vector<EmitterObj> out;
    n_entries = 0;
    for (uint32_t i = 0; i < d->n_objects; i++) {
        const fw_object &o = d->objects[i];
        if (o.shape < 0 || (uint32_t)o.shape >= d->n_shapes) continue;
        const fw_shape &s = d->shapes[o.shape];
        if (s.material < 0 || (uint32_t)s.material >= d->n_materials || d->materials[s.material].kind != FW_MAT_EMISSIVE) continue;
        const double power = emitter_power(d, d->materials[s.material]);
        if (!(power > 0.0)) continue;        // a black emitter: no entries (it emits nothing, so nothing is lost)
        EmitterObj e{}; e.obj = i; e.kind = (uint32_t)s.kind; e.first = n_entries;
        e.shape = o.shape; e.power = power; e.pos[0] = o.position.x; e.pos[1] = o.position.y; e.pos[2] = o.position.z;
        rotor_rows(o.rotation, e.rot);
        if (s.kind == FW_SHAPE_TRIANGLE_MESH) { e.count = (s.verts && s.indices) ? s.n_indices / 3 : 0u; e.pre[0] = (float)power; }
        else {
            double area[6];
            e.count = emitter_areas(s, area);
            for (uint32_t k = 0; k < e.count; k++) e.pre[k] = (float)emitter_weight(area[k] * power);
        }
        if (e.count == 0) continue;
        n_entries += e.count;
        out.push_back(e);
    }
    return out;
}

// the device's copy (object indices) and the scene's light-sampling facts; at creation and after every fw_scene_update
static int upload_lights(fw_scene *sc, const fw_scene_desc *d) {
    sc->emit_objs = scene_emitters(d, sc->n_entries);
    sc->es_state = 0;             // (the objects may have moved: §9zc's records are built again by the next call that needs them)
    const std::vector<LightRec> L = scene_lights(d);
    std::vector<uint32_t> objs(L.size());
    for (size_t i = 0; i < L.size(); i++) objs[i] = L[i].obj;
    if (int rc = sc->lights.upload(objs.data(), objs.size() * 4)) return rc;
    std::vector<float> recs(L.size() * FW_LIGHT_RECORD_FLOATS);
    for (size_t i = 0; i < L.size(); i++) light_record_floats(L[i], &recs[i * FW_LIGHT_RECORD_FLOATS]);
    if (int rc = sc->area_recs.upload(recs.data(), recs.size() * 4)) return rc;
    sc->light_recs.swap(recs);
    sc->n_lights = (uint32_t)L.size();
    sc->ls_vertices = false;
    sc->has_ggx = false;
    for (uint32_t m = 0; m < d->n_materials; m++) {
        sc->has_ggx = sc->has_ggx || d->materials[m].kind == FW_MAT_GGX;
        sc->ls_vertices = sc->ls_vertices || d->materials[m].kind == FW_MAT_LAMBERTIAN || d->materials[m].kind == FW_MAT_ISOTROPIC || d->materials[m].kind == FW_MAT_GGX;
    }
    return FW_OK;
}

// ---- every emitter at surface points: §9i's entries as world-space records ---------------------------------------------
// A record is FW_EMITTERS_RECORD_FLOATS floats: object, kind, 12 geometry floats, area, weight; codes holds (object, prim) per entry.
// Spheres and rectangles are scene_lights' records float for float; every other point is the float64 image of its object-space point,
// ((R0 x + R1 y) + R2 z) + position per component with rotor_rows' float32 rows, rotated exactly where the walks rotate (OF_ROTATED),
// rounded to float32 once.  tris: a mesh's triangles in object space, 9 floats each.
static void emitters_world(const EmitterObj &e, bool rotated, double x, double y, double z, float *out) {
    const double p[3] = {x, y, z};
    for (int c = 0; c < 3; c++) {
        const double w = rotated ? ((double)e.rot[c][0] * x + (double)e.rot[c][1] * y) + (double)e.rot[c][2] * z : p[c];
        out[c] = (float)(w + (double)e.pos[c]);
    }
}
static void emitters_object_records(const EmitterObj &e, const fw_shape &s, const float *tris, float *rec, uint32_t *codes) {
    const bool rotated = 0.5f * ((e.rot[0][0] + e.rot[1][1] + e.rot[2][2]) - 1.f) < 0.999f;     // fw::OF_ROTATED
    const V3 pos{e.pos[0], e.pos[1], e.pos[2]};
    double area[6] = {0, 0, 0, 0, 0, 0};
    if (e.kind != FW_SHAPE_TRIANGLE_MESH) emitter_areas(s, area);
    for (uint32_t k = 0; k < e.count; k++) {
        float *r = rec + (size_t)k * FW_EMITTERS_RECORD_FLOATS;
        std::memset(r, 0, FW_EMITTERS_RECORD_FLOATS * 4);
        float *g = r + 2;
        double a = area[e.kind == FW_SHAPE_TRIANGLE_MESH ? 0 : k];
        r[0] = (float)e.obj; r[1] = (float)e.kind;
        codes[2 * (size_t)k] = e.obj; codes[2 * (size_t)k + 1] = k;
        if (e.kind == FW_SHAPE_SPHERE) { g[0] = pos.x; g[1] = pos.y; g[2] = pos.z; g[3] = s.radius; }
        else if (e.kind >= FW_SHAPE_XYRECT && e.kind <= FW_SHAPE_YZRECT) {                     // scene_lights' corners
            const float ca[4] = {s.a_min, s.a_max, s.a_max, s.a_min}, cb[4] = {s.b_min, s.b_min, s.b_max, s.b_max};
            for (int c = 0; c < 4; c++) {
                const V3 p = e.kind == FW_SHAPE_XYRECT ? V3{ca[c], cb[c], s.k} : (e.kind == FW_SHAPE_XZRECT ? V3{ca[c], s.k, cb[c]} : V3{s.k, ca[c], cb[c]});
                const V3 w = (rotated ? mat_mul(e.rot, p) : p) + pos;
                g[3 * c] = w.x; g[3 * c + 1] = w.y; g[3 * c + 2] = w.z;
            }
        } else if (e.kind == FW_SHAPE_RECT3D) {                                               // box_face's bounds, float32 as the walks form them
            const float lo[3] = {s.pos.x, s.pos.y, s.pos.z}, hi[3] = {s.pos.x + s.size.x, s.pos.y + s.size.y, s.pos.z + s.size.z};
            const uint32_t ax = k >> 1;                                                       // 0: an XY face at z, 1: XZ at y, 2: YZ at x
            const int ia = ax == 2 ? 1 : 0, ib = ax == 0 ? 1 : 2, ik = ax == 0 ? 2 : (ax == 1 ? 1 : 0);
            const float kk = (k & 1u) ? lo[ik] : hi[ik];
            const float ca[4] = {lo[ia], hi[ia], hi[ia], lo[ia]}, cb[4] = {lo[ib], lo[ib], hi[ib], hi[ib]};
            for (int c = 0; c < 4; c++) {
                double p[3]; p[ia] = ca[c]; p[ib] = cb[c]; p[ik] = kk;
                emitters_world(e, rotated, p[0], p[1], p[2], g + 3 * c);
            }
        } else if (e.kind == FW_SHAPE_TRIANGLE_MESH) {
            const float *t = tris + (size_t)k * 9;
            for (int c = 0; c < 3; c++) emitters_world(e, rotated, t[3 * c], t[3 * c + 1], t[3 * c + 2], g + 3 * c);
            const double e1[3] = {(double)t[3] - t[0], (double)t[4] - t[1], (double)t[5] - t[2]}, e2[3] = {(double)t[6] - t[0], (double)t[7] - t[1], (double)t[8] - t[2]};
            const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
            a = 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);                                 // fw_selftest_emitters' area
        } else {                                                                              // a disk: the y = 0 plane of its object
            g[0] = pos.x; g[1] = pos.y; g[2] = pos.z;
            for (int c = 0; c < 3; c++) { g[3 + c] = rotated ? e.rot[c][0] : (c == 0 ? 1.f : 0.f); g[6 + c] = rotated ? e.rot[c][2] : (c == 2 ? 1.f : 0.f); }
            g[9] = s.radius; g[10] = s.inner_radius; g[11] = s.phi_max;
        }
        r[14] = (float)a; r[15] = (float)emitter_weight(a * e.power);
    }
}
// fw_emitters_cdf: float64 inclusive prefix sums of the float32 weights in entry order (negative and non-finite weights count as 0),
// each divided by the last.  Returns the total; 0 (or a total that is not finite): no emitters, cdf is zeros.
static double emitters_cdf(const float *w, uint64_t n, double *cdf) {
    double total = 0;
    for (uint64_t i = 0; i < n; i++) { total = total + emitter_weight((double)w[i]); cdf[i] = total; }
    if (!(total > 0.0) || !std::isfinite(total)) { for (uint64_t i = 0; i < n; i++) cdf[i] = 0.0; return 0.0; }
    for (uint64_t i = 0; i < n; i++) cdf[i] = cdf[i] / total;
    return total;
}
// the records, codes, CDF and objects of a resident scene as it now stands, on the host and in es_dev; a mesh's triangles come from the
// device's copy of them (the description's arrays are the caller's and may be gone).  FW_ERR_UNSUPPORTED above 2^24 entries.
static int ensure_emitters_surface(fw_scene *sc) {
    if (sc->es_state == 1) return FW_OK;
    const uint64_t N = sc->n_entries;
    if (N > (1ull << 24)) return fail(FW_ERR_UNSUPPORTED, "more than 2^24 emitter entries");
    HIPCHK(hipSetDevice(sc->device));
    std::vector<float> rec((size_t)N * FW_EMITTERS_RECORD_FLOATS), w((size_t)N);
    std::vector<uint32_t> codes((size_t)N * 2), objs;
    std::vector<double> cdf((size_t)N);
    std::vector<float> tri4, tris;
    int32_t tris_of = -1;                  // the shape whose triangles `tris` holds: objects that share a mesh read it once
    bool synced = false;
    for (const EmitterObj &e : sc->emit_objs) {
        if (e.shape < 0 || (size_t)e.shape >= sc->keep.shapes.size()) return fail(FW_ERR_BAD_ARG, "emitter object without a shape");
        if (e.kind == FW_SHAPE_TRIANGLE_MESH && e.shape != tris_of) {
            if ((size_t)e.shape >= sc->keep.sp.size() || !sc->d.tri) return fail(FW_ERR_BAD_ARG, "emitter mesh without triangles");
            tri4.resize((size_t)e.count * 12); tris.resize((size_t)e.count * 9);
            if (!synced) { HIPCHK(hipDeviceSynchronize()); synced = true; }                   // (the scene's upload has landed)
            HIPCHK(hipMemcpy(tri4.data(), sc->d.tri + 3 * (size_t)sc->keep.sp[e.shape].aux1, tri4.size() * 4, hipMemcpyDeviceToHost));
            for (size_t v = 0; v < (size_t)e.count * 3; v++) for (int c = 0; c < 3; c++) tris[v * 3 + c] = tri4[v * 4 + c];
            tris_of = e.shape;
        }
        emitters_object_records(e, sc->keep.shapes[e.shape], tris.data(), &rec[(size_t)e.first * FW_EMITTERS_RECORD_FLOATS], &codes[(size_t)e.first * 2]);
        objs.push_back(e.obj);                                                                // (scene_emitters walks the objects in ascending order)
    }
    for (uint64_t i = 0; i < N; i++) w[i] = rec[(size_t)i * FW_EMITTERS_RECORD_FLOATS + 15];
    const double total = emitters_cdf(w.data(), N, cdf.data());
    const size_t b_rec = (size_t)N * 64, b_cdf = (size_t)N * 8, b_codes = (size_t)N * 8, b_objs = objs.size() * 4;
    std::vector<uint8_t> blob(b_rec + b_cdf + b_codes + b_objs);
    if (b_rec) { std::memcpy(blob.data(), rec.data(), b_rec); std::memcpy(blob.data() + b_rec, cdf.data(), b_cdf); std::memcpy(blob.data() + b_rec + b_cdf, codes.data(), b_codes); }
    if (b_objs) std::memcpy(blob.data() + b_rec + b_cdf + b_codes, objs.data(), b_objs);
    if (int rc = sc->es_dev.upload(blob.data(), blob.size())) return rc;
    sc->es_rec.swap(rec); sc->es_codes.swap(codes); sc->es_cdf.swap(cdf); sc->es_objs.swap(objs);
    sc->es_total = total;
    sc->es_state = 1;
    return FW_OK;
}
static const float4 *emitters_surface_records(const fw_scene *sc) { return (const float4 *)sc->es_dev.p; }
static const double *emitters_surface_cdf(const fw_scene *sc) { return (const double *)((const uint8_t *)sc->es_dev.p + sc->es_cdf.size() * 64); }
static const uint32_t *emitters_surface_codes(const fw_scene *sc) { return (const uint32_t *)((const uint8_t *)sc->es_dev.p + sc->es_cdf.size() * 72); }
static const uint32_t *emitters_surface_objs(const fw_scene *sc) { return (const uint32_t *)((const uint8_t *)sc->es_dev.p + sc->es_cdf.size() * 80); }

int create_scene_impl(const fw_scene_desc *desc, int device, fw_scene **out, const std::vector<float> *reach = nullptr) {
    if (!desc || !out) return fail(FW_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FW_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (desc->n_objects == 0 || !desc->objects) return fail(FW_ERR_EMPTY_SCENE, "No render objects added to scene!");
    if (desc->n_objects > fw::NODE_MASK) return fail(FW_ERR_UNSUPPORTED, "too many objects");
    HIPCHK(hipSetDevice(device));
    const int n_cus_dev = device_cus(device);
    if (n_cus_dev <= 0) return fail(FW_ERR_HIP, "hipGetDeviceProperties failed");
    // FIREWORK_TRACE=1: where a scene creation spends its time (host flatten + BVH builds | staging blob | alloc | copy)
    const Options O = options();
    const bool trace = O.trace;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(now() - t).count(); };
    const auto tr0 = now();

    Flattener fl{desc};
    fl.device = device;
    std::vector<float> ext = shape_extents(desc);
    fl.frame_reach = reach ? *reach : reach_in_frames(desc, ext);
    // every shape an object uses, in the objects' order (a mesh is flattened and its trees built where its first user is met)
    std::vector<ShapeParams> sps(desc->n_shapes);
    {
        std::vector<uint8_t> known(desc->n_shapes, 0);
        for (uint32_t i = 0; i < desc->n_objects; i++) {
            const int32_t si = desc->objects[i].shape;
            if (si >= 0 && (uint32_t)si < desc->n_shapes && known[si]) continue;
            ShapeParams sp;
            if (int rc = fl.shape_params(si, sp, 0)) return rc;
            sps[si] = sp; known[si] = 1;
        }
    }
    std::vector<uint32_t> obj_ref_blas(desc->n_objects, 0xffffffffu);
    std::vector<uint32_t> obj_wroot_f32(desc->n_objects, 0xffffffffu), obj_wroot_q8(desc->n_objects, 0xffffffffu);
    bool has_medium = false, has_perlin = false;
    for (uint32_t i = 0; i < desc->n_objects; i++) {
        const ShapeParams &sp = sps[desc->objects[i].shape];
        obj_ref_blas[i] = sp.ref_root;
        if ((sp.kind & 0xffu) == FW_SHAPE_TRIANGLE_MESH) { obj_wroot_f32[i] = sp.wroot_f32; obj_wroot_q8[i] = sp.wroot_q8; }
        if ((sp.kind & 0xffu) == FW_SHAPE_CONSTANT_MEDIUM) has_medium = true;
    }
    // packed hit records: object << prim_bits | primitive must fit 32 bits with all-ones left for MISS
    uint32_t prim_bits = 3;                                   // rect3d faces 0..5
    while (prim_bits < 31 && (1ull << prim_bits) < (uint64_t)fl.max_tris) prim_bits++;
    {
        uint32_t obj_bits = 1; while (obj_bits < 32 && (1ull << obj_bits) < (uint64_t)desc->n_objects + 1) obj_bits++;
        if (obj_bits + prim_bits > 32) return fail(FW_ERR_UNSUPPORTED, "objects x triangles-per-mesh exceed the 32-bit hit code");
    }
    const auto tl0 = now();
    ObjectLevel L;
    if (int rc = object_level(desc, device, O, sps, !fl.tri.empty(), L)) return rc;
    const double ms_objects = ms_since(tl0);
    const bool wide_on = use_sah() && O.wide != 0;
    int wblas_fmt = fw::WIDE_NONE;
    if (wide_on && !fl.tri.empty()) {
        const bool force_q8 = O.wide == 2, force_f32 = O.wide == 1;
        if (fl.wide_ok[0] && !force_q8 && wide_lds_bytes(fl.wblas_f32, 8) <= fw::LDS_TREE_LIMIT) wblas_fmt = fw::WIDE_F32;
        else if (fl.wide_ok[1] && !force_f32 && wide_lds_bytes(fl.wblas_q8, 8) <= fw::LDS_TREE_LIMIT) wblas_fmt = fw::WIDE_Q8;
    }
    const WideBvh &wblas = wblas_fmt == fw::WIDE_Q8 ? fl.wblas_q8 : fl.wblas_f32;
    std::vector<uint32_t> obj_wroot(desc->n_objects, fw::W_DONE);
    for (uint32_t i = 0; i < desc->n_objects; i++) obj_wroot[i] = wblas_fmt == fw::WIDE_Q8 ? obj_wroot_q8[i] : obj_wroot_f32[i];

    // materials / textures / images
    std::vector<float> mats((size_t)std::max(1u, desc->n_materials) * 8, 0.f), texs((size_t)std::max(1u, desc->n_textures) * 8, 0.f);
    std::vector<uint8_t> images;
    for (uint32_t i = 0; i < desc->n_textures; i++) {
        const fw_texture &t = desc->textures[i];
        float *q = &texs[(size_t)i * 8];
        q[0] = bits_f((uint32_t)t.kind); q[1] = t.scale; q[2] = bits_f(t.depth);
        switch (t.kind) {
        case FW_TEX_CONSTANT: q[4] = t.color.x; q[5] = t.color.y; q[6] = t.color.z; break;
        case FW_TEX_CHECKER:
            if (t.odd < 0 || t.even < 0 || (uint32_t)t.odd >= desc->n_textures || (uint32_t)t.even >= desc->n_textures) return fail(FW_ERR_BAD_ARG, "checker child texture out of range");
            q[3] = bits_f((uint32_t)t.odd); q[4] = bits_f((uint32_t)t.even); break;
        case FW_TEX_PERLIN: case FW_TEX_TURBULENCE: case FW_TEX_MARBLE: has_perlin = true; break;
        case FW_TEX_IMAGE: {
            if (!t.img_rgb8 || !t.img_w || !t.img_h) return fail(FW_ERR_BAD_ARG, "ImageTexture without pixels");
            size_t off = images.size(), nb = (size_t)t.img_w * t.img_h * 3;
            if (off + nb > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image textures exceed 4 GiB");
            images.insert(images.end(), t.img_rgb8, t.img_rgb8 + nb);
            q[4] = bits_f((uint32_t)off); q[5] = bits_f(t.img_w); q[6] = bits_f(t.img_h); break; }
        default: return fail(FW_ERR_BAD_ARG, "unknown texture kind");
        }
    }
    // CheckerTexture children must form a finite tree no deeper than the device's bounded walk (the reference would
    // recurse forever on a cycle: texture.rs:59-72)
    for (uint32_t i = 0; i < desc->n_textures; i++) {
        std::vector<std::pair<int32_t, int>> todo{{(int32_t)i, 0}};
        size_t visited = 0;
        while (!todo.empty()) {
            auto [ti, depth] = todo.back(); todo.pop_back();
            if (depth > 14 || ++visited > 65536) return fail(FW_ERR_BAD_ARG, "CheckerTexture nesting too deep or cyclic");
            const fw_texture &t = desc->textures[ti];
            if (t.kind == FW_TEX_CHECKER) { todo.push_back({t.odd, depth + 1}); todo.push_back({t.even, depth + 1}); }
        }
    }
    for (uint32_t i = 0; i < desc->n_materials; i++) {
        const fw_material &m = desc->materials[i];
        float *q = &mats[(size_t)i * 8];
        if (m.kind < FW_MAT_LAMBERTIAN || m.kind > FW_MAT_GGX) return fail(FW_ERR_BAD_ARG, "unknown material kind");
        if (m.kind == FW_MAT_GGX) {       // (negated comparisons: a NaN is out of range)
            if (!(m.roughness >= 0.03f && m.roughness <= 1.f)) return fail(FW_ERR_BAD_ARG, "material " + std::to_string(i) + ": GgxMat roughness must be in [0.03, 1]");
            if (!(m.albedo.x >= 0.f && m.albedo.x <= 1.f && m.albedo.y >= 0.f && m.albedo.y <= 1.f && m.albedo.z >= 0.f && m.albedo.z <= 1.f))
                return fail(FW_ERR_BAD_ARG, "material " + std::to_string(i) + ": GgxMat albedo components must be in [0, 1]");
        }
        bool needs_tex = m.kind == FW_MAT_LAMBERTIAN || m.kind == FW_MAT_EMISSIVE || m.kind == FW_MAT_ISOTROPIC;
        if (needs_tex && (m.texture < 0 || (uint32_t)m.texture >= desc->n_textures)) return fail(FW_ERR_BAD_ARG, "material texture out of range");
        uint32_t mbits = (uint32_t)m.kind;
        q[4] = m.albedo.x; q[5] = m.albedo.y; q[6] = m.albedo.z;
        if (needs_tex) {
            const fw_texture &t = desc->textures[m.texture];
            if (t.kind == FW_TEX_CONSTANT) { mbits |= fw::MF_TEX_CONST; q[4] = t.color.x; q[5] = t.color.y; q[6] = t.color.z; }
            // uv are consumed by ImageTexture only: walk the (checker) tree
            std::vector<int32_t> todo{m.texture};
            for (int guard = 0; !todo.empty() && guard < 4096; guard++) {
                const fw_texture &c = desc->textures[todo.back()];
                todo.pop_back();
                if (c.kind == FW_TEX_IMAGE) mbits |= fw::MF_NEEDS_UV;
                if (c.kind == FW_TEX_CHECKER) { todo.push_back(c.odd); todo.push_back(c.even); }
            }
        }
        if (m.kind == FW_MAT_DIELECTRIC) { q[4] = q[5] = q[6] = 1.f; }          // its attenuation (material.rs:128), for the chain state's product
        q[0] = bits_f(mbits); q[1] = bits_f((uint32_t)(needs_tex ? m.texture : 0)); q[2] = m.roughness; q[3] = m.ref_idx;
        if (m.kind == FW_MAT_GGX) q[2] = m.roughness * m.roughness;              // alpha
    }
    const fw_environment &e = desc->environment;
    if (e.kind < FW_ENV_COLOR || e.kind > FW_ENV_HDR) return fail(FW_ERR_BAD_ARG, "unknown environment kind");
    if (e.kind == FW_ENV_HDR && (!e.hdr_rgb || !e.hdr_w || !e.hdr_h)) return fail(FW_ERR_BAD_ARG, "HdrEnv without pixels");

    // stack depth the kernels will be given
    if (L.tlas_p.depth + 1 + fl.blas_depth + 1 > 120) return fail(FW_ERR_BVH_DEPTH, "BVH deeper than the LDS traversal stack (120 levels)");

    fw_scene *sc = new (std::nothrow) fw_scene();
    if (!sc) return fail(FW_ERR_OOM, "host allocation failed");
    sc->device = device;
    sc->n_cus = n_cus_dev;
    int rc = FW_OK;
    // one device allocation + one copy for the whole scene (12 separate hipMalloc/hipFree pairs cost up to 30 ms of a
    // one-shot render): sections are 256-byte aligned inside a host staging blob
    struct Sec { const void *src; size_t bytes, off; };
    Sec secs[21] = {
        {L.objs.data(), L.objs.size() * 4, 0}, {L.tlas_p.nodes.data(), L.tlas_p.nodes.size() * 4, 0}, {fl.blas.nodes.data(), fl.blas.nodes.size() * 4, 0},
        {fl.tri.data(), fl.tri.size() * 4, 0}, {fl.any_attr ? fl.tri_attr.data() : nullptr, fl.any_attr ? fl.tri_attr.size() * 4 : 0, 0},
        {fl.tri_rank.data(), fl.tri_rank.size() * 4, 0}, {L.obj_rank.data(), L.obj_rank.size() * 4, 0}, {L.gate.data(), L.gate.size() * 4, 0},
        {mats.data(), mats.size() * 4, 0}, {texs.data(), texs.size() * 4, 0}, {images.data(), images.size(), 0},
        // the HDR map as 16-byte texels (rgb + pad), written straight into the blob below: a 12-byte texel straddles a 32-byte
        // sector in two offsets of eight, and a miss's lookup is one gather per path out of 100 MB
        {nullptr, e.kind == FW_ENV_HDR ? (size_t)e.hdr_w * e.hdr_h * 4 * 4 : 0, 0},
        {L.cull.data(), L.cull.size() * 4, 0},
        {L.ref_tlas.data(), L.ref_tlas.size() * 4, 0}, {fl.ref_blas.data(), fl.ref_blas.size() * 4, 0}, {obj_ref_blas.data(), obj_ref_blas.size() * 4, 0},
        {L.leafb.data(), L.leafb.size() * 4, 0},
        {wblas_fmt ? wblas.words.data() : nullptr, wblas_fmt ? wblas.words.size() * 4 : 0, 0}, {L.wtlas.words.data(), L.wtlas.words.size() * 4, 0},
        {obj_wroot.data(), obj_wroot.size() * 4, 0}, {fl.tri_gate.data(), fl.tri_gate.size() * 4, 0}};
    size_t total = 0;
    for (Sec &x : secs) { x.off = total; total += (x.bytes + 255) & ~(size_t)255; }
    total = std::max<size_t>(total, 256);                  // a multiple of 256: k_upload copies 16-byte words
    const double tr_build = ms_since(tr0);
    const auto tr1 = now();
    Workspace *ws = workspace_for(device);
    if (!ws) { delete sc; return fail(FW_ERR_OOM, "no workspace for this device"); }
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    if ((rc = init_device_locked(ws, device)) != FW_OK) { delete sc; return rc; }      // a host that never called fw_init pays for the device here, once
    // the blob is assembled in pinned host memory (grown on demand, kept per device) and copied by a kernel on the null
    // stream; renders of this scene wait for ws->ev_upload in stream order, the host never blocks here
    if ((rc = staging_reserve_locked(ws, total)) != FW_OK) { delete sc; return rc; }
    uint8_t *blob = (uint8_t *)ws->staging;
    size_t prev_end = 0;
    for (const Sec &x : secs) {       // sections + zeroed padding between them
        if (x.off > prev_end) std::memset(blob + prev_end, 0, x.off - prev_end);
        if (&x == &secs[11] && x.bytes) {
            float *dst = reinterpret_cast<float *>(blob + x.off);
            const float *src = e.hdr_rgb;
            for (size_t k = 0, n = (size_t)e.hdr_w * e.hdr_h; k < n; k++) { dst[4 * k] = src[3 * k]; dst[4 * k + 1] = src[3 * k + 1]; dst[4 * k + 2] = src[3 * k + 2]; dst[4 * k + 3] = 0.f; }
        }
        else if (x.bytes) std::memcpy(blob + x.off, x.src, x.bytes);
        prev_end = x.off + x.bytes;
    }
    if (total > prev_end) std::memset(blob + prev_end, 0, total - prev_end);
    const double tr_blob = ms_since(tr1);
    if (ws->scene_cache.p && ws->scene_cache.bytes >= total) { sc->data = ws->scene_cache; ws->scene_cache = DevBuf{}; }   // reuse the previous scene's allocation
    const auto tr2 = now();
    const bool reused = sc->data.p != nullptr;
    rc = sc->data.alloc(total);
    const double tr_alloc = ms_since(tr2);
    const auto tr3 = now();
    if (!rc && !ws->upload_stream && hipStreamCreateWithFlags(&ws->upload_stream, hipStreamNonBlocking) != hipSuccess) rc = fail(FW_ERR_HIP, "upload stream creation failed");
    if (!rc) {
        fw::launch_upload(ws->upload_stream, blob, sc->data.p, total);
        if (hipEventRecord(ws->ev_upload, ws->upload_stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = fail(FW_ERR_HIP, "scene upload failed");
    }
    if (trace) fprintf(stderr, "[firework] scene_create: build %.2f ms, blob %.2f ms (%zu B), alloc %.2f ms (%s), upload launch %.2f ms\n",
                       tr_build, tr_blob, total, tr_alloc, reused ? "cached" : "hipMalloc", ms_since(tr3));
    if (trace && !fl.tri.empty() && fl.dev_times.kernel_ms == 0) fprintf(stderr, "[firework] scene_create: meshes (%zu triangles, %d host threads): gather %.2f ms | SAH tree, the reference tree beside it %.2f | wait for the reference tree + ranks %.2f | gate boxes %.2f | pair + wide f32 + wide q8 side by side %.2f\n",
                                          fl.tri.size() / 12, host_build_threads(), fl.ms_gather, fl.ms_sah, fl.ms_ref, fl.ms_gate, fl.ms_pair + fl.ms_wide);
    if (trace && !fl.tri.empty() && fl.dev_times.kernel_ms > 0) fprintf(stderr, "[firework] scene_create: meshes (%zu triangles, trees on the device): gather %.2f ms | both trees %.2f (upload %.2f | kernels %.2f | copy back %.2f) | wait + ranks %.2f | gate boxes %.2f | pair + wide f32 + wide q8 side by side %.2f\n",
                                          fl.tri.size() / 12, fl.ms_gather, fl.ms_sah, fl.dev_times.upload_ms, fl.dev_times.kernel_ms, fl.dev_times.copy_ms, fl.ms_ref, fl.ms_gate, fl.ms_pair + fl.ms_wide);
    if (trace && L.dev_times.kernel_ms > 0) fprintf(stderr, "[firework] scene_create: TLAS trees on the device (%u objects): upload %.2f ms | kernels %.2f | copy back %.2f\n",
                                                    desc->n_objects, L.dev_times.upload_ms, L.dev_times.kernel_ms, L.dev_times.copy_ms);
    if (rc) { delete sc; return rc; }
    const uint8_t *base = (const uint8_t *)sc->data.p;
    fw::DScene &d = sc->d;
    d.blas = (const float4 *)(base + secs[2].off);
    d.tri = (const float4 *)(base + secs[3].off); d.tri_nrm = (const float4 *)(base + secs[4].off);
    d.tri_rank = (const uint32_t *)(base + secs[5].off);
    d.mat = (const float4 *)(base + secs[8].off); d.tex = (const float4 *)(base + secs[9].off); d.images = base + secs[10].off;
    const float *hdr_dev = (const float *)(base + secs[11].off);
    d.ref_blas = (const float4 *)(base + secs[14].off);
    d.obj_ref_blas = (const uint32_t *)(base + secs[15].off);
    d.wblas = wblas_fmt ? (const uint32_t *)(base + secs[17].off) : nullptr;
    d.obj_wroot = (const uint32_t *)(base + secs[19].off);
    d.tri_gate = (const float4 *)(base + secs[20].off);
    {
        const uint8_t *obj_dev[8] = {base + secs[0].off, base + secs[1].off, base + secs[6].off, base + secs[7].off, base + secs[12].off, base + secs[13].off, base + secs[16].off, base + secs[18].off};
        apply_object_level(sc, L, obj_dev);
    }
    sc->wblas_fmt = wblas_fmt;
    sc->wblas_nodes = wblas_fmt ? wblas.count() : 0;
    sc->wblas_depth = wblas_fmt ? wblas.depth : 0;
    sc->ref_blas_depth = fl.ref_blas_depth;
    d.n_objects = desc->n_objects; d.has_medium = has_medium ? 1u : 0u; d.has_perlin = has_perlin ? 1u : 0u; d.has_mesh = fl.tri.empty() ? 0u : 1u;
    d.prim_bits = prim_bits;
    d.soft_shear = O.soft_shear_log2 > 0 ? std::ldexp(1.f, -O.soft_shear_log2) : 0.f;
    d.env.kind = e.kind;
    d.env.color[0] = e.color.x; d.env.color[1] = e.color.y; d.env.color[2] = e.color.z;
    d.env.zenith[0] = e.zenith.x; d.env.zenith[1] = e.zenith.y; d.env.zenith[2] = e.zenith.z;
    d.env.horizon[0] = e.horizon.x; d.env.horizon[1] = e.horizon.y; d.env.horizon[2] = e.horizon.z;
    d.env.hdr = hdr_dev; d.env.hdr_w = e.hdr_w; d.env.hdr_h = e.hdr_h;
    sc->hdr_env = e.kind == FW_ENV_HDR;
    sc->has_expensive = sc->hdr_env;
    for (uint32_t i = 0; i < desc->n_materials; i++) {
        uint32_t mb; std::memcpy(&mb, &mats[(size_t)i * 8], 4);
        const uint32_t mk = mb & 0xffu;
        if (mk == (uint32_t)FW_MAT_DIELECTRIC || (!(mb & fw::MF_TEX_CONST) && (mk == (uint32_t)FW_MAT_LAMBERTIAN || mk == (uint32_t)FW_MAT_EMISSIVE || mk == (uint32_t)FW_MAT_ISOTROPIC))) sc->has_expensive = true;
    }
    // chain state (fw_kernels.hip: load_state_chain): every attenuation a constant of its material, and ten material ids in 32 bits
    sc->chain_bits = 0;
    {
        bool constant = desc->n_materials > 0;
        for (uint32_t i = 0; i < desc->n_materials; i++) {
            uint32_t mb; std::memcpy(&mb, &mats[(size_t)i * 8], 4);
            const uint32_t mk = mb & 0xffu;
            if (!(mb & fw::MF_TEX_CONST) && (mk == (uint32_t)FW_MAT_LAMBERTIAN || mk == (uint32_t)FW_MAT_EMISSIVE || mk == (uint32_t)FW_MAT_ISOTROPIC)) constant = false;
            if (mk == (uint32_t)FW_MAT_GGX) constant = false;          // its attenuation depends on the directions
        }
        uint32_t bits = 1; while ((1u << bits) < desc->n_materials) bits++;
        if (constant && 10u * bits <= 32u) sc->chain_bits = bits;
    }
    sc->simple_shapes = true;
    sc->simple_set = true; sc->simple_but_meshes = true;
    for (uint32_t i = 0; i < desc->n_objects; i++) {
        uint32_t kf; std::memcpy(&kf, &L.objs[(size_t)i * fw::OBJ_Q * 4 + 3], 4);
        if ((kf & 0xffu) > 4u) sc->simple_shapes = false;
        if ((kf & 0xffu) > 5u) sc->simple_but_meshes = false;
        if ((kf & 0xffu) > 4u && !((kf & 0xffu) == FW_SHAPE_CONSTANT_MEDIUM && (kf >> 24) == FW_SHAPE_SPHERE)) sc->simple_set = false;
    }
    // the trailing plain boxes of a linear scene (k_extend_linear_defer): at most two, no media or meshes anywhere in the scene
    sc->n_defer = 0;
    if (!has_medium && fl.tri.empty())
        for (uint32_t i = desc->n_objects; i-- > 0 && sc->n_defer < 2u;) {
            uint32_t kf; std::memcpy(&kf, &L.objs[(size_t)i * fw::OBJ_Q * 4 + 3], 4);
            if ((kf & 0xffu) == (uint32_t)FW_SHAPE_RECT3D && (((kf >> 8) & 0xffffu) & fw::OF_CULL0) && !(((kf >> 8) & 0xffffu) & fw::OF_GATE)) sc->n_defer++; else break;
        }
    sc->blas_nodes = fl.ref_blas_nodes;   // reported: the reference topology (bvh.rs); the TLAS's: apply_object_level
    sc->blas_depth = fl.blas_depth;
    sc->blas_pair_nodes = fl.blas.count(); sc->max_tris = fl.max_tris; sc->n_tris = (uint32_t)(fl.tri.size() / 12);
    sc->n_mat = desc->n_materials; sc->n_tex = desc->n_textures;
    {   // what fw_scene_update needs
        SceneKeep &k = sc->keep;
        k.obj_shape.resize(desc->n_objects);
        for (uint32_t i = 0; i < desc->n_objects; i++) k.obj_shape[i] = desc->objects[i].shape;
        k.shapes.assign(desc->shapes, desc->shapes + desc->n_shapes);
        if (desc->n_materials) k.materials.assign(desc->materials, desc->materials + desc->n_materials);
        if (desc->n_textures) k.textures.assign(desc->textures, desc->textures + desc->n_textures);
        k.env = desc->environment;
        k.sp = std::move(sps); k.ext = std::move(ext); k.reach = fl.frame_reach;
    }
    sc->blob_bytes = total; sc->ms_objects = ms_objects; sc->ms_objects_dev = L.dev_times.upload_ms + L.dev_times.kernel_ms + L.dev_times.copy_ms;
    if (int rc = upload_lights(sc, desc)) { fw_scene_destroy(sc); return rc; }
    *out = sc;
    return FW_OK;
}

// ---- fw_scene_update ----------------------------------------------------------------------------------------------
// FW_OK iff `d` differs from the description the scene was made from in its objects' placements alone: every field that is not a pointer
// compared bit for bit, of the pointers only whether they are null (the arrays' contents are the caller's promise)
int check_same_scene(const SceneKeep &k, const fw_scene_desc *d) {
    auto differs = [](const char *what) { return fail(FW_ERR_BAD_ARG, std::string("fw_scene_update: ") + what + " differs from the scene's"); };
    if (d->n_objects != k.obj_shape.size() || d->n_shapes != k.shapes.size() || d->n_materials != k.materials.size() || d->n_textures != k.textures.size())
        return differs("the number of objects, shapes, materials or textures");
    if (!d->objects || (d->n_shapes && !d->shapes) || (d->n_materials && !d->materials) || (d->n_textures && !d->textures)) return fail(FW_ERR_BAD_ARG, "null argument");
    auto same = [](const auto &x, const auto &y) { return std::memcmp(&x, &y, sizeof x) == 0; };
    auto same_null = [](const void *x, const void *y) { return (x == nullptr) == (y == nullptr); };
    for (uint32_t i = 0; i < d->n_objects; i++) if (d->objects[i].shape != k.obj_shape[i]) return differs("an object's shape index");
    for (uint32_t i = 0; i < d->n_shapes; i++) {
        const fw_shape &a = d->shapes[i], &b = k.shapes[i];
        if (!(same(a.kind, b.kind) && same(a.material, b.material) && same(a.radius, b.radius) && same(a.height, b.height) && same(a.phi_max, b.phi_max)
              && same(a.inner_radius, b.inner_radius) && same(a.a_min, b.a_min) && same(a.a_max, b.a_max) && same(a.b_min, b.b_min) && same(a.b_max, b.b_max)
              && same(a.k, b.k) && same(a.flip_normal, b.flip_normal) && same(a.pos, b.pos) && same(a.size, b.size) && same(a.n_verts, b.n_verts)
              && same(a.n_indices, b.n_indices) && same(a.inner, b.inner) && same(a.density, b.density) && same_null(a.verts, b.verts)
              && same_null(a.indices, b.indices) && same_null(a.normals, b.normals) && same_null(a.uvs, b.uvs))) return differs("a shape");
    }
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const fw_material &a = d->materials[i], &b = k.materials[i];
        if (!(same(a.kind, b.kind) && same(a.texture, b.texture) && same(a.albedo, b.albedo) && same(a.roughness, b.roughness) && same(a.ref_idx, b.ref_idx)))
            return differs("a material");
    }
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const fw_texture &a = d->textures[i], &b = k.textures[i];
        if (!(same(a.kind, b.kind) && same(a.color, b.color) && same(a.scale, b.scale) && same(a.depth, b.depth) && same(a.odd, b.odd) && same(a.even, b.even)
              && same(a.img_w, b.img_w) && same(a.img_h, b.img_h) && same_null(a.img_rgb8, b.img_rgb8))) return differs("a texture");
    }
    const fw_environment &a = d->environment, &b = k.env;
    if (!(same(a.kind, b.kind) && same(a.color, b.color) && same(a.zenith, b.zenith) && same(a.horizon, b.horizon) && same(a.hdr_w, b.hdr_w) && same(a.hdr_h, b.hdr_h)
          && same_null(a.hdr_rgb, b.hdr_rgb))) return differs("the environment");
    return FW_OK;
}

int update_scene_impl(fw_scene *sc, const fw_scene_desc *desc) {
    if (!sc || !desc) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = check_same_scene(sc->keep, desc)) return rc;
    HIPCHK(hipSetDevice(sc->device));
    const Options O = options();
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(now() - t).count(); };
    const SceneKeep &k = sc->keep;
    // A mesh's walked boxes grew by 2^-21 of its reach (reach_in_frames), which every object's position enters.  Where the new placements
    // raise it above what the mesh's trees were built with, the scene is re-created (below); a lower reach keeps the trees (boxes grown by
    // more than needed cull nothing a walk must reach).
    std::vector<float> reach = k.reach;
    uint32_t raised = 0, n_meshes = 0;
    {
        const std::vector<float> want = reach_in_frames(desc, k.ext);
        std::vector<uint8_t> is_mesh(desc->n_shapes, 0);     // the meshes creation flattened: an object's shape, or a medium's inner one
        for (int32_t si : k.obj_shape) {
            const fw_shape &s = desc->shapes[si];
            if (s.kind == FW_SHAPE_TRIANGLE_MESH) is_mesh[si] = 1;
            else if (s.kind == FW_SHAPE_CONSTANT_MEDIUM && s.inner >= 0 && (uint32_t)s.inner < desc->n_shapes && desc->shapes[s.inner].kind == FW_SHAPE_TRIANGLE_MESH) is_mesh[s.inner] = 1;
        }
        for (uint32_t si = 0; si < desc->n_shapes; si++) {
            n_meshes += is_mesh[si];
            if (is_mesh[si] && want[si] > reach[si]) { reach[si] = want[si]; raised++; }
        }
    }
    if (raised) {
        // the meshes' trees share one array per form (pair, wide f32, wide q8) and their sizes change: the whole scene is re-created — every
        // mesh flattened and its trees built again, the textures and environment uploaded again — with the raised reach (the other meshes
        // at their kept reach, so their trees come out as they were), and the new scene takes the old one's place behind this handle
        const auto t0 = now();
        fw_scene *ns = nullptr;
        if (int rc = create_scene_impl(desc, sc->device, &ns, &reach)) return rc;
        DevBuf old_data = sc->data, old_obj = sc->obj_data, old_lights = sc->lights, old_area = sc->area_recs, kept_env = sc->env_dist, old_emitters = sc->emitters, old_es = sc->es_dev;
        const int kept_env_state = sc->env_state; const double kept_env_ms = sc->env_build_ms;
        const DevBuf kept_dl = sc->dlights; const uint32_t kept_n_dl = sc->n_dlights;     // (the delta lights stay: `ns` has none, and frees none)
        *sc = *ns;
        sc->dlights = kept_dl; sc->n_dlights = kept_n_dl;                                     // (the handle stays the caller's; its DevBufs now name the new allocations)
        ns->data = old_data; ns->obj_data = old_obj; ns->lights = old_lights; ns->area_recs = old_area;   // ... and the old ones go with `ns`
        // (the emitters' table is built again for the new scene, whose triangles are new allocations: the old one goes with `ns`)
        ns->emitters = old_emitters;
        ns->es_dev = old_es;                  // (§9zc's records too: `ns` has built none)
        // (the environment's table stays: the map is the same)
        ns->env_dist = sc->env_dist; sc->env_dist = kept_env; sc->env_state = kept_env_state; sc->env_build_ms = kept_env_ms;
        fw_scene_destroy(ns);
        if (O.trace) fprintf(stderr, "[firework] scene_update: %u objects, TLAS build %.2f ms host, %.2f ms device, %u meshes rebuilt, %zu B uploaded, %u hoisted (scene re-created: the reach of %u meshes rose; %.2f ms)\n",
                             desc->n_objects, sc->ms_objects, sc->ms_objects_dev, n_meshes, sc->blob_bytes, sc->d.n_hoisted, raised, ms_since(t0));
        return FW_OK;
    }
    const auto t0 = now();
    ObjectLevel L;
    if (int rc = object_level(desc, sc->device, O, k.sp, sc->d.has_mesh != 0, L)) return rc;
    if (L.tlas_p.depth + 1 + sc->blas_depth + 1 > 120) return fail(FW_ERR_BVH_DEPTH, "BVH deeper than the LDS traversal stack (120 levels)");
    const double ms_objects = ms_since(t0);
    // the object-level sections, 256-byte aligned, in one allocation of the scene's own (grown on demand, reused by later updates)
    struct Sec { const void *src; size_t bytes, off; };
    Sec secs[8] = {{L.objs.data(), L.objs.size() * 4, 0}, {L.tlas_p.nodes.data(), L.tlas_p.nodes.size() * 4, 0}, {L.obj_rank.data(), L.obj_rank.size() * 4, 0},
                   {L.gate.data(), L.gate.size() * 4, 0}, {L.cull.data(), L.cull.size() * 4, 0}, {L.ref_tlas.data(), L.ref_tlas.size() * 4, 0},
                   {L.leafb.data(), L.leafb.size() * 4, 0}, {L.wtlas.words.data(), L.wtlas.words.size() * 4, 0}};
    size_t total = 0;
    for (Sec &x : secs) { x.off = total; total += (x.bytes + 255) & ~(size_t)255; }
    total = std::max<size_t>(total, 256);
    Workspace *ws = workspace_for(sc->device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    if (int rc = init_device_locked(ws, sc->device)) return rc;
    if (int rc = staging_reserve_locked(ws, total)) return rc;
    if (sc->obj_data.bytes < total || !sc->obj_data.p) {
        DevBuf nb;
        if (int rc = nb.alloc(total)) return rc;
        sc->obj_data.release();                      // (no render of this scene is in flight: every call drains its stream before it returns)
        sc->obj_data = nb;
    }
    uint8_t *blob = (uint8_t *)ws->staging;
    std::memset(blob, 0, total);
    for (const Sec &x : secs) if (x.bytes) std::memcpy(blob + x.off, x.src, x.bytes);
    fw::launch_upload(ws->upload_stream, blob, sc->obj_data.p, total);
    if (hipEventRecord(ws->ev_upload, ws->upload_stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail(FW_ERR_HIP, "scene upload failed");
    const uint8_t *base = (const uint8_t *)sc->obj_data.p;
    const uint8_t *dev[8];
    for (int s = 0; s < 8; s++) dev[s] = base + secs[s].off;
    apply_object_level(sc, L, dev);
    if (int rc = upload_lights(sc, desc)) return rc;
    sc->ms_objects = ms_objects; sc->ms_objects_dev = L.dev_times.upload_ms + L.dev_times.kernel_ms + L.dev_times.copy_ms;
    if (O.trace) fprintf(stderr, "[firework] scene_update: %u objects, TLAS build %.2f ms host, %.2f ms device, %u meshes rebuilt, %zu B uploaded, %u hoisted\n",
                         desc->n_objects, sc->ms_objects, sc->ms_objects_dev, 0u, total, sc->d.n_hoisted);
    return FW_OK;
}

// ---- fw_scene_set_lights, fw_check_lights ---------------------------------------------------------------------------------
int check_lights_impl(const fw_light *lights, uint32_t n) {
    if (n > FW_MAX_LIGHTS) return fail(FW_ERR_BAD_ARG, "lights: more than FW_MAX_LIGHTS (65536) lights");
    if (n && !lights) return fail(FW_ERR_BAD_ARG, "lights: null argument");
    for (uint32_t i = 0; i < n; i++) {
        const fw_light &l = lights[i];
        auto bad = [&](const char *what) { return fail(FW_ERR_BAD_ARG, "lights[" + std::to_string(i) + "]: " + what); };
        if (l.kind != FW_LIGHT_POINT && l.kind != FW_LIGHT_SPOT && l.kind != FW_LIGHT_DIRECTIONAL) return bad("unknown kind");
        for (float v : {l.position.x, l.position.y, l.position.z, l.direction.x, l.direction.y, l.direction.z, l.intensity.x, l.intensity.y,
                        l.intensity.z, l.cos_inner, l.cos_outer})
            if (!std::isfinite(v)) return bad("a field is not finite");
        if (l.intensity.x < 0.f || l.intensity.y < 0.f || l.intensity.z < 0.f) return bad("negative intensity");
        if (l.kind != FW_LIGHT_POINT && l.direction.x == 0.f && l.direction.y == 0.f && l.direction.z == 0.f) return bad("zero direction");
        if (l.kind == FW_LIGHT_SPOT && !(-1.f <= l.cos_outer && l.cos_outer <= l.cos_inner && l.cos_inner <= 1.f))
            return bad("spot cosines must satisfy -1 <= cos_outer <= cos_inner <= 1");
    }
    return FW_OK;
}
// fw::DDeltaLights.rec of checked lights (fw_scene_set_lights, fw_direct_rays, fw_direct_reduce): (position, kind), (unit direction,
// cos_inner), (intensity, cos_outer); the direction normalised in double
std::vector<float> light_records(const fw_light *lights, uint32_t n) {
    std::vector<float> rec((size_t)n * 12, 0.f);
    for (uint32_t i = 0; i < n; i++) {
        const fw_light &l = lights[i];
        float *r = &rec[(size_t)i * 12];
        const uint32_t kind = (uint32_t)l.kind;
        r[0] = l.position.x; r[1] = l.position.y; r[2] = l.position.z; std::memcpy(&r[3], &kind, 4);
        const double dx = l.direction.x, dy = l.direction.y, dz = l.direction.z, len = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (len > 0) { r[4] = (float)(dx / len); r[5] = (float)(dy / len); r[6] = (float)(dz / len); }
        r[7] = l.cos_inner;
        r[8] = l.intensity.x; r[9] = l.intensity.y; r[10] = l.intensity.z; r[11] = l.cos_outer;
    }
    return rec;
}
int set_lights_impl(fw_scene *sc, const fw_light *lights, uint32_t n) {
    if (!sc) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = check_lights_impl(lights, n)) return rc;
    if (n == 0) { sc->n_dlights = 0; return FW_OK; }
    // (the shadow queue marks a point light's ray with fw::SHADOW_NEAR, which no emitter's object index may equal)
    if (sc->d.n_objects >= fw::SHADOW_NEAR) return fail(FW_ERR_UNSUPPORTED, "too many objects for a scene with lights");
    const std::vector<float> rec = light_records(lights, n);
    const size_t bytes = rec.size() * 4, total = (bytes + 255) & ~(size_t)255;
    HIPCHK(hipSetDevice(sc->device));
    Workspace *ws = workspace_for(sc->device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    if (int rc = init_device_locked(ws, sc->device)) return rc;
    if (int rc = staging_reserve_locked(ws, total)) return rc;
    if (sc->dlights.bytes < total || !sc->dlights.p) {
        DevBuf nb;
        if (int rc = nb.alloc(total)) return rc;
        sc->dlights.release();                       // (no render of this scene is in flight: every call drains its stream before it returns)
        sc->dlights = nb;
    }
    uint8_t *blob = (uint8_t *)ws->staging;
    std::memset(blob, 0, total);
    std::memcpy(blob, rec.data(), bytes);
    // (a failed upload leaves the scene without lights rather than with half-written ones)
    sc->n_dlights = 0;
    fw::launch_upload(ws->upload_stream, blob, sc->dlights.p, total);
    if (hipEventRecord(ws->ev_upload, ws->upload_stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail(FW_ERR_HIP, "light upload failed");
    sc->n_dlights = n;
    return FW_OK;
}

// camera.rs:74-107
fw::DCamera make_camera(const fw_camera_settings &s, uint32_t width, uint32_t height) {
    const float PI_F = 3.14159265358979323846f;
    float theta = s.vfov * PI_F / 180.f;
    V3 cam_pos = tov(s.cam_pos), look_at = tov(s.look_at);
    V3 w = normalized(cam_pos - look_at);
    V3 u = normalized(cross(V3{0, 1, 0}, w));
    V3 v = cross(w, u);
    float half_height = std::tan(theta / 2.0f);
    float half_width = half_height * (float)width / (float)height;
    V3 lower_left = cam_pos - half_width * s.focus_dist * u - half_height * s.focus_dist * v - w * s.focus_dist;
    V3 horizontal = 2.0f * half_width * s.focus_dist * u;
    V3 vertical = 2.0f * half_height * s.focus_dist * v;
    fw::DCamera c;
    auto put = [](float *d, V3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; };
    put(c.position, cam_pos); put(c.horizontal, horizontal); put(c.vertical, vertical); put(c.lower_left, lower_left); put(c.u, u); put(c.v, v);
    c.lens_radius = s.aperture / 2.f;
    return c;
}

// Wavefront pool size.  Bigger is better on this part: fewer, fuller launches and longer wave-private queues
// (measured on cornell 512x512@1024: 4 Mi paths 85 ms/frame, 16 Mi 64 ms, 256 Mi = the whole frame 55 ms).
// Default: up to 2^28 paths (104 B per slot + 40 B for parked mesh rays, and up to twice as many slots as paths because a
// wave's queue capacity is a power of two: 28-77 GB), never more than half of the free HBM.
uint32_t default_paths_per_batch(const Options &O, size_t arena_bytes) {
    if (O.paths_per_batch > 0) return (uint32_t)std::min<long long>(O.paths_per_batch, 0x7fffffffll);
    size_t free_b = 0, total_b = 0;
    uint64_t budget = 1ull << 28;
    // (the arena's own bytes count as available: the pools are carved out of it)
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b + arena_bytes > 0) budget = std::min<uint64_t>(budget, (uint64_t)((free_b + arena_bytes) / 2) / 288u);
    return (uint32_t)std::max<uint64_t>(budget, 1u << 16);
}

// The fields of the launch configuration that select and size the walks (launch_extend / launch_extend_exact): the scene's trees and
// the options.  One function for render_impl and trace_impl, so that a trace runs the kernels a render of the scene runs.  Assigns
// fields of a struct the caller has zeroed (the frame graph's key hashes its bytes, padding included).
// k_shade's shading mode for a frame (LaunchCfg.shade_mode); cap: slots per queue (the A/B build's list mode holds 16-bit positions)
static int frame_shade_mode(const fw_scene *sc, const Options &O, uint32_t cap) {
    int mode = !sc->has_expensive ? 1 : 0;
#if FW_AB
    if (O.no_shade_defer) mode = 0; else if (sc->has_expensive && O.shade_list && cap <= 65536u && !sc->has_ggx) mode = 2;
#else
    (void)O; (void)cap;
#endif
    return mode;
}
void set_walk_cfg(fw::LaunchCfg &cfg, const fw_scene *sc, const Options &O, const fw::DQueue &q, bool use_bvh, bool tlas_refill) {
    cfg.q = q;
    cfg.tlas_depth = (int)sc->tlas_depth; cfg.blas_depth = (int)sc->blas_depth;
    cfg.n_mat = sc->n_mat; cfg.n_tex = sc->n_tex;
    cfg.lds_tables = !O.no_lds_tables;
    cfg.has_mesh = sc->d.has_mesh != 0;
    cfg.simple_set = sc->simple_set; cfg.simple_but_meshes = sc->simple_but_meshes;
#ifdef FW_NO_SIMPLE      // A/B build: the kernels of round 4 (every shape's code in every kernel that calls hit_object)
    cfg.simple_set = cfg.simple_but_meshes = false;
#endif
    cfg.tlas_refill = tlas_refill;
    cfg.n_cus = sc->n_cus;
    cfg.blas_pair_nodes = sc->blas_pair_nodes; cfg.tlas_pair_nodes = sc->tlas_pair_nodes; cfg.max_tris = sc->max_tris; cfg.n_tris = sc->n_tris;
    cfg.no_lds_tris = O.no_lds_tris;
    cfg.n_defer = (!use_bvh && !O.no_defer) ? sc->n_defer : 0u;
    cfg.lds_trees = !O.no_lds_trees;
    cfg.wblas_fmt = sc->wblas_fmt; cfg.wtlas_fmt = sc->wtlas_fmt; cfg.wblas_nodes = sc->wblas_nodes; cfg.wtlas_nodes = sc->wtlas_nodes;
    cfg.wblas_depth = sc->wblas_depth; cfg.wtlas_depth = sc->wtlas_depth;
    cfg.exact_form = O.exact_form;
    cfg.debug_wide_levels = 0;
#if FW_AB
    cfg.debug_wide_levels = (uint32_t)O.debug_wide_levels;
#endif
    cfg.ref_tlas_nodes = sc->tlas_nodes; cfg.ref_blas_nodes = sc->blas_nodes; cfg.ref_tlas_depth = sc->ref_tlas_depth; cfg.ref_blas_depth = sc->ref_blas_depth;
}

// FW_FLAG_LIGHT_SAMPLING takes effect where the scene has a sampled light and a material whose vertices sample them;
// otherwise the frame is the default frame
static bool light_sampling(const fw_scene *sc, const fw_render_params *p) {
    return (p->flags & FW_FLAG_LIGHT_SAMPLING) != 0 && sc->n_lights > 0 && sc->ls_vertices;
}
// The scene's point, spot and directional lights are active where it has some and a material whose vertices sample them:
// no flag, a delta light can be reached in no other way.  Such a frame takes the light-sampling layout whatever its flags.
static bool delta_lights(const fw_scene *sc) { return sc->n_dlights > 0 && sc->ls_vertices; }
// ---- environment sampling -------------------------------------------------------------------------------------------
// The table of an HDR map on the current device: buf = cdf_m (h floats), cdf_c (w h), dens (w h); p_out (optional, device): the per-texel
// probabilities; total = the map's total weight.
static int build_env_table(const fw::DEnv &env, DevBuf &buf, float *p_out, double &total, hipEvent_t after = nullptr) {
    const size_t n = (size_t)env.hdr_w * env.hdr_h;
    if (int rc = buf.alloc((env.hdr_h + 2 * n) * 4)) return rc;
    DevBuf scratch;
    if (int rc = scratch.alloc((2 * (size_t)env.hdr_h + 1) * 8)) return rc;
    float *base = (float *)buf.p;
    if (after && hipStreamWaitEvent(nullptr, after, 0) != hipSuccess) { scratch.release(); return fail(FW_ERR_HIP, "hipStreamWaitEvent failed"); }
    const int rc = fw::build_env_dist(nullptr, env, base, base + env.hdr_h, base + env.hdr_h + n, p_out, (double *)scratch.p, &total);
    scratch.release();
    return rc ? fail(rc, "environment table build failed") : FW_OK;
}
static fw::DEnvDist env_dist_of(const DevBuf &buf, const fw::DEnv &env, float p_env) {
    const float *base = (const float *)buf.p;
    const size_t n = (size_t)env.hdr_w * env.hdr_h;
    return fw::DEnvDist{base, base + env.hdr_h, base + env.hdr_h + n, p_env, env.hdr_w, env.hdr_h};
}
// The table, at the first render whose flags ask for it (the caller has set the scene's device and holds the workspace's lock).  The build
// waits for the scene's upload (ws->ev_upload: the map is copied to the device on the upload stream).  A map of 2^32 texels or more (the
// sampler's texel index is 32-bit) is not sampled.
static int ensure_env_dist(fw_scene *sc, const fw_render_params *p, const Workspace *ws) {
    if (!(p->flags & FW_FLAG_ENV_SAMPLING) || sc->d.env.kind != FW_ENV_HDR || !sc->ls_vertices || sc->env_state != 0) return FW_OK;
    if ((uint64_t)sc->d.env.hdr_w * sc->d.env.hdr_h > 0xffffffffull) { sc->env_state = 2; return FW_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    double total = 0;
    if (int rc = build_env_table(sc->d.env, sc->env_dist, nullptr, total, ws->ev_upload)) return rc;
    sc->env_state = total > 0 ? 1 : 2;
    sc->env_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (options().trace) fprintf(stderr, "[firework] environment table: %u x %u texels, total weight %.6g, %.2f ms\n", sc->d.env.hdr_w, sc->d.env.hdr_h, total, sc->env_build_ms);
    return FW_OK;
}
// FW_FLAG_ENV_SAMPLING takes effect where the environment is an HDR map of positive total weight and a material's vertices
// sample lights; otherwise the frame is the frame without the flag (ensure_env_dist has run)
static bool env_sampling(const fw_scene *sc, const fw_render_params *p) {
    return (p->flags & FW_FLAG_ENV_SAMPLING) != 0 && sc->env_state == 1 && sc->ls_vertices;
}
// ---- every emitter ----------------------------------------------------------------------------------------------------
// The table of the scene's entries on the current device: the weights (the triangles' areas on the device, 4 bytes per entry read back),
// Vose's alias table over the entries of positive weight in double on the host, and the probability each entry has under the table as
// stored — its columns' 64-bit thresholds — which is what every estimate uses.  One allocation: tab (16 B per column), ent (16 B per
// entry), first (4 B per object).  `after`: the scene's upload, which the weight pass reads.
static int build_emitter_table(fw_scene *sc, hipEvent_t after) {
    const uint64_t N = sc->n_entries;
    const uint32_t n_obj = sc->d.n_objects;
    std::vector<uint32_t> ent((size_t)N * 4), first(n_obj, fw::MISS);
    for (const EmitterObj &e : sc->emit_objs) {
        first[e.obj] = (uint32_t)e.first;
        for (uint32_t k = 0; k < e.count; k++) {
            uint32_t *r = &ent[(size_t)(e.first + k) * 4];
            float pre = e.kind == FW_SHAPE_TRIANGLE_MESH ? e.pre[0] : e.pre[k];
            r[0] = e.obj; r[1] = k; std::memcpy(&r[2], &pre, 4); r[3] = e.kind;
        }
    }
    // the weights
    std::vector<float> w((size_t)N);
    {
        DevBuf dent, dw;
        if (int rc = dent.upload(ent.data(), ent.size() * 4)) return rc;
        if (int rc = dw.alloc((size_t)N * 4)) { dent.release(); return rc; }
        int rc = FW_OK;
        if (after && hipStreamWaitEvent(nullptr, after, 0) != hipSuccess) rc = fail(FW_ERR_HIP, "hipStreamWaitEvent failed");
        if (!rc) {
            fw::launch_emitter_weights(nullptr, sc->d, (const uint4 *)dent.p, (uint32_t)N, (float *)dw.p);
            if (hipGetLastError() != hipSuccess || hipMemcpy(w.data(), dw.p, (size_t)N * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FW_ERR_HIP, "emitter weights failed");
        }
        dent.release(); dw.release();
        if (rc) return rc;
    }
    // Vose's alias table over the entries of positive weight (in entry order), in double
    std::vector<uint32_t> pos;
    double total = 0;
    for (uint64_t i = 0; i < N; i++) { const double wi = emitter_weight((double)w[i]); if (wi > 0.0) { pos.push_back((uint32_t)i); total += wi; } }
    const uint32_t K = (uint32_t)pos.size();
    sc->emit_cols = K;
    if (K == 0 || !(total > 0.0) || !std::isfinite(total)) { sc->emit_state = 2; return FW_OK; }
    std::vector<double> q(K);
    std::vector<uint32_t> alias(K), small, large;
    for (uint32_t c = 0; c < K; c++) { q[c] = (double)w[pos[c]] / total * (double)K; (q[c] < 1.0 ? small : large).push_back(c); }
    while (!small.empty() && !large.empty()) {
        const uint32_t s_ = small.back(), l = large.back();
        small.pop_back(); large.pop_back();
        alias[s_] = l;
        q[l] = (q[l] + q[s_]) - 1.0;
        (q[l] < 1.0 ? small : large).push_back(l);
    }
    for (uint32_t c : large) { q[c] = 1.0; alias[c] = c; }
    for (uint32_t c : small) { q[c] = 1.0; alias[c] = c; }     // (rounding leftovers)
    // the stored table: threshold = q 2^64 (an entry that keeps its whole column aliases itself), and the probability it gives each entry
    std::vector<uint32_t> tab((size_t)K * 4);
    std::vector<long double> prob((size_t)N, 0.0L);
    const long double two64 = 18446744073709551616.0L;
    for (uint32_t c = 0; c < K; c++) {
        uint64_t thr;
        if (alias[c] == c || q[c] >= 1.0) { thr = ~0ull; alias[c] = c; }
        else if (!(q[c] > 0.0)) thr = 0;
        else { const long double t = std::floor((long double)q[c] * two64 + 0.5L); thr = t >= two64 ? ~0ull : (uint64_t)t; }
        const long double keep = alias[c] == c ? 1.0L : (long double)thr / two64;
        prob[pos[c]] += keep / K;
        prob[pos[alias[c]]] += (1.0L - keep) / K;
        uint32_t *r = &tab[(size_t)c * 4];
        r[0] = (uint32_t)thr; r[1] = (uint32_t)(thr >> 32); r[2] = pos[c]; r[3] = pos[alias[c]];
    }
    for (uint64_t i = 0; i < N; i++) { const float pk = (float)prob[i]; std::memcpy(&ent[(size_t)i * 4 + 2], &pk, 4); }
    const size_t tab_b = ((size_t)K * 16 + 255) & ~(size_t)255, ent_b = ((size_t)N * 16 + 255) & ~(size_t)255;
    std::vector<uint8_t> blob(tab_b + ent_b + (size_t)n_obj * 4, 0);
    std::memcpy(blob.data(), tab.data(), (size_t)K * 16);
    std::memcpy(blob.data() + tab_b, ent.data(), (size_t)N * 16);
    std::memcpy(blob.data() + tab_b + ent_b, first.data(), (size_t)n_obj * 4);
    if (int rc = sc->emitters.upload(blob.data(), blob.size())) return rc;
    sc->emit_ent_off = tab_b; sc->emit_first_off = tab_b + ent_b;
    sc->emit_state = 1;
    return FW_OK;
}
static fw::DEmitters emitters_of(const fw_scene *sc, float p_env) {
    const uint8_t *b = (const uint8_t *)sc->emitters.p;
    return fw::DEmitters{(const uint4 *)b, (const uint4 *)(b + sc->emit_ent_off), (const uint32_t *)(b + sc->emit_first_off), sc->emit_cols, 1.f - p_env};
}
static bool all_emitters_asked(const fw_render_params *p) {
    return (p->flags & FW_FLAG_LIGHT_SAMPLING) != 0 && (p->flags & FW_FLAG_ALL_EMITTERS) != 0;
}
// The table, at the first render whose flags ask for it (the caller has set the scene's device and holds the workspace's lock); more than
// 2^26 entries: FW_ERR_UNSUPPORTED, before any launch
static int ensure_emitters(fw_scene *sc, const fw_render_params *p, const Workspace *ws) {
    if (!all_emitters_asked(p)) return FW_OK;
    if (sc->n_entries > fw::EMITTER_MAX_ENTRIES) return fail(FW_ERR_UNSUPPORTED, "FW_FLAG_ALL_EMITTERS: more than 2^26 emitter entries");
    if (!sc->ls_vertices || sc->emit_state != 0) return FW_OK;
    if (sc->n_entries == 0) { sc->emit_state = 2; return FW_OK; }
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = build_emitter_table(sc, ws->ev_upload)) return rc;
    sc->emit_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (options().trace) fprintf(stderr, "[firework] emitter table: %llu entries, %u of positive weight, %.2f ms\n", (unsigned long long)sc->n_entries, sc->emit_cols, sc->emit_build_ms);
    return FW_OK;
}
// FW_FLAG_ALL_EMITTERS takes effect with FW_FLAG_LIGHT_SAMPLING where some entry has positive weight and a material's vertices
// sample lights; otherwise the frame is the frame without the bit (ensure_emitters has run)
static bool all_emitters(const fw_scene *sc, const fw_render_params *p) {
    return all_emitters_asked(p) && sc->emit_state == 1 && sc->ls_vertices;
}

// render_impl's lanes (batches in flight) and paths per batch and lane for `p` (fw_render_views sizes its view groups by the same budget)
struct BatchBudget { int n_lanes; bool exact_product; uint32_t budget; };
BatchBudget batch_budget(const fw_scene *sc, const fw_render_params *p, const Options &O, size_t arena_bytes) {
    int n_lanes = 2;     // (render_impl: why two)
    if (O.streams >= 1) n_lanes = std::min(O.streams, (int)Workspace::MAX_LANES);
    n_lanes = (int)std::min<uint32_t>((uint32_t)n_lanes, p->samples);
    // EXACT_PRODUCT: 160 more bytes per slot (ten attenuation records) where the scene has no chain state: half the default batch
    const bool exact_product = O.exact_product && (sc->chain_bits == 0 || O.no_chain);
    // light sampling: 92 more bytes per slot (fw::DShadow) — half the default batch as well (and so with environment sampling)
    const bool ls = light_sampling(sc, p) || env_sampling(sc, p) || all_emitters(sc, p) || delta_lights(sc);
    const uint32_t budget = p->paths_per_batch ? p->paths_per_batch : default_paths_per_batch(O, arena_bytes) / (uint32_t)n_lanes / (exact_product || ls ? 2u : 1u);
    return BatchBudget{n_lanes, exact_product, budget};
}

// One round of fw_render_adaptive (adaptive_impl), rendered by render_impl: the samples [first_sample, first_sample + samples) of the
// n pixels of a device-resident id list (nullptr: pixels 0..n-1), added to whole-frame sums and squares (k_accumulate_adaptive).  The
// caller holds the workspace's lock.  A round does no id validation, no copy of the list, no resolve, never runs as a frame graph, and
// clears the cached frame-graph key if it grows the path arena.
struct AdaptiveRound { const uint32_t *ids; uint32_t n; float4 *accum, *moments; };

// One view group of fw_render_views (views_impl), rendered by render_impl: n views of the frame `p` describes, view v seen through cams[v]
// (host memory, make_camera's).  The frame's pixel space is n x N entries, view-major (N = one view's pixels); the key of every path is
// that of its real pixel, so each view is the fw_render of its camera.  The outputs are the group's n x N x 3 values.
struct ViewGroup { const fw::DCamera *cams; uint32_t n; };

// The caller's rays of fw_render_rays (rays_impl), rendered by render_impl: a frame of n entries (p: width n, height 1, no camera, no
// pixel ids) whose paths start from `rays` (per_sample: sample-major, rays[s] of the call's sample first_sample + s; otherwise one ray
// per entry) instead of the camera's, keyed by keys[i] or key_base + i.  on_device: rays and keys are device pointers (p's outputs and
// accum follow p->outputs_on_device).  Entries stay in ray order (no tile order), the rays take the exact walk by fw_trace_rays' rule,
// and the frame never runs as a frame graph; the cached graph's key is cleared if the call grows the path arena.
struct RayInput { const float *rays; uint32_t n; bool per_sample; const uint32_t *keys; uint32_t key_base; bool on_device; };

// first_sample / user_accum: fw_render_progressive (0 / nullptr for a plain render); rd: a round of fw_render_adaptive; vg: a view group of
// fw_render_views; ri: the rays of fw_render_rays
int render_impl(fw_scene *sc, const fw_render_params *p, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats,
                uint32_t first_sample = 0, float *user_accum = nullptr, const AdaptiveRound *rd = nullptr, const ViewGroup *vg = nullptr,
                const RayInput *ri = nullptr) {
    if (!sc || !p) return fail(FW_ERR_BAD_ARG, "null argument");
    if (p->width == 0 || p->height == 0 || p->samples == 0) return fail(FW_ERR_BAD_ARG, "width, height and samples must be > 0");
    if (!(p->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be > 0");
    if (p->rng_mode != FW_RNG_CTR) return fail(FW_ERR_UNSUPPORTED, "the HIP path implements FW_RNG_CTR only (FW_RNG_LCG is a sequential stream)");
    uint64_t full = (uint64_t)p->width * p->height;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    const uint32_t n_view = rd ? rd->n : ri ? ri->n : (p->pixel_ids ? p->n_pixels : (uint32_t)full);     // the pixels of one view
    if (n_view == 0) return fail(FW_ERR_BAD_ARG, "no pixels to render");
    if ((uint64_t)first_sample + p->samples > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_sample + samples overflows");
    if (p->pixel_ids) for (uint32_t i = 0; i < n_view; i++) if (p->pixel_ids[i] >= full) return fail(FW_ERR_BAD_ARG, "pixel id out of range");
    // a view group's pixel space; key_of_linear and k_raygen_views find a path's entry from a float quotient whose int32 fix-up needs
    // 2 n_pix < 2^31 (the sample quotient's own bound, spp_batch < 2^21, is checked below with the batch size)
    if (vg && (uint64_t)n_view * vg->n >= (1ull << 30)) return fail(FW_ERR_UNSUPPORTED, "too many pixels in one view group");
    const uint32_t n_pix = vg ? n_view * vg->n : n_view;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(sc->device));
    hipStream_t stream = (hipStream_t)p->stream;
    Workspace *ws = workspace_for(sc->device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::unique_lock<std::mutex> ws_guard(ws->mu, std::defer_lock);
    if (!rd) ws_guard.lock();                                                        // (an adaptive round's caller holds it)
    { const int irc = init_device_locked(ws, sc->device); if (irc) return irc; }     // after fw_release_workspace, or a scene made before it
    if (!rd) ws->kernels.clear();                                                    // (an adaptive call's rounds add up: adaptive_impl clears)
    const bool dl = delta_lights(sc);
    if (dl && (p->flags & (FW_FLAG_ENV_SAMPLING | FW_FLAG_ALL_EMITTERS)))
        return fail(FW_ERR_UNSUPPORTED, "point, spot and directional lights do not combine with FW_FLAG_ENV_SAMPLING or FW_FLAG_ALL_EMITTERS");
    if (int erc = ensure_emitters(sc, p, ws)) return erc;     // (first: its FW_ERR_UNSUPPORTED comes before any launch)
    if (int erc = ensure_env_dist(sc, p, ws)) return erc;
    const Options O = options();

    // ---- batches and lanes -----------------------------------------------------------------------------------
    // Two batches in flight on two streams under use_bvh: the tree walks leave issue slots and HBM idle (the LDS-resident
    // ones run 4 waves per SIMD) that the other batch's k_shade / k_extend_scan fills.  Full-size configs, interleaved on one
    // box (tools/configs.sh): suzanne 92.2 -> 81.1 ms, random_spheres 2.0 -> 1.8, part2 2287 -> 2271; 3 or 4 lanes gain less.
    // The linear scan stays at one batch in flight: cornell gains 4-5 % (42.2 -> 40.3 ms), hdri and volume lose 1-3 %
    // (both of their kernels wait for HBM), and with one lane every kernel's HIP-event time is its own — what bench.py's
    // roofline object divides by.  FIREWORK_STREAMS=n overrides.  Results do not depend on n (batches accumulate in order).
    // Round 3: a linear scene whose scan runs the box lists (k_extend_linear_defer: cornell) takes two lanes as well — its scan is
    // bound by instruction issue, its k_shade by HBM, and they overlap (42.2 -> 40.3 ms in round 2's A/B); per-kernel times for
    // the roofline come from an exclusive pass (FIREWORK_STREAMS=1) that bench.py runs next to the timed loop.
    // (Small frames too: random_spheres, 5.8 M paths, 1.83 ms in two batches against 1.92-1.97 in one, round 3.)
    // Round 5: two lanes for every scene.  hdri and volume (linear scans without box lists) had lost 1-3 % with two in rounds 2-4; with the
    // XCD-contiguous queues and the SIMPLE-set scans they gain: hdri 32.4-33.4 -> 31.0-32.0 ms, volume 33.8-36.1 -> 32.4-34.2 (each setting twice in a
    // row on a box whose processes alternate between two k_shade modes: profiles/r05k_lanes2.txt).
    const BatchBudget bb = batch_budget(sc, p, O, ws->arena.bytes);
    int n_lanes = bb.n_lanes;
    // light sampling: a path deposits its visible light samples with its own end, so the frame keeps the running product (no
    // chain state, no EXACT_PRODUCT records), deposits every path (no elided zeros) and keeps t in its hit records (no hit4).  Environment
    // sampling (§9h) takes the same frame: ls = either; es = the environment is among the sampled lights (k_shade_env).  Every emitter (§9i):
    // pl = the entries replace §9g's lights (k_shade_pl, k_shade_pl_env)
    const bool pl = all_emitters(sc, p);
    const bool ls_lights = !pl && light_sampling(sc, p), es = env_sampling(sc, p);
    // Delta lights (§9l): dl = the scene's are active (k_shade_dl; never with es or pl), beside §9g's emitters where ls_lights
    const bool ls = ls_lights || es || pl || dl;
    const bool exact_product = bb.exact_product && !ls;
    const uint32_t budget = bb.budget;
    uint32_t spp_b = std::max<uint32_t>(1u, budget / n_pix);
    spp_b = std::min(spp_b, (p->samples + (uint32_t)n_lanes - 1) / (uint32_t)n_lanes);     // at least one batch per lane
    // (caller rays: k_raygen_rays finds a fixed ray's entry from the sample quotient, exact only while spp_batch < 2^21 — key_of_linear's
    //  bound.  Batching changes no result: the sums are taken in sample order whatever the batches)
    if (ri) spp_b = std::min(spp_b, (1u << 21) - 1u);
    uint64_t paths64 = (uint64_t)n_pix * spp_b;
    if (paths64 > 0x7fffffffull) return fail(FW_ERR_UNSUPPORTED, "too many paths per batch");
    uint32_t max_paths = (uint32_t)paths64;
    uint32_t n_batches = (p->samples + spp_b - 1) / spp_b;
    // equal batches (round 4): 512 samples at up to 145 per batch were 145 + 145 + 145 + 77; four times 128 keep the two lanes level, and the
    // pools — sized by the largest batch, with a power of two of chunks per wave — shrink with it (suzanne: 73 -> 37 GB; the arena no longer
    // has to grow between cornell and suzanne: hipFree of a 35 GB arena cost 2.4 s of the caller's time)
    spp_b = (p->samples + n_batches - 1) / n_batches;
    max_paths = n_pix * spp_b;
    n_lanes = (int)std::min<uint32_t>((uint32_t)n_lanes, n_batches);
    if (vg && spp_b >= (1u << 21)) return fail(FW_ERR_UNSUPPORTED, "too many samples per batch for a view group");   // (the quotients: key_of_linear, dep_bit_of)

    // the exact walk: ill-conditioned mesh rays in any mode, far origins and "every ray" (FIREWORK_EXACT_ALL) under use_bvh only
    // (the linear scan tests every object anyway: only a mesh's BLAS is walked there)
    // (FIREWORK_FUSED=1, the one-launch-per-segment A/B kernel, has no second pass: it runs without the exact walk)
#if FW_AB
    const bool fused_req = O.fused && !ls && !(p->use_bvh && sc->d.has_mesh) && !sc->has_ggx;      // (k_bounce has no GgxMat)
    const bool tlas_refill = !O.tlas_refill_off;
#else
    const bool fused_req = false, tlas_refill = true;
#endif
    // (caller rays: fw_trace_rays' rule — under use_bvh the flag rule stays on (EX_TRACE_ZERO) for rays with a zero direction component,
    //  which caller rays along an axis have and camera rays practically never)
    const uint32_t exact_mode = fused_req ? 0u : ((sc->ex.mode & 1u) | (p->use_bvh ? (sc->ex.mode & 6u) | (ri ? fw::EX_TRACE_ZERO : 0u)
                                                                                   : ((sc->ex.mode & 4u) && sc->d.has_mesh ? 4u : 0u)));
    // FUSE_SEGMENTS=1: a batch's 11 x (extend, shade) as ONE launch of k_segments_boxlist (fw_kernels.hip; DESIGN §5 "Fused segments") where
    // the frame takes k_extend_linear_defer and k_shade<1,1,*> and nothing else between k_raygen and k_accumulate: no trees, no exact walk,
    // no light sampling, no GgxMat, and neither per-launch timing nor the one-path dump, which want the launches apart.  An ineligible frame
    // keeps its launches.  Decided here, before the queue count, which follows from it.  Off by default: DESIGN §8.
    const bool timing = (p->flags & FW_FLAG_TIME_KERNELS) != 0;
#if FW_AB
    const bool stagger = n_lanes > 1 && O.stagger;   // experiment: batch b's first k_extend waits for batch b-1's
#else
    const bool stagger = false;
#endif
    // FIREWORK_DUMP_PATH=file, one pixel x one sample: after every k_extend the path's ray, state and hit record are copied out
    // and written to `file` as 11 x 16 floats (ray_a[4] ray_b[2] state[4] hit[2] alive pad[3]) behind a header of 8 u32
    // (magic, pinhole0, hit4, prim_bits, bits of cam_pos[3], n_defer).  Debug aid of tools/diverge.py; never on a timed path.
    const char *dump_file = O.dump_path.c_str();
    const bool dump_one = *dump_file && n_pix == 1 && p->samples == 1 && !fused_req;
    fw::LaunchCfg cfg{};
    {
        fw::DQueue none{};
        set_walk_cfg(cfg, sc, O, none, p->use_bvh != 0, tlas_refill);      // (again below, with the queues)
        cfg.shade_mode = frame_shade_mode(sc, O, 0u); cfg.gx = sc->has_ggx;
    }
    const bool fuse_segments = O.fuse_segments == 1 && !p->use_bvh && exact_mode == 0 && !ls && !fused_req && !stagger && !timing && !dump_one &&
                               fw::can_fuse_segments(cfg, sc->d);
    // wave-private queues: many more waves than are resident, each owning >= 8 chunks of 64 paths when the batch allows
    fw::DQueue q{};
    constexpr uint64_t BIG_BATCH_CHUNKS = 1u << 20;     // batches of 67 M paths and more (what the counts below were measured at: 134 M)
    // How many: whole rounds of resident waves for BOTH queue kernels (k_extend_linear holds 7 waves per SIMD, k_extend_bvh 5,
    // k_shade 4 -> multiples of lcm x SIMDs), and 16-50 chunks per wave so that the half-empty last chunk of a queue stays
    // small; measured on cornell (tools/waves_sweep.sh): whole frame 86 016 waves 41.1 ms vs 131 072: 42.0; the 1/4 share of
    // a 4-GPU frame 57 344: 12.7 vs 13.7 ms; the 1/8 share 28 672: 6.30 vs 6.67 ms.
    const uint32_t unit = (uint32_t)sc->n_cus * 4u * (p->use_bvh ? 20u : 28u);
    const uint64_t chunks = ((uint64_t)max_paths + 63u) / 64u;
    uint32_t want_waves = unit * (uint32_t)std::min<uint64_t>(3u, std::max<uint64_t>(1u, chunks / ((uint64_t)unit * 16u)));
    // Round 4 (gpurun_out/r04i/share_waves.txt, r04j/cornell_waves.txt): with TWO batches in flight on a linear scene (the box lists: cornell)
    // fewer, longer queues overlap better — whole frame 86 016 waves 36.4-37.0 ms, 28 672: 35.2-35.3 (its exclusive pass is slower: 40.6 vs
    // 37.8) — and a small share keeps its queues long with 12 288: rank 0's eighth of the frame 5.9 -> 5.5 ms (79 -> 85 % of ideal).
    if (!p->use_bvh && n_lanes > 1) want_waves = chunks >= BIG_BATCH_CHUNKS ? unit : (uint32_t)sc->n_cus * 48u;
    // The kernels have changed since (k_extend 17.1 -> 13.7 ms), and the big box-list batches of the cheap shading mode (cornell: k_extend_linear_defer and
    // k_shade<1,1,*>) now run faster on twice the queues (profiles/fused_segments_ab.txt, seven interleaved rounds at 134 M paths per batch:
    // 28 672 queues 31.15 ms, 57 344: 30.15, 86 016: 30.89; an earlier set 114 688: 31.59).  Other scenes and smaller batches: not measured, as they were.
    if (!p->use_bvh && n_lanes > 1 && chunks >= BIG_BATCH_CHUNKS && cfg.n_defer > 0 && cfg.shade_mode == 1 && !ls) want_waves = 2u * unit;
    // A fused frame wants MORE queues still: with one round of resident waves it is slower than its two kernels apart.  Same file: 6 144 queues 39.2 ms, 12 288: 35.4, 28 672: 31.5, 57 344: 29.98,
    // 86 016: 29.85, 114 688: 29.61, 229 376: 30.5.  (Why more rounds help was not looked into: that waves of later rounds sit in other phases
    // is a guess.)  A smaller batch keeps the count it has.
    if (fuse_segments && chunks >= BIG_BATCH_CHUNKS) want_waves = 4u * unit;
    if (O.waves > 0) want_waves = (uint32_t)O.waves;
    q.n_waves = std::max(4u, std::min(want_waves, (max_paths + 511u) / 512u));
    q.n_waves = (q.n_waves + 7u) & ~7u;       // a multiple of 8: one contiguous eighth of the queues per XCD (fw_kernels.hip: wave_index)
    uint32_t chunks_per_wave = (max_paths + q.n_waves * 64u - 1) / (q.n_waves * 64u);
    q.cpw_shift = 0;
    while ((1u << q.cpw_shift) < chunks_per_wave) q.cpw_shift++;      // power of two: chunk -> (wave, row) is a shift
    q.cap = 64u << q.cpw_shift;
    uint64_t cap64 = (uint64_t)q.cap * q.n_waves;
    if (cap64 > 0x7fffffffull) return fail(FW_ERR_UNSUPPORTED, "too many path slots");
    uint32_t cap = (uint32_t)cap64;

    const bool park_meshes = p->use_bvh && sc->d.has_mesh != 0 && tlas_refill;
    const bool stage_rays = ri && ri->per_sample && !ri->on_device;      // host rays of every sample: one batch's slab per lane
    int rc = FW_OK;
    auto need = [&](DevBuf &b, size_t n) { if (!rc) rc = b.alloc(n); };
    // the lanes' buffers: slices of the workspace's arena (Workspace::Lane), laid out twice — sizes first, then pointers
    auto layout = [&](uint8_t *arena_base) -> size_t {
        size_t off = 0;
        auto put = [&](void *&dst, size_t n) { dst = arena_base ? arena_base + off : nullptr; off += (n + 255) & ~(size_t)255; };
        for (int l = 0; l < n_lanes; l++) {
            Workspace::Lane &L = ws->lanes[l];
            for (int k = 0; k < 2; k++) { put(L.ray_a[k], (size_t)cap * 16); put(L.ray_b[k], (size_t)cap * 8); put(L.state[k], (size_t)cap * 16); }
            put(L.hits, (size_t)cap * 8);
            put(L.sample_rad, (size_t)cap * 16);              // indexed by home slot
            put(L.dep_bits, ((size_t)cap + 31) / 32 * 4);     // one bit per slot: "a radiance record was written here" (black environments)
            if (exact_product && !fused_req) put(L.atten, (size_t)cap * (fw::MAX_SEGMENTS - 1) * fw::B_ATTEN); else L.atten = nullptr;
            if (exact_mode) put(L.exact_slots, 2 * (size_t)max_paths * 4 + 64);   // two lists of at most every ray of a segment, + the counters
            put(L.wcount, (size_t)(fw::MAX_SEGMENTS + 1) * q.n_waves * 4);
            if (stage_rays) put(L.rays, (size_t)max_paths * 24); else L.rays = nullptr;
            if (ls) {
                put(L.s_ray_a, (size_t)cap * 16); put(L.s_ray_b, (size_t)cap * 8); put(L.s_state, (size_t)cap * 16); put(L.s_obj, (size_t)cap * 4);
                put(L.s_hits, (size_t)cap * 8); put(L.s_wcount, (size_t)(fw::MAX_SEGMENTS + 1) * q.n_waves * 4);
                put(L.pb[0], (size_t)cap * 4); put(L.pb[1], (size_t)cap * 4); put(L.nee, (size_t)cap * 16);
            }
            if (park_meshes) {     // rays handed from k_extend_scan / k_extend_tlas_park to k_blas*: 40 B per slot
                const size_t pcap = (size_t)(q.cap + 64u) * q.n_waves;     // park regions: q.cap + 64 entries per queue (DPark.stride)
                put(L.park_a, pcap * 16); put(L.park_b, pcap * 8); put(L.park_m, pcap * 16); put(L.pcount, (size_t)q.n_waves * 8);   // pcount[n_waves] + ptotal[n_waves]
            }
        }
        return off;
    };
    {
        size_t want = (layout(nullptr) + ((size_t)1 << 30) - 1) & ~(((size_t)1 << 30) - 1);
        // Round 5: the arena is sized by what is asked of it — fw_init(device, bytes) where the host reserved one, else this call's own
        // layout — and grows by a quarter at least, the new allocation made first and the old one freed on a background thread
        // (arena_reserve_locked): hipFree + hipMalloc in line cost 2.8 s for 35 -> 36 GiB (gpurun_out/r04j/oneshot.txt).
        if (want > ws->arena.bytes && ws->arena.bytes) want = std::max(want, (ws->arena.bytes + ws->arena.bytes / 4 + ((size_t)1 << 30) - 1) & ~(((size_t)1 << 30) - 1));
        const auto ta = std::chrono::steady_clock::now();
        const bool grow = want > ws->arena.bytes;
        if (!rc && grow) rc = arena_reserve_locked(ws, sc->device, want);
        if ((rd || ri) && grow) { ws->fg.key = 0; ws->fg.seen = 0; }     // a later plain render never replays launches against the moved arena
        if (O.trace && grow) fprintf(stderr, "[firework] render: path arena grown to %.1f GiB in %.2f ms\n", (double)want / (double)(1 << 30),
                                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count());
        if (!rc) layout((uint8_t *)ws->arena.p);
    }
    for (int l = 0; l < n_lanes && !rc; l++)
        if (!ws->lanes[l].stream && n_lanes > 1) HIPCHK(hipStreamCreateWithFlags(&ws->lanes[l].stream, hipStreamNonBlocking));
    if (!rd) need(ws->accum, (size_t)n_pix * 16);
    need(ws->totals, (size_t)n_batches * fw::COUNT_STRIDE * 4);
    if (p->pixel_ids) need(ws->pixel_ids, (size_t)n_view * 4);
    // a whole frame is traced in the library's own 16x16-tile order (k_tile_order); k_resolve undoes it.  Not for progressive
    // renders: their accumulation buffer belongs to the caller and stays in pixel order.
    const bool own_order = !p->pixel_ids && !user_accum && !rd && !ri && n_view >= 1024 && !O.no_tile_order;
    if (own_order) { const void *before = ws->tile_ids.p; need(ws->tile_ids, (size_t)n_view * 4); if (ws->tile_ids.p != before) ws->tile_w = ws->tile_h = 0; }
    if (vg) { need(ws->view_ids, (size_t)n_pix * 4); need(ws->view_cams, (size_t)vg->n * sizeof(fw::DCamera)); }
    const bool ray_table = ri && (ri->keys || ri->key_base != 0);       // (keys 0..n-1 need no table: key_of_linear's p_local)
    if (ri) {
        need(ws->ray_err, 256);
        if (ray_table) need(ws->ray_keys, (size_t)n_pix * 4);
        if (!ri->per_sample && !ri->on_device) need(ws->ray_fixed, (size_t)n_pix * 24);
        const size_t host_bytes = ri->on_device ? 0 : ri->per_sample ? (size_t)n_lanes * max_paths * 24 : (size_t)n_pix * 24;
        if (!rc && ws->ray_host_bytes < host_bytes) {
            if (ws->ray_host) (void)hipHostFree(ws->ray_host);
            ws->ray_host = nullptr; ws->ray_host_bytes = 0;
            if (hipHostMalloc(&ws->ray_host, host_bytes, hipHostMallocDefault) != hipSuccess) return fail(FW_ERR_OOM, "pinned ray staging allocation failed");
            ws->ray_host_bytes = host_bytes;
        }
    }
    uint8_t *d_rgb8 = rgb8; float *d_gamma = gamma_rgb, *d_linear = linear_rgb;
    if (!p->outputs_on_device) {
        if (rgb8) { need(ws->out_rgb8, (size_t)n_pix * 3); d_rgb8 = (uint8_t *)ws->out_rgb8.p; }
        if (gamma_rgb) { need(ws->out_gamma, (size_t)n_pix * 12); d_gamma = (float *)ws->out_gamma.p; }
        if (linear_rgb) { need(ws->out_linear, (size_t)n_pix * 12); d_linear = (float *)ws->out_linear.p; }
    }
    if (rc) return rc;
    while (ws->events.size() < 3 + 2 * (size_t)n_batches) {      // [3 + b] accumulated, [3 + n_batches + b] batch b's first k_extend finished (stagger)
         hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, ws->events.size() < 2 ? hipEventDefault : hipEventDisableTiming)); ws->events.push_back(e); }

    if (ws->ev_upload) HIPCHK(hipStreamWaitEvent(stream, ws->ev_upload, 0));     // the scene's upload kernel (null stream)
    if (p->pixel_ids) HIPCHK(hipMemcpyAsync(ws->pixel_ids.p, p->pixel_ids, (size_t)n_view * 4, hipMemcpyHostToDevice, stream));
    if (own_order && (ws->tile_w != p->width || ws->tile_h != p->height)) {
        ws->tile_w = ws->tile_h = 0;                                               // invalid until the launch below has been queued
        fw::launch_tile_order(stream, p->width, p->height, (uint32_t *)ws->tile_ids.p);
        ws->tile_w = p->width; ws->tile_h = p->height;
    }
    // a view group: one view's ids (the caller's, the tile order or row order) repeated per view, and the group's cameras, written in
    // stream order before the frame's launches
    if (vg) {
        fw::launch_view_ids(stream, p->pixel_ids ? (const uint32_t *)ws->pixel_ids.p : (own_order ? (const uint32_t *)ws->tile_ids.p : nullptr), n_view, n_pix,
                            (uint32_t *)ws->view_ids.p);
        HIPCHK(hipMemcpyAsync(ws->view_cams.p, vg->cams, (size_t)vg->n * sizeof(fw::DCamera), hipMemcpyHostToDevice, stream));
    }
    // caller rays: the error word, the key table (the caller's keys, or key_base + i) and fixed host rays, in stream order before the frame
    if (ri) {
        HIPCHK(hipMemsetAsync(ws->ray_err.p, 0, 4, stream));
        if (ri->keys) HIPCHK(hipMemcpyAsync(ws->ray_keys.p, ri->keys, (size_t)n_pix * 4, ri->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        else if (ray_table) fw::launch_ray_keys(stream, ri->key_base, n_pix, (uint32_t *)ws->ray_keys.p);
        if (!ri->per_sample && !ri->on_device) {
            std::memcpy(ws->ray_host, ri->rays, (size_t)n_pix * 24);
            HIPCHK(hipMemcpyAsync(ws->ray_fixed.p, ws->ray_host, (size_t)n_pix * 24, hipMemcpyHostToDevice, stream));
        }
    }
    if (user_accum)     // resume: the sums of the samples rendered so far (host or device memory, like the outputs)
        HIPCHK(hipMemcpyAsync(ws->accum.p, user_accum, (size_t)n_pix * 16, p->outputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    else if (!rd) HIPCHK(hipMemsetAsync(ws->accum.p, 0, (size_t)n_pix * 16, stream));
    HIPCHK(hipMemsetAsync(ws->totals.p, 0, (size_t)n_batches * fw::COUNT_STRIDE * 4, stream));

    set_walk_cfg(cfg, sc, O, q, p->use_bvh != 0, tlas_refill);
    cfg.log = &ws->kernels;
    int max_blocks = sc->n_cus * 8;
    cfg.blocks_other = (int)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n_pix + fw::BLOCK - 1) / fw::BLOCK, (uint64_t)max_blocks));
    // k_shade's list entries are 16-bit queue positions: longer queues (cap > 65536: never with the default geometry) shade in line
    // Default: the cheap loop alone where the scene has nothing expensive (cornell k_shade -5 %), everything in line otherwise — the
    // list (mode 2) is slower wherever it was measured (gpurun_out/r03h: part2@16 11.7 -> 12.0 ms, hdri@64 5.5 -> 6.1, random_spheres
    // 1.90 -> 1.98, volume@64 6.08 -> 6.12) and stays behind FIREWORK_SHADE_LIST=1; FIREWORK_NO_SHADE_DEFER=1 forces mode 0.
    cfg.shade_mode = frame_shade_mode(sc, O, q.cap);
    cfg.gx = sc->has_ggx;

    fw::DCamera cam = vg ? vg->cams[0] : ri ? fw::DCamera{} : make_camera(p->camera, p->width, p->height);
    fw::DFrame fr{};         // (zeroed: the frame graph's key hashes these structs, padding and not-yet-set per-batch fields included)
    fr.width = p->width; fr.height = p->height; fr.n_pixels = n_pix; fr.inv_n_pixels = 1.0f / (float)n_pix; fr.inv_width = 1.0f / (float)p->width;
    fr.pixel_ids = rd ? rd->ids : vg ? (const uint32_t *)ws->view_ids.p : ri ? (ray_table ? (const uint32_t *)ws->ray_keys.p : nullptr)
                 : (p->pixel_ids ? (const uint32_t *)ws->pixel_ids.p : (own_order ? (const uint32_t *)ws->tile_ids.p : nullptr));
    fr.scatter_out = own_order ? 1u : 0u;
    fr.seed32 = seed32_of(p->seed);
    fr.q_n_waves = q.n_waves; fr.q_shift = q.cpw_shift;
    fr.cam_pos[0] = cam.position[0]; fr.cam_pos[1] = cam.position[1]; fr.cam_pos[2] = cam.position[2];
    // (what must not occur in the position is a NEGATIVE zero: -0 + (+0) = +0 is not the position any more, while +0 + (+-0) = +0 is.  Until round 5
    //  this read "!= 0.f", which kept hdri_test's and volume_test's cameras — at x = 0.0 — on 24-byte camera rays)
    auto not_negative_zero = [](float x) { uint32_t b; std::memcpy(&b, &x, 4); return b != 0x80000000u; };
    // (a view group: the 16-byte rays stand for one position, so every view must be a pinhole at cam's position, bit for bit; otherwise the
    //  24-byte form, which gives the same bits)
    bool one_position = true;
    if (vg) for (uint32_t v = 1; v < vg->n; v++) one_position = one_position && vg->cams[v].lens_radius == 0.f && std::memcmp(vg->cams[v].position, cam.position, sizeof cam.position) == 0;
    fr.pinhole0 = (!ri && one_position && cam.lens_radius == 0.f && not_negative_zero(cam.position[0]) && not_negative_zero(cam.position[1]) && not_negative_zero(cam.position[2]) &&
                   !O.no_short_rays) ? 1u : 0u;
    // 4-byte hit records where k_shade can recompute t cheaply and exactly: the linear scan over spheres, rects and Rect3d
    fr.hit4 = (!p->use_bvh && sc->simple_shapes && !exact_mode && !O.no_hit4 && !fused_req && !ls) ? 1u : 0u;
    const fw::DEnv &env = sc->d.env;
    // (pixel-major bits need the sample index of a path from a float quotient that is exact only while spp_batch < 2^21: dep_bit_of)
    fr.dep_pixel_major = (((n_pix <= 65536u && !O.dep_slot_major) || O.dep_pixel_major) && spp_b < (1u << 21)) ? 1u : 0u;
    fr.ex = sc->ex; fr.ex.mode = exact_mode;
    fr.chain_bits = (O.no_chain || fused_req || cfg.shade_mode == 2 || ls) ? 0u : sc->chain_bits;      // k_bounce and k_shade's list mode (A/B build) carry the running product
    fr.skip_zero_deposits = (env.kind == 0 && env.color[0] == 0.f && env.color[1] == 0.f && env.color[2] == 0.f && !O.no_zero_skip && !ls) ? 1u : 0u;

    // per-launch timing (FW_FLAG_TIME_KERNELS, `timing` above): one event after every launch on the launch's own stream; the end of
    // launch k is the start of launch k+1 of that lane.  With several lanes the intervals overlap in wall time.
    const bool count_deposits = (p->flags & FW_FLAG_COUNT_DEPOSITS) != 0 && fr.skip_zero_deposits != 0;   // otherwise every terminated path writes one
    const size_t per_batch_launches = 1 + 3 * fw::MAX_SEGMENTS + 2 + (ls ? 2 * (fw::MAX_SEGMENTS - 1) : 0);     // raygen, 11 x (extend, exact extend, shade), queue totals, accumulate; light sampling: 10 x (shadow walk, resolve)
    std::vector<std::vector<int>> ev_class(n_lanes);   // per lane: class of the launch that ENDS at events[1 + k]
    std::vector<size_t> ev_next(n_lanes, 0);
    if (timing) for (int l = 0; l < n_lanes; l++) {
        size_t want = 1 + per_batch_launches * ((n_batches + n_lanes - 1) / n_lanes);
        auto &ev = ws->lanes[l].events;
        while (ev.size() < want) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); }
    }
    const bool use_bvh = p->use_bvh != 0;
    // FIREWORK_FUSED=1: one launch per segment (k_bounce = intersect + shade in registers, 80 instead of 120 B per ray).
    // Off by default: the frame is VALU-bound, not HBM-bound, and the fused kernel's lower occupancy costs more than the
    // bytes save (cornell 62.0 vs 55.5 ms, hdri 35.5 vs 38.5 ms, 1/8-frame shares 9.2 vs 8.3 ms).  Never with parked mesh rays.
    const bool fused = fused_req;
    std::vector<float> dump_rec(dump_one ? (size_t)fw::MAX_SEGMENTS * 16 : 0, 0.f);

    HIPCHK(hipEventRecord(ws->events[0], stream));
    hipStream_t origin = stream;       // the stream the frame's launches fork from and join: the caller's, or the capture's own (GRAPH)
    bool graph_replayed = false;       // this frame's launches went out as one hipGraphLaunch (fw_stats.reserved bit 31)
    auto fork_lanes = [&]() -> int {
        if (n_lanes > 1) {     // fork: the lane streams start after everything queued on the origin stream so far
            HIPCHK(hipEventRecord(ws->events[2], origin));
            for (int l = 0; l < n_lanes; l++) HIPCHK(hipStreamWaitEvent(ws->lanes[l].stream, ws->events[2], 0));
        }
        return FW_OK;
    };
    // The batches of a frame, n_lanes at a time.  Each batch's launches go to its lane's stream in order; the HOST enqueues a group segment by
    // segment (A.extend(s) A.shade(s) B.extend(s) B.shade(s) A.extend(s+1) ...), which changes nothing for independent streams and is what lets
    // PHASE_LOCK tie them: B's extend of a segment waits for A's extend of that segment, A's next extend for B's — so that an issue-bound
    // extend always runs beside the other batch's memory-bound shade (left alone, the two lanes drift INTO phase within three segments:
    // profiles/r05a_share_trace.txt).
    struct BatchCtx { fw::DFrame fr; fw::LaunchCfg cfg; fw::DPaths buf[2]; float2 *hits; float4 *srad; fw::DPark park; uint32_t *totals; uint32_t n_paths; int cur; int lane; hipStream_t ls;
                      fw::DShadow sh; fw::DEnvDist ed; fw::DEmitters em; fw::DDeltaLights dl; };
    // Measured (profiles/r05j_phase_lock.txt, three interleaved pairs): cornell 33.4-33.8 -> 32.2-32.4 ms — the lock holds the frame in the faster
    // of the two phases it otherwise lands in by chance (profiles/r05h_layout_pad.txt) —, where extend and shade last about as long as each
    // other.  Under use_bvh an extend lasts three shades and waiting for the other batch's costs: suzanne 62.7 -> 67.7, part2 @256 119.6 ->
    // 124.5, teapot @128 46.4 -> 47.9, random_spheres 1.64 -> 1.98.  And short launches pay for every wait: a rank's share of a cornell frame
    // (profiles/r05n_share_lock.txt, each setting twice) 1/4: 8.8 ms without the lock, 10.0 with it; 1/8: 4.5 vs 5.3; 1/2 (67 M paths per
    // batch): 16.7-16.8 vs 16.6 on one box, 16.3 vs 16.8-17.2 on another; the whole frame (134 M per batch) 33.4-33.8 vs 32.3-32.5.  Hence:
    // on for the box-list scenes of the linear scan when a batch holds PHASE_LOCK_MIN_CHUNKS chunks of 64 paths (between the two sizes it
    // was measured to pay and not to pay at), off elsewhere.
    constexpr uint64_t PHASE_LOCK_MIN_CHUNKS = 3u << 19;      // 100 M paths
    // (the lock ties launches that a fused frame, FUSE_SEGMENTS=1, does not have)
    const bool phase_lock = !fuse_segments && n_lanes == 2 && !fused && (O.phase_lock == 1 || (O.phase_lock < 0 && !p->use_bvh && cfg.n_defer > 0 && chunks >= PHASE_LOCK_MIN_CHUNKS));
    std::vector<hipEvent_t> &pe = ws->phase_events;
    while (phase_lock && pe.size() < 2 * (size_t)fw::MAX_SEGMENTS) { hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); pe.push_back(e); }
    float4 *const accum = rd ? rd->accum : (float4 *)ws->accum.p;
    auto begin_batch = [&](uint32_t b, BatchCtx &c) -> int {
        const int l = (int)(b % (uint32_t)n_lanes);
        Workspace::Lane &L = ws->lanes[l];
        c.lane = l; c.ls = n_lanes > 1 ? L.stream : origin;
        c.cfg = cfg; c.cfg.stream = c.ls; c.cfg.q.wcount = (uint32_t *)L.wcount;
        c.fr = fr;
        if (timing && ev_next[l] == 0) (void)hipEventRecord(L.events[0], c.ls);
        c.fr.sample0 = first_sample + b * spp_b;
        c.fr.dep_bits = (uint32_t *)L.dep_bits;
        c.fr.atten = (c.fr.chain_bits == 0 && exact_product && !fused_req) ? (float4 *)L.atten : nullptr; c.fr.atten_stride = cap;
        if (c.fr.skip_zero_deposits) HIPCHK(hipMemsetAsync(c.fr.dep_bits, 0, ((size_t)cap + 31) / 32 * 4, c.ls));
        if (exact_mode) {
            c.fr.ex.slots[0] = (uint32_t *)L.exact_slots; c.fr.ex.slots[1] = c.fr.ex.slots[0] + max_paths;
            c.fr.ex.count = c.fr.ex.slots[1] + max_paths; c.fr.ex.cap = max_paths;
            HIPCHK(hipMemsetAsync(c.fr.ex.count, 0, 64, c.ls));
        }
        c.fr.spp_batch = std::min(spp_b, p->samples - b * spp_b);
        c.n_paths = n_pix * c.fr.spp_batch;
        c.totals = (uint32_t *)ws->totals.p + (size_t)b * fw::COUNT_STRIDE;
        for (int k = 0; k < 2; k++) c.buf[k] = {(float4 *)L.ray_a[k], (float2 *)L.ray_b[k], (float4 *)L.state[k]};
        c.hits = (float2 *)L.hits;
        c.srad = (float4 *)L.sample_rad;
        c.park = fw::DPark{(float4 *)L.park_a, (float2 *)L.park_b, (float4 *)L.park_m, q.cap + 64u, (uint32_t *)L.pcount,
                           park_meshes ? (uint32_t *)L.pcount + q.n_waves : nullptr};
        if (park_meshes) HIPCHK(hipMemsetAsync(c.park.ptotal, 0, (size_t)q.n_waves * 4, c.ls));
        c.sh = fw::DShadow{}; c.ed = fw::DEnvDist{}; c.em = fw::DEmitters{}; c.dl = fw::DDeltaLights{};
        if (ls) {
            // picking a light: the environment with p_env (1 alone, 1/2 beside emitters), each emitter with (1 - p_env) / n, each entry (§9i)
            // with (1 - p_env) p_i
            // the delta lights as a group (§9l) with p_delta (1 alone, 1/2 beside emitters), each emitter then with (1 - p_delta) / n
            const float p_env = es ? ((ls_lights || pl) ? 0.5f : 1.f) : (dl ? (ls_lights ? 0.5f : 1.f) : 0.f);
            if (dl) c.dl = fw::DDeltaLights{(const float4 *)sc->dlights.p, sc->n_dlights, p_env};
            if (pl) c.em = emitters_of(sc, p_env);
            c.sh.lt = ls_lights ? fw::DLights{(const uint32_t *)sc->lights.p, sc->n_lights, (es || dl) ? (1.f - p_env) / (float)sc->n_lights : 1.f / (float)sc->n_lights}
                                : fw::DLights{(const uint32_t *)sc->lights.p, 0u, 0.f};
            if (es) c.ed = env_dist_of(sc->env_dist, sc->d.env, p_env);
            c.sh.ray_a = (float4 *)L.s_ray_a; c.sh.ray_b = (float2 *)L.s_ray_b; c.sh.state = (float4 *)L.s_state; c.sh.obj = (uint32_t *)L.s_obj;
            c.sh.wcount = (uint32_t *)L.s_wcount; c.sh.nee = (float4 *)L.nee;
            HIPCHK(hipMemsetAsync(c.sh.nee, 0, (size_t)cap * 16, c.ls));
        }
        c.cur = 0;
        return FW_OK;
    };
    auto timed = [&](BatchCtx &c, int cls, auto &&launch) {
        launch();
        if (timing) { (void)hipEventRecord(ws->lanes[c.lane].events[1 + ev_next[c.lane]], c.ls); ev_next[c.lane]++; ev_class[c.lane].push_back(cls); }
    };
    // which: index of the batch inside its group (0 or 1 under PHASE_LOCK)
    auto segment = [&](uint32_t b, BatchCtx &c, int seg, int which, int group_size) -> int {
#if FW_AB
        if (fused) { timed(c, 2, [&] { fw::launch_bounce(c.cfg, sc->d, c.fr, c.buf[c.cur], c.buf[c.cur ^ 1], c.srad, seg, use_bvh); }); c.cur ^= 1; return FW_OK; }
#endif
        if (stagger && seg == 0 && b > 0) HIPCHK(hipStreamWaitEvent(c.ls, ws->events[3 + n_batches + b - 1], 0));   // start half a segment behind the batch before
        if (phase_lock && group_size == 2) {
            if (which == 1) HIPCHK(hipStreamWaitEvent(c.ls, pe[(size_t)seg], 0));                                     // B.extend(s) beside A.shade(s)
            else if (seg > 0) HIPCHK(hipStreamWaitEvent(c.ls, pe[(size_t)fw::MAX_SEGMENTS + (size_t)seg - 1], 0));   // A.extend(s) beside B.shade(s - 1)
        }
        timed(c, 1, [&] { fw::launch_extend(c.cfg, sc->d, c.fr, c.buf[c.cur], c.hits, seg, use_bvh, c.park); });
        if (phase_lock && group_size == 2) HIPCHK(hipEventRecord(pe[(size_t)which * fw::MAX_SEGMENTS + (size_t)seg], c.ls));
        if (stagger && seg == 0) HIPCHK(hipEventRecord(ws->events[3 + n_batches + b], c.ls));
        // the rays whose result depends on how the trees are walked (DExact), walked the reference's way: their hit records replaced
        if (exact_mode) timed(c, 1, [&] { fw::launch_extend_exact(c.cfg, sc->d, c.fr, c.buf[c.cur], c.hits, seg, use_bvh); });
        if (dump_one) {     // debug (tools/diverge.py): the one path of this call sits in slot 0 of wave 0 in every segment
            float *r = &dump_rec[(size_t)seg * 16];
            uint32_t alive = 0;
            HIPCHK(hipMemcpyAsync(&alive, c.cfg.q.wcount + (size_t)seg * q.n_waves, 4, hipMemcpyDeviceToHost, c.ls));
            HIPCHK(hipMemcpyAsync(r, c.buf[c.cur].ray_a, 16, hipMemcpyDeviceToHost, c.ls));
            HIPCHK(hipMemcpyAsync(r + 4, c.buf[c.cur].ray_b, 8, hipMemcpyDeviceToHost, c.ls));
            HIPCHK(hipMemcpyAsync(r + 6, c.buf[c.cur].state, 16, hipMemcpyDeviceToHost, c.ls));
            HIPCHK(hipMemcpyAsync(r + 10, c.hits, 8, hipMemcpyDeviceToHost, c.ls));
            HIPCHK(hipStreamSynchronize(c.ls));
            r[12] = (float)alive;
        }
        if (ls) {
            Workspace::Lane &L = ws->lanes[c.lane];
            c.sh.pb_in = (const float *)L.pb[c.cur]; c.sh.pb_out = (float *)L.pb[c.cur ^ 1];
            timed(c, 2, [&] { fw::launch_shade_nee(c.cfg, sc->d, c.fr, c.buf[c.cur], c.buf[c.cur ^ 1], c.hits, c.srad, seg, c.sh, es ? &c.ed : nullptr, pl ? &c.em : nullptr, dl ? &c.dl : nullptr); });
            if (seg < fw::MAX_SEGMENTS - 1) {     // segments 0-9 scatter (render.rs:21): their shadow rays through the ordinary walks, then the resolve
                fw::LaunchCfg scfg = c.cfg; scfg.q.wcount = c.sh.wcount;
                fw::DFrame sfr = c.fr; sfr.seed32 ^= fw::SHADOW_SEED; sfr.ex.mode = 0;
                const fw::DPaths sp{c.sh.ray_a, c.sh.ray_b, c.sh.state};
                timed(c, 1, [&] { fw::launch_extend(scfg, sc->d, sfr, sp, (float2 *)L.s_hits, seg + 1, use_bvh, c.park); });
                timed(c, 2, [&] { fw::launch_shadow_resolve(scfg, sc->d, c.sh, (const float2 *)L.s_hits, seg, es, pl, dl, c.srad); });
            }
        } else
        timed(c, 2, [&] { fw::launch_shade(c.cfg, sc->d, c.fr, c.buf[c.cur], c.buf[c.cur ^ 1], c.hits, c.srad, seg); });
        c.cur ^= 1;
        return FW_OK;
    };
    auto end_batch = [&](uint32_t b, BatchCtx &c) -> int {
        timed(c, 3, [&] { fw::launch_queue_totals(c.cfg, c.totals, c.park.ptotal); });       // reads this batch's queue counts: before the lane's next batch overwrites them
        if (count_deposits) fw::launch_count_deposits(c.cfg, c.fr.dep_bits, c.totals + 12);   // not a kernel class: after the last timed event of its neighbours
        // `total_color += color(..)` in sample order (render.rs:181): batch b is accumulated after batch b-1, whichever
        // lanes they ran on, so the image does not depend on the number of lanes or batches
        if (n_lanes > 1 && b > 0) HIPCHK(hipStreamWaitEvent(c.ls, ws->events[3 + b - 1], 0));
        if (rd) timed(c, 3, [&] { fw::launch_accumulate_adaptive(c.cfg, c.fr, c.srad, accum, rd->moments); });
        else timed(c, 3, [&] { fw::launch_accumulate(c.cfg, c.fr, c.srad, accum); });
        if (n_lanes > 1) HIPCHK(hipEventRecord(ws->events[3 + b], c.ls));
        return FW_OK;
    };
    // caller rays: where batch b's rays lie.  Host rays of every sample are copied into the lane's slab through the lane's pinned
    // slab, after the lane's previous batch has finished with both (a wait on the lane's stream: correct, not fast)
    auto batch_rays = [&](uint32_t b, const BatchCtx &c, const float *&src) -> int {
        if (!ri->per_sample) { src = ri->on_device ? ri->rays : (const float *)ws->ray_fixed.p; return FW_OK; }
        const size_t first = (size_t)b * spp_b * n_pix * 6, bytes = (size_t)c.n_paths * 24;
        if (ri->on_device) { src = ri->rays + first; return FW_OK; }
        HIPCHK(hipStreamSynchronize(c.ls));
        uint8_t *slab = (uint8_t *)ws->ray_host + (size_t)c.lane * max_paths * 24;
        std::memcpy(slab, ri->rays + first, bytes);
        HIPCHK(hipMemcpyAsync(ws->lanes[c.lane].rays, slab, bytes, hipMemcpyHostToDevice, c.ls));
        src = (const float *)ws->lanes[c.lane].rays;
        return FW_OK;
    };
    auto enqueue_frame = [&]() -> int {
    if (int frc = fork_lanes()) return frc;
    for (uint32_t b0 = 0; b0 < n_batches; b0 += (uint32_t)n_lanes) {
        const int group = (int)std::min<uint32_t>((uint32_t)n_lanes, n_batches - b0);
        BatchCtx ctx[Workspace::MAX_LANES];
        for (int g = 0; g < group; g++) {
            if (int brc = begin_batch(b0 + (uint32_t)g, ctx[g])) return brc;
            if (ri) {
                const float *src = nullptr;
                if (int src_rc = batch_rays(b0 + (uint32_t)g, ctx[g], src)) return src_rc;
                timed(ctx[g], 0, [&] { fw::launch_raygen_rays(ctx[g].cfg, src, ri->per_sample, (uint32_t *)ws->ray_err.p, ctx[g].fr, ctx[g].buf[0], ctx[g].n_paths); });
            }
            else if (vg) timed(ctx[g], 0, [&] { fw::launch_raygen_views(ctx[g].cfg, (const fw::DCamera *)ws->view_cams.p, n_view, ctx[g].fr, ctx[g].buf[0], ctx[g].srad, ctx[g].n_paths); });
            else timed(ctx[g], 0, [&] { fw::launch_raygen(ctx[g].cfg, cam, ctx[g].fr, ctx[g].buf[0], ctx[g].srad, ctx[g].n_paths); });
        }
        if (fuse_segments)
            for (int g = 0; g < group; g++) {
                BatchCtx &c = ctx[g];
                fw::launch_segments(c.cfg, sc->d, c.fr, c.buf[0], c.buf[1], c.hits, c.srad, 0, fw::MAX_SEGMENTS - 1);
                c.cur = fw::MAX_SEGMENTS & 1;
            }
        else
        for (int seg = 0; seg < fw::MAX_SEGMENTS; seg++)
            for (int g = 0; g < group; g++)
                if (int src = segment(b0 + (uint32_t)g, ctx[g], seg, g, group)) return src;
        for (int g = 0; g < group; g++)
            if (int erc = end_batch(b0 + (uint32_t)g, ctx[g])) return erc;
        fr = ctx[group - 1].fr;        // (the frame-level fields the code below reads are the same in every batch)
    }
    if (n_lanes > 1) HIPCHK(hipStreamWaitEvent(origin, ws->events[3 + n_batches - 1], 0));    // join
    return FW_OK;
    };
    // GRAPH: launch-bound frames (random_spheres: 37 launches of 10-80 us with ~6 us between them; a rank's eighth of a frame) replayed as
    // one graph.  The first time a frame is asked for it runs as ever; the second time in a row it is captured (on a stream of the
    // workspace's own: the caller's may be the legacy stream, which cannot be captured), instantiated and launched; from then on launched.
    // Any failure on the way turns the feature off for the workspace and the frame runs as ever.
    {
        Workspace::FrameGraph &fg = ws->fg;
        constexpr uint64_t GRAPH_MAX_CHUNKS = 1u << 19;      // batches below 33 M paths
        // (a view group of fw_render_views never runs as a frame graph: one call already spreads a frame's launches over all its views,
        //  and the groups of one call share a key, so a capture would be replayed inside the same call.  A group leaves the cached graph as it is)
        // (nor do the caller rays of fw_render_rays: their launches read the caller's memory, which a replay would not see change)
        const bool graph_ok = O.graph != 0 && !rd && !vg && !ri && !ls && !fg.broken && !timing && !dump_one && !phase_lock && !stagger && (O.graph == 1 || chunks < GRAPH_MAX_CHUNKS);   // (a capture with PHASE_LOCK's events crashed inside the runtime: the two never meet by default — the lock wants batches of 100 M paths)
        uint64_t key = 0;
        if (graph_ok) {
            uint64_t h = 1469598103934665603ull;
            auto mix = [&](const void *ptr, size_t n) { const unsigned char *b = (const unsigned char *)ptr; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
            fw::LaunchCfg kc = cfg; kc.stream = nullptr;
            mix(&cam, sizeof cam); mix(&fr, sizeof fr); mix(&kc, sizeof kc); mix(&sc->d, sizeof sc->d); mix(&q, sizeof q);
            const uint64_t scalars[] = {n_batches, (uint64_t)n_lanes, spp_b, first_sample, p->samples, n_pix, max_paths, cap, exact_mode, (uint64_t)park_meshes, (uint64_t)phase_lock, (uint64_t)fuse_segments,
                                        (uint64_t)count_deposits, (uint64_t)exact_product, (uint64_t)use_bvh, (uint64_t)fused, (uint64_t)stagger, (uint64_t)(uintptr_t)accum, (uint64_t)(uintptr_t)ws->totals.p,
                                        (uint64_t)(uintptr_t)ws->arena.p, (uint64_t)ws->arena.bytes};
            mix(scalars, sizeof scalars);
            for (int l = 0; l < n_lanes; l++) { const Workspace::Lane &L = ws->lanes[l]; const void *ptrs[] = {L.ray_a[0], L.ray_a[1], L.ray_b[0], L.ray_b[1], L.state[0], L.state[1], L.hits, L.sample_rad, L.wcount, L.park_a, L.park_b, L.park_m, L.pcount, L.dep_bits, L.exact_slots, L.atten}; mix(ptrs, sizeof ptrs); }
            key = h | 1ull;
        }
        bool done = false;
        if (graph_ok && fg.exec && fg.key == key) {
            HIPCHK(hipGraphLaunch(fg.exec, stream));
            fr = fg.fr_after; done = true; graph_replayed = true;
            ws->kernels.merge(fg.kernels);
        } else if (graph_ok && fg.seen == key) {
            if (!fg.origin && hipStreamCreateWithFlags(&fg.origin, hipStreamNonBlocking) != hipSuccess) { fg.origin = nullptr; fg.broken = true; }
            if (!fg.broken && hipStreamBeginCapture(fg.origin, hipStreamCaptureModeRelaxed) == hipSuccess) {
                origin = fg.origin;
                if (O.trace) fprintf(stderr, "[firework] GRAPH: capturing (%u batches, %d lanes, phase lock %d)\n", n_batches, n_lanes, (int)phase_lock);
                const fw::KernelLog before = ws->kernels;      // the capture alone: what the replays will report
                ws->kernels.clear();
                const int crc = enqueue_frame();
                fg.kernels = ws->kernels;
                ws->kernels.merge(before);
                origin = stream;
                hipGraph_t g = nullptr;
                const hipError_t ee = hipStreamEndCapture(fg.origin, &g);
                if (O.trace) fprintf(stderr, "[firework] GRAPH: capture ended: enqueue %d, end %s\n", crc, hipGetErrorString(ee));
                if (fg.exec) { (void)hipGraphExecDestroy(fg.exec); fg.exec = nullptr; fg.key = 0; }
                if (crc == FW_OK && ee == hipSuccess && g && hipGraphInstantiate(&fg.exec, g, nullptr, nullptr, 0) == hipSuccess) {
                    fg.key = key; fg.fr_after = fr;
                    (void)hipGraphDestroy(g);
                    if (O.trace) fprintf(stderr, "[firework] GRAPH: instantiated\n");
                    HIPCHK(hipGraphLaunch(fg.exec, stream));
                    if (O.trace) fprintf(stderr, "[firework] GRAPH: launched\n");
                    graph_replayed = true;
                    done = true;
                } else {
                    if (g) (void)hipGraphDestroy(g);
                    fg.exec = nullptr; fg.broken = true; (void)hipGetLastError();
                    if (O.trace) fprintf(stderr, "[firework] GRAPH: capture failed (%d, %s): frames run as plain launches from here on\n", crc, hipGetErrorString(ee));
                }
            } else { fg.broken = true; (void)hipGetLastError(); }
        }
        if (graph_ok) fg.seen = key;
        if (!done) { if (int frc = enqueue_frame()) return frc; }
    }
    cfg.stream = stream;
    if (vg) fw::launch_resolve_views(cfg, fr, n_view, (const float4 *)ws->accum.p, p->samples, p->gamma, d_rgb8, d_gamma, d_linear);
    else if (!rd) fw::launch_resolve(cfg, fr, (const float4 *)ws->accum.p, first_sample + p->samples, p->gamma, d_rgb8, d_gamma, d_linear);
    if (user_accum) HIPCHK(hipMemcpyAsync(user_accum, ws->accum.p, (size_t)n_pix * 16, p->outputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(ws->events[1], stream));
    HIPCHK(hipGetLastError());

    if (dump_one) {
        if (FILE *fp = fopen(dump_file, "wb")) {
            uint32_t hdr[8] = {0x46574450u, fr.pinhole0, fr.hit4, sc->d.prim_bits, 0, 0, 0, cfg.n_defer};
            std::memcpy(&hdr[4], fr.cam_pos, 12);
            fwrite(hdr, 4, 8, fp); fwrite(dump_rec.data(), 4, dump_rec.size(), fp); fclose(fp);
        }
    }
    const bool trace = O.trace;
    const auto tq0 = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    // Device -> host through PINNED memory, then a host memcpy into the caller's buffers.  A hipMemcpyAsync into pageable
    // memory blocks inside the runtime until the stream has drained, and that wait returned 15-30 ms late every few calls
    // (FIREWORK_TRACE=1, tools/oneshot.py: "counters copy returned +69 ms" for 43 ms of device work); with pinned
    // destinations the copies are queued and the only host wait is the hipStreamSynchronize below.
    const size_t n_counts = (size_t)n_batches * fw::COUNT_STRIDE;
    const size_t off_c = 0, off_8 = (n_counts * 4 + 255) & ~(size_t)255;
    const size_t off_g = off_8 + ((!p->outputs_on_device && rgb8 ? (size_t)n_pix * 3 : 0) + 255 & ~(size_t)255);
    const size_t off_l = off_g + ((!p->outputs_on_device && gamma_rgb ? (size_t)n_pix * 12 : 0) + 255 & ~(size_t)255);
    const size_t off_e = off_l + ((!p->outputs_on_device && linear_rgb ? (size_t)n_pix * 12 : 0) + 255 & ~(size_t)255);   // fw_render_rays' error word
    const size_t host_need = off_e + 256;
    if (ws->host_out_bytes < host_need) {
        if (ws->host_out) (void)hipHostFree(ws->host_out);
        ws->host_out = nullptr; ws->host_out_bytes = 0;
        if (hipHostMalloc(&ws->host_out, host_need + host_need / 4, hipHostMallocDefault) != hipSuccess) return fail(FW_ERR_OOM, "pinned output staging allocation failed");
        ws->host_out_bytes = host_need + host_need / 4;
    }
    uint8_t *ho = (uint8_t *)ws->host_out;
    const uint32_t *h_counts = (const uint32_t *)(ho + off_c);
    HIPCHK(hipMemcpyAsync(ho + off_c, ws->totals.p, n_counts * 4, hipMemcpyDeviceToHost, stream));
    const double t_counts = since(tq0);
    if (!p->outputs_on_device) {
        if (rgb8) HIPCHK(hipMemcpyAsync(ho + off_8, d_rgb8, (size_t)n_pix * 3, hipMemcpyDeviceToHost, stream));
        if (gamma_rgb) HIPCHK(hipMemcpyAsync(ho + off_g, d_gamma, (size_t)n_pix * 12, hipMemcpyDeviceToHost, stream));
        if (linear_rgb) HIPCHK(hipMemcpyAsync(ho + off_l, d_linear, (size_t)n_pix * 12, hipMemcpyDeviceToHost, stream));
    }
    if (ri) HIPCHK(hipMemcpyAsync(ho + off_e, ws->ray_err.p, 4, hipMemcpyDeviceToHost, stream));
    const double t_outs = since(tq0);
    if (!ws->ev_d2h) HIPCHK(hipEventCreate(&ws->ev_d2h));
    HIPCHK(hipEventRecord(ws->ev_d2h, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (!p->outputs_on_device) {
        if (rgb8) std::memcpy(rgb8, ho + off_8, (size_t)n_pix * 3);
        if (gamma_rgb) std::memcpy(gamma_rgb, ho + off_g, (size_t)n_pix * 12);
        if (linear_rgb) std::memcpy(linear_rgb, ho + off_l, (size_t)n_pix * 12);
    }
#if FW_AB
    if (const uint32_t ew = fw::take_error_word())      // the A/B build's device-side guards (fw_kernels.hip: g_err_word): the frame is not to be trusted
        return fail(FW_ERR_HIP, std::string("device error word: ") + ((ew & 1u) ? "LDS traversal stack overflow (a push beyond the levels the launch reserved) " : "") +
                                    ((ew & 2u) ? "a walk kernel's wave made no progress for 2^24 rounds (left its loop) " : ""));
#endif
    if (ri && *(const uint32_t *)(ho + off_e)) return fail(FW_ERR_BAD_ARG, "a ray has a non-finite component or an all-zero direction");
    if (trace) fprintf(stderr, "[firework] render: enqueue %.2f ms | counters copy queued +%.2f | output copies queued +%.2f | sync + host memcpy returned +%.2f\n",
                       std::chrono::duration<double, std::milli>(tq0 - wall0).count(), t_counts, t_outs, since(tq0));
    const auto wall1 = std::chrono::steady_clock::now();

    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->samples = (uint64_t)n_pix * p->samples;
        uint64_t deposits = 0;
        for (uint32_t b = 0; b < n_batches; b++) {
            for (int s = 0; s < fw::MAX_SEGMENTS; s++) { uint64_t c = h_counts[(size_t)b * fw::COUNT_STRIDE + s]; stats->rays_per_depth[s] += c; stats->rays += c; }
            stats->parked_rays += h_counts[(size_t)b * fw::COUNT_STRIDE + fw::MAX_SEGMENTS];
            deposits += h_counts[(size_t)b * fw::COUNT_STRIDE + 12];
        }
        stats->deposits = count_deposits ? deposits : stats->samples;      // every path ends exactly once (render.rs:19-31)
        {   // HBM bytes this layout moves (fw_device.h B_*): queue streams only, scene tables are cache-resident
            const uint64_t *R = stats->rays_per_depth;
            const uint64_t S = stats->samples, ray0 = fr.pinhole0 ? fw::B_RAY_PINHOLE0 : fw::B_RAY, b_hit = fr.hit4 ? fw::B_HIT4 : fw::B_HIT;
            uint64_t rd_ray = R[0] * ray0, later = 0, survivors = 0;
            for (int s = 1; s < fw::MAX_SEGMENTS; s++) { rd_ray += R[s] * fw::B_RAY; later += R[s]; survivors += R[s]; }
            stats->bytes_raygen = S * ray0 + (fr.pixel_ids ? S * 4 : 0) + (ri ? S * 24 : 0);     // (caller rays: read, then written)
            const uint64_t medium = sc->d.has_medium ? later * 4 : 0;       // the path's home slot (RNG key of the medium's draw)
            const uint64_t b_state = fr.chain_bits ? fw::B_STATE_CHAIN : fw::B_STATE;
            // (EXACT_PRODUCT: one attenuation record written per survivor; a depositing path reads back its own — at most its length: not counted)
            const uint64_t shade_in = rd_ray + later * b_state, shade_out = survivors * (fw::B_RAY + b_state + (fr.atten ? fw::B_ATTEN : 0u)) + stats->deposits * fw::B_DEPOSIT;
            if (fused) { stats->bytes_extend = 0; stats->bytes_shade = shade_in + shade_out; }
            else {
                stats->bytes_extend = rd_ray + medium + stats->rays * b_hit + stats->parked_rays * 2 * fw::B_PARK;
                stats->bytes_shade = shade_in + stats->rays * b_hit + shade_out;
            }
            stats->bytes_accumulate = (fr.skip_zero_deposits ? stats->deposits * fw::B_DEPOSIT + S / 8 : S * fw::B_DEPOSIT) + (uint64_t)n_batches * n_pix * 2 * fw::B_ACCUM * (rd ? 2u : 1u);   // (a round reads and writes the squares too)
        }
        stats->ms_wall = std::chrono::duration<double, std::milli>(wall1 - wall0).count();
        float ms_copy = 0.f;
        HIPCHK(hipEventElapsedTime(&ms_copy, ws->events[1], ws->ev_d2h));   // counters (a few hundred bytes) + the outputs
        stats->ms_d2h = ms_copy;
        stats->algorithmic_bytes = 160 * stats->rays + 24 * stats->samples;   // SURVEY §8(d); HDR env misses are added by the caller that knows them
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ws->events[0], ws->events[1]));
        stats->ms_render = ms;
        if (timing) {
            double acc[4] = {0, 0, 0, 0};
            for (int l = 0; l < n_lanes; l++)
                for (size_t i = 0; i < ev_class[l].size(); i++) {
                    float t = 0.f;
                    HIPCHK(hipEventElapsedTime(&t, ws->lanes[l].events[i], ws->lanes[l].events[i + 1]));
                    acc[ev_class[l][i]] += t;
                }
            stats->ms_raygen = acc[0]; stats->ms_extend = acc[1]; stats->ms_shade = acc[2]; stats->ms_accumulate = acc[3];
        }
        stats->n_extend_launches = fused ? 0 : n_batches * fw::MAX_SEGMENTS; stats->n_shade_launches = n_batches * fw::MAX_SEGMENTS;
        stats->n_batches = n_batches; stats->tlas_nodes = sc->tlas_nodes; stats->blas_nodes = sc->blas_nodes;
        stats->reserved = ((sc->tlas_depth & 0x7fffu) << 16) | (sc->blas_depth & 0xffffu) | (graph_replayed ? 0x80000000u : 0u);   // depths of the trees actually walked; bit 31: the frame ran as a hipGraph (GRAPH)
    }
    return FW_OK;
}

// fw_render_adaptive: rounds of render_impl over the still-active pixels of a whole frame (include/firework_hip.h has the contract).
// Round 0 renders every pixel (in the tile order render_impl would use) to min_samples; after each round k_adaptive_select applies the
// convergence rule on the device and compacts the survivors into the other id list, whose length comes back in one 4-byte copy; the
// next round takes them from n to min(2n, max) samples.  Every pixel's sums are those of fw_render at its final count, bit for bit.
constexpr uint32_t ADAPTIVE_MAX_ROUNDS = 32;
int adaptive_impl(fw_scene *sc, const fw_render_params *p, float tol, uint32_t min_samples, float *accum, float *moments, uint8_t *rgb8,
                  float *gamma_rgb, float *linear_rgb, uint32_t *round_pixels, fw_stats *stats) {
    // (arguments first: nothing below dereferences the scene before they are all valid)
    if (!sc || !p) return fail(FW_ERR_BAD_ARG, "null argument");
    if (p->pixel_ids) return fail(FW_ERR_BAD_ARG, "fw_render_adaptive renders whole frames: pixel_ids must be NULL");
    if (min_samples < 2) return fail(FW_ERR_BAD_ARG, "min_samples must be >= 2 (the rule needs a variance)");
    if (p->samples < min_samples) return fail(FW_ERR_BAD_ARG, "samples (the cap) must be >= min_samples");
    if (p->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be <= 2^24 (the count is exact as a float)");
    if (!std::isfinite(tol) || !(tol > 0.f)) return fail(FW_ERR_BAD_ARG, "tolerance must be finite and > 0");
    if (p->width == 0 || p->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    if (!(p->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be > 0");
    if (p->rng_mode != FW_RNG_CTR) return fail(FW_ERR_UNSUPPORTED, "the HIP path implements FW_RNG_CTR only (FW_RNG_LCG is a sequential stream)");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    const uint32_t n = (uint32_t)full;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(sc->device));
    hipStream_t stream = (hipStream_t)p->stream;
    Workspace *ws = workspace_for(sc->device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    { const int irc = init_device_locked(ws, sc->device); if (irc) return irc; }
    ws->kernels.clear();
    const Options O = options();
    int rc = FW_OK;
    auto need = [&](DevBuf &b, size_t bytes) { if (!rc) rc = b.alloc(bytes); };
    need(ws->ad_accum, (size_t)n * 16); need(ws->ad_moments, (size_t)n * 16);
    need(ws->ad_ids[0], (size_t)n * 4); need(ws->ad_ids[1], (size_t)n * 4);
    need(ws->ad_mask, ((size_t)n + 63) / 64 * 8); need(ws->ad_counts, ((size_t)fw::ADAPTIVE_MAX_BLOCKS + 1) * 4);
    uint8_t *d_rgb8 = rgb8; float *d_gamma = gamma_rgb, *d_linear = linear_rgb;
    if (!p->outputs_on_device) {
        if (rgb8) { need(ws->out_rgb8, (size_t)n * 3); d_rgb8 = (uint8_t *)ws->out_rgb8.p; }
        if (gamma_rgb) { need(ws->out_gamma, (size_t)n * 12); d_gamma = (float *)ws->out_gamma.p; }
        if (linear_rgb) { need(ws->out_linear, (size_t)n * 12); d_linear = (float *)ws->out_linear.p; }
    }
    if (rc) return rc;
    if (!ws->ad_count_host) HIPCHK(hipHostMalloc((void **)&ws->ad_count_host, 4, hipHostMallocDefault));
    for (hipEvent_t &e : ws->ad_ev) if (!e) HIPCHK(hipEventCreate(&e));
    float4 *d_accum = (float4 *)ws->ad_accum.p, *d_moments = (float4 *)ws->ad_moments.p;
    uint32_t *d_count = (uint32_t *)ws->ad_counts.p + fw::ADAPTIVE_MAX_BLOCKS;

    if (ws->ev_upload) HIPCHK(hipStreamWaitEvent(stream, ws->ev_upload, 0));
    HIPCHK(hipEventRecord(ws->ad_ev[0], stream));
    HIPCHK(hipMemsetAsync(d_accum, 0, (size_t)n * 16, stream));
    HIPCHK(hipMemsetAsync(d_moments, 0, (size_t)n * 16, stream));
    // round 0's list: render_impl's choice for a whole frame (16x16 tiles from 1024 pixels on, unless NO_TILE_ORDER), row order = no list
    const uint32_t *cur = nullptr;
    if (n >= 1024 && !O.no_tile_order) { fw::launch_tile_order(stream, p->width, p->height, (uint32_t *)ws->ad_ids[0].p); cur = (const uint32_t *)ws->ad_ids[0].p; }

    fw_stats total{};
    uint32_t rounds[ADAPTIVE_MAX_ROUNDS] = {};
    uint32_t n_rounds = 0, active = n, done = 0;
    while (active > 0) {
        if (n_rounds >= ADAPTIVE_MAX_ROUNDS) return fail(FW_ERR_HIP, "adaptive render: more rounds than the schedule allows");
        const uint32_t target = n_rounds == 0 ? min_samples : std::min<uint32_t>(2u * done, p->samples);
        fw_render_params rp = *p;
        rp.samples = target - done; rp.pixel_ids = nullptr; rp.n_pixels = 0;
        const AdaptiveRound rd{cur, active, d_accum, d_moments};
        fw_stats rs{};
        if (int rrc = render_impl(sc, &rp, nullptr, nullptr, nullptr, &rs, done, nullptr, &rd)) return rrc;
        rounds[n_rounds++] = active;
        stats_add(total, rs);      // (the per-class times add up to zero unless FW_FLAG_TIME_KERNELS: render_impl reports none then)
        done = target;
        uint32_t *next = (uint32_t *)ws->ad_ids[cur == (const uint32_t *)ws->ad_ids[0].p ? 1 : 0].p;
        fw::launch_adaptive_select(stream, cur, active, d_accum, d_moments, done, done < p->samples, tol, (unsigned long long *)ws->ad_mask.p,
                                   (uint32_t *)ws->ad_counts.p, next, d_count);
        HIPCHK(hipMemcpyAsync(ws->ad_count_host, d_count, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (*ws->ad_count_host > active) return fail(FW_ERR_HIP, "adaptive render: survivor count out of range");
        active = *ws->ad_count_host;
        cur = next;
    }
    fw::launch_resolve_adaptive(stream, sc->n_cus, n, d_accum, d_moments, p->gamma, d_rgb8, d_gamma, d_linear);
    HIPCHK(hipEventRecord(ws->ad_ev[1], stream));
    const hipMemcpyKind kind = p->outputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (accum) HIPCHK(hipMemcpyAsync(accum, d_accum, (size_t)n * 16, kind, stream));
    if (moments) HIPCHK(hipMemcpyAsync(moments, d_moments, (size_t)n * 16, kind, stream));
    if (!p->outputs_on_device) {
        if (rgb8) HIPCHK(hipMemcpyAsync(rgb8, d_rgb8, (size_t)n * 3, kind, stream));
        if (gamma_rgb) HIPCHK(hipMemcpyAsync(gamma_rgb, d_gamma, (size_t)n * 12, kind, stream));
        if (linear_rgb) HIPCHK(hipMemcpyAsync(linear_rgb, d_linear, (size_t)n * 12, kind, stream));
    }
    if (round_pixels && p->outputs_on_device) HIPCHK(hipMemcpyAsync(round_pixels, rounds, sizeof rounds, hipMemcpyHostToDevice, stream));
    if (!ws->ev_d2h) HIPCHK(hipEventCreate(&ws->ev_d2h));
    HIPCHK(hipEventRecord(ws->ev_d2h, stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    if (round_pixels && !p->outputs_on_device) std::memcpy(round_pixels, rounds, sizeof rounds);
    if (stats) {
        *stats = total;
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ws->ad_ev[0], ws->ad_ev[1]));
        stats->ms_render = ms;
        HIPCHK(hipEventElapsedTime(&ms, ws->ad_ev[1], ws->ev_d2h));
        stats->ms_d2h = p->outputs_on_device ? 0.0 : ms;      // (both over the whole call, in place of the rounds' sums)
        stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FW_OK;
}

// fw_render_views: the views in consecutive groups, each rendered by render_impl as one frame over a pixel space of (views of the group) x N
// entries (include/firework_hip.h has the contract).  A group holds as many views as one sample of each of their pixels fits the batch budget
// render_impl would use (at least one), and at most VIEW_GROUP_MAX_PIXELS pixels: beyond that a group's batches stay just as full (they take
// more samples per pixel), while its accumulation and output staging would keep growing.
constexpr uint64_t VIEW_GROUP_MAX_PIXELS = 1ull << 24;
int views_impl(fw_scene *sc, const fw_render_params *p, const fw_camera_settings *cameras, uint32_t n_views, uint8_t *rgb8, float *gamma_rgb,
               float *linear_rgb, fw_stats *stats) {
    // (arguments first, in a fixed order: nothing below dereferences the scene or calls HIP before they are all valid)
    if (!sc || !p || !cameras) return fail(FW_ERR_BAD_ARG, "null argument");
    if (n_views == 0) return fail(FW_ERR_BAD_ARG, "n_views must be > 0");
    if (p->width == 0 || p->height == 0 || p->samples == 0) return fail(FW_ERR_BAD_ARG, "width, height and samples must be > 0");
    if (!(p->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be > 0");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (p->pixel_ids && p->n_pixels == 0) return fail(FW_ERR_BAD_ARG, "no pixels to render");
    if (p->pixel_ids) for (uint32_t i = 0; i < p->n_pixels; i++) if (p->pixel_ids[i] >= full) return fail(FW_ERR_BAD_ARG, "pixel id out of range");
    for (uint32_t v = 0; v < n_views; v++) {
        const fw_camera_settings &c = cameras[v];
        const float f[] = {c.cam_pos.x, c.cam_pos.y, c.cam_pos.z, c.look_at.x, c.look_at.y, c.look_at.z, c.vfov, c.aperture, c.focus_dist};
        for (float x : f) if (!std::isfinite(x)) return fail(FW_ERR_BAD_ARG, "camera " + std::to_string(v) + " has a non-finite field");
    }
    if (p->rng_mode != FW_RNG_CTR) return fail(FW_ERR_UNSUPPORTED, "the HIP path implements FW_RNG_CTR only (FW_RNG_LCG is a sequential stream)");
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    const uint32_t N = p->pixel_ids ? p->n_pixels : (uint32_t)full;
    if ((uint64_t)n_views * N > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "n_views x pixels must be below 2^32");

    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(sc->device));
    Workspace *ws = workspace_for(sc->device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    uint32_t budget = 0;
    {
        std::lock_guard<std::mutex> ws_guard(ws->mu);
        { const int irc = init_device_locked(ws, sc->device); if (irc) return irc; }
        if (int erc = ensure_emitters(sc, p, ws)) return erc;
        if (int erc = ensure_env_dist(sc, p, ws)) return erc;
        budget = batch_budget(sc, p, options(), ws->arena.bytes).budget;
    }
    const uint32_t per_group = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)n_views, budget / N, VIEW_GROUP_MAX_PIXELS / N}));
    std::vector<fw::DCamera> cams(n_views);
    for (uint32_t v = 0; v < n_views; v++) cams[v] = make_camera(cameras[v], p->width, p->height);

    fw_stats total{};
    for (uint32_t v0 = 0; v0 < n_views; v0 += per_group) {
        const ViewGroup vg{cams.data() + v0, std::min(per_group, n_views - v0)};
        const size_t off = (size_t)v0 * N * 3;
        fw_stats gs{};
        if (int rc = render_impl(sc, p, rgb8 ? rgb8 + off : nullptr, gamma_rgb ? gamma_rgb + off : nullptr, linear_rgb ? linear_rgb + off : nullptr,
                                 stats ? &gs : nullptr, 0, nullptr, nullptr, &vg)) return rc;
        if (stats) stats_add(total, gs);
    }
    if (stats) {
        *stats = total;
        stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FW_OK;
}

// fw_render_rays: render_impl over a frame of n_rays entries whose paths start from the caller's rays (RayInput; include/firework_hip.h has
// the contract).  The frame is n_rays x 1 pixels without a camera; batches, lanes, queues, walks, k_shade, the accumulation in sample
// order and the resolve are the render's own.
// The frame of a fw_render_rays call as render_impl takes it: n_rays x 1 pixels without a camera.  rays_impl and render_model_impl (whose
// every chunk is such a call) both build it here, so the two cannot drift apart.
fw_render_params rays_frame(const fw_render_rays_params *rp, uint32_t samples) {
    fw_render_params P{};
    P.width = rp->n_rays; P.height = 1; P.samples = samples; P.gamma = rp->gamma; P.use_bvh = rp->use_bvh; P.seed = rp->seed;
    P.rng_mode = FW_RNG_CTR; P.paths_per_batch = rp->paths_per_batch; P.flags = rp->flags; P.outputs_on_device = rp->on_device; P.stream = rp->stream;
    return P;
}

int rays_impl(fw_scene *sc, const fw_render_rays_params *rp, const float *rays, float *accum, uint8_t *rgb8, float *gamma_rgb,
              float *linear_rgb, fw_stats *stats) {
    // (arguments first, in a fixed order: nothing below dereferences the scene or calls HIP before they are all valid)
    if (!sc || !rp || !rays) return fail(FW_ERR_BAD_ARG, "null argument");
    if (rp->n_rays == 0) return fail(FW_ERR_BAD_ARG, "n_rays must be > 0");
    if (rp->samples == 0 || rp->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if ((uint64_t)rp->first_sample + rp->samples > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_sample + samples overflows");
    if (!std::isfinite(rp->gamma) || !(rp->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be finite and > 0");
    if (!accum && rp->first_sample > 0) return fail(FW_ERR_BAD_ARG, "first_sample > 0 needs the accumulation buffer of the samples before it");
    if (rp->on_device && (((uintptr_t)accum & 15u) || ((uintptr_t)rays & 3u))) return fail(FW_ERR_BAD_ARG, "device accum must be 16-byte aligned, device rays 4-byte aligned");
    if (int rc = need_device()) return rc;
    const fw_render_params P = rays_frame(rp, rp->samples);
    const RayInput ri{rays, rp->n_rays, rp->per_sample_rays != 0, rp->keys, rp->key_base, rp->on_device != 0};
    return render_impl(sc, &P, rgb8, gamma_rgb, linear_rgb, stats, rp->first_sample, accum, nullptr, nullptr, &ri);
}

// Device memory of a ray query (trace_impl, camera_rays_impl): the front of the path arena, grown like render_impl grows it.  A render
// lays its own buffers out from the arena's start on every call, so nothing of a render outlives it there.  What a render does keep is
// a frame graph (GRAPH) whose launches name arena addresses: its key hashes the arena's address and size, which a growth changes, and
// the key is cleared here as well, so a graph recorded before a growth is never replayed.  Caller holds ws->mu.
int query_arena_locked(Workspace *ws, int dev, size_t bytes, uint8_t *&base) {
    size_t want = (bytes + ((size_t)1 << 30) - 1) & ~(((size_t)1 << 30) - 1);
    if (want > ws->arena.bytes) {
        if (ws->arena.bytes) want = std::max(want, (ws->arena.bytes + ws->arena.bytes / 4 + ((size_t)1 << 30) - 1) & ~(((size_t)1 << 30) - 1));
        ws->fg.key = 0; ws->fg.seen = 0;
        if (int rc = arena_reserve_locked(ws, dev, want)) return rc;
    }
    base = (uint8_t *)ws->arena.p;
    return FW_OK;
}
// pinned host staging of a ray query's transfers (Workspace::host_out, which render_impl grows the same way)
int query_host_locked(Workspace *ws, size_t bytes, uint8_t *&host) {
    if (ws->host_out_bytes < bytes) {
        if (ws->host_out) (void)hipHostFree(ws->host_out);
        ws->host_out = nullptr; ws->host_out_bytes = 0;
        if (hipHostMalloc(&ws->host_out, bytes + bytes / 4, hipHostMallocDefault) != hipSuccess) return fail(FW_ERR_OOM, "pinned staging allocation failed");
        ws->host_out_bytes = bytes + bytes / 4;
    }
    host = (uint8_t *)ws->host_out;
    return FW_OK;
}

static_assert(sizeof(fw_hit) == 48, "fw_hit is three 16-byte stores of k_trace_store");
// fw_trace_rays: segment 0 of a render over the caller's rays.  Per batch, on the caller's stream: k_trace_load (the queues, the exact
// walk's list) -> the render's launch_extend -> launch_extend_exact -> k_trace_store; with host memory the rays and hits pass through
// pinned staging.  The queue geometry, the walk configuration and the hit-record form are chosen as render_impl chooses them for one
// batch in flight, so every kernel-selecting option selects the same walks here.
int trace_impl(fw_scene *sc, const fw_trace_params *p, const float *rays, uint32_t n, fw_hit *hits, fw_stats *stats) {
    if (!sc || !p) return fail(FW_ERR_BAD_ARG, "null argument");
    if (n == 0) return FW_OK;
    if (!rays || !hits) return fail(FW_ERR_BAD_ARG, "null rays or hits");
    if (((uintptr_t)rays & 3u) || (p->on_device && ((uintptr_t)hits & 15u))) return fail(FW_ERR_BAD_ARG, "rays must be 4-byte aligned, device hits 16-byte aligned");
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(sc->device));
    hipStream_t stream = (hipStream_t)p->stream;
    Workspace *ws = workspace_for(sc->device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    { const int irc = init_device_locked(ws, sc->device); if (irc) return irc; }
    const Options O = options();
    const bool use_bvh = p->use_bvh != 0;
    const uint32_t per = std::min(n, p->rays_per_batch ? p->rays_per_batch : default_paths_per_batch(O, ws->arena.bytes));
    const uint32_t n_batches = (uint32_t)(((uint64_t)n + per - 1) / per);

    // render_impl's queue geometry for a batch of `per` paths (one batch in flight)
    fw::DQueue q{};
    const uint32_t unit = (uint32_t)sc->n_cus * 4u * (use_bvh ? 20u : 28u);
    const uint64_t chunks = ((uint64_t)per + 63u) / 64u;
    uint32_t want_waves = unit * (uint32_t)std::min<uint64_t>(3u, std::max<uint64_t>(1u, chunks / ((uint64_t)unit * 16u)));
    if (O.waves > 0) want_waves = (uint32_t)O.waves;
    q.n_waves = std::max(4u, std::min(want_waves, (per + 511u) / 512u));
    q.n_waves = (q.n_waves + 7u) & ~7u;
    const uint32_t chunks_per_wave = (per + q.n_waves * 64u - 1) / (q.n_waves * 64u);
    while ((1u << q.cpw_shift) < chunks_per_wave) q.cpw_shift++;
    q.cap = 64u << q.cpw_shift;
    const uint64_t cap64 = (uint64_t)q.cap * q.n_waves;
    if (cap64 > 0x7fffffffull) return fail(FW_ERR_UNSUPPORTED, "too many rays per batch");
    const size_t cap = (size_t)cap64;
#if FW_AB
    const bool tlas_refill = !O.tlas_refill_off;
#else
    const bool tlas_refill = true;
#endif
    // render_impl's exact walk; under use_bvh always on (fw::EX_TRACE_ZERO), for the caller rays with a zero direction component
    const uint32_t exact_mode = (sc->ex.mode & 1u) | (use_bvh ? (sc->ex.mode & 6u) | fw::EX_TRACE_ZERO : ((sc->ex.mode & 4u) && sc->d.has_mesh ? 4u : 0u));
    const bool park_meshes = use_bvh && sc->d.has_mesh != 0 && tlas_refill;

    // device memory: the front of the arena
    const size_t pcap = (size_t)(q.cap + 64u) * q.n_waves;
    const size_t totals_bytes = (size_t)n_batches * fw::COUNT_STRIDE * 4;
    size_t off = 0;
    auto put = [&](size_t b) { const size_t at = off; off += (b + 255) & ~(size_t)255; return at; };
    const size_t o_ra = put(cap * 16), o_rb = put(cap * 8), o_hits = put(cap * 8), o_wc = put((size_t)(fw::MAX_SEGMENTS + 1) * q.n_waves * 4);
    const size_t o_ids = put((size_t)per * 4), o_slot = put((size_t)per * 4), o_tot = put(totals_bytes);
    const size_t o_ex = exact_mode ? put(2 * (size_t)per * 4 + 64) : 0;
    const size_t o_pa = park_meshes ? put(pcap * 16) : 0, o_pb = park_meshes ? put(pcap * 8) : 0, o_pm = park_meshes ? put(pcap * 16) : 0;
    const size_t o_pc = park_meshes ? put((size_t)q.n_waves * 8) : 0;
    const size_t o_in = p->on_device ? 0 : put((size_t)per * 24), o_out = p->on_device ? 0 : put((size_t)per * sizeof(fw_hit));
    uint8_t *base = nullptr;
    if (int rc = query_arena_locked(ws, sc->device, off, base)) return rc;
    // pinned staging: the batches' queue counters, then (host memory) one batch of rays and one of hits
    const size_t h_tot = 0, h_in = (totals_bytes + 255) & ~(size_t)255, h_out = h_in + (p->on_device ? 0 : ((size_t)per * 24 + 255) & ~(size_t)255);
    uint8_t *host = nullptr;
    if (int rc = query_host_locked(ws, h_out + (p->on_device ? 0 : (size_t)per * sizeof(fw_hit)), host)) return rc;
    const bool timing = (p->flags & FW_FLAG_TIME_KERNELS) != 0;
    while (ws->events.size() < 3) { hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, ws->events.size() < 2 ? hipEventDefault : hipEventDisableTiming)); ws->events.push_back(e); }
    std::vector<hipEvent_t> &tev = ws->lanes[0].events;
    while (timing && tev.size() < 2) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); tev.push_back(e); }

    fw::LaunchCfg cfg{};
    set_walk_cfg(cfg, sc, O, q, use_bvh, tlas_refill);
    cfg.log = &ws->kernels; ws->kernels.clear();
    cfg.stream = stream;
    cfg.q.wcount = (uint32_t *)(base + o_wc);
    fw::DPaths paths{(float4 *)(base + o_ra), (float2 *)(base + o_rb), nullptr};     // segment 0 reads no path state
    float2 *const hit_rec = (float2 *)(base + o_hits);
    uint32_t *const ids = (uint32_t *)(base + o_ids), *const slot_of = (uint32_t *)(base + o_slot), *const totals = (uint32_t *)(base + o_tot);
    const fw::DPark park{(float4 *)(base + o_pa), (float2 *)(base + o_pb), (float4 *)(base + o_pm), q.cap + 64u,
                         park_meshes ? (uint32_t *)(base + o_pc) : nullptr, park_meshes ? (uint32_t *)(base + o_pc) + q.n_waves : nullptr};
    fw::DFrame fr{};
    fr.width = 1; fr.height = 1; fr.inv_width = 1.f;              // (camera fields: unused by a trace)
    fr.pixel_ids = ids;
    fr.seed32 = seed32_of(p->seed);
    fr.sample0 = 0; fr.spp_batch = 1;
    fr.q_n_waves = q.n_waves; fr.q_shift = q.cpw_shift;
    fr.pinhole0 = 0;                                             // caller rays are whole rays
    fr.hit4 = (!use_bvh && sc->simple_shapes && !exact_mode && !O.no_hit4) ? 1u : 0u;
    fr.ex = sc->ex; fr.ex.mode = exact_mode;
    if (exact_mode) {
        fr.ex.slots[0] = (uint32_t *)(base + o_ex); fr.ex.slots[1] = fr.ex.slots[0] + per;
        fr.ex.count = fr.ex.slots[1] + per; fr.ex.cap = per;
    }

    if (ws->ev_upload) HIPCHK(hipStreamWaitEvent(stream, ws->ev_upload, 0));     // the scene's upload kernel
    HIPCHK(hipEventRecord(ws->events[0], stream));
    HIPCHK(hipMemsetAsync(totals, 0, totals_bytes, stream));
    double ms_extend = 0.0;
    for (uint32_t b = 0; b < n_batches; b++) {
        const size_t first = (size_t)b * per;
        const uint32_t nb = (uint32_t)std::min<size_t>(per, (size_t)n - first);
        fr.n_pixels = nb; fr.inv_n_pixels = 1.0f / (float)nb;
        HIPCHK(hipMemsetAsync(cfg.q.wcount, 0, (size_t)(fw::MAX_SEGMENTS + 1) * q.n_waves * 4, stream));
        if (exact_mode) HIPCHK(hipMemsetAsync(fr.ex.count, 0, 64, stream));
        if (park_meshes) HIPCHK(hipMemsetAsync(park.ptotal, 0, (size_t)q.n_waves * 4, stream));
        const float *src = rays + first * 6;
        if (!p->on_device) {
            std::memcpy(host + h_in, src, (size_t)nb * 24);
            HIPCHK(hipMemcpyAsync(base + o_in, host + h_in, (size_t)nb * 24, hipMemcpyHostToDevice, stream));
            src = (const float *)(base + o_in);
        }
        fw::launch_trace_load(cfg, fr, src, paths, nb, p->key_base + (uint32_t)first, ids, slot_of);
        if (timing) HIPCHK(hipEventRecord(tev[0], stream));
        fw::launch_extend(cfg, sc->d, fr, paths, hit_rec, 0, use_bvh, park);
        if (exact_mode) fw::launch_extend_exact(cfg, sc->d, fr, paths, hit_rec, 0, use_bvh);
        if (timing) HIPCHK(hipEventRecord(tev[1], stream));
        fw::launch_queue_totals(cfg, totals + (size_t)b * fw::COUNT_STRIDE, park.ptotal);
        fw_hit *dst = p->on_device ? hits + first : (fw_hit *)(base + o_out);
        fw::launch_trace_store(cfg, sc->d, fr, paths, hit_rec, slot_of, nb, (float4 *)dst);
        if (!p->on_device) HIPCHK(hipMemcpyAsync(host + h_out, dst, (size_t)nb * sizeof(fw_hit), hipMemcpyDeviceToHost, stream));
        if (timing || !p->on_device) HIPCHK(hipStreamSynchronize(stream));
        if (timing) { float t = 0.f; HIPCHK(hipEventElapsedTime(&t, tev[0], tev[1])); ms_extend += t; }
        if (!p->on_device) std::memcpy(hits + first, host + h_out, (size_t)nb * sizeof(fw_hit));
    }
    HIPCHK(hipEventRecord(ws->events[1], stream));
    HIPCHK(hipMemcpyAsync(host + h_tot, totals, totals_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        const uint32_t *h_counts = (const uint32_t *)(host + h_tot);
        for (uint32_t b = 0; b < n_batches; b++) {
            stats->rays += h_counts[(size_t)b * fw::COUNT_STRIDE];
            stats->parked_rays += h_counts[(size_t)b * fw::COUNT_STRIDE + fw::MAX_SEGMENTS];
        }
        stats->rays_per_depth[0] = stats->rays;
        stats->n_batches = n_batches; stats->n_extend_launches = n_batches;
        stats->tlas_nodes = sc->tlas_nodes; stats->blas_nodes = sc->blas_nodes;
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ws->events[0], ws->events[1]));
        stats->ms_render = ms;
        stats->ms_extend = ms_extend;
        stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FW_OK;
}

// fw_camera_rays: k_camera_rays over render_impl's camera and keys for one sample of the pixels
int camera_rays_impl(const fw_render_params *p, int device, uint32_t sample, float *rays) {
    if (!p || !rays) return fail(FW_ERR_BAD_ARG, "null argument");
    if (p->width == 0 || p->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    const uint32_t n_pix = p->pixel_ids ? p->n_pixels : (uint32_t)full;
    if (n_pix == 0) return fail(FW_ERR_BAD_ARG, "no pixels");
    if (p->pixel_ids) for (uint32_t i = 0; i < n_pix; i++) if (p->pixel_ids[i] >= full) return fail(FW_ERR_BAD_ARG, "pixel id out of range");
    int ndev = 0;
    if (int rc = need_device(&ndev)) return rc;
    if (device < 0 || device >= ndev) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (p->outputs_on_device && ((uintptr_t)rays & 3u)) return fail(FW_ERR_BAD_ARG, "rays must be 4-byte aligned");
    HIPCHK(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)p->stream;
    Workspace *ws = workspace_for(device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    { const int irc = init_device_locked(ws, device); if (irc) return irc; }
    const size_t o_ids = 0, o_out = p->pixel_ids ? ((size_t)n_pix * 4 + 255) & ~(size_t)255 : 0;
    uint8_t *base = nullptr;
    if (int rc = query_arena_locked(ws, device, o_out + (p->outputs_on_device ? 0 : (size_t)n_pix * 24), base)) return rc;
    const fw::DCamera cam = make_camera(p->camera, p->width, p->height);
    fw::DFrame fr{};      // render_impl's frame fields that camera_ray / key_of_linear read, for a batch of one sample
    fr.width = p->width; fr.height = p->height; fr.n_pixels = n_pix; fr.inv_n_pixels = 1.0f / (float)n_pix; fr.inv_width = 1.0f / (float)p->width;
    fr.pixel_ids = p->pixel_ids ? (const uint32_t *)(base + o_ids) : nullptr;
    fr.seed32 = seed32_of(p->seed);
    fr.sample0 = sample; fr.spp_batch = 1;
    if (p->pixel_ids) HIPCHK(hipMemcpyAsync(base + o_ids, p->pixel_ids, (size_t)n_pix * 4, hipMemcpyHostToDevice, stream));
    float *dst = p->outputs_on_device ? rays : (float *)(base + o_out);
    fw::launch_camera_rays(stream, device_cus(device), cam, fr, n_pix, dst);
    if (!p->outputs_on_device) {
        uint8_t *host = nullptr;
        if (int rc = query_host_locked(ws, (size_t)n_pix * 24, host)) return rc;
        HIPCHK(hipMemcpyAsync(host, dst, (size_t)n_pix * 24, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        std::memcpy(rays, host, (size_t)n_pix * 24);
    } else HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    return FW_OK;
}

// fw_render_aovs: for every sample s, the frame's camera rays (k_camera_rays, the render's keys) are traced in batches as fw_trace_rays
// traces the caller's rays — k_trace_load with the real pixel keys (key0 = the batch's first pixel, DFrame.sample0 = s), the render's
// launch_extend + launch_extend_exact — and k_aov_accumulate adds the batch's values to its pixels' sums; k_aov_finish divides.  The
// queue geometry, walk configuration and hit-record form are trace_impl's, so every kernel-selecting option selects the same walks.
// dm: fw_render_model_aovs — the one-sample ray buffer is filled by k_model_rays (the model's rays of sample s) instead of k_camera_rays.
int aovs_impl(fw_scene *sc, const fw_render_params *p, float *aov, fw_stats *stats, const fw::DModel *dm = nullptr) {
    // (arguments first: nothing below dereferences the scene before they are all valid)
    if (!sc || !p || !aov) return fail(FW_ERR_BAD_ARG, "null argument");
    if (p->pixel_ids) return fail(FW_ERR_BAD_ARG, "fw_render_aovs renders whole frames: pixel_ids must be NULL");
    if (p->samples == 0 || p->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if (p->width == 0 || p->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    if (p->outputs_on_device && ((uintptr_t)aov & 15u)) return fail(FW_ERR_BAD_ARG, "a device aov must be 16-byte aligned");
    if (p->rng_mode != FW_RNG_CTR) return fail(FW_ERR_UNSUPPORTED, "the HIP path implements FW_RNG_CTR only (FW_RNG_LCG is a sequential stream)");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    if (int rc = need_device()) return rc;
    const uint32_t n = (uint32_t)full;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(sc->device));
    hipStream_t stream = (hipStream_t)p->stream;
    Workspace *ws = workspace_for(sc->device);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    { const int irc = init_device_locked(ws, sc->device); if (irc) return irc; }
    const Options O = options();
    const bool use_bvh = p->use_bvh != 0;
    const uint32_t per = std::min(n, default_paths_per_batch(O, ws->arena.bytes));
    const uint32_t n_batches = (uint32_t)(((uint64_t)n + per - 1) / per), S = p->samples;

    // trace_impl's queue geometry, exact walk and parking for a batch of `per` rays
    fw::DQueue q{};
    const uint32_t unit = (uint32_t)sc->n_cus * 4u * (use_bvh ? 20u : 28u);
    const uint64_t chunks = ((uint64_t)per + 63u) / 64u;
    uint32_t want_waves = unit * (uint32_t)std::min<uint64_t>(3u, std::max<uint64_t>(1u, chunks / ((uint64_t)unit * 16u)));
    if (O.waves > 0) want_waves = (uint32_t)O.waves;
    q.n_waves = std::max(4u, std::min(want_waves, (per + 511u) / 512u));
    q.n_waves = (q.n_waves + 7u) & ~7u;
    const uint32_t chunks_per_wave = (per + q.n_waves * 64u - 1) / (q.n_waves * 64u);
    while ((1u << q.cpw_shift) < chunks_per_wave) q.cpw_shift++;
    q.cap = 64u << q.cpw_shift;
    const uint64_t cap64 = (uint64_t)q.cap * q.n_waves;
    if (cap64 > 0x7fffffffull) return fail(FW_ERR_UNSUPPORTED, "too many rays per batch");
    const size_t cap = (size_t)cap64;
#if FW_AB
    const bool tlas_refill = !O.tlas_refill_off;
#else
    const bool tlas_refill = true;
#endif
    const uint32_t exact_mode = (sc->ex.mode & 1u) | (use_bvh ? (sc->ex.mode & 6u) | fw::EX_TRACE_ZERO : ((sc->ex.mode & 4u) && sc->d.has_mesh ? 4u : 0u));
    const bool park_meshes = use_bvh && sc->d.has_mesh != 0 && tlas_refill;

    // device memory: the front of the arena — trace_impl's buffers, one sample's camera rays, and (host output) the sums
    const size_t pcap = (size_t)(q.cap + 64u) * q.n_waves;
    const size_t totals_bytes = (size_t)S * n_batches * fw::COUNT_STRIDE * 4;
    size_t off = 0;
    auto put = [&](size_t b) { const size_t at = off; off += (b + 255) & ~(size_t)255; return at; };
    const size_t o_ra = put(cap * 16), o_rb = put(cap * 8), o_hits = put(cap * 8), o_wc = put((size_t)(fw::MAX_SEGMENTS + 1) * q.n_waves * 4);
    const size_t o_ids = put((size_t)per * 4), o_slot = put((size_t)per * 4), o_tot = put(totals_bytes);
    const size_t o_ex = exact_mode ? put(2 * (size_t)per * 4 + 64) : 0;
    const size_t o_pa = park_meshes ? put(pcap * 16) : 0, o_pb = park_meshes ? put(pcap * 8) : 0, o_pm = park_meshes ? put(pcap * 16) : 0;
    const size_t o_pc = park_meshes ? put((size_t)q.n_waves * 8) : 0;
    const size_t o_rays = put((size_t)n * 24), o_sum = p->outputs_on_device ? 0 : put((size_t)n * 48);
    uint8_t *base = nullptr;
    if (int rc = query_arena_locked(ws, sc->device, off, base)) return rc;
    const size_t h_out = (totals_bytes + 255) & ~(size_t)255;
    uint8_t *host = nullptr;
    if (int rc = query_host_locked(ws, h_out + (p->outputs_on_device ? 0 : (size_t)n * 48), host)) return rc;
    while (ws->events.size() < 3) { hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, ws->events.size() < 2 ? hipEventDefault : hipEventDisableTiming)); ws->events.push_back(e); }

    fw::LaunchCfg cfg{};
    set_walk_cfg(cfg, sc, O, q, use_bvh, tlas_refill);
    cfg.log = &ws->kernels; ws->kernels.clear();
    cfg.stream = stream;
    cfg.q.wcount = (uint32_t *)(base + o_wc);
    fw::DPaths paths{(float4 *)(base + o_ra), (float2 *)(base + o_rb), nullptr};
    float2 *const hit_rec = (float2 *)(base + o_hits);
    uint32_t *const ids = (uint32_t *)(base + o_ids), *const slot_of = (uint32_t *)(base + o_slot), *const totals = (uint32_t *)(base + o_tot);
    const fw::DPark park{(float4 *)(base + o_pa), (float2 *)(base + o_pb), (float4 *)(base + o_pm), q.cap + 64u,
                         park_meshes ? (uint32_t *)(base + o_pc) : nullptr, park_meshes ? (uint32_t *)(base + o_pc) + q.n_waves : nullptr};
    const uint32_t seed32 = seed32_of(p->seed);
    fw::DFrame fr{};
    fr.width = 1; fr.height = 1; fr.inv_width = 1.f;
    fr.pixel_ids = ids;
    fr.seed32 = seed32;
    fr.spp_batch = 1;
    fr.q_n_waves = q.n_waves; fr.q_shift = q.cpw_shift;
    fr.pinhole0 = 0;
    fr.hit4 = (!use_bvh && sc->simple_shapes && !exact_mode && !O.no_hit4) ? 1u : 0u;
    fr.ex = sc->ex; fr.ex.mode = exact_mode;
    if (exact_mode) {
        fr.ex.slots[0] = (uint32_t *)(base + o_ex); fr.ex.slots[1] = fr.ex.slots[0] + per;
        fr.ex.count = fr.ex.slots[1] + per; fr.ex.cap = per;
    }
    // camera_rays_impl's frame for one sample of the whole frame
    const fw::DCamera cam = make_camera(p->camera, p->width, p->height);
    fw::DFrame cf{};
    cf.width = p->width; cf.height = p->height; cf.n_pixels = n; cf.inv_n_pixels = 1.0f / (float)n; cf.inv_width = 1.0f / (float)p->width;
    cf.pixel_ids = nullptr; cf.seed32 = seed32; cf.spp_batch = 1;
    float *const rays = (float *)(base + o_rays);
    float4 *const sum = p->outputs_on_device ? (float4 *)aov : (float4 *)(base + o_sum);

    if (ws->ev_upload) HIPCHK(hipStreamWaitEvent(stream, ws->ev_upload, 0));
    HIPCHK(hipEventRecord(ws->events[0], stream));
    HIPCHK(hipMemsetAsync(totals, 0, totals_bytes, stream));
    HIPCHK(hipMemsetAsync(sum, 0, (size_t)n * 48, stream));
    for (uint32_t s = 0; s < S; s++) {
        cf.sample0 = s;
        if (dm) fw::launch_model_rays(stream, sc->n_cus, *dm, s, 1, rays);
        else fw::launch_camera_rays(stream, sc->n_cus, cam, cf, n, rays);
        fr.sample0 = s;
        for (uint32_t b = 0; b < n_batches; b++) {
            const uint32_t first = b * per, nb = std::min(per, n - first);
            fr.n_pixels = nb; fr.inv_n_pixels = 1.0f / (float)nb;
            HIPCHK(hipMemsetAsync(cfg.q.wcount, 0, (size_t)(fw::MAX_SEGMENTS + 1) * q.n_waves * 4, stream));
            if (exact_mode) HIPCHK(hipMemsetAsync(fr.ex.count, 0, 64, stream));
            if (park_meshes) HIPCHK(hipMemsetAsync(park.ptotal, 0, (size_t)q.n_waves * 4, stream));
            fw::launch_trace_load(cfg, fr, rays + (size_t)first * 6, paths, nb, first, ids, slot_of);
            fw::launch_extend(cfg, sc->d, fr, paths, hit_rec, 0, use_bvh, park);
            if (exact_mode) fw::launch_extend_exact(cfg, sc->d, fr, paths, hit_rec, 0, use_bvh);
            fw::launch_queue_totals(cfg, totals + ((size_t)s * n_batches + b) * fw::COUNT_STRIDE, park.ptotal);
            fw::launch_aov_accumulate(stream, sc->n_cus, sc->d, fr, paths, hit_rec, slot_of, nb, first, sum);
        }
    }
    fw::launch_aov_finish(stream, sc->n_cus, n, S, sum);
    HIPCHK(hipEventRecord(ws->events[1], stream));
    HIPCHK(hipMemcpyAsync(host, totals, totals_bytes, hipMemcpyDeviceToHost, stream));
    if (!p->outputs_on_device) HIPCHK(hipMemcpyAsync(host + h_out, sum, (size_t)n * 48, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    if (!p->outputs_on_device) std::memcpy(aov, host + h_out, (size_t)n * 48);
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        const uint32_t *h_counts = (const uint32_t *)host;
        for (size_t b = 0; b < (size_t)S * n_batches; b++) stats->rays += h_counts[b * fw::COUNT_STRIDE];
        stats->rays_per_depth[0] = stats->rays;
        stats->n_batches = S * n_batches;
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ws->events[0], ws->events[1]));
        stats->ms_render = ms;
        stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FW_OK;
}

// fw_denoise: one device allocation per call — the packed guide (32 B per pixel) and the ping-pong e / v buffers (2 x 16 B per pixel), and
// with host arrays the inputs and outputs staged behind them — released on every way out of this function.
int denoise_impl(const fw_denoise_params *p, const float *color, const float *aov, const float *moments, float *linear_rgb, float *gamma_rgb,
                 uint8_t *rgb8) {
    if (!p || !color || !aov) return fail(FW_ERR_BAD_ARG, "null argument");
    if (p->width == 0 || p->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    if (p->iterations > FW_DENOISE_MAX_ITERATIONS) return fail(FW_ERR_BAD_ARG, "iterations must be in 0..10");
    if (!std::isfinite(p->gamma) || !(p->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be finite and > 0");
    if (p->device < 0 || p->device >= MAX_DEVICES) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (p->on_device && (((uintptr_t)aov & 15u) || ((uintptr_t)moments & 15u))) return fail(FW_ERR_BAD_ARG, "device aov and moments must be 16-byte aligned");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    int ndev = 0;
    if (int rc = need_device(&ndev)) return rc;
    if (p->device >= ndev) return fail(FW_ERR_BAD_ARG, "device index out of range");
    const uint32_t n = (uint32_t)full, L = p->iterations;
    const int dev = p->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)p->stream;
    const bool host_io = !p->on_device;
    size_t off = 0;
    auto put = [&](size_t b) { const size_t at = off; off += (b + 255) & ~(size_t)255; return at; };
    const size_t o_guide = L ? put((size_t)n * 32) : 0, o_ev0 = L ? put((size_t)n * 16) : 0, o_ev1 = L ? put((size_t)n * 16) : 0;
    const size_t o_col = host_io ? put((size_t)n * 12) : 0, o_aov = host_io ? put((size_t)n * 48) : 0;
    const size_t o_mom = host_io && moments ? put((size_t)n * 16) : 0;
    const size_t o_lin = host_io && linear_rgb ? put((size_t)n * 12) : 0, o_gam = host_io && gamma_rgb ? put((size_t)n * 12) : 0;
    const size_t o_8 = host_io && rgb8 ? put((size_t)n * 3) : 0;
    struct Scratch : DevBuf { int dev; explicit Scratch(int d) : dev(d) {} ~Scratch() { if (p) { (void)hipSetDevice(dev); release(); } } };
    Scratch scratch(dev);
    if (int rc = scratch.alloc(std::max<size_t>(off, 256))) return rc;
    uint8_t *base = (uint8_t *)scratch.p;
    const float *d_col = color; const float4 *d_aov = (const float4 *)aov, *d_mom = (const float4 *)moments;
    float *d_lin = linear_rgb, *d_gam = gamma_rgb; uint8_t *d_8 = rgb8;
    if (host_io) {
        HIPCHK(hipMemcpyAsync(base + o_col, color, (size_t)n * 12, hipMemcpyHostToDevice, stream)); d_col = (const float *)(base + o_col);
        HIPCHK(hipMemcpyAsync(base + o_aov, aov, (size_t)n * 48, hipMemcpyHostToDevice, stream)); d_aov = (const float4 *)(base + o_aov);
        if (moments) { HIPCHK(hipMemcpyAsync(base + o_mom, moments, (size_t)n * 16, hipMemcpyHostToDevice, stream)); d_mom = (const float4 *)(base + o_mom); }
        d_lin = linear_rgb ? (float *)(base + o_lin) : nullptr; d_gam = gamma_rgb ? (float *)(base + o_gam) : nullptr; d_8 = rgb8 ? base + o_8 : nullptr;
    }
    fw::launch_denoise(stream, device_cus(dev), p->width, p->height, L, d_col, d_aov, d_mom, (float4 *)(base + o_guide), (float4 *)(base + o_ev0),
                       (float4 *)(base + o_ev1), p->gamma, d_8, d_gam, d_lin);
    if (host_io) {
        if (linear_rgb) HIPCHK(hipMemcpyAsync(linear_rgb, d_lin, (size_t)n * 12, hipMemcpyDeviceToHost, stream));
        if (gamma_rgb) HIPCHK(hipMemcpyAsync(gamma_rgb, d_gam, (size_t)n * 12, hipMemcpyDeviceToHost, stream));
        if (rgb8) HIPCHK(hipMemcpyAsync(rgb8, d_8, (size_t)n * 3, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    return FW_OK;
}

// fw_temporal's view of the previous camera: make_camera's position and basis, and w and the half extents as make_camera forms them
static fw::TpCamera temporal_camera(const fw_camera_settings &s, uint32_t width, uint32_t height) {
    const fw::DCamera c = make_camera(s, width, height);
    const float PI_F = 3.14159265358979323846f;
    const float theta = s.vfov * PI_F / 180.f;
    const V3 w = normalized(tov(s.cam_pos) - tov(s.look_at));
    fw::TpCamera t;
    for (int k = 0; k < 3; k++) { t.pos[k] = c.position[k]; t.u[k] = c.u[k]; t.v[k] = c.v[k]; }
    t.w[0] = w.x; t.w[1] = w.y; t.w[2] = w.z;
    t.half_height = std::tan(theta / 2.0f);
    t.half_width = t.half_height * (float)width / (float)height;
    return t;
}

static bool camera_finite(const fw_camera_settings &c) {
    const float f[9] = {c.cam_pos.x, c.cam_pos.y, c.cam_pos.z, c.look_at.x, c.look_at.y, c.look_at.z, c.vfov, c.aperture, c.focus_dist};
    for (float v : f) if (!std::isfinite(v)) return false;
    return true;
}

// fw_temporal: with host arrays one device allocation per call holds the inputs and outputs, released on every way out of this function;
// with device arrays the kernel works on the caller's memory and nothing is allocated.
int temporal_impl(const fw_temporal_params *p, const float *color, const float *moments, const float *aov, const float *hist_color,
                  const float *hist_moments, const float *hist_aov, const float *prev_position, float *out_color, float *out_moments,
                  float *out_history) {
    if (!p || !color || !aov) return fail(FW_ERR_BAD_ARG, "null argument");
    if (p->width == 0 || p->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    const int n_hist = (hist_color ? 1 : 0) + (hist_moments ? 1 : 0) + (hist_aov ? 1 : 0);
    if (n_hist != 0 && n_hist != 3) return fail(FW_ERR_BAD_ARG, "hist_color, hist_moments and hist_aov must be all NULL or all given");
    {
        const uint64_t px = (uint64_t)p->width * p->height;
        const struct { const void *ptr; uint64_t bytes; } outs[3] = {{out_color, px * 12}, {out_moments, px * 16}, {out_history, px * 4}},
                                                          hist[3] = {{hist_color, px * 12}, {hist_moments, px * 16}, {hist_aov, px * 48}};
        for (const auto &o : outs)
            for (const auto &h : hist)
                if (o.ptr && h.ptr && (uintptr_t)o.ptr < (uintptr_t)h.ptr + h.bytes && (uintptr_t)h.ptr < (uintptr_t)o.ptr + o.bytes)
                    return fail(FW_ERR_BAD_ARG, "an output overlaps a history array");
    }
    if (!(p->max_history > 0.f)) return fail(FW_ERR_BAD_ARG, "max_history must be > 0");
    if (!camera_finite(p->camera) || !camera_finite(p->prev_camera)) return fail(FW_ERR_BAD_ARG, "camera fields must be finite");
    if (p->device < 0 || p->device >= MAX_DEVICES) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (p->on_device && (((uintptr_t)aov | (uintptr_t)moments | (uintptr_t)hist_color | (uintptr_t)hist_moments | (uintptr_t)hist_aov |
                          (uintptr_t)out_moments) & 15u))
        return fail(FW_ERR_BAD_ARG, "device aov, moments, history and out_moments must be 16-byte aligned");
    if (!moments && p->samples == 0) return fail(FW_ERR_BAD_ARG, "samples must be > 0 without moments");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    int ndev = 0;
    if (int rc = need_device(&ndev)) return rc;
    if (p->device >= ndev) return fail(FW_ERR_BAD_ARG, "device index out of range");
    const size_t n = (size_t)full;
    const int dev = p->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)p->stream;
    const fw::TpCamera cam = temporal_camera(p->prev_camera, p->width, p->height);
    const float *d_col = color, *d_hc = hist_color, *d_pp = prev_position;
    const float4 *d_mom = (const float4 *)moments, *d_aov = (const float4 *)aov, *d_hm = (const float4 *)hist_moments, *d_ha = (const float4 *)hist_aov;
    float *d_oc = out_color, *d_oh = out_history; float4 *d_om = (float4 *)out_moments;
    struct Scratch : DevBuf { int dev; explicit Scratch(int d) : dev(d) {} ~Scratch() { if (p) { (void)hipSetDevice(dev); release(); } } };
    Scratch scratch(dev);
    if (!p->on_device) {
        size_t off = 0;
        auto put = [&](const void *have, size_t b) { const size_t at = off; if (have) off += (b + 255) & ~(size_t)255; return at; };
        const size_t o_col = put(color, n * 12), o_mom = put(moments, n * 16), o_aov = put(aov, n * 48), o_hc = put(hist_color, n * 12),
                     o_hm = put(hist_moments, n * 16), o_ha = put(hist_aov, n * 48), o_pp = put(prev_position, n * 12),
                     o_oc = put(out_color, n * 12), o_om = put(out_moments, n * 16), o_oh = put(out_history, n * 4);
        if (int rc = scratch.alloc(std::max<size_t>(off, 256))) return rc;
        uint8_t *base = (uint8_t *)scratch.p;
#define FW_TP_UP(dst, type, src, at, bytes) \
        if (src) { HIPCHK(hipMemcpyAsync(base + (at), src, bytes, hipMemcpyHostToDevice, stream)); dst = (type)(base + (at)); }
        FW_TP_UP(d_col, const float *, color, o_col, n * 12) FW_TP_UP(d_aov, const float4 *, aov, o_aov, n * 48)
        FW_TP_UP(d_mom, const float4 *, moments, o_mom, n * 16) FW_TP_UP(d_hc, const float *, hist_color, o_hc, n * 12)
        FW_TP_UP(d_hm, const float4 *, hist_moments, o_hm, n * 16) FW_TP_UP(d_ha, const float4 *, hist_aov, o_ha, n * 48)
        FW_TP_UP(d_pp, const float *, prev_position, o_pp, n * 12)
#undef FW_TP_UP
        d_oc = out_color ? (float *)(base + o_oc) : nullptr; d_om = out_moments ? (float4 *)(base + o_om) : nullptr;
        d_oh = out_history ? (float *)(base + o_oh) : nullptr;
    }
    fw::launch_temporal(stream, p->width, p->height, cam, (float)p->samples, p->max_history, d_col, d_mom, d_aov, d_hc, d_hm, d_ha, d_pp, d_oc, d_om, d_oh);
    if (!p->on_device) {
        if (out_color) HIPCHK(hipMemcpyAsync(out_color, d_oc, n * 12, hipMemcpyDeviceToHost, stream));
        if (out_moments) HIPCHK(hipMemcpyAsync(out_moments, d_om, n * 16, hipMemcpyDeviceToHost, stream));
        if (out_history) HIPCHK(hipMemcpyAsync(out_history, d_oh, n * 4, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    return FW_OK;
}

// ---- what the calls that stage arrays, generate rays, render or trace them and reduce the result share --------
// device scratch of one call, released on every way out of the function that owns it
struct CallScratch : DevBuf { int dev; explicit CallScratch(int d) : dev(d) {} ~CallScratch() { if (p) { (void)hipSetDevice(dev); release(); } } };
// events around a call's own kernels, created only when the caller reads stats
template <int N> struct CallEvents { hipEvent_t e[N] = {}; ~CallEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } };

// the rays (and, in a bake, their accum or hits) of an automatic chunk of fw_render_model and the bakers, and the slab of a host call's
// per-item arrays
constexpr size_t CALL_SCRATCH_BYTES = (size_t)256 << 20;
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The arrays of one call on the device.  Each is declared once, with its byte size, as read (IN), read and written (INOUT), overwritten
// (OUT), the call's own work space (WORK) or work space that starts as zeros (ZERO).  A caller's device array is used where it lies; a
// host array (every array of a host call, and whatever is declared `host_always`) and the work space get 256-byte aligned slots of one
// allocation: none at all when no slot is needed.  up() allocates and enqueues the uploads and the zeroing in declaration order;
// finish() enqueues the downloads not made yet in declaration order, drains the stream and reports the kernels' error.  From up() to
// the end of finish() every way out drains the stream before the scratch is released.  A NULL array takes no slot and stays NULL.
struct Staged {
    enum Kind { IN, INOUT, OUT, WORK, ZERO };
    struct Slot { Kind kind; void *host; size_t bytes, at; bool staged, back; };
    hipStream_t stream; bool on_device; CallScratch scratch;
    Slot slots[20] = {}; int n_slots = 0; size_t off = 0; bool armed = false;
    Staged(int device, hipStream_t stream_, bool on_device_) : stream(stream_), on_device(on_device_), scratch(device) {}
    ~Staged() { if (armed) (void)hipStreamSynchronize(stream); }
    int add(Kind kind, const void *p, size_t bytes, bool host_always = false) {
        const bool staged = kind == WORK || kind == ZERO || (p && (host_always || !on_device));
        slots[n_slots] = Slot{kind, const_cast<void *>(p), bytes, off, staged, staged && (kind == INOUT || kind == OUT)};
        if (staged) off += align256(bytes);
        return n_slots++;
    }
    // running sums: the caller's device memory, a host caller's staged in and out, or — NULL — zeros in the scratch that nobody reads back
    int add_sums(float *sums, size_t bytes) { return sums ? add(INOUT, sums, bytes) : add(ZERO, nullptr, bytes); }
    template <class T> T *ptr(int i) const { const Slot &s = slots[i]; return s.staged ? (T *)((uint8_t *)scratch.p + s.at) : (T *)s.host; }
    int put(int i, const void *src) { HIPCHK(hipMemcpyAsync(ptr<void>(i), src, slots[i].bytes, hipMemcpyHostToDevice, stream)); return FW_OK; }
    int get(int i, void *dst) { HIPCHK(hipMemcpyAsync(dst, ptr<void>(i), slots[i].bytes, hipMemcpyDeviceToHost, stream)); return FW_OK; }
    int up() {
        if (int rc = scratch.alloc(off)) return rc;
        armed = true;
        for (int i = 0; i < n_slots; i++) {
            const Slot &s = slots[i];
            if (!s.staged || !s.bytes) continue;
            if (s.kind == IN || s.kind == INOUT) { if (int rc = put(i, s.host)) return rc; }
            else if (s.kind == ZERO) HIPCHK(hipMemsetAsync(ptr<void>(i), 0, s.bytes, stream));
        }
        return FW_OK;
    }
    // a staged INOUT or OUT slot goes back to its host array, once
    int download(int i) {
        if (!slots[i].back) return FW_OK;
        slots[i].back = false;
        return get(i, slots[i].host);
    }
    // where the slot's content lands on the host: a host caller's own array (its download), else — if `need` — `keep`; else nowhere (NULL)
    int fetch(int i, bool need, std::vector<float> &keep, const float *&landed) {
        landed = nullptr;
        if (slots[i].back) { landed = (const float *)slots[i].host; return download(i); }
        if (!need) return FW_OK;
        keep.resize(slots[i].bytes / 4);
        landed = keep.data();
        return get(i, keep.data());
    }
    int finish() {
        for (int i = 0; i < n_slots; i++) if (int rc = download(i)) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        armed = false;
        HIPCHK(hipGetLastError());
        return FW_OK;
    }
};

// The per-item arrays of a call over n items.  Device arrays: one launch over the caller's memory.  Host arrays: slabs of `per` items
// through slots of `st` — declare every array before st.up() — and per slab: the inputs copied in (a strided one packed first: three
// floats per item from `host`, three more from `with`), launch(first_item, k), the outputs copied back, the stream drained.  `pack` is
// the one strided input's host staging: a call declares at most one.
struct HostSlabs {
    struct Arr { void *host; size_t item; uint32_t stride; const float *with; int slot; bool out; };
    Staged &st; uint32_t n, per;
    Arr arrs[8] = {}; int n_arrs = 0; std::vector<float> pack;
    HostSlabs(Staged &st_, uint32_t n_, size_t slab_item_bytes) : st(st_), n(n_), per((uint32_t)std::min<uint64_t>(n_, std::max<uint64_t>(1, CALL_SCRATCH_BYTES / slab_item_bytes))) {}
    int add(const void *host, size_t item, uint32_t stride, const float *with, bool out) {
        const bool slab = host && !st.on_device;
        arrs[n_arrs] = Arr{const_cast<void *>(host), item, stride, with, slab ? st.add(Staged::WORK, nullptr, (size_t)per * item) : -1, out};
        if (slab && stride) pack.resize((size_t)per * item / 4);
        return n_arrs++;
    }
    int in(const void *host, size_t item, uint32_t stride = 0, const float *with = nullptr) { return add(host, item, stride, with, false); }
    int out(void *host, size_t item) { return add(host, item, 0, nullptr, true); }
    template <class T> T *ptr(int a) const { return arrs[a].slot < 0 ? (T *)arrs[a].host : st.ptr<T>(arrs[a].slot); }
    // of a strided input: where its second three floats are, and its stride on the device
    const float *with(int a) const { return arrs[a].slot < 0 ? arrs[a].with : ptr<float>(a) + 3; }
    uint32_t stride(int a) const { return arrs[a].slot < 0 ? arrs[a].stride : (uint32_t)(arrs[a].item / 4); }
    template <class Launch> int run(Launch launch) {
        if (st.on_device) launch(0u, n);
        else for (uint32_t done = 0; done < n; done += per) {
            const uint32_t k = std::min(per, n - done);
            for (int a = 0; a < n_arrs; a++) {
                const Arr &A = arrs[a];
                if (A.slot < 0 || A.out) continue;
                const void *src = (const uint8_t *)A.host + (size_t)done * A.item;
                if (A.stride) {
                    const size_t w = A.item / 4;
                    for (uint32_t i = 0; i < k; i++) {
                        const float *ps = (const float *)A.host + (size_t)(done + i) * A.stride;
                        float *o = pack.data() + (size_t)i * w;
                        o[0] = ps[0]; o[1] = ps[1]; o[2] = ps[2];
                        if (A.with) { const float *ns = A.with + (size_t)(done + i) * A.stride; o[3] = ns[0]; o[4] = ns[1]; o[5] = ns[2]; }
                    }
                    src = pack.data();
                }
                HIPCHK(hipMemcpyAsync(st.ptr<void>(A.slot), src, (size_t)k * A.item, hipMemcpyHostToDevice, st.stream));
            }
            launch(done, k);
            for (int a = 0; a < n_arrs; a++) {
                const Arr &A = arrs[a];
                if (A.slot >= 0 && A.out) HIPCHK(hipMemcpyAsync((uint8_t *)A.host + (size_t)done * A.item, st.ptr<void>(A.slot), (size_t)k * A.item, hipMemcpyDeviceToHost, st.stream));
            }
            HIPCHK(hipStreamSynchronize(st.stream));
        }
        if (st.on_device) HIPCHK(hipStreamSynchronize(st.stream));
        st.armed = false;
        HIPCHK(hipGetLastError());
        return FW_OK;
    }
};

// Host output of a ray generator: `n` items of `item_bytes` of rays each go to `dst` in slabs through scratch of the call's own.
// launch(first_item, k, d_slab) enqueues the generator for the items [first_item, first_item + k).  Returns with the stream drained.
template <class Launch> int host_slabs(hipStream_t stream, int device, uint32_t n, size_t item_bytes, float *dst, Launch launch) {
    Staged st(device, stream, false);
    HostSlabs sl(st, n, item_bytes);
    const int rays = sl.out(dst, item_bytes);
    if (int rc = st.up()) { (void)hipStreamSynchronize(stream); return rc; }
    return sl.run([&](uint32_t done, uint32_t k) { launch(done, k, sl.ptr<float>(rays)); });
}

// A float output that the host computes: fill(out) writes its n floats — into a host caller's array, or into a temporary that is then
// copied to the caller's device memory
template <class Fill> int host_output(hipStream_t stream, float *dst, size_t n, bool on_device, Fill fill) {
    std::vector<float> tmp;
    float *out = dst;
    if (on_device) { tmp.resize(n); out = tmp.data(); }
    fill(out);
    if (on_device) {
        HIPCHK(hipMemcpyAsync(dst, tmp.data(), n * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    return FW_OK;
}
// sh = sums / rounds so far, divided on the host in double and rounded once (fw_bake_probes, fw_bake_probe_radiance)
int sh_from_sums(hipStream_t stream, const float *h_sums, size_t n, uint32_t first_round, uint32_t rounds, float *sh, bool on_device) {
    const double n_rounds = (double)((uint64_t)first_round + rounds);
    return host_output(stream, sh, n, on_device, [&](float *out) { for (size_t i = 0; i < n; i++) out[i] = (float)((double)h_sums[i] / n_rounds); });
}
// the stats of a chunked call, handed to the caller that reads them
void stats_finish(fw_stats *stats, const fw_stats &total, std::chrono::steady_clock::time_point wall0) {
    if (!stats) return;
    *stats = total;
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
}

// The chunks of one round of a bake: per chunk of the `n_items` items (probes, covered texels, points) generate(first_item,
// k) enqueues the rays of k items, middle(first_item, k, stats or NULL) renders or traces them and reduce(first_item, k) enqueues the
// chunk's reduction.  total (the caller reads stats): the middle steps' stats, plus the two kernels' time — in ms_render always, in
// ms_raygen / ms_accumulate with FW_FLAG_TIME_KERNELS.  The caller owns the checks, the scratch, the outputs and the draining.
struct BakeChunks {
    hipStream_t stream; uint32_t n_items, chunk; bool timing; fw_stats *total;
    CallEvents<4> ev;                                 // around the two kernels' launches
    int begin() { if (total) for (hipEvent_t &e : ev.e) HIPCHK(hipEventCreate(&e)); return FW_OK; }
    template <class Generate, class Middle, class Reduce> int round(Generate generate, Middle middle, Reduce reduce) {
        for (uint32_t i0 = 0; i0 < n_items; i0 += chunk) {
            const uint32_t k = std::min(chunk, n_items - i0);
            if (total) HIPCHK(hipEventRecord(ev.e[0], stream));
            generate(i0, k);
            if (total) HIPCHK(hipEventRecord(ev.e[1], stream));
            fw_stats gs{};
            if (int rc = middle(i0, k, total ? &gs : nullptr)) return rc;
            if (total) HIPCHK(hipEventRecord(ev.e[2], stream));
            reduce(i0, k);
            if (!total) continue;
            HIPCHK(hipEventRecord(ev.e[3], stream));
            HIPCHK(hipEventSynchronize(ev.e[3]));
            float gen_ms = 0.f, red_ms = 0.f;
            HIPCHK(hipEventElapsedTime(&gen_ms, ev.e[0], ev.e[1]));
            HIPCHK(hipEventElapsedTime(&red_ms, ev.e[2], ev.e[3]));
            stats_add(*total, gs);
            total->ms_render += gen_ms + red_ms;
            if (timing) { total->ms_raygen += gen_ms; total->ms_accumulate += red_ms; }
        }
        return FW_OK;
    }
};

// The rounds of a bake that renders (fw_bake_probes, fw_bake_lightmap, fw_bake_probe_radiance): per round r of [first_round, first_round
// + rounds) BakeChunks' chunks with render_impl as the middle step: the chunk's `directions` rays per item rendered into the zeroed
// d_acc — the fw_render_rays call of the chunk (rays_impl's frame) with gamma 1, seed + r and key_base = first_item x directions.
// generate(r, first_item, k, d_rays) and reduce(first_item, k, d_rays, d_acc) are the caller's kernels; their bytes join the chunk's
// stats: 24 per ray and gen_item per item generated, red_ray per ray and red_item per item reduced.
struct BakeRounds {
    uint32_t first_round, rounds, n_items, directions, chunk;
    float *d_rays, *d_acc;                             // chunk x directions x 24 and x 16 bytes of the call's scratch
    uint32_t gen_item, red_ray, red_item;
};
template <class Generate, class Reduce>
int bake_rounds(fw_scene *sc, const fw_render_rays_params *rp, const BakeRounds &b, fw_stats *total, Generate generate, Reduce reduce) {
    hipStream_t stream = (hipStream_t)rp->stream;
    BakeChunks c{stream, b.n_items, b.chunk, (rp->flags & FW_FLAG_TIME_KERNELS) != 0, total};
    if (int rc = c.begin()) return rc;
    for (uint32_t r = b.first_round; r - b.first_round < b.rounds; r++) {      // (first_round + rounds may be 2^32 - 1: r itself never gets there)
        fw_render_rays_params q = *rp;
        q.gamma = 1.f; q.on_device = 1; q.seed = rp->seed + r;
        const auto render = [&](uint32_t i0, uint32_t k, fw_stats *gs) {
            const uint32_t n = k * b.directions;
            q.n_rays = n;
            HIPCHK(hipMemsetAsync(b.d_acc, 0, (size_t)n * 16, stream));
            const fw_render_params P = rays_frame(&q, rp->samples);
            const RayInput ri{b.d_rays, n, false, nullptr, i0 * b.directions, true};
            if (int rc = render_impl(sc, &P, nullptr, nullptr, nullptr, gs, 0, b.d_acc, nullptr, nullptr, &ri)) return rc;
            if (gs) {
                gs->bytes_raygen += (uint64_t)n * 24 + (uint64_t)k * b.gen_item;
                gs->bytes_accumulate += (uint64_t)n * b.red_ray + (uint64_t)k * b.red_item;
            }
            return (int)FW_OK;
        };
        if (int rc = c.round([&](uint32_t i0, uint32_t k) { generate(r, i0, k, b.d_rays); }, render,
                             [&](uint32_t i0, uint32_t k) { reduce(i0, k, b.d_rays, b.d_acc); }))
            return rc;
    }
    return FW_OK;
}

// The same for a bake that traces (fw_bake_probe_depth, fw_bake_ao, and fw_relocate_probes one step at a time): the middle step of round
// r is trace_impl over the chunk's rays with seed + r and key_base = first_item x directions.  The traced bakes count no bytes of their own.
struct TraceRounds {
    uint32_t n_items, directions, chunk;
    float *d_rays; fw_hit *d_hits;                     // chunk x directions x 24 bytes and x one fw_hit of the call's scratch
};
template <class Generate, class Reduce>
int trace_round(fw_scene *sc, const fw_trace_params *tp, const TraceRounds &b, BakeChunks &c, uint32_t r, Generate generate, Reduce reduce) {
    fw_trace_params q = *tp;
    q.on_device = 1; q.seed = tp->seed + r;
    return c.round([&](uint32_t i0, uint32_t k) { generate(r, i0, k, b.d_rays); },
                   [&](uint32_t i0, uint32_t k, fw_stats *gs) { q.key_base = i0 * b.directions; return trace_impl(sc, &q, b.d_rays, k * b.directions, b.d_hits, gs); },
                   [&](uint32_t i0, uint32_t k) { reduce(i0, k, b.d_rays, b.d_hits); });
}
template <class Generate, class Reduce>
int trace_rounds(fw_scene *sc, const fw_trace_params *tp, const TraceRounds &b, uint32_t first_round, uint32_t rounds, fw_stats *total, Generate generate,
                 Reduce reduce) {
    BakeChunks c{(hipStream_t)tp->stream, b.n_items, b.chunk, (tp->flags & FW_FLAG_TIME_KERNELS) != 0, total};
    if (int rc = c.begin()) return rc;
    for (uint32_t r = first_round; r - first_round < rounds; r++)      // (first_round + rounds may be 2^32 - 1: r itself never gets there)
        if (int rc = trace_round(sc, tp, b, c, r, generate, reduce)) return rc;
    return FW_OK;
}

// ---- camera models (include/firework_hip.h) ------------------------------------------------------------------
// The model's own argument checks (FW_ERR_BAD_ARG only) and its device form: camera.rs's basis in float64.  too_large: W x H >= 2^31, which
// the callers report as FW_ERR_UNSUPPORTED after their own argument checks.
int model_prepare(const fw_camera_model *m, fw::DModel &d, bool &too_large) {
    if (m->kind != FW_MODEL_PANORAMA && m->kind != FW_MODEL_ORTHOGRAPHIC && m->kind != FW_MODEL_FISHEYE) return fail(FW_ERR_BAD_ARG, "unknown camera model kind");
    if (m->width == 0 || m->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    if (!camera_finite(m->camera)) return fail(FW_ERR_BAD_ARG, "camera fields must be finite");
    d = fw::DModel{};
    d.kind = m->kind; d.width = m->width; d.height = m->height;
    d.seed32 = seed32_of(m->seed);
    d.jitter = m->jitter ? 1u : 0u;
    const double pos[3] = {m->camera.cam_pos.x, m->camera.cam_pos.y, m->camera.cam_pos.z};
    const double at[3] = {m->camera.look_at.x, m->camera.look_at.y, m->camera.look_at.z};
    for (int k = 0; k < 3; k++) d.pos[k] = pos[k];
    if (m->kind != FW_MODEL_PANORAMA) {
        double w[3] = {pos[0] - at[0], pos[1] - at[1], pos[2] - at[2]};
        const double wl = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
        if (!(wl > 0.0)) return fail(FW_ERR_BAD_ARG, "cam_pos and look_at must differ");
        for (double &c : w) c /= wl;
        double u[3] = {w[2], 0.0, -w[0]};                                   // Y x w
        const double ul = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
        if (!(ul > 0.0)) return fail(FW_ERR_BAD_ARG, "the view direction must not be parallel to Y");
        for (double &c : u) c /= ul;
        const double v[3] = {w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]};     // w x u
        for (int k = 0; k < 3; k++) { d.u[k] = u[k]; d.v[k] = v[k]; d.w[k] = w[k]; d.dir[k] = at[k] - pos[k]; }
    }
    if (m->kind == FW_MODEL_ORTHOGRAPHIC) {
        if (!std::isfinite(m->view_height) || !(m->view_height > 0.0)) return fail(FW_ERR_BAD_ARG, "view_height must be finite and > 0");
        d.view_h = m->view_height;
        d.view_w = m->view_height * (double)m->width / (double)m->height;
    }
    if (m->kind == FW_MODEL_FISHEYE) {
        if (!(m->fov > 0.0 && m->fov <= 360.0)) return fail(FW_ERR_BAD_ARG, "fov must be in (0, 360] degrees");
        d.half_fov = (m->fov * (3.141592653589793 / 180.0)) / 2.0;
        d.diag = std::sqrt((double)m->width * (double)m->width + (double)m->height * (double)m->height);
    }
    too_large = (uint64_t)m->width * m->height >= (1ull << 31);
    return FW_OK;
}

// fw_model_rays: device output — one launch into the caller's memory; host output — host_slabs of samples
int model_rays_impl(const fw_camera_model *m, int device, uint32_t first, uint32_t n_samples, float *rays, int on_device, void *stream_) {
    if (!m || !rays) return fail(FW_ERR_BAD_ARG, "null argument");
    fw::DModel dm; bool too_large = false;
    if (int rc = model_prepare(m, dm, too_large)) return rc;
    if (n_samples == 0) return fail(FW_ERR_BAD_ARG, "n_samples must be > 0");
    if ((uint64_t)first + n_samples > (1ull << 32)) return fail(FW_ERR_BAD_ARG, "first_sample + n_samples overflows");
    if (on_device && ((uintptr_t)rays & 3u)) return fail(FW_ERR_BAD_ARG, "rays must be 4-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "W x H must be below 2^31 (the jitter's counter is 32-bit)");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n_pix = (size_t)m->width * m->height;
    if (on_device) {
        fw::launch_model_rays(stream, device_cus(device), dm, first, n_samples, rays);
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipGetLastError());
        return FW_OK;
    }
    return host_slabs(stream, device, n_samples, n_pix * 24, rays, [&](uint32_t done, uint32_t k, float *d_rays) {
        fw::launch_model_rays(stream, device_cus(device), dm, first + done, k, d_rays);
    });
}

// fw_render_model: per chunk of samples, k_model_rays into the call's scratch, then render_impl over those device rays on top of the
// running sums — the fw_render_rays call of the chunk (rays_impl's frame), so the sums and the resolve are its own.  Its loop is not
// bake_rounds': it chunks samples, not items, keeps one accum across the chunks, and only its last chunk resolves.
int render_model_impl(fw_scene *sc, const fw_camera_model *m, const fw_render_rays_params *rp, float *accum, uint8_t *rgb8, float *gamma_rgb,
                      float *linear_rgb, fw_stats *stats) {
    if (!sc || !m || !rp) return fail(FW_ERR_BAD_ARG, "null argument");
    fw::DModel dm; bool too_large = false;
    if (int rc = model_prepare(m, dm, too_large)) return rc;
    if (rp->samples == 0 || rp->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if ((uint64_t)rp->first_sample + rp->samples > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_sample + samples overflows");
    if (!std::isfinite(rp->gamma) || !(rp->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be finite and > 0");
    if ((uint64_t)m->width * m->height != rp->n_rays) return fail(FW_ERR_BAD_ARG, "n_rays must be width x height");
    if (!accum && rp->first_sample > 0) return fail(FW_ERR_BAD_ARG, "first_sample > 0 needs the accumulation buffer of the samples before it");
    if (rp->on_device && ((uintptr_t)accum & 15u)) return fail(FW_ERR_BAD_ARG, "device accum must be 16-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "W x H must be below 2^31 (the jitter's counter is 32-bit)");
    if (int rc = need_device()) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)rp->stream;
    const size_t n_pix = rp->n_rays;
    const uint32_t S = rp->samples;
    const uint32_t chunk = std::min<uint32_t>(S, m->chunk_samples ? m->chunk_samples : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / (n_pix * 24)));
    // the running sums between chunks when the caller keeps none: device memory behind the rays, or a host array
    const bool own_accum = !accum && chunk < S;
    const size_t ray_bytes = ((size_t)chunk * n_pix * 24 + 255) & ~(size_t)255;
    CallScratch scratch(dev);
    if (int rc = scratch.alloc(ray_bytes + (own_accum && rp->on_device ? n_pix * 16 : 0))) return rc;
    std::vector<float> host_accum;
    float *acc = accum;
    if (own_accum) {
        if (rp->on_device) { acc = (float *)((uint8_t *)scratch.p + ray_bytes); HIPCHK(hipMemsetAsync(acc, 0, n_pix * 16, stream)); }
        else { host_accum.assign(n_pix * 4, 0.f); acc = host_accum.data(); }
    }
    CallEvents<2> ev;                                 // around the generator's launch
    if (stats) for (hipEvent_t &e : ev.e) HIPCHK(hipEventCreate(&e));
    const int n_cus = device_cus(dev);
    const bool timing = (rp->flags & FW_FLAG_TIME_KERNELS) != 0;

    fw_stats total{};
    for (uint32_t done = 0; done < S; done += chunk) {
        const uint32_t k = std::min(chunk, S - done), first = rp->first_sample + done;
        const bool last = done + k == S;
        if (stats) HIPCHK(hipEventRecord(ev.e[0], stream));
        fw::launch_model_rays(stream, n_cus, dm, first, k, (float *)scratch.p);
        if (stats) HIPCHK(hipEventRecord(ev.e[1], stream));
        const fw_render_params P = rays_frame(rp, k);
        const RayInput ri{(const float *)scratch.p, rp->n_rays, true, nullptr, rp->key_base, true};
        fw_stats gs{};
        if (int rc = render_impl(sc, &P, last ? rgb8 : nullptr, last ? gamma_rgb : nullptr, last ? linear_rgb : nullptr, stats ? &gs : nullptr,
                                 first, acc, nullptr, nullptr, &ri)) return rc;      // (returns with the stream drained)
        if (!stats) continue;
        float gen_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&gen_ms, ev.e[0], ev.e[1]));
        stats_add(total, gs);
        total.ms_render += gen_ms;
        if (timing) total.ms_raygen += gen_ms;
        total.bytes_raygen += (uint64_t)k * n_pix * 24;                                    // (the generator's stores)
    }
    if (stats) {
        *stats = total;
        stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FW_OK;
}

// fw_render_model_aovs: aovs_impl over a frame of the model's size whose one-sample ray buffer k_model_rays fills
int model_aovs_impl(fw_scene *sc, const fw_camera_model *m, const fw_render_params *p, float *aov, fw_stats *stats) {
    if (!sc || !m || !p || !aov) return fail(FW_ERR_BAD_ARG, "null argument");
    fw::DModel dm; bool too_large = false;
    if (int rc = model_prepare(m, dm, too_large)) return rc;
    if (p->samples == 0 || p->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if (p->outputs_on_device && ((uintptr_t)aov & 15u)) return fail(FW_ERR_BAD_ARG, "a device aov must be 16-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "W x H must be below 2^31 (the jitter's counter is 32-bit)");
    fw_render_params P{};
    P.width = m->width; P.height = m->height; P.samples = p->samples; P.gamma = 1.f; P.use_bvh = p->use_bvh; P.seed = p->seed;
    P.rng_mode = FW_RNG_CTR; P.outputs_on_device = p->outputs_on_device; P.stream = p->stream;
    return aovs_impl(sc, &P, aov, stats, &dm);
}

// ---- irradiance probes (include/firework_hip.h) ----------------------------------------------------------------
// The set's own argument checks (FW_ERR_BAD_ARG only).  too_large: n_probes x D >= 2^31, which the callers report as FW_ERR_UNSUPPORTED
// after their own argument checks.
int probe_set_check(const fw_probe_set *s, bool &too_large) {
    if (!s->positions) return fail(FW_ERR_BAD_ARG, "null positions");
    if (s->n_probes == 0) return fail(FW_ERR_BAD_ARG, "n_probes must be > 0");
    if (s->directions == 0 || s->directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    for (uint64_t i = 0; i < (uint64_t)s->n_probes * 3; i++)
        if (!std::isfinite(s->positions[i])) return fail(FW_ERR_BAD_ARG, "probe " + std::to_string(i / 3) + " has a non-finite position");
    too_large = (uint64_t)s->n_probes * s->directions >= (1ull << 31);
    return FW_OK;
}

fw::DProbes probes_device(const fw_probe_set *s, uint32_t round, uint32_t first_probe, const float *d_positions) {
    fw::DProbes d{};
    d.directions = s->directions;
    d.seed32 = seed32_of(s->seed);
    d.jitter = s->jitter ? 1u : 0u;
    d.round = round; d.first_probe = first_probe; d.positions = d_positions;
    return d;
}

// fw_probe_rays: the positions of the probes asked for go to scratch of the call's own; device output — one launch into the caller's
// memory; host output — host_slabs of probes
int probe_rays_impl(const fw_probe_set *s, int device, uint32_t round, uint32_t first_probe, uint32_t n, float *rays, int on_device, void *stream_) {
    if (!s || !rays) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = probe_set_check(s, too_large)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if ((uint64_t)first_probe + n > s->n_probes) return fail(FW_ERR_BAD_ARG, "first_probe + n exceeds n_probes");
    if (on_device && ((uintptr_t)rays & 3u)) return fail(FW_ERR_BAD_ARG, "rays must be 4-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    CallScratch scratch(device);
    if (int rc = scratch.alloc((size_t)n * 12)) return rc;
    const float *d_pos = (const float *)scratch.p;
    HIPCHK(hipMemcpyAsync(scratch.p, s->positions + (size_t)first_probe * 3, (size_t)n * 12, hipMemcpyHostToDevice, stream));
    if (on_device) {
        fw::launch_probe_rays(stream, device_cus(device), probes_device(s, round, first_probe, d_pos), n, rays);
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipGetLastError());
        return FW_OK;
    }
    return host_slabs(stream, device, n, (size_t)s->directions * 24, rays, [&](uint32_t done, uint32_t k, float *d_rays) {
        fw::launch_probe_rays(stream, device_cus(device), probes_device(s, round, first_probe + done, d_pos + (size_t)done * 3), k, d_rays);
    });
}

// fw_probe_project: a one-shot call over Staged arrays — with host arrays one device allocation per call holds the inputs and the sums,
// released on every way out; with device arrays the kernel works on the caller's memory and nothing is allocated
int probe_project_impl(int device, uint32_t n_probes, uint32_t directions, uint32_t samples, const float *rays, const float *accum, float *sums,
                       int on_device, void *stream_) {
    if (!rays || !accum || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (n_probes == 0) return fail(FW_ERR_BAD_ARG, "n_probes must be > 0");
    if (directions == 0 || directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (samples == 0 || samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if (on_device && (((uintptr_t)accum & 15u) || (((uintptr_t)rays | (uintptr_t)sums) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device accum must be 16-byte aligned, device rays and sums 4-byte aligned");
    if ((uint64_t)n_probes * directions >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)n_probes * directions;
    Staged st(device, stream, on_device != 0);
    const int i_rays = st.add(Staged::IN, rays, n * 24), i_acc = st.add(Staged::IN, accum, n * 16), i_sums = st.add(Staged::INOUT, sums, (size_t)n_probes * 108);
    if (int rc = st.up()) return rc;
    fw::launch_probe_project(stream, device_cus(device), n_probes, directions, samples, st.ptr<const float>(i_rays), st.ptr<const float>(i_acc), st.ptr<float>(i_sums));
    return st.finish();
}

// fw_bake_probes: its own are the argument checks, the Staged arrays (positions, a chunk's rays and accum, the running sums unless the
// caller's device memory holds them), k_probe_rays and k_probe_project as bake_rounds' generator and reducer, and sh, divided on the host.
int bake_probes_impl(fw_scene *sc, const fw_probe_set *s, const fw_render_rays_params *rp, uint32_t first_round, uint32_t rounds, float *sums,
                     float *sh, fw_stats *stats) {
    if (!sc || !s || !rp) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = probe_set_check(s, too_large)) return rc;
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (rp->samples == 0 || rp->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (rp->on_device && (((uintptr_t)sums | (uintptr_t)sh) & 3u)) return fail(FW_ERR_BAD_ARG, "device sums and sh must be 4-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if (int rc = need_device()) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)rp->stream;
    const uint32_t N = s->n_probes, D = s->directions, S = rp->samples;
    const uint32_t chunk = std::min<uint32_t>(N, s->chunk_probes ? s->chunk_probes : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * 40)));
    Staged st(dev, stream, rp->on_device != 0);
    const int i_pos = st.add(Staged::IN, s->positions, (size_t)N * 12, true), i_rays = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 24),
              i_acc = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 16), i_sums = st.add_sums(sums, (size_t)N * 108);
    if (int rc = st.up()) return rc;
    const float *d_pos = st.ptr<const float>(i_pos);
    float *d_sums = st.ptr<float>(i_sums);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    const BakeRounds b{first_round, rounds, N, D, chunk, st.ptr<float>(i_rays), st.ptr<float>(i_acc), 0, 40, 216};       // (the projection's loads and its sums)
    if (int rc = bake_rounds(sc, rp, b, stats ? &total : nullptr,
            [&](uint32_t r, uint32_t p0, uint32_t k, float *rays) { fw::launch_probe_rays(stream, n_cus, probes_device(s, r, p0, d_pos + (size_t)p0 * 3), k, rays); },
            [&](uint32_t p0, uint32_t k, const float *rays, const float *acc) { fw::launch_probe_project(stream, n_cus, k, D, S, rays, acc, d_sums + (size_t)p0 * 27); }))
        return rc;
    // the outputs: sums where the caller keeps them, and sh = sums / rounds so far
    std::vector<float> keep;
    const float *h_sums = nullptr;
    if (int rc = st.fetch(i_sums, sh != nullptr, keep, h_sums)) return rc;
    if (int rc = st.finish()) return rc;
    if (sh) if (int rc = sh_from_sums(stream, h_sums, (size_t)N * 27, first_round, rounds, sh, rp->on_device != 0)) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- lightmaps (include/firework_hip.h) -------------------------------------------------------------------------
// The lightmap's own argument checks (FW_ERR_BAD_ARG only).  too_large: the host's upper bound of n_cov x D is >= 2^31, which the callers
// report as FW_ERR_UNSUPPORTED after their own argument checks.
int lightmap_check(const fw_lightmap *lm, bool &too_large) {
    if (!lm->verts || !lm->indices || !lm->uvs) return fail(FW_ERR_BAD_ARG, "null verts, indices or uvs");
    if (lm->n_verts == 0) return fail(FW_ERR_BAD_ARG, "n_verts must be > 0");
    if (lm->n_indices == 0 || lm->n_indices % 3u) return fail(FW_ERR_BAD_ARG, "n_indices must be a positive multiple of 3");
    if (lm->width == 0 || lm->width > 16384u || lm->height == 0 || lm->height > 16384u) return fail(FW_ERR_BAD_ARG, "width and height must be in 1..16384");
    if (lm->directions == 0 || lm->directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (!std::isfinite(lm->bias) || lm->bias < 0.f) return fail(FW_ERR_BAD_ARG, "bias must be finite and >= 0");
    const float place[7] = {lm->position.x, lm->position.y, lm->position.z, lm->rotation.s, lm->rotation.xy, lm->rotation.xz, lm->rotation.yz};
    for (float v : place) if (!std::isfinite(v)) return fail(FW_ERR_BAD_ARG, "the placement (position, rotation) is not finite");
    for (uint32_t i = 0; i < lm->n_indices; i++)
        if (lm->indices[i] >= lm->n_verts) return fail(FW_ERR_BAD_ARG, "index " + std::to_string(i) + " is not below n_verts");
    for (uint64_t i = 0; i < (uint64_t)lm->n_verts * 3; i++)
        if (!std::isfinite(lm->verts[i])) return fail(FW_ERR_BAD_ARG, "vert " + std::to_string(i / 3) + " is not finite");
    for (uint64_t i = 0; i < (uint64_t)lm->n_verts * 2; i++)
        if (!std::isfinite(lm->uvs[i])) return fail(FW_ERR_BAD_ARG, "uv " + std::to_string(i / 2) + " is not finite");
    if (lm->normals)
        for (uint64_t i = 0; i < (uint64_t)lm->n_verts * 3; i++)
            if (!std::isfinite(lm->normals[i])) return fail(FW_ERR_BAD_ARG, "normal " + std::to_string(i / 3) + " is not finite");
    // an upper bound of the covered texels: the triangles' UV bounding boxes, one texel wider than k_lm_cover's, clipped to the image
    const double W = lm->width, H = lm->height;
    const uint64_t all = (uint64_t)lm->width * lm->height;
    uint64_t cover = 0;
    for (uint32_t t = 0; t < lm->n_indices / 3u && cover < all; t++) {
        double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
        for (int k = 0; k < 3; k++) {
            const float *uv = lm->uvs + (size_t)lm->indices[t * 3u + k] * 2;
            lo[0] = std::min(lo[0], (double)uv[0]); hi[0] = std::max(hi[0], (double)uv[0]);
            lo[1] = std::min(lo[1], 1.0 - (double)uv[1]); hi[1] = std::max(hi[1], 1.0 - (double)uv[1]);
        }
        const double x0 = std::max(0.0, std::floor(lo[0] * W - 0.5) - 1.0), x1 = std::min(W - 1.0, std::ceil(hi[0] * W - 0.5) + 1.0);
        const double y0 = std::max(0.0, std::floor(lo[1] * H - 0.5) - 1.0), y1 = std::min(H - 1.0, std::ceil(hi[1] * H - 0.5) + 1.0);
        if (x1 >= x0 && y1 >= y0) cover += (uint64_t)(x1 - x0 + 1.0) * (uint64_t)(y1 - y0 + 1.0);
    }
    too_large = std::min(cover, all) * lm->directions >= (1ull << 31);
    return FW_OK;
}

// What every lightmap call makes first, once: the mesh on the device, k_lm_cover and k_lm_texels, the owner map back on the host and the
// covered list (one host pass over the 4 B / texel owner map: ascending, deterministic) on both sides.  Its Staged arrays live as long as
// the call's, and drain the stream before they are released.
struct LightmapTexels {
    Staged st;                                                                 // the mesh, the owner map, the records and the list
    float *records = nullptr; uint32_t *owner = nullptr, *list = nullptr;      // device: W H x 8 floats, W H, n_cov
    std::vector<uint32_t> h_owner, h_list;
    explicit LightmapTexels(int dev) : st(dev, nullptr, false) {}
};

int lightmap_texels_make(const fw_lightmap *lm, int device, hipStream_t stream, LightmapTexels &T) {
    const size_t n_tex = (size_t)lm->width * lm->height, nv = lm->n_verts;
    Staged &st = T.st;
    st.stream = stream;
    const int i_verts = st.add(Staged::IN, lm->verts, nv * 12), i_idx = st.add(Staged::IN, lm->indices, (size_t)lm->n_indices * 4),
              i_nrm = st.add(Staged::IN, lm->normals, nv * 12), i_uv = st.add(Staged::IN, lm->uvs, nv * 8),
              i_own = st.add(Staged::WORK, nullptr, n_tex * 4), i_rec = st.add(Staged::WORK, nullptr, n_tex * 32), i_list = st.add(Staged::WORK, nullptr, n_tex * 4);
    if (int rc = st.up()) return rc;
    T.owner = st.ptr<uint32_t>(i_own); T.records = st.ptr<float>(i_rec); T.list = st.ptr<uint32_t>(i_list);
    HIPCHK(hipMemsetAsync(T.owner, 0xff, n_tex * 4, stream));
    fw::DLightmapMesh m{};
    m.verts = st.ptr<const float>(i_verts); m.indices = st.ptr<const uint32_t>(i_idx);
    m.normals = st.ptr<const float>(i_nrm); m.uvs = st.ptr<const float>(i_uv);
    m.n_tris = lm->n_indices / 3u; m.width = lm->width; m.height = lm->height;
    rotor_rows(lm->rotation, m.rows);
    m.rotated = 0.5f * ((m.rows[0][0] + m.rows[1][1] + m.rows[2][2]) - 1.f) < 0.999f ? 1u : 0u;
    m.negate = ((lm->flip_normals != 0) != (lm->flip != 0)) ? 1u : 0u;
    m.position[0] = lm->position.x; m.position[1] = lm->position.y; m.position[2] = lm->position.z;
    const int n_cus = device_cus(device);
    fw::launch_lm_cover(stream, n_cus, m, T.owner);
    fw::launch_lm_texels(stream, n_cus, m, T.owner, (float4 *)T.records);
    T.h_owner.resize(n_tex);
    if (int rc = st.get(i_own, T.h_owner.data())) return rc;
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    T.h_list.clear();
    for (size_t i = 0; i < n_tex; i++) if (T.h_owner[i] != FW_NO_HIT) T.h_list.push_back((uint32_t)i);
    if (!T.h_list.empty()) HIPCHK(hipMemcpyAsync(T.list, T.h_list.data(), T.h_list.size() * 4, hipMemcpyHostToDevice, stream));
    return FW_OK;
}

fw::DLightmapRays lightmap_rays_device(const fw_lightmap *lm, uint32_t round, const LightmapTexels &T, uint32_t first) {
    fw::DLightmapRays d{};
    d.directions = lm->directions;
    d.seed32 = seed32_of(lm->seed);
    d.jitter = lm->jitter ? 1u : 0u;
    d.round = round; d.bias = lm->bias;
    d.texel_ids = T.list + first; d.records = (const float4 *)T.records;
    return d;
}

int lightmap_texels_impl(const fw_lightmap *lm, int device, float *records, uint32_t *owner, uint32_t *n_covered, int on_device, void *stream_) {
    if (!lm) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = lightmap_check(lm, too_large)) return rc;
    if (on_device && (((uintptr_t)records & 15u) || ((uintptr_t)owner & 3u))) return fail(FW_ERR_BAD_ARG, "device records must be 16-byte aligned, device owner 4-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "covered texels x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    LightmapTexels T(device);
    if (int rc = lightmap_texels_make(lm, device, stream, T)) return rc;
    const size_t n_tex = (size_t)lm->width * lm->height;
    if (records) HIPCHK(hipMemcpyAsync(records, T.records, n_tex * 32, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    if (owner) {
        if (on_device) HIPCHK(hipMemcpyAsync(owner, T.owner, n_tex * 4, hipMemcpyDeviceToDevice, stream));
        else std::memcpy(owner, T.h_owner.data(), n_tex * 4);
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    if (n_covered) *n_covered = (uint32_t)T.h_list.size();
    return FW_OK;
}

int lightmap_rays_impl(const fw_lightmap *lm, int device, uint32_t round, uint32_t first, uint32_t n, float *rays, int on_device, void *stream_) {
    if (!lm || !rays) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = lightmap_check(lm, too_large)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((uintptr_t)rays & 3u)) return fail(FW_ERR_BAD_ARG, "rays must be 4-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "covered texels x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    LightmapTexels T(device);
    if (int rc = lightmap_texels_make(lm, device, stream, T)) return rc;
    if ((uint64_t)first + n > T.h_list.size()) { (void)hipStreamSynchronize(stream); return fail(FW_ERR_BAD_ARG, "first + n exceeds the covered list (" + std::to_string(T.h_list.size()) + " texels)"); }
    const int n_cus = device_cus(device);
    if (on_device) {
        fw::launch_lm_rays(stream, n_cus, lightmap_rays_device(lm, round, T, first), n, rays);
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipGetLastError());
        return FW_OK;
    }
    return host_slabs(stream, device, n, (size_t)lm->directions * 24, rays, [&](uint32_t done, uint32_t k, float *d_rays) {
        fw::launch_lm_rays(stream, n_cus, lightmap_rays_device(lm, round, T, first + done), k, d_rays);
    });
}

int lightmap_reduce_impl(int device, uint32_t n, uint32_t directions, uint32_t samples, const uint32_t *texel_ids, const float *accum, float *sums,
                         uint32_t n_texels, int on_device, void *stream_) {
    if (!accum || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (n == 0 || n_texels == 0) return fail(FW_ERR_BAD_ARG, "n and n_texels must be > 0");
    if (directions == 0 || directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (samples == 0 || samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if (!texel_ids && n > n_texels) return fail(FW_ERR_BAD_ARG, "n exceeds n_texels");
    if (texel_ids && !on_device)
        for (uint32_t q = 0; q < n; q++)
            if (texel_ids[q] >= n_texels) return fail(FW_ERR_BAD_ARG, "texel id " + std::to_string(q) + " is not below n_texels");
    if (on_device && ((((uintptr_t)accum | (uintptr_t)sums) & 15u) || ((uintptr_t)texel_ids & 3u)))
        return fail(FW_ERR_BAD_ARG, "device accum and sums must be 16-byte aligned, device texel_ids 4-byte aligned");
    if ((uint64_t)n * directions >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Staged st(device, stream, on_device != 0);
    const int i_acc = st.add(Staged::IN, accum, (size_t)n * directions * 16), i_sums = st.add(Staged::INOUT, sums, (size_t)n_texels * 16),
              i_ids = st.add(Staged::IN, texel_ids, (size_t)n * 4);
    if (int rc = st.up()) return rc;
    fw::launch_lm_reduce(stream, device_cus(device), n, directions, samples, st.ptr<const uint32_t>(i_ids), st.ptr<const float>(i_acc), st.ptr<float>(i_sums));
    return st.finish();
}

// `passes` dilation passes of the image at d_img through the second buffer d_tmp; the result ends in d_img
int lightmap_dilate_device(hipStream_t stream, uint32_t width, uint32_t height, uint32_t passes, float *d_img, float *d_tmp) {
    float *src = d_img, *dst = d_tmp;
    for (uint32_t k = 0; k < passes; k++) { fw::launch_lm_dilate(stream, width, height, src, dst); std::swap(src, dst); }
    if (src != d_img) HIPCHK(hipMemcpyAsync(d_img, src, (size_t)width * height * 16, hipMemcpyDeviceToDevice, stream));
    return FW_OK;
}

int lightmap_dilate_impl(int device, uint32_t width, uint32_t height, uint32_t passes, float *image, int on_device, void *stream_) {
    if (!image) return fail(FW_ERR_BAD_ARG, "null argument");
    if (width == 0 || width > 16384u || height == 0 || height > 16384u) return fail(FW_ERR_BAD_ARG, "width and height must be in 1..16384");
    if (passes > 64u) return fail(FW_ERR_BAD_ARG, "passes must be in 0..64");
    if (on_device && ((uintptr_t)image & 15u)) return fail(FW_ERR_BAD_ARG, "a device image must be 16-byte aligned");
    if (int rc = use_device(device)) return rc;
    if (passes == 0) return FW_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bytes = (size_t)width * height * 16;
    Staged st(device, stream, on_device != 0);
    const int i_tmp = st.add(Staged::WORK, nullptr, bytes), i_img = st.add(Staged::INOUT, image, bytes);
    if (int rc = st.up()) return rc;
    if (int rc = lightmap_dilate_device(stream, width, height, passes, st.ptr<float>(i_img), st.ptr<float>(i_tmp))) return rc;
    return st.finish();
}

// fw_bake_lightmap: its own are the argument checks, the texels, the Staged arrays (a chunk's rays and accum, the running sums and the
// irradiance unless the caller's device memory holds them, the dilation's second image), k_lm_rays and k_lm_reduce over the covered list
// as bake_rounds' generator and reducer, and the irradiance: k_lm_resolve and the dilation.
int bake_lightmap_impl(fw_scene *sc, const fw_lightmap *lm, const fw_render_rays_params *rp, uint32_t first_round, uint32_t rounds, uint32_t dilate,
                       float *sums, float *irradiance, fw_stats *stats) {
    if (!sc || !lm || !rp) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = lightmap_check(lm, too_large)) return rc;
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (rp->samples == 0 || rp->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if (dilate > 64u) return fail(FW_ERR_BAD_ARG, "dilate must be in 0..64");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (rp->on_device && (((uintptr_t)sums | (uintptr_t)irradiance) & 15u)) return fail(FW_ERR_BAD_ARG, "device sums and irradiance must be 16-byte aligned");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "covered texels x directions must be below 2^31");
    if (int rc = need_device()) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)rp->stream;
    LightmapTexels T(dev);
    if (int rc = lightmap_texels_make(lm, dev, stream, T)) return rc;
    const uint32_t N = (uint32_t)T.h_list.size(), D = lm->directions, S = rp->samples;
    const size_t n_tex = (size_t)lm->width * lm->height, img_bytes = n_tex * 16;
    const uint32_t chunk = std::max<uint32_t>(1u, std::min<uint32_t>(N, lm->chunk_texels ? lm->chunk_texels
                                                                                         : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * 40))));
    Staged st(dev, stream, rp->on_device != 0);
    const int i_rays = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 24), i_acc = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 16),
              i_sums = st.add_sums(sums, img_bytes), i_irr = st.add(Staged::OUT, irradiance, img_bytes),
              i_tmp = st.add(Staged::WORK, nullptr, irradiance && dilate ? img_bytes : 0);
    if (int rc = st.up()) return rc;
    float *d_sums = st.ptr<float>(i_sums);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    const BakeRounds b{first_round, rounds, N, D, chunk, st.ptr<float>(i_rays), st.ptr<float>(i_acc), 36, 16, 28};       // (the generator's records and ids; the reduction's loads and its sums)
    if (int rc = bake_rounds(sc, rp, b, stats ? &total : nullptr,
            [&](uint32_t r, uint32_t q0, uint32_t k, float *rays) { fw::launch_lm_rays(stream, n_cus, lightmap_rays_device(lm, r, T, q0), k, rays); },
            [&](uint32_t q0, uint32_t k, const float *, const float *acc) { fw::launch_lm_reduce(stream, n_cus, k, D, S, T.list + q0, acc, d_sums); }))
        return rc;
    // the outputs: sums where the caller keeps them; irradiance = sums / rounds so far on covered texels, then the dilation
    if (int rc = st.download(i_sums)) return rc;
    if (irradiance) {
        float *d_irr = st.ptr<float>(i_irr);
        fw::launch_lm_resolve(stream, (uint32_t)n_tex, (double)((uint64_t)first_round + rounds), T.owner, d_sums, d_irr);
        if (int rc = lightmap_dilate_device(stream, lm->width, lm->height, dilate, d_irr, st.ptr<float>(i_tmp))) return rc;
    }
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- baked probes read back (include/firework_hip.h) -------------------------------------------------------------
// The grid's own argument checks (FW_ERR_BAD_ARG only) and what the kernels need of it.  too_large: nx ny nz >= 2^31, which the callers
// report as FW_ERR_UNSUPPORTED after their own argument checks.
int probe_grid_check(const fw_probe_grid *g, bool &too_large, fw::DProbeGrid &d) {
    for (int k = 0; k < 3; k++)
        if (g->counts[k] == 0) return fail(FW_ERR_BAD_ARG, "every count of a probe grid must be > 0");
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(g->lo[k]) || !std::isfinite(g->hi[k])) return fail(FW_ERR_BAD_ARG, "a probe grid's corners must be finite");
        if (g->counts[k] > 1 && g->hi[k] == g->lo[k]) return fail(FW_ERR_BAD_ARG, "a probe grid axis with more than one probe needs hi != lo");
        if (!std::isfinite(g->hi[k] - g->lo[k])) return fail(FW_ERR_BAD_ARG, "a probe grid's hi - lo must be finite");
    }
    if (g->flags & ~(uint32_t)FW_PROBE_WRAP) return fail(FW_ERR_BAD_ARG, "unknown probe grid flags");
    const uint64_t xy = (uint64_t)g->counts[0] * g->counts[1];
    too_large = xy >= (1ull << 31) || xy * g->counts[2] >= (1ull << 31);
    for (int k = 0; k < 3; k++) {
        d.lo[k] = g->lo[k];
        d.span[k] = g->hi[k] - g->lo[k];
        d.step[k] = g->counts[k] > 1 ? (g->hi[k] - g->lo[k]) / (double)(g->counts[k] - 1) : 0.0;
        d.mid[k] = 0.5 * (g->lo[k] + g->hi[k]);
        d.counts[k] = g->counts[k];
    }
    d.wrap = g->flags & FW_PROBE_WRAP;
    return FW_OK;
}

// ---- probe visibility (include/firework_hip.h) --------------------------------------------------------------------
// A depth description's own argument checks (FW_ERR_BAD_ARG only)
int probe_depth_check(const fw_probe_depth *pd) {
    if (pd->resolution != 4 && pd->resolution != 8 && pd->resolution != 16 && pd->resolution != 32)
        return fail(FW_ERR_BAD_ARG, "a probe depth map's resolution must be 4, 8, 16 or 32");
    if (pd->sharpness_log2 > 8) return fail(FW_ERR_BAD_ARG, "sharpness_log2 must be in 0..8");
    if (!std::isfinite(pd->max_distance) || !(pd->max_distance > 0.f)) return fail(FW_ERR_BAD_ARG, "max_distance must be finite and > 0");
    return FW_OK;
}
// What the probe lookups (fw_probe_irradiance and fw_probe_shade with their _vis and _placed forms, fw_probe_radiance_lookup and
// fw_probe_shade_glossy) take beside the grid, in one form: the tables, and which of the optional ones the entry point uses (DESIGN.md
// §9s, §9u, §9v).  vis / placed: their pointers must not be NULL; otherwise they are not looked at.
struct ProbeLookupArgs {
    const float *sh;
    const fw_probe_radiance *pr; const float *maps;
    const fw_probe_depth *pd; const float *moments; float normal_bias;
    const float *placement;
    bool vis, placed;
};
// what the checks make of them for the kernels
struct ProbeLookup { fw::DProbeGrid g{}; fw::DProbeRadiance d{}; bool too_large = false; size_t n_probes = 0; };
int probe_radiance_check(const fw_probe_radiance *pr, fw::DProbeRadiance &d);

// The lookups' shared checks, first part (FW_ERR_BAD_ARG only): the null pointers (own_null: the call's own), the shades' outputs, the
// radiance description, the visibility and the grid.  The call's own checks and its alignment check follow, then probe_lookup_sizes.
int probe_lookup_check(const fw_probe_grid *grid, const ProbeLookupArgs &a, bool own_null, bool no_output, ProbeLookup &L) {
    if (!grid || own_null || (a.vis && (!a.pd || !a.moments)) || (a.placed && !a.placement)) return fail(FW_ERR_BAD_ARG, "null argument");
    if (no_output) return fail(FW_ERR_BAD_ARG, "at least one output is needed");
    if (a.pr) if (int rc = probe_radiance_check(a.pr, L.d)) return rc;
    if (a.vis) {
        if (int rc = probe_depth_check(a.pd)) return rc;
        if (!std::isfinite(a.normal_bias) || a.normal_bias < 0.f) return fail(FW_ERR_BAD_ARG, "normal_bias must be finite and >= 0");
    }
    if (int rc = probe_grid_check(grid, L.too_large, L.g)) return rc;
    L.n_probes = (size_t)L.g.counts[0] * L.g.counts[1] * L.g.counts[2];
    return FW_OK;
}
// second part (FW_ERR_UNSUPPORTED only): the tables' sizes
int probe_lookup_sizes(const ProbeLookupArgs &a, const ProbeLookup &L) {
    if (L.too_large) return fail(FW_ERR_UNSUPPORTED, "nx x ny x nz must be below 2^31");
    if (a.vis && (uint64_t)L.n_probes * a.pd->resolution * a.pd->resolution >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x resolution^2 must be below 2^31");
    if (a.pr && (uint64_t)L.n_probes * L.d.texels >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x texels must be below 2^31");
    return FW_OK;
}
// the tables as Staged inputs, in the order a host call uploads them; one that is not in use takes no slot and is NULL
struct ProbeTables { int sh, maps, mom, pl; };
ProbeTables probe_tables_stage(Staged &st, const ProbeLookupArgs &a, const ProbeLookup &L) {
    const size_t R = a.vis ? a.pd->resolution : 0;
    return ProbeTables{st.add(Staged::IN, a.sh, L.n_probes * 108), st.add(Staged::IN, a.pr ? a.maps : nullptr, L.n_probes * L.d.texels * 16),
                       st.add(Staged::IN, a.vis ? a.moments : nullptr, L.n_probes * R * R * 8), st.add(Staged::IN, a.placed ? a.placement : nullptr, L.n_probes * 16)};
}
fw::DProbeVis probe_vis_device(const ProbeLookupArgs &a, const float *d_moments) {
    return fw::DProbeVis{d_moments, a.vis ? (double)a.normal_bias : 0.0, a.vis ? a.pd->resolution : 0u};
}

// fw_probe_irradiance and its _vis and _placed forms: with device arrays the kernel works on the caller's memory and nothing is allocated;
// with host arrays one device allocation per call holds the tables and a slab of points (24 B in, 12 B out each), released on every way out
int probe_irradiance_impl(const fw_probe_grid *grid, const ProbeLookupArgs &a, int device, uint32_t n, const float *positions, const float *normals,
                          uint32_t stride, float *irradiance, int on_device, void *stream_) {
    ProbeLookup L;
    if (int rc = probe_lookup_check(grid, a, !a.sh || !positions || !normals || !irradiance, false, L)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (device < 0) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (on_device && (((uintptr_t)a.sh | (uintptr_t)positions | (uintptr_t)normals | (uintptr_t)irradiance | (uintptr_t)(a.vis ? a.moments : nullptr) |
                       (uintptr_t)(a.placed ? a.placement : nullptr)) & 3u))
        return fail(FW_ERR_BAD_ARG, "device arrays must be 4-byte aligned");
    if (int rc = probe_lookup_sizes(a, L)) return rc;
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Staged st(device, stream, on_device != 0);
    const ProbeTables t = probe_tables_stage(st, a, L);
    HostSlabs sl(st, n, 36);
    const int a_pts = sl.in(positions, 24, stride, normals), a_out = sl.out(irradiance, 12);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) {
        const float *d_sh = st.ptr<const float>(t.sh), *pos = sl.ptr<const float>(a_pts), *nrm = sl.with(a_pts);
        float *out = sl.ptr<float>(a_out);
        const fw::DProbeVis v = probe_vis_device(a, st.ptr<const float>(t.mom));
        fw::launch_probe_irradiance(stream, L.g, a.vis ? &v : nullptr, d_sh, st.ptr<const float>(t.pl), k, pos, nrm, sl.stride(a_pts), out);
    });
}

// fw_probe_shade and its _vis and _placed forms: as fw_probe_irradiance; a host call's slab holds 48 B of record and up to 27 B of outputs
// per pixel
int probe_shade_impl(const fw_probe_grid *grid, const ProbeLookupArgs &a, const fw_probe_shade_params *p, const float *aov, float *linear_rgb,
                     float *gamma_rgb, uint8_t *rgb8) {
    ProbeLookup L;
    if (int rc = probe_lookup_check(grid, a, !a.sh || !p || !aov, !linear_rgb && !gamma_rgb && !rgb8, L)) return rc;
    if (p->width == 0 || p->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    if (!std::isfinite(p->gamma) || !(p->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be finite and > 0");
    if (p->device < 0) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (p->on_device && (((uintptr_t)aov & 15u) || (((uintptr_t)a.sh | (uintptr_t)linear_rgb | (uintptr_t)gamma_rgb) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device aov must be 16-byte aligned, device sh, linear_rgb and gamma_rgb 4-byte aligned");
    if (a.vis && p->on_device && ((uintptr_t)a.moments & 3u)) return fail(FW_ERR_BAD_ARG, "device moments must be 4-byte aligned");
    if (a.placed && p->on_device && ((uintptr_t)a.placement & 3u)) return fail(FW_ERR_BAD_ARG, "device placement must be 4-byte aligned");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (int rc = probe_lookup_sizes(a, L)) return rc;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    const int dev = p->device;
    if (int rc = use_device(dev)) return rc;
    hipStream_t stream = (hipStream_t)p->stream;
    Staged st(dev, stream, p->on_device != 0);
    const ProbeTables t = probe_tables_stage(st, a, L);
    HostSlabs sl(st, (uint32_t)full, 75);
    const int a_aov = sl.in(aov, 48), a_lin = sl.out(linear_rgb, 12), a_gam = sl.out(gamma_rgb, 12), a_8 = sl.out(rgb8, 3);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) {
        const float *d_sh = st.ptr<const float>(t.sh), *d_aov = sl.ptr<const float>(a_aov);
        uint8_t *o8 = sl.ptr<uint8_t>(a_8);
        float *og = sl.ptr<float>(a_gam), *ol = sl.ptr<float>(a_lin);
        const fw::DProbeVis v = probe_vis_device(a, st.ptr<const float>(t.mom));
        fw::launch_probe_shade(stream, L.g, a.vis ? &v : nullptr, d_sh, st.ptr<const float>(t.pl), k, d_aov, p->gamma, o8, og, ol);
    });
}

// fw_probe_depth_reduce: fw_probe_project's shape
int probe_depth_reduce_impl(int device, const fw_probe_depth *pd, uint32_t n_probes, uint32_t directions, const float *rays, const fw_hit *hits,
                            float *sums, int on_device, void *stream_) {
    if (!pd || !rays || !hits || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = probe_depth_check(pd)) return rc;
    if (n_probes == 0) return fail(FW_ERR_BAD_ARG, "n_probes must be > 0");
    if (directions == 0 || directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (on_device && ((((uintptr_t)sums | (uintptr_t)hits) & 15u) || ((uintptr_t)rays & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and hits must be 16-byte aligned, device rays 4-byte aligned");
    const uint32_t R = pd->resolution;
    if ((uint64_t)n_probes * directions >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if ((uint64_t)n_probes * R * R >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x resolution^2 must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)n_probes * directions;
    Staged st(device, stream, on_device != 0);
    const int i_rays = st.add(Staged::IN, rays, n * 24), i_hits = st.add(Staged::IN, hits, n * sizeof(fw_hit)),
              i_sums = st.add(Staged::INOUT, sums, (size_t)n_probes * R * R * 16);
    if (int rc = st.up()) return rc;
    fw::launch_probe_depth(stream, n_probes, directions, R, pd->sharpness_log2, pd->max_distance, st.ptr<const float>(i_rays), st.ptr<const fw_hit>(i_hits),
                           st.ptr<float>(i_sums));
    return st.finish();
}

// fw_bake_probe_depth: its own are the argument checks, the Staged arrays (positions, a chunk's rays and hits, the running sums unless the
// caller's device memory holds them), k_probe_rays and k_probe_depth as trace_rounds' generator and reducer, and the moments, divided on
// the host.
int bake_probe_depth_impl(fw_scene *sc, const fw_probe_set *s, const fw_probe_depth *pd, const fw_trace_params *tp, uint32_t first_round,
                          uint32_t rounds, float *sums, float *moments, fw_stats *stats) {
    if (!sc || !s || !pd || !tp) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = probe_set_check(s, too_large)) return rc;
    if (int rc = probe_depth_check(pd)) return rc;
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (tp->on_device && (((uintptr_t)sums & 15u) || ((uintptr_t)moments & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums must be 16-byte aligned, device moments 4-byte aligned");
    const uint32_t N = s->n_probes, D = s->directions, R = pd->resolution;
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if ((uint64_t)N * R * R >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x resolution^2 must be below 2^31");
    if (int rc = need_device()) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)tp->stream;
    const uint32_t chunk = std::min<uint32_t>(N, s->chunk_probes ? s->chunk_probes : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * 72)));
    const size_t n_tex = (size_t)N * R * R;
    Staged st(dev, stream, tp->on_device != 0);
    const int i_pos = st.add(Staged::IN, s->positions, (size_t)N * 12, true), i_rays = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 24),
              i_hits = st.add(Staged::WORK, nullptr, (size_t)chunk * D * sizeof(fw_hit)), i_sums = st.add_sums(sums, n_tex * 16);
    if (int rc = st.up()) return rc;
    const float *d_pos = st.ptr<const float>(i_pos);
    float *d_sums = st.ptr<float>(i_sums);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    const TraceRounds b{N, D, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
    if (int rc = trace_rounds(sc, tp, b, first_round, rounds, stats ? &total : nullptr,
            [&](uint32_t r, uint32_t p0, uint32_t k, float *rays) { fw::launch_probe_rays(stream, n_cus, probes_device(s, r, p0, d_pos + (size_t)p0 * 3), k, rays); },
            [&](uint32_t p0, uint32_t k, const float *rays, const fw_hit *hits) {
                fw::launch_probe_depth(stream, k, D, R, pd->sharpness_log2, pd->max_distance, rays, hits, d_sums + (size_t)p0 * R * R * 4);
            }))
        return rc;
    // the outputs: sums where the caller keeps them, and the moments, divided on the host in double and rounded once
    std::vector<float> keep;
    const float *h_sums = nullptr;
    if (int rc = st.fetch(i_sums, moments != nullptr, keep, h_sums)) return rc;
    if (int rc = st.finish()) return rc;
    if (moments) {
        const float far1 = pd->max_distance, far2 = (float)((double)pd->max_distance * (double)pd->max_distance);
        if (int rc = host_output(stream, moments, n_tex * 2, tp->on_device != 0, [&](float *out) {
                for (size_t i = 0; i < n_tex; i++) {
                    const float *t = h_sums + i * 4;
                    const bool none = t[2] == 0.f;
                    out[2 * i] = none ? far1 : (float)((double)t[0] / (double)t[2]);
                    out[2 * i + 1] = none ? far2 : (float)((double)t[1] / (double)t[2]);
                }
            }))
            return rc;
    }
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- probe relocation and classification (include/firework_hip.h) -------------------------------------------------
// A relocation's own argument checks (FW_ERR_BAD_ARG only) and what the step kernel needs of it
int probe_relocate_check(const fw_probe_relocate *rl, fw::DRelocate &d) {
    if (!std::isfinite(rl->min_front) || !(rl->min_front > 0.f)) return fail(FW_ERR_BAD_ARG, "min_front must be finite and > 0");
    if (!(rl->back_fraction >= 0.f && rl->back_fraction <= 1.f)) return fail(FW_ERR_BAD_ARG, "back_fraction must be in [0, 1]");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(rl->max_offset[k]) || rl->max_offset[k] < 0.f) return fail(FW_ERR_BAD_ARG, "every max_offset must be finite and >= 0");
    d.min_front = (double)rl->min_front;
    d.back_fraction = (double)rl->back_fraction;
    for (int k = 0; k < 3; k++) d.max_offset[k] = (double)rl->max_offset[k];
    return FW_OK;
}

// fw_probe_survey: fw_probe_depth_reduce's shape; the survey is overwritten, so a host caller's is not uploaded
int probe_survey_impl(int device, uint32_t n_probes, uint32_t directions, const float *rays, const fw_hit *hits, float *survey, int on_device,
                      void *stream_) {
    if (!rays || !hits || !survey) return fail(FW_ERR_BAD_ARG, "null argument");
    if (n_probes == 0) return fail(FW_ERR_BAD_ARG, "n_probes must be > 0");
    if (directions == 0 || directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (on_device && ((((uintptr_t)survey | (uintptr_t)hits) & 15u) || ((uintptr_t)rays & 3u)))
        return fail(FW_ERR_BAD_ARG, "device survey and hits must be 16-byte aligned, device rays 4-byte aligned");
    if ((uint64_t)n_probes * directions >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)n_probes * directions;
    Staged st(device, stream, on_device != 0);
    const int i_rays = st.add(Staged::IN, rays, n * 24), i_hits = st.add(Staged::IN, hits, n * sizeof(fw_hit)),
              i_survey = st.add(Staged::OUT, survey, (size_t)n_probes * 48);
    if (int rc = st.up()) return rc;
    fw::launch_probe_survey(stream, device_cus(device), n_probes, directions, st.ptr<const float>(i_rays), st.ptr<const fw_hit>(i_hits), st.ptr<float>(i_survey));
    return st.finish();
}

// fw_probe_relocate_step: the same shape over the survey (read) and the placement (read and written)
int probe_relocate_step_impl(int device, const fw_probe_relocate *rl, uint32_t n_probes, uint32_t directions, const float *survey, float *placement,
                             int move, int on_device, void *stream_) {
    if (!rl || !survey || !placement) return fail(FW_ERR_BAD_ARG, "null argument");
    fw::DRelocate L{};
    if (int rc = probe_relocate_check(rl, L)) return rc;
    if (n_probes == 0) return fail(FW_ERR_BAD_ARG, "n_probes must be > 0");
    if (directions == 0 || directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (on_device && (((uintptr_t)survey | (uintptr_t)placement) & 15u)) return fail(FW_ERR_BAD_ARG, "device survey and placement must be 16-byte aligned");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Staged st(device, stream, on_device != 0);
    const int i_survey = st.add(Staged::IN, survey, (size_t)n_probes * 48), i_place = st.add(Staged::INOUT, placement, (size_t)n_probes * 16);
    if (int rc = st.up()) return rc;
    fw::launch_probe_relocate_step(stream, L, n_probes, directions, st.ptr<const float>(i_survey), st.ptr<float>(i_place), move ? 1 : 0);
    return st.finish();
}

// fw_relocate_probes: per step one round of the traced bakes' chunks (trace_round) with the survey and the step as the
// reduction.  Its own are the argument checks, the Staged arrays (the moved positions, a chunk's rays and hits, the survey and the
// placement), and the moved positions, formed on the host before every step from the placement the step before it copied back.
int relocate_probes_impl(fw_scene *sc, const fw_probe_set *s, const fw_probe_relocate *rl, const fw_trace_params *tp, uint32_t first_step,
                         uint32_t steps, float *placement, float *survey, fw_stats *stats) {
    if (!sc || !s || !rl || !tp || !placement) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = probe_set_check(s, too_large)) return rc;
    fw::DRelocate L{};
    if (int rc = probe_relocate_check(rl, L)) return rc;
    const uint32_t N = s->n_probes, D = s->directions;
    for (uint64_t i = 0; i < (uint64_t)N; i++) {
        const float *r = placement + i * 4;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]) || !(r[3] == 0.f || r[3] == 1.f))
            return fail(FW_ERR_BAD_ARG, "placement " + std::to_string(i) + " must have a finite offset and a state of 0 or 1");
    }
    if ((uint64_t)first_step + steps + 1 > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_step + steps + 1 overflows");
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if (int rc = need_device()) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)tp->stream;
    const uint32_t chunk = std::min<uint32_t>(N, s->chunk_probes ? s->chunk_probes : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * 72)));
    Staged st(dev, stream, false);                        // (the placement and the survey are host arrays whatever tp->on_device says)
    const int i_pos = st.add(Staged::WORK, nullptr, (size_t)N * 12), i_rays = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 24),
              i_hits = st.add(Staged::WORK, nullptr, (size_t)chunk * D * sizeof(fw_hit)), i_survey = st.add(Staged::WORK, nullptr, (size_t)N * 48),
              i_place = st.add(Staged::IN, placement, (size_t)N * 16);
    if (int rc = st.up()) return rc;
    const float *d_pos = st.ptr<const float>(i_pos);
    float *d_survey = st.ptr<float>(i_survey), *d_place = st.ptr<float>(i_place);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    const TraceRounds b{N, D, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
    BakeChunks c{stream, N, chunk, (tp->flags & FW_FLAG_TIME_KERNELS) != 0, stats ? &total : nullptr};
    if (int rc = c.begin()) return rc;
    std::vector<float> moved((size_t)N * 3);
    for (uint32_t i = 0; i <= steps; i++) {               // the last one classifies: move = 0
        const int move = i < steps ? 1 : 0;
        for (size_t q = 0; q < (size_t)N; q++)
            for (int k = 0; k < 3; k++) moved[q * 3 + k] = (float)((double)s->positions[q * 3 + k] + (double)placement[q * 4 + k]);
        if (int rc = st.put(i_pos, moved.data())) return rc;
        if (int rc = trace_round(sc, tp, b, c, first_step + i,
                [&](uint32_t r, uint32_t p0, uint32_t k, float *rays) { fw::launch_probe_rays(stream, n_cus, probes_device(s, r, p0, d_pos + (size_t)p0 * 3), k, rays); },
                [&](uint32_t p0, uint32_t k, const float *rays, const fw_hit *hits) {
                    fw::launch_probe_survey(stream, n_cus, k, D, rays, hits, d_survey + (size_t)p0 * 12);
                    fw::launch_probe_relocate_step(stream, L, k, D, d_survey + (size_t)p0 * 12, d_place + (size_t)p0 * 4, move);
                }))
            return rc;
        // the placement comes back after every step: the next one's positions are formed from it
        if (int rc = st.get(i_place, placement)) return rc;
        HIPCHK(hipStreamSynchronize(stream));
    }
    if (survey) if (int rc = st.get(i_survey, survey)) return rc;
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- ambient occlusion (include/firework_hip.h) -------------------------------------------------------------------
// An AO description's own argument checks (FW_ERR_BAD_ARG only)
int ao_check(const fw_ao *ao) {
    if (ao->directions == 0 || ao->directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (ao->falloff > 1u) return fail(FW_ERR_BAD_ARG, "falloff must be 0 or 1");
    if (!(ao->radius > 0.f)) return fail(FW_ERR_BAD_ARG, "radius must be > 0");
    if (std::isinf(ao->radius) && ao->falloff) return fail(FW_ERR_BAD_ARG, "an infinite radius needs falloff 0");
    if (!std::isfinite(ao->bias) || ao->bias < 0.f) return fail(FW_ERR_BAD_ARG, "bias must be finite and >= 0");
    return FW_OK;
}

// how many entries an array indexed by id spans: max(ids) + 1, or n without ids (host ids)
inline uint64_t ao_extent(uint32_t n, const uint32_t *ids) {
    if (!ids) return n;
    uint32_t top = 0;
    for (uint32_t q = 0; q < n; q++) top = std::max(top, ids[q]);
    return (uint64_t)top + 1u;
}

// Surface points as Staged inputs: a host caller's positions and normals over `extent` ids and its ids go to the device, a device caller's
// are read where they lie
struct AoSlots { int pos, nrm, ids; };
AoSlots ao_points_stage(Staged &st, uint32_t n, const float *positions, const float *normals, uint32_t stride, const uint32_t *ids, uint64_t extent) {
    const size_t arr = (size_t)((extent - 1u) * stride + 3u) * 4u;
    return AoSlots{st.add(Staged::IN, positions, arr), st.add(Staged::IN, normals, arr), st.add(Staged::IN, ids, (size_t)n * 4u)};
}
fw::DAoPoints ao_points_device(const Staged &st, const AoSlots &a, uint32_t stride) {
    return fw::DAoPoints{st.ptr<const float>(a.pos), st.ptr<const float>(a.nrm), st.ptr<const uint32_t>(a.ids), stride};
}

fw::DAoRays ao_rays_device(const fw_ao *ao, uint32_t round, const fw::DAoPoints &pts, uint32_t first) {
    fw::DAoRays d{};
    d.pts = pts; d.first = first;
    d.directions = ao->directions;
    d.seed32 = seed32_of(ao->seed);
    d.jitter = ao->jitter ? 1u : 0u;
    d.round = round; d.bias = ao->bias;
    return d;
}

// fw_ao_rays: fw_lightmap_rays' shape — with device arrays the kernel works on the caller's memory; with host arrays the points are
// staged once and the rays come back in slabs
int ao_rays_impl(const fw_ao *ao, int device, uint32_t round, uint32_t n, const float *positions, const float *normals, uint32_t stride,
                 const uint32_t *ids, float *rays, int on_device, void *stream_) {
    if (!ao || !positions || !normals || !rays) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = ao_check(ao)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (on_device && (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)rays) & 3u))
        return fail(FW_ERR_BAD_ARG, "device arrays must be 4-byte aligned");
    if ((uint64_t)n * ao->directions >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    Staged st(device, stream, on_device != 0);
    const AoSlots slots = ao_points_stage(st, n, positions, normals, stride, ids, on_device ? n : ao_extent(n, ids));
    if (int rc = st.up()) return rc;
    const fw::DAoPoints pts = ao_points_device(st, slots, stride);
    if (on_device) {
        fw::launch_ao_rays(stream, n_cus, ao_rays_device(ao, round, pts, 0), n, rays);
        return st.finish();
    }
    return host_slabs(stream, device, n, (size_t)ao->directions * 24, rays, [&](uint32_t done, uint32_t k, float *d_rays) {
        fw::launch_ao_rays(stream, n_cus, ao_rays_device(ao, round, pts, done), k, d_rays);
    });
}

// fw_ao_reduce: fw_probe_depth_reduce's shape
int ao_reduce_impl(int device, const fw_ao *ao, uint32_t n, const uint32_t *ids, const float *rays, const fw_hit *hits, float *sums, int on_device,
                   void *stream_) {
    if (!ao || !rays || !hits || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = ao_check(ao)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((((uintptr_t)sums | (uintptr_t)hits) & 15u) || (((uintptr_t)rays | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and hits must be 16-byte aligned, device rays and ids 4-byte aligned");
    const uint32_t D = ao->directions;
    if ((uint64_t)n * D >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t entries = (size_t)n * D;
    Staged st(device, stream, on_device != 0);
    const int i_rays = st.add(Staged::IN, rays, entries * 24), i_hits = st.add(Staged::IN, hits, entries * sizeof(fw_hit)),
              i_sums = st.add(Staged::INOUT, sums, on_device ? 0 : (size_t)ao_extent(n, ids) * 16), i_ids = st.add(Staged::IN, ids, (size_t)n * 4);
    if (int rc = st.up()) return rc;
    fw::launch_ao_reduce(stream, device_cus(device), 0, n, D, ao->falloff, ao->radius, st.ptr<const uint32_t>(i_ids), st.ptr<const float>(i_rays),
                         st.ptr<const fw_hit>(i_hits), st.ptr<float>(i_sums));
    return st.finish();
}

// fw_bake_ao: its own are the argument checks, the Staged arrays (a host caller's points, a chunk's rays and hits, the running sums and
// the output unless the caller's device memory holds them), k_ao_rays and k_ao_reduce as trace_rounds' generator and reducer, and
// k_ao_resolve.
int bake_ao_impl(fw_scene *sc, const fw_ao *ao, const fw_trace_params *tp, uint32_t N, const float *positions, const float *normals, uint32_t stride,
                 const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    if (!sc || !ao || !tp || !positions || !normals) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = ao_check(ao)) return rc;
    if (N == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (tp->on_device && ((((uintptr_t)sums | (uintptr_t)out) & 15u) || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and out must be 16-byte aligned, device positions, normals and ids 4-byte aligned");
    const uint32_t D = ao->directions;
    if ((uint64_t)N * D >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = need_device()) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)tp->stream;
    const bool on_device = tp->on_device != 0;
    const uint32_t chunk = std::min<uint32_t>(N, ao->chunk_points ? ao->chunk_points : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * 72)));
    // how many records sums and out span: only scratch copies of them need it (a host caller's, or the sums nobody keeps)
    uint64_t extent = N;
    if (ids && (!on_device || !sums)) {
        if (on_device) {
            std::vector<uint32_t> h_ids(N);
            HIPCHK(hipMemcpyAsync(h_ids.data(), ids, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            extent = ao_extent(N, h_ids.data());
        } else extent = ao_extent(N, ids);
    }
    const size_t rec_bytes = (size_t)extent * 16;
    Staged st(dev, stream, on_device);
    const AoSlots slots = ao_points_stage(st, N, positions, normals, stride, ids, extent);
    const int i_rays = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 24), i_hits = st.add(Staged::WORK, nullptr, (size_t)chunk * D * sizeof(fw_hit)),
              i_sums = st.add_sums(sums, rec_bytes), i_out = st.add(ids ? Staged::INOUT : Staged::OUT, out, rec_bytes);      // (with ids, entries outside the list stay)
    if (int rc = st.up()) return rc;
    const fw::DAoPoints pts = ao_points_device(st, slots, stride);
    float *d_sums = st.ptr<float>(i_sums);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    const TraceRounds b{N, D, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
    if (int rc = trace_rounds(sc, tp, b, first_round, rounds, stats ? &total : nullptr,
            [&](uint32_t r, uint32_t q0, uint32_t k, float *rays) { fw::launch_ao_rays(stream, n_cus, ao_rays_device(ao, r, pts, q0), k, rays); },
            [&](uint32_t q0, uint32_t k, const float *rays, const fw_hit *hits) {
                fw::launch_ao_reduce(stream, n_cus, q0, k, D, ao->falloff, ao->radius, pts.ids, rays, hits, d_sums);
            }))
        return rc;
    if (int rc = st.download(i_sums)) return rc;
    if (out) fw::launch_ao_resolve(stream, N, (double)((uint64_t)first_round + rounds), pts.ids, d_sums, st.ptr<float>(i_out));
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- direct light of point, spot and directional lights at surface points (include/firework_hip.h) --------------------
// A description's own argument checks (FW_ERR_BAD_ARG only)
int direct_check(const fw_direct *dp) {
    if (dp->lobe > 1u) return fail(FW_ERR_BAD_ARG, "lobe must be 0 or 1");
    if (dp->face_view > 1u) return fail(FW_ERR_BAD_ARG, "face_view must be 0 or 1");
    if (!std::isfinite(dp->bias) || dp->bias < 0.f) return fail(FW_ERR_BAD_ARG, "bias must be finite and >= 0");
    return FW_OK;
}
// the checks of the points that the three calls share, after the description's and before the alignment's
int direct_points_check(uint32_t n, uint32_t stride, const float *view, uint32_t view_stride, const float *spec) {
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (view && view_stride < 3) return fail(FW_ERR_BAD_ARG, "view_stride_floats must be >= 3");
    if (spec && !view) return fail(FW_ERR_BAD_ARG, "spec needs view: a glossy point is lit towards the eye");
    return FW_OK;
}

// Surface points with their optional view directions and spec records as Staged inputs (ao_points_stage's rule)
struct DirectSlots { AoSlots pts; int view, spec; };
DirectSlots direct_points_stage(Staged &st, uint32_t n, const float *positions, const float *normals, uint32_t stride, const uint32_t *ids,
                                const float *view, uint32_t view_stride, const float *spec, uint64_t extent) {
    DirectSlots s;
    s.pts = ao_points_stage(st, n, positions, normals, stride, ids, extent);
    s.view = st.add(Staged::IN, view, (size_t)((extent - 1u) * view_stride + 3u) * 4u);
    s.spec = st.add(Staged::IN, spec, (size_t)extent * 16u);
    return s;
}
fw::DDirect direct_device(const Staged &st, const DirectSlots &s, uint32_t stride, uint32_t view_stride, const fw_direct *dp, const float4 *lights,
                          uint32_t n_lights, uint32_t first) {
    fw::DDirect d{};
    d.pts = fw::DDirectPoints{st.ptr<const float>(s.pts.pos), st.ptr<const float>(s.pts.nrm), st.ptr<const uint32_t>(s.pts.ids),
                              st.ptr<const float>(s.view), st.ptr<const float4>(s.spec), stride, view_stride};
    d.lights = lights; d.n_lights = n_lights; d.first = first;
    d.lobe = dp->lobe; d.face_view = dp->face_view; d.bias = dp->bias;
    return d;
}

// fw_direct_rays: fw_ao_rays' shape, plus the light records built on the host (fw_scene_set_lights' own) and staged with the points
int direct_rays_impl(const fw_direct *dp, const fw_light *lights, uint32_t n_lights, int device, uint32_t n, const float *positions, const float *normals,
                     uint32_t stride, const uint32_t *ids, const float *view, uint32_t view_stride, const float *spec, float *rays, int on_device,
                     void *stream_) {
    if (!dp || !lights || !positions || !normals || !rays) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = direct_check(dp)) return rc;
    if (n_lights == 0) return fail(FW_ERR_BAD_ARG, "n_lights must be > 0");
    if (int rc = check_lights_impl(lights, n_lights)) return rc;
    if (int rc = direct_points_check(n, stride, view, view_stride, spec)) return rc;
    if (on_device && (((uintptr_t)spec & 15u) || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)view | (uintptr_t)rays) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device spec must be 16-byte aligned, device positions, normals, ids, view and rays 4-byte aligned");
    if ((uint64_t)n * n_lights >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x n_lights must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    const std::vector<float> rec = light_records(lights, n_lights);
    Staged st(device, stream, on_device != 0);
    const DirectSlots slots = direct_points_stage(st, n, positions, normals, stride, ids, view, view_stride, spec, on_device ? n : ao_extent(n, ids));
    const int i_rec = st.add(Staged::IN, rec.data(), rec.size() * 4, true);
    if (int rc = st.up()) return rc;
    const float4 *d_rec = st.ptr<const float4>(i_rec);
    if (on_device) {
        fw::launch_direct_rays(stream, n_cus, direct_device(st, slots, stride, view_stride, dp, d_rec, n_lights, 0), n, rays);
        return st.finish();
    }
    return host_slabs(stream, device, n, (size_t)n_lights * 24, rays, [&](uint32_t done, uint32_t k, float *d_rays) {
        fw::launch_direct_rays(stream, n_cus, direct_device(st, slots, stride, view_stride, dp, d_rec, n_lights, done), k, d_rays);
    });
}

// fw_direct_reduce: fw_ao_reduce's shape with the points and the light records it reads again
int direct_reduce_impl(int device, const fw_direct *dp, const fw_light *lights, uint32_t n_lights, uint32_t n, const float *positions, const float *normals,
                       uint32_t stride, const uint32_t *ids, const float *view, uint32_t view_stride, const float *spec, const float *rays,
                       const fw_hit *hits, float *sums, int on_device, void *stream_) {
    if (!dp || !lights || !positions || !normals || !rays || !hits || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = direct_check(dp)) return rc;
    if (n_lights == 0) return fail(FW_ERR_BAD_ARG, "n_lights must be > 0");
    if (int rc = check_lights_impl(lights, n_lights)) return rc;
    if (int rc = direct_points_check(n, stride, view, view_stride, spec)) return rc;
    if (on_device && ((((uintptr_t)sums | (uintptr_t)hits | (uintptr_t)spec) & 15u)
                      || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)view | (uintptr_t)rays) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums, hits and spec must be 16-byte aligned, device positions, normals, ids, view and rays 4-byte aligned");
    if ((uint64_t)n * n_lights >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x n_lights must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t entries = (size_t)n * n_lights;
    const std::vector<float> rec = light_records(lights, n_lights);
    const uint64_t extent = on_device ? n : ao_extent(n, ids);
    Staged st(device, stream, on_device != 0);
    const DirectSlots slots = direct_points_stage(st, n, positions, normals, stride, ids, view, view_stride, spec, extent);
    const int i_rec = st.add(Staged::IN, rec.data(), rec.size() * 4, true), i_rays = st.add(Staged::IN, rays, entries * 24),
              i_hits = st.add(Staged::IN, hits, entries * sizeof(fw_hit)), i_sums = st.add(Staged::INOUT, sums, on_device ? 0 : (size_t)extent * 32);
    if (int rc = st.up()) return rc;
    fw::launch_direct_reduce(stream, device_cus(device), direct_device(st, slots, stride, view_stride, dp, st.ptr<const float4>(i_rec), n_lights, 0), n,
                             st.ptr<const float>(i_rays), st.ptr<const fw_hit>(i_hits), st.ptr<float>(i_sums));
    return st.finish();
}

// fw_bake_direct: fw_bake_ao's shape — its own are the argument checks, the Staged arrays, k_direct_rays and k_direct_reduce as
// trace_rounds' generator and reducer over the scene's own light records where they lie, and k_direct_resolve.  The scene is looked at
// only after a device was found: Ln is the scene's, and a scene exists only where a device does.
int bake_direct_impl(fw_scene *sc, const fw_direct *dp, const fw_trace_params *tp, uint32_t N, const float *positions, const float *normals,
                     uint32_t stride, const uint32_t *ids, const float *view, uint32_t view_stride, const float *spec, uint32_t first_round,
                     uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    if (!sc || !dp || !tp || !positions || !normals) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = direct_check(dp)) return rc;
    if (int rc = direct_points_check(N, stride, view, view_stride, spec)) return rc;
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (tp->on_device && ((((uintptr_t)sums | (uintptr_t)out | (uintptr_t)spec) & 15u)
                          || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)view) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums, out and spec must be 16-byte aligned, device positions, normals, ids and view 4-byte aligned");
    if (int rc = need_device()) return rc;
    const uint32_t Ln = sc->n_dlights;
    if ((uint64_t)N * Ln >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x the scene's lights must be below 2^31");
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)tp->stream;
    const bool on_device = tp->on_device != 0;
    const uint32_t chunk = std::min<uint32_t>(N, dp->chunk_points ? dp->chunk_points
                                                                  : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)std::max(Ln, 1u) * 72)));
    // how many records sums and out span: only scratch copies of them need it (a host caller's, or the sums nobody keeps)
    uint64_t extent = N;
    if (ids && (!on_device || !sums)) {
        if (on_device) {
            std::vector<uint32_t> h_ids(N);
            HIPCHK(hipMemcpyAsync(h_ids.data(), ids, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            extent = ao_extent(N, h_ids.data());
        } else extent = ao_extent(N, ids);
    }
    const size_t rec_bytes = (size_t)extent * 32;
    Staged st(dev, stream, on_device);
    const DirectSlots slots = direct_points_stage(st, N, positions, normals, stride, ids, view, view_stride, spec, extent);
    const int i_rays = st.add(Staged::WORK, nullptr, (size_t)chunk * Ln * 24), i_hits = st.add(Staged::WORK, nullptr, (size_t)chunk * Ln * sizeof(fw_hit)),
              i_sums = st.add_sums(sums, rec_bytes), i_out = st.add(ids ? Staged::INOUT : Staged::OUT, out, rec_bytes);      // (with ids, entries outside the list stay)
    if (int rc = st.up()) return rc;
    float *d_sums = st.ptr<float>(i_sums);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    const uint32_t *d_ids = st.ptr<const uint32_t>(slots.pts.ids);
    if (Ln > 0) {
        {   // the light records arrive on the upload stream: the first kernel here reads them before any trace has waited for them
            Workspace *ws = workspace_for(dev);
            if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
            std::lock_guard<std::mutex> ws_guard(ws->mu);
            if (ws->ev_upload) HIPCHK(hipStreamWaitEvent(stream, ws->ev_upload, 0));
        }
        const float4 *d_rec = (const float4 *)sc->dlights.p;
        const TraceRounds b{N, Ln, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
        if (int rc = trace_rounds(sc, tp, b, first_round, rounds, stats ? &total : nullptr,
                [&](uint32_t, uint32_t q0, uint32_t k, float *rays) {
                    fw::launch_direct_rays(stream, n_cus, direct_device(st, slots, stride, view_stride, dp, d_rec, Ln, q0), k, rays);
                },
                [&](uint32_t q0, uint32_t k, const float *rays, const fw_hit *hits) {
                    fw::launch_direct_reduce(stream, n_cus, direct_device(st, slots, stride, view_stride, dp, d_rec, Ln, q0), k, rays, hits, d_sums);
                }))
            return rc;
    }
    if (int rc = st.download(i_sums)) return rc;
    if (out) fw::launch_direct_resolve(stream, N, (double)((uint64_t)first_round + rounds), d_ids, d_sums, st.ptr<float>(i_out));
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- final gather (include/firework_hip.h) -------------------------------------------------------------------------
// the stream waits for the scene's upload, as a trace's does
int wait_scene_upload(int dev, hipStream_t stream) {
    Workspace *ws = workspace_for(dev);
    if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
    std::lock_guard<std::mutex> ws_guard(ws->mu);
    if (ws->ev_upload) HIPCHK(hipStreamWaitEvent(stream, ws->ev_upload, 0));
    return FW_OK;
}

// fw_hit_surface: fw_trace_rays' argument pattern; with device arrays the kernel works on the caller's memory, with host arrays the rays,
// hits and records pass through slabs of one device allocation (136 B per ray)
int hit_surface_impl(fw_scene *sc, const float *rays, const fw_hit *hits, uint32_t n, float *surface, int on_device, void *stream_) {
    if (!sc) return fail(FW_ERR_BAD_ARG, "null argument");
    if (n == 0) return FW_OK;
    if (!rays || !hits || !surface) return fail(FW_ERR_BAD_ARG, "null rays, hits or surface");
    if (((uintptr_t)rays & 3u) || (on_device && (((uintptr_t)hits | (uintptr_t)surface) & 15u)))
        return fail(FW_ERR_BAD_ARG, "rays must be 4-byte aligned, device hits and surface 16-byte aligned");
    if (int rc = need_device()) return rc;
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = wait_scene_upload(dev, stream)) return rc;
    Staged st(dev, stream, on_device != 0);
    HostSlabs sl(st, n, 24 + sizeof(fw_hit) + 64);
    const int a_rays = sl.in(rays, 24), a_hits = sl.in(hits, sizeof(fw_hit)), a_out = sl.out(surface, 64);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) {
        fw::launch_hit_surface(stream, sc->n_cus, sc->d, sc->n_mat, sl.ptr<const float>(a_rays), sl.ptr<const float4>(a_hits), k, sl.ptr<float4>(a_out));
    });
}

// fw_gather_reduce: fw_ao_reduce's shape
int gather_reduce_impl(int device, uint32_t D, uint32_t n, const uint32_t *ids, const float *surface, const float *irradiance, const float *direct,
                       float *sums, int on_device, void *stream_) {
    if (!surface || !irradiance || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (D == 0 || D > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((((uintptr_t)sums | (uintptr_t)surface) & 15u) || (((uintptr_t)irradiance | (uintptr_t)direct | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and surface must be 16-byte aligned, device irradiance, direct and ids 4-byte aligned");
    if ((uint64_t)n * D >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t entries = (size_t)n * D;
    Staged st(device, stream, on_device != 0);
    const int i_surf = st.add(Staged::IN, surface, entries * 64), i_irr = st.add(Staged::IN, irradiance, entries * 12),
              i_dir = st.add(Staged::IN, direct, entries * 32), i_sums = st.add(Staged::INOUT, sums, on_device ? 0 : (size_t)ao_extent(n, ids) * 16),
              i_ids = st.add(Staged::IN, ids, (size_t)n * 4);
    if (int rc = st.up()) return rc;
    fw::launch_gather_reduce(stream, device_cus(device), 0, n, D, st.ptr<const uint32_t>(i_ids), st.ptr<const float>(i_surf), st.ptr<const float>(i_irr),
                             st.ptr<const float>(i_dir), st.ptr<float>(i_sums));
    return st.finish();
}

// A gather description's own argument checks (FW_ERR_BAD_ARG only); the flags are checked after the probe tables
int gather_check(const fw_gather *g) {
    if (g->directions == 0 || g->directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (!std::isfinite(g->bias) || g->bias < 0.f) return fail(FW_ERR_BAD_ARG, "bias must be finite and >= 0");
    if (!std::isfinite(g->direct_bias) || g->direct_bias < 0.f) return fail(FW_ERR_BAD_ARG, "direct_bias must be finite and >= 0");
    return FW_OK;
}

// how many records a point call's sums and out span: only scratch copies of them need it (a host caller's, or the sums nobody keeps)
int points_extent(hipStream_t stream, uint32_t N, const uint32_t *ids, bool on_device, const float *sums, uint64_t &extent) {
    extent = N;
    if (!ids || (on_device && sums)) return FW_OK;
    if (on_device) {
        std::vector<uint32_t> h_ids(N);
        HIPCHK(hipMemcpyAsync(h_ids.data(), ids, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        extent = ao_extent(N, h_ids.data());
    } else extent = ao_extent(N, ids);
    return FW_OK;
}

// What fw_bake_gather and fw_bake_reflect do with a chunk's rays and hits before their own reduction (fw_bake_gather's steps 3 to 5):
// k_hit_surface, the probe lookup at the records read in place and, on a scene with Ln lights, fw_bake_direct's kernels for one round
// around a second trace.  The drivers' reducer returns nothing, so the second trace's code leaves through `rc`: once it is set nothing
// more is launched and the call returns it.
struct HitLightSlots { int surf, irr, drays, dhits, dsums; };
HitLightSlots hit_light_stage(Staged &st, size_t cd, uint32_t Ln) {
    HitLightSlots s;
    s.surf = st.add(Staged::WORK, nullptr, cd * 64); s.irr = st.add(Staged::WORK, nullptr, cd * 12);
    s.drays = Ln ? st.add(Staged::WORK, nullptr, cd * Ln * 24) : -1; s.dhits = Ln ? st.add(Staged::WORK, nullptr, cd * Ln * sizeof(fw_hit)) : -1;
    s.dsums = Ln ? st.add(Staged::WORK, nullptr, cd * 32) : -1;
    return s;
}
struct HitLight {
    fw_scene *sc; const fw_trace_params *tp; const Staged &st; HitLightSlots s; uint32_t D, Ln; float direct_bias;
    const ProbeLookup &L; const fw::DProbeVis *vis; const float *d_sh, *d_pl; fw_stats *total;
    int rc = FW_OK;
    const uint32_t *mask_objs = nullptr; uint32_t n_mask = 0;      // FW_GATHER_NO_LIGHTS: the scene's sampled lights, masked out of the records
    float *surf() const { return st.ptr<float>(s.surf); }
    float *irr() const { return st.ptr<float>(s.irr); }
    // the chunk [q0, q0 + k) of round `round`: fills surf() and irr(); returns the chunk's direct records (fw_bake_direct's out), or NULL
    const float *run(uint32_t round, uint32_t q0, uint32_t k, const float *rays, const fw_hit *hits) {
        hipStream_t stream = (hipStream_t)tp->stream;
        const int n_cus = device_cus(sc->device);
        const uint32_t kd = k * D;
        float *d_surf = surf();
        fw::launch_hit_surface(stream, sc->n_cus, sc->d, sc->n_mat, rays, (const float4 *)hits, kd, (float4 *)d_surf);
        if (n_mask) fw::launch_area_mask(stream, n_cus, kd, mask_objs, n_mask, hits, d_surf);
        fw::launch_probe_irradiance(stream, L.g, vis, d_sh, d_pl, kd, d_surf + 8, d_surf + 4, 16, irr());
        if (!Ln) return nullptr;
        fw::DDirect dd{};
        dd.pts = fw::DDirectPoints{d_surf + 8, d_surf + 4, nullptr, nullptr, nullptr, 16, 3};
        dd.lights = (const float4 *)sc->dlights.p; dd.n_lights = Ln; dd.first = 0;
        dd.lobe = 0; dd.face_view = 0; dd.bias = direct_bias;
        float *drays = st.ptr<float>(s.drays), *dsums = st.ptr<float>(s.dsums);
        fw_hit *dhits = st.ptr<fw_hit>(s.dhits);
        fw::launch_direct_rays(stream, n_cus, dd, kd, drays);
        fw_trace_params q = *tp;
        q.on_device = 1; q.seed = tp->seed + round; q.key_base = q0 * D * Ln;
        fw_stats gs{};
        rc = trace_impl(sc, &q, drays, kd * Ln, dhits, total ? &gs : nullptr);
        if (rc) return nullptr;
        if (total) { gs.ms_render = 0.0; stats_add(*total, gs); }          // (its time lies inside the reducer's own span)
        if (hipMemsetAsync(dsums, 0, (size_t)kd * 32, stream) != hipSuccess) { rc = fail(FW_ERR_HIP, "hipMemsetAsync failed"); return nullptr; }
        fw::launch_direct_reduce(stream, n_cus, dd, kd, drays, dhits, dsums);
        return dsums;                                                      // one round: out = float(sums / 1) = sums
    }
};

// fw_bake_gather: fw_bake_ao's shape — k_ao_rays as trace_rounds' generator; its reducer is the rest of the chain over the chunk's rays and
// hits: HitLight's steps and k_gather_reduce.
int bake_gather_impl(fw_scene *sc, const fw_gather *g, const fw_trace_params *tp, const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd,
                     const float *moments, float normal_bias, const float *placement, uint32_t N, const float *positions, const float *normals,
                     uint32_t stride, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    if (!sc || !g || !tp || !positions || !normals) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = gather_check(g)) return rc;
    if (N == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (tp->on_device && ((((uintptr_t)sums | (uintptr_t)out) & 15u) || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and out must be 16-byte aligned, device positions, normals and ids 4-byte aligned");
    const ProbeLookupArgs a{sh, nullptr, nullptr, pd, moments, normal_bias, placement, pd || moments, placement != nullptr};
    ProbeLookup L;
    if (int rc = probe_lookup_check(grid, a, !sh, false, L)) return rc;
    if (tp->on_device && (((uintptr_t)sh | (uintptr_t)moments | (uintptr_t)placement) & 3u)) return fail(FW_ERR_BAD_ARG, "device sh, moments and placement must be 4-byte aligned");
    if (g->flags & ~(uint32_t)(FW_GATHER_DIRECT | FW_GATHER_NO_LIGHTS | FW_GATHER_NO_EMITTERS)) return fail(FW_ERR_BAD_ARG, "unknown gather flags");
    if ((g->flags & FW_GATHER_NO_LIGHTS) && (g->flags & FW_GATHER_NO_EMITTERS))
        return fail(FW_ERR_BAD_ARG, "gather flags: FW_GATHER_NO_LIGHTS and FW_GATHER_NO_EMITTERS exclude each other");
    const uint32_t D = g->directions;
    if ((uint64_t)N * D >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = probe_lookup_sizes(a, L)) return rc;
    if (int rc = need_device()) return rc;
    const uint32_t Ln = (g->flags & FW_GATHER_DIRECT) ? sc->n_dlights : 0u;
    if ((uint64_t)N * D * Ln >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions x the scene's lights must be below 2^31");
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    if (g->flags & FW_GATHER_NO_EMITTERS) if (int rc = ensure_emitters_surface(sc)) return rc;     // (§9zc: the entries' objects, built on first use)
    hipStream_t stream = (hipStream_t)tp->stream;
    const bool on_device = tp->on_device != 0;
    const uint64_t ray_bytes = 24 + sizeof(fw_hit) + 64 + 12 + (Ln ? (uint64_t)Ln * 72 + 64 : 0);
    const uint32_t chunk = std::min<uint32_t>(N, g->chunk_points ? g->chunk_points : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * ray_bytes)));
    uint64_t extent;
    if (int rc = points_extent(stream, N, ids, on_device, sums, extent)) return rc;
    const size_t rec_bytes = (size_t)extent * 16, cd = (size_t)chunk * D;
    Staged st(dev, stream, on_device);
    const AoSlots slots = ao_points_stage(st, N, positions, normals, stride, ids, extent);
    const ProbeTables t = probe_tables_stage(st, a, L);
    const int i_rays = st.add(Staged::WORK, nullptr, cd * 24), i_hits = st.add(Staged::WORK, nullptr, cd * sizeof(fw_hit));
    const HitLightSlots hs = hit_light_stage(st, cd, Ln);
    const int i_sums = st.add_sums(sums, rec_bytes), i_out = st.add(ids ? Staged::INOUT : Staged::OUT, out, rec_bytes);      // (with ids, entries outside the list stay)
    if (int rc = st.up()) return rc;
    const fw::DAoPoints pts = ao_points_device(st, slots, stride);
    float *d_sums = st.ptr<float>(i_sums);
    const fw::DProbeVis vis = probe_vis_device(a, st.ptr<const float>(t.mom));
    const int n_cus = device_cus(dev);
    fw_ao ao{};
    ao.directions = D; ao.falloff = 0; ao.radius = std::numeric_limits<float>::infinity(); ao.bias = g->bias; ao.jitter = g->jitter; ao.seed = g->seed;
    fw_stats total{};
    HitLight hl{sc, tp, st, hs, D, Ln, g->direct_bias, L, a.vis ? &vis : nullptr, st.ptr<const float>(t.sh), st.ptr<const float>(t.pl), stats ? &total : nullptr};
    if (g->flags & FW_GATHER_NO_LIGHTS) { hl.mask_objs = (const uint32_t *)sc->lights.p; hl.n_mask = sc->n_lights; }
    if (g->flags & FW_GATHER_NO_EMITTERS) { hl.mask_objs = emitters_surface_objs(sc); hl.n_mask = (uint32_t)sc->es_objs.size(); }
    uint32_t round = first_round;              // the reducer's round: trace_rounds hands it to the generator only
    const TraceRounds b{N, D, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
    if (int rc = trace_rounds(sc, tp, b, first_round, rounds, stats ? &total : nullptr,
            [&](uint32_t r, uint32_t q0, uint32_t k, float *rays) {
                round = r;
                if (!hl.rc) fw::launch_ao_rays(stream, n_cus, ao_rays_device(&ao, r, pts, q0), k, rays);
            },
            [&](uint32_t q0, uint32_t k, const float *rays, const fw_hit *hits) {
                if (hl.rc) return;
                const float *d_direct = hl.run(round, q0, k, rays, hits);
                if (!hl.rc) fw::launch_gather_reduce(stream, n_cus, q0, k, D, pts.ids, hl.surf(), hl.irr(), d_direct, d_sums);
            }))
        return rc;
    if (hl.rc) return hl.rc;
    if (int rc = st.download(i_sums)) return rc;
    if (out) fw::launch_gather_resolve(stream, N, (double)((uint64_t)first_round + rounds), pts.ids, d_sums, st.ptr<float>(i_out));
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- reflection gather (include/firework_hip.h) -------------------------------------------------------------------
// A reflection description's own argument checks (FW_ERR_BAD_ARG only); the flags are checked after the probe tables
int reflect_check(const fw_reflect *g) {
    if (g->directions == 0 || g->directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (!std::isfinite(g->bias) || g->bias < 0.f) return fail(FW_ERR_BAD_ARG, "bias must be finite and >= 0");
    if (!std::isfinite(g->direct_bias) || g->direct_bias < 0.f) return fail(FW_ERR_BAD_ARG, "direct_bias must be finite and >= 0");
    return FW_OK;
}
// the checks of the points that fw_reflect_rays and fw_bake_reflect share, after the description's and before the alignment's
int reflect_points_check(uint32_t n, uint32_t stride, uint32_t view_stride) {
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (view_stride < 3) return fail(FW_ERR_BAD_ARG, "view_stride_floats must be >= 3");
    return FW_OK;
}
fw::DReflectRays reflect_rays_device(const Staged &st, const DirectSlots &s, uint32_t stride, uint32_t view_stride, const fw_reflect *g, uint32_t round,
                                     uint32_t first) {
    fw::DReflectRays d{};
    d.pts = fw::DReflectPoints{st.ptr<const float>(s.pts.pos), st.ptr<const float>(s.pts.nrm), st.ptr<const uint32_t>(s.pts.ids),
                               st.ptr<const float>(s.view), st.ptr<const float4>(s.spec), stride, view_stride};
    d.first = first; d.directions = g->directions;
    d.seed32 = seed32_of(g->seed);
    d.jitter = g->jitter ? 1u : 0u;
    d.round = round; d.bias = g->bias;
    return d;
}

// fw_reflect_rays: fw_ao_rays' shape with two outputs — with device arrays the kernel works on the caller's memory; with host arrays the
// points are staged once and the rays and weights come back in slabs (32 B per ray)
int reflect_rays_impl(const fw_reflect *g, int device, uint32_t round, uint32_t n, const float *positions, const float *normals, uint32_t stride,
                      const uint32_t *ids, const float *view, uint32_t view_stride, const float *spec, float *rays, float *weights, int on_device,
                      void *stream_) {
    if (!g || !positions || !normals || !view || !spec || !rays || !weights) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = reflect_check(g)) return rc;
    if (int rc = reflect_points_check(n, stride, view_stride)) return rc;
    if (on_device && (((uintptr_t)spec & 15u) || ((uintptr_t)weights & 7u)
                      || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)view | (uintptr_t)rays) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device spec must be 16-byte aligned, device weights 8-byte aligned, device positions, normals, ids, view and rays 4-byte aligned");
    const uint32_t D = g->directions;
    if ((uint64_t)n * D >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    Staged st(device, stream, on_device != 0);
    const DirectSlots slots = direct_points_stage(st, n, positions, normals, stride, ids, view, view_stride, spec, on_device ? n : ao_extent(n, ids));
    HostSlabs sl(st, n, (size_t)D * 32);
    const int a_rays = sl.out(rays, (size_t)D * 24), a_w = sl.out(weights, (size_t)D * 8);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t done, uint32_t k) {
        fw::launch_reflect_rays(stream, n_cus, reflect_rays_device(st, slots, stride, view_stride, g, round, done), k, sl.ptr<float>(a_rays), sl.ptr<float>(a_w));
    });
}

// fw_reflect_reduce: fw_gather_reduce's shape with the weights
int reflect_reduce_impl(int device, uint32_t D, uint32_t n, const uint32_t *ids, const float *surface, const float *irradiance, const float *direct,
                        const float *weights, float *sums, int on_device, void *stream_) {
    if (!surface || !irradiance || !weights || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (D == 0 || D > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((((uintptr_t)sums | (uintptr_t)surface) & 15u) || ((uintptr_t)weights & 7u)
                      || (((uintptr_t)irradiance | (uintptr_t)direct | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and surface must be 16-byte aligned, device weights 8-byte aligned, device irradiance, direct and ids 4-byte aligned");
    if ((uint64_t)n * D >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t entries = (size_t)n * D;
    Staged st(device, stream, on_device != 0);
    const int i_surf = st.add(Staged::IN, surface, entries * 64), i_irr = st.add(Staged::IN, irradiance, entries * 12),
              i_dir = st.add(Staged::IN, direct, entries * 32), i_w = st.add(Staged::IN, weights, entries * 8),
              i_sums = st.add(Staged::INOUT, sums, on_device ? 0 : (size_t)ao_extent(n, ids) * 32), i_ids = st.add(Staged::IN, ids, (size_t)n * 4);
    if (int rc = st.up()) return rc;
    fw::launch_reflect_reduce(stream, device_cus(device), 0, n, D, st.ptr<const uint32_t>(i_ids), st.ptr<const float>(i_surf), st.ptr<const float>(i_irr),
                              st.ptr<const float>(i_dir), st.ptr<const float>(i_w), st.ptr<float>(i_sums));
    return st.finish();
}

// fw_bake_reflect: fw_bake_gather's shape — k_reflect_rays as trace_rounds' generator, which fills the chunk's weights beside its rays;
// the reducer is HitLight's steps over the chunk's rays and hits and k_reflect_reduce
int bake_reflect_impl(fw_scene *sc, const fw_reflect *g, const fw_trace_params *tp, const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd,
                      const float *moments, float normal_bias, const float *placement, uint32_t N, const float *positions, const float *normals,
                      uint32_t stride, const uint32_t *ids, const float *view, uint32_t view_stride, const float *spec, uint32_t first_round,
                      uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    if (!sc || !g || !tp || !positions || !normals || !view || !spec) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = reflect_check(g)) return rc;
    if (int rc = reflect_points_check(N, stride, view_stride)) return rc;
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (tp->on_device && ((((uintptr_t)sums | (uintptr_t)out | (uintptr_t)spec) & 15u)
                          || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)view) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums, out and spec must be 16-byte aligned, device positions, normals, ids and view 4-byte aligned");
    const ProbeLookupArgs a{sh, nullptr, nullptr, pd, moments, normal_bias, placement, pd || moments, placement != nullptr};
    ProbeLookup L;
    if (int rc = probe_lookup_check(grid, a, !sh, false, L)) return rc;
    if (tp->on_device && (((uintptr_t)sh | (uintptr_t)moments | (uintptr_t)placement) & 3u)) return fail(FW_ERR_BAD_ARG, "device sh, moments and placement must be 4-byte aligned");
    if (g->flags & ~(uint32_t)FW_REFLECT_DIRECT) return fail(FW_ERR_BAD_ARG, "unknown reflect flags");
    const uint32_t D = g->directions;
    if ((uint64_t)N * D >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions must be below 2^31");
    if (int rc = probe_lookup_sizes(a, L)) return rc;
    if (int rc = need_device()) return rc;
    const uint32_t Ln = (g->flags & FW_REFLECT_DIRECT) ? sc->n_dlights : 0u;
    if ((uint64_t)N * D * Ln >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x directions x the scene's lights must be below 2^31");
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)tp->stream;
    const bool on_device = tp->on_device != 0;
    const uint64_t ray_bytes = 24 + sizeof(fw_hit) + 8 + 64 + 12 + (Ln ? (uint64_t)Ln * 72 + 64 : 0);
    const uint32_t chunk = std::min<uint32_t>(N, g->chunk_points ? g->chunk_points : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * ray_bytes)));
    uint64_t extent;
    if (int rc = points_extent(stream, N, ids, on_device, sums, extent)) return rc;
    const size_t cd = (size_t)chunk * D;
    Staged st(dev, stream, on_device);
    const DirectSlots slots = direct_points_stage(st, N, positions, normals, stride, ids, view, view_stride, spec, extent);
    const ProbeTables t = probe_tables_stage(st, a, L);
    const int i_rays = st.add(Staged::WORK, nullptr, cd * 24), i_hits = st.add(Staged::WORK, nullptr, cd * sizeof(fw_hit)),
              i_w = st.add(Staged::WORK, nullptr, cd * 8);
    const HitLightSlots hs = hit_light_stage(st, cd, Ln);
    const int i_sums = st.add_sums(sums, (size_t)extent * 32), i_out = st.add(ids ? Staged::INOUT : Staged::OUT, out, (size_t)extent * 16);      // (with ids, entries outside the list stay)
    if (int rc = st.up()) return rc;
    float *d_sums = st.ptr<float>(i_sums), *d_w = st.ptr<float>(i_w);
    const uint32_t *d_ids = st.ptr<const uint32_t>(slots.pts.ids);
    const fw::DProbeVis vis = probe_vis_device(a, st.ptr<const float>(t.mom));
    const int n_cus = device_cus(dev);
    fw_stats total{};
    HitLight hl{sc, tp, st, hs, D, Ln, g->direct_bias, L, a.vis ? &vis : nullptr, st.ptr<const float>(t.sh), st.ptr<const float>(t.pl), stats ? &total : nullptr};
    uint32_t round = first_round;              // the reducer's round: trace_rounds hands it to the generator only
    const TraceRounds b{N, D, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
    if (int rc = trace_rounds(sc, tp, b, first_round, rounds, stats ? &total : nullptr,
            [&](uint32_t r, uint32_t q0, uint32_t k, float *rays) {
                round = r;
                if (!hl.rc) fw::launch_reflect_rays(stream, n_cus, reflect_rays_device(st, slots, stride, view_stride, g, r, q0), k, rays, d_w);
            },
            [&](uint32_t q0, uint32_t k, const float *rays, const fw_hit *hits) {
                if (hl.rc) return;
                const float *d_direct = hl.run(round, q0, k, rays, hits);
                if (!hl.rc) fw::launch_reflect_reduce(stream, n_cus, q0, k, D, d_ids, hl.surf(), hl.irr(), d_direct, d_w, d_sums);
            }))
        return rc;
    if (hl.rc) return hl.rc;
    if (int rc = st.download(i_sums)) return rc;
    if (out) fw::launch_reflect_resolve(stream, N, (double)((uint64_t)first_round + rounds), d_ids, st.ptr<const float>(slots.spec), d_sums, st.ptr<float>(i_out));
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- sphere and rectangle emitters sampled at surface points (include/firework_hip.h) ------------------------------
// A description's own argument checks (FW_ERR_BAD_ARG only)
int area_check(const fw_area *ap) {
    if (ap->samples == 0 || ap->samples > (1u << 20)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^20");
    if (!std::isfinite(ap->bias) || ap->bias < 0.f) return fail(FW_ERR_BAD_ARG, "bias must be finite and >= 0");
    return FW_OK;
}
// caller-made light records: a count in 1..FW_MAX_LIGHTS and a shape kind that fw_selftest_lights writes in each
int area_lights_check(const float *lights, uint32_t n_lights) {
    if (n_lights == 0 || n_lights > FW_MAX_LIGHTS) return fail(FW_ERR_BAD_ARG, "n_lights must be in 1..FW_MAX_LIGHTS");
    for (uint32_t i = 0; i < n_lights; i++) {
        const float k = lights[(size_t)i * FW_LIGHT_RECORD_FLOATS + 1];
        if (!(k == 0.f || k == 1.f || k == 2.f || k == 3.f)) return fail(FW_ERR_BAD_ARG, "lights[" + std::to_string(i) + "]: unknown kind");
    }
    return FW_OK;
}
// a list of light objects: a count in 1..FW_MAX_LIGHTS, strictly ascending where the call searches it
int area_objects_check(const uint32_t *objects, uint32_t n_objects, bool ascending) {
    if (n_objects == 0 || n_objects > FW_MAX_LIGHTS) return fail(FW_ERR_BAD_ARG, "n_objects must be in 1..FW_MAX_LIGHTS");
    if (ascending) for (uint32_t i = 1; i < n_objects; i++) if (!(objects[i - 1] < objects[i])) return fail(FW_ERR_BAD_ARG, "objects must ascend strictly");
    return FW_OK;
}
fw::DAreaRays area_rays_device(const fw_area *ap, uint32_t round, const fw::DAoPoints &pts, const float4 *lights, uint32_t n_lights, uint32_t first) {
    fw::DAreaRays d{};
    d.pts = pts; d.lights = lights; d.n_lights = n_lights; d.samples = ap->samples; d.first = first;
    d.seed32 = seed32_of(ap->seed);
    d.jitter = ap->jitter ? 1u : 0u;
    d.round = round; d.bias = ap->bias;
    return d;
}

// fw_scene_area_lights: the records kept with the scene since its creation or its last update
int scene_area_lights_impl(fw_scene *sc, float *out, uint32_t cap, uint32_t *n) {
    if (!sc || !n || (!out && cap > 0)) return fail(FW_ERR_BAD_ARG, "null argument");
    *n = sc->n_lights;
    const size_t k = std::min<size_t>(cap, sc->n_lights);
    if (k) std::memcpy(out, sc->light_recs.data(), k * FW_LIGHT_RECORD_FLOATS * 4);
    return FW_OK;
}

// fw_area_rays: fw_reflect_rays' shape — the light records are the caller's host array, staged with the points
int area_rays_impl(const fw_area *ap, const float *lights, uint32_t n_lights, int device, uint32_t round, uint32_t n, const float *positions,
                   const float *normals, uint32_t stride, const uint32_t *ids, float *rays, float *weights, int on_device, void *stream_) {
    if (!ap || !lights || !positions || !normals || !rays || !weights) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = area_check(ap)) return rc;
    if (int rc = area_lights_check(lights, n_lights)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (on_device && (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)rays | (uintptr_t)weights) & 3u))
        return fail(FW_ERR_BAD_ARG, "device arrays must be 4-byte aligned");
    const uint64_t M = (uint64_t)n_lights * ap->samples;
    if ((uint64_t)n * M >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x n_lights x samples must be below 2^31");
    const uint64_t extent = on_device ? n : ao_extent(n, ids);
    if (extent * n_lights >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "id x n_lights must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    Staged st(device, stream, on_device != 0);
    const AoSlots slots = ao_points_stage(st, n, positions, normals, stride, ids, extent);
    const int i_rec = st.add(Staged::IN, lights, (size_t)n_lights * 64, true);
    HostSlabs sl(st, n, (size_t)M * 28);
    const int a_rays = sl.out(rays, (size_t)M * 24), a_w = sl.out(weights, (size_t)M * 4);
    if (int rc = st.up()) return rc;
    const fw::DAoPoints pts = ao_points_device(st, slots, stride);
    return sl.run([&](uint32_t done, uint32_t k) {
        fw::launch_area_rays(stream, n_cus, area_rays_device(ap, round, pts, st.ptr<const float4>(i_rec), n_lights, done), k, sl.ptr<float>(a_rays),
                             sl.ptr<float>(a_w));
    });
}

// fw_area_reduce: fw_gather_reduce's shape with the weights, the hits and the lights' objects
int area_reduce_impl(int device, uint32_t S, const uint32_t *objects, uint32_t n_objects, uint32_t n, const uint32_t *ids, const float *weights,
                     const fw_hit *hits, const float *surface, float *sums, int on_device, void *stream_) {
    if (!objects || !weights || !hits || !surface || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (S == 0 || S > (1u << 20)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^20");
    if (int rc = area_objects_check(objects, n_objects, false)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((((uintptr_t)sums | (uintptr_t)hits | (uintptr_t)surface) & 15u) || (((uintptr_t)weights | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums, hits and surface must be 16-byte aligned, device weights and ids 4-byte aligned");
    const uint64_t M = (uint64_t)n_objects * S;
    if ((uint64_t)n * M >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x n_objects x samples must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t entries = (size_t)n * M;
    Staged st(device, stream, on_device != 0);
    const int i_obj = st.add(Staged::IN, objects, (size_t)n_objects * 4, true), i_w = st.add(Staged::IN, weights, entries * 4),
              i_hits = st.add(Staged::IN, hits, entries * sizeof(fw_hit)), i_surf = st.add(Staged::IN, surface, entries * 64),
              i_sums = st.add(Staged::INOUT, sums, on_device ? 0 : (size_t)ao_extent(n, ids) * 16), i_ids = st.add(Staged::IN, ids, (size_t)n * 4);
    if (int rc = st.up()) return rc;
    fw::launch_area_reduce(stream, device_cus(device), 0, n, n_objects, S, st.ptr<const uint32_t>(i_ids), st.ptr<const uint32_t>(i_obj),
                           st.ptr<const float>(i_w), st.ptr<const fw_hit>(i_hits), st.ptr<const float>(i_surf), st.ptr<float>(i_sums));
    return st.finish();
}

// fw_area_mask: the records are rewritten where they lie (device arrays) or pass through the call's own copy (host arrays)
int area_mask_impl(int device, const uint32_t *objects, uint32_t n_objects, uint32_t n, const fw_hit *hits, float *surface, int on_device, void *stream_) {
    if (!objects || !hits || !surface) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = area_objects_check(objects, n_objects, true)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && (((uintptr_t)hits | (uintptr_t)surface) & 15u)) return fail(FW_ERR_BAD_ARG, "device hits and surface must be 16-byte aligned");
    if (n >= (1u << 31)) return fail(FW_ERR_UNSUPPORTED, "n must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Staged st(device, stream, on_device != 0);
    const int i_obj = st.add(Staged::IN, objects, (size_t)n_objects * 4, true), i_hits = st.add(Staged::IN, hits, (size_t)n * sizeof(fw_hit)),
              i_surf = st.add(Staged::INOUT, surface, on_device ? 0 : (size_t)n * 64);
    if (int rc = st.up()) return rc;
    fw::launch_area_mask(stream, device_cus(device), n, st.ptr<const uint32_t>(i_obj), n_objects, st.ptr<const fw_hit>(i_hits), st.ptr<float>(i_surf));
    return st.finish();
}

// fw_bake_area: fw_bake_ao's shape — k_area_rays as trace_rounds' generator over the scene's own light records where they lie, which
// fills the chunk's weights beside its rays; the reducer is k_hit_surface over the chunk's rays and hits and k_area_reduce.  The scene
// is looked at only after a device was found: Ln is the scene's, and a scene exists only where a device does.
int bake_area_impl(fw_scene *sc, const fw_area *ap, const fw_trace_params *tp, uint32_t N, const float *positions, const float *normals, uint32_t stride,
                   const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    if (!sc || !ap || !tp || !positions || !normals) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = area_check(ap)) return rc;
    if (N == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (tp->on_device && ((((uintptr_t)sums | (uintptr_t)out) & 15u) || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and out must be 16-byte aligned, device positions, normals and ids 4-byte aligned");
    if (int rc = need_device()) return rc;
    const uint32_t Ln = sc->n_lights, S = ap->samples;
    const uint64_t M = (uint64_t)Ln * S;
    if ((uint64_t)N * M >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x the scene's sampled lights x samples must be below 2^31");
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)tp->stream;
    const bool on_device = tp->on_device != 0;
    uint64_t extent;
    if (int rc = points_extent(stream, N, ids, on_device, sums, extent)) return rc;
    if (extent * std::max(Ln, 1u) >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "id x the scene's sampled lights must be below 2^31");
    const uint32_t chunk = std::min<uint32_t>(N, ap->chunk_points ? ap->chunk_points : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / (std::max<uint64_t>(M, 1) * 140)));
    const size_t rec_bytes = (size_t)extent * 16, cm = (size_t)chunk * M;
    Staged st(dev, stream, on_device);
    const AoSlots slots = ao_points_stage(st, N, positions, normals, stride, ids, extent);
    const int i_rays = st.add(Staged::WORK, nullptr, cm * 24), i_hits = st.add(Staged::WORK, nullptr, cm * sizeof(fw_hit)),
              i_w = st.add(Staged::WORK, nullptr, cm * 4), i_surf = st.add(Staged::WORK, nullptr, cm * 64);
    const int i_sums = st.add_sums(sums, rec_bytes), i_out = st.add(ids ? Staged::INOUT : Staged::OUT, out, rec_bytes);      // (with ids, entries outside the list stay)
    if (int rc = st.up()) return rc;
    const fw::DAoPoints pts = ao_points_device(st, slots, stride);
    float *d_sums = st.ptr<float>(i_sums), *d_w = st.ptr<float>(i_w), *d_surf = st.ptr<float>(i_surf);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    if (Ln > 0) {
        const float4 *d_rec = (const float4 *)sc->area_recs.p;
        const uint32_t *d_obj = (const uint32_t *)sc->lights.p;
        const TraceRounds b{N, (uint32_t)M, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
        if (int rc = trace_rounds(sc, tp, b, first_round, rounds, stats ? &total : nullptr,
                [&](uint32_t r, uint32_t q0, uint32_t k, float *rays) {
                    fw::launch_area_rays(stream, n_cus, area_rays_device(ap, r, pts, d_rec, Ln, q0), k, rays, d_w);
                },
                [&](uint32_t q0, uint32_t k, const float *rays, const fw_hit *hits) {
                    const uint32_t km = k * (uint32_t)M;
                    fw::launch_hit_surface(stream, sc->n_cus, sc->d, sc->n_mat, rays, (const float4 *)hits, km, (float4 *)d_surf);
                    fw::launch_area_reduce(stream, n_cus, q0, k, Ln, S, pts.ids, d_obj, d_w, hits, d_surf, d_sums);
                }))
            return rc;
    }
    if (int rc = st.download(i_sums)) return rc;
    if (out) fw::launch_area_resolve(stream, N, (double)((uint64_t)first_round + rounds), pts.ids, d_sums, st.ptr<float>(i_out));
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- every emitter sampled at surface points, picked by power (include/firework_hip.h) -------------------------------
int emitters_check(const fw_emitters *ep) {
    if (ep->samples == 0 || ep->samples > (1u << 20)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^20");
    if (!std::isfinite(ep->bias) || ep->bias < 0.f) return fail(FW_ERR_BAD_ARG, "bias must be finite and >= 0");
    return FW_OK;
}
// caller-made records and their cdf: a count in 1..2^24, a kind fw_scene_emitters writes in each, and a cdf the kernel's searches end in
int emitters_list_check(const float *records, const double *cdf, uint32_t n_entries) {
    if (n_entries == 0 || n_entries > (1u << 24)) return fail(FW_ERR_BAD_ARG, "n_entries must be in 1..2^24");
    double prev = 0.0;
    for (uint32_t i = 0; i < n_entries; i++) {
        const float k = records[(size_t)i * FW_EMITTERS_RECORD_FLOATS + 1];
        if (!(k == 0.f || k == 1.f || k == 2.f || k == 3.f || k == 4.f || k == 5.f || k == 9.f)) return fail(FW_ERR_BAD_ARG, "records[" + std::to_string(i) + "]: unknown kind");
        if (!(cdf[i] >= prev && cdf[i] <= 1.0)) return fail(FW_ERR_BAD_ARG, "cdf must not decrease and must stay in [0, 1]");
        prev = cdf[i];
    }
    if (prev != 1.0) return fail(FW_ERR_BAD_ARG, "cdf must end in 1");
    return FW_OK;
}
fw::DEmittersRays emitters_rays_device(const fw_emitters *ep, uint32_t round, const fw::DAoPoints &pts, const float4 *records, const double *cdf,
                                       uint32_t n_entries, uint32_t first) {
    fw::DEmittersRays d{};
    d.pts = pts; d.records = records; d.cdf = cdf; d.n_entries = n_entries; d.samples = ep->samples; d.first = first;
    d.seed32 = seed32_of(ep->seed);
    d.jitter = ep->jitter ? 1u : 0u;
    d.round = round; d.bias = ep->bias;
    return d;
}

// fw_selftest_emitters_records: the description's own arrays give a mesh's triangles
int selftest_emitters_records_impl(const fw_scene_desc *desc, float *records, uint32_t *codes, uint32_t cap, uint32_t *n) {
    if (!desc || !n || ((!records || !codes) && cap > 0)) return fail(FW_ERR_BAD_ARG, "null argument");
    uint64_t total = 0;
    const std::vector<EmitterObj> E = scene_emitters(desc, total);
    *n = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
    std::vector<float> rec, tris;
    std::vector<uint32_t> cod;
    for (const EmitterObj &e : E) {
        if (e.first >= cap) break;
        const fw_shape &s = desc->shapes[e.shape];
        rec.assign((size_t)e.count * FW_EMITTERS_RECORD_FLOATS, 0.f); cod.assign((size_t)e.count * 2, 0u);
        if (e.kind == FW_SHAPE_TRIANGLE_MESH) {
            tris.assign((size_t)e.count * 9, 0.f);
            for (size_t v = 0; v < (size_t)e.count * 3; v++) { const uint32_t vi = s.indices[v]; if (vi < s.n_verts) for (int c = 0; c < 3; c++) tris[v * 3 + c] = s.verts[3 * (size_t)vi + c]; }
        }
        emitters_object_records(e, s, tris.data(), rec.data(), cod.data());
        const size_t k = (size_t)std::min<uint64_t>(e.count, cap - e.first);
        std::memcpy(records + (size_t)e.first * FW_EMITTERS_RECORD_FLOATS, rec.data(), k * FW_EMITTERS_RECORD_FLOATS * 4);
        std::memcpy(codes + (size_t)e.first * 2, cod.data(), k * 8);
    }
    return FW_OK;
}

int scene_emitters_impl(fw_scene *sc, float *records, uint32_t *codes, uint32_t cap, uint32_t *n) {
    if (!sc || !n || ((!records || !codes) && cap > 0)) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = ensure_emitters_surface(sc)) return rc;
    *n = (uint32_t)sc->es_cdf.size();
    const size_t k = std::min<size_t>(cap, sc->es_cdf.size());
    if (k) { std::memcpy(records, sc->es_rec.data(), k * FW_EMITTERS_RECORD_FLOATS * 4); std::memcpy(codes, sc->es_codes.data(), k * 8); }
    return FW_OK;
}

int emitters_cdf_impl(const float *weights, uint32_t n, double *cdf, double *total) {
    if (!weights || !cdf || n == 0) return fail(FW_ERR_BAD_ARG, "null argument or n == 0");
    const double t = emitters_cdf(weights, n, cdf);
    if (total) *total = t;
    return FW_OK;
}

// fw_emitters_rays: fw_area_rays' shape with a third output; the records and the cdf are the caller's host arrays, staged with the points
int emitters_rays_impl(const fw_emitters *ep, const float *records, const double *cdf, uint32_t n_entries, int device, uint32_t round, uint32_t n,
                       const float *positions, const float *normals, uint32_t stride, const uint32_t *ids, float *rays, float *weights, uint32_t *picks,
                       int on_device, void *stream_) {
    if (!ep || !records || !cdf || !positions || !normals || !rays || !weights || !picks) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = emitters_check(ep)) return rc;
    if (int rc = emitters_list_check(records, cdf, n_entries)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (on_device && (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids | (uintptr_t)rays | (uintptr_t)weights | (uintptr_t)picks) & 3u))
        return fail(FW_ERR_BAD_ARG, "device arrays must be 4-byte aligned");
    const uint64_t S = ep->samples;
    if ((uint64_t)n * S >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x samples must be below 2^31");
    const uint64_t extent = on_device ? n : ao_extent(n, ids);
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    Staged st(device, stream, on_device != 0);
    const AoSlots slots = ao_points_stage(st, n, positions, normals, stride, ids, extent);
    const int i_rec = st.add(Staged::IN, records, (size_t)n_entries * 64, true), i_cdf = st.add(Staged::IN, cdf, (size_t)n_entries * 8, true);
    HostSlabs sl(st, n, (size_t)S * 32);
    const int a_rays = sl.out(rays, (size_t)S * 24), a_w = sl.out(weights, (size_t)S * 4), a_p = sl.out(picks, (size_t)S * 4);
    if (int rc = st.up()) return rc;
    const fw::DAoPoints pts = ao_points_device(st, slots, stride);
    return sl.run([&](uint32_t done, uint32_t k) {
        fw::launch_emitters_rays(stream, n_cus, emitters_rays_device(ep, round, pts, st.ptr<const float4>(i_rec), st.ptr<const double>(i_cdf), n_entries, done),
                                 k, sl.ptr<float>(a_rays), sl.ptr<float>(a_w), sl.ptr<uint32_t>(a_p));
    });
}

// fw_emitters_reduce: fw_area_reduce's shape with the picks and the entries' codes
int emitters_reduce_impl(int device, uint32_t S, const uint32_t *codes, uint32_t n_entries, uint32_t n, const uint32_t *ids, const uint32_t *picks,
                         const float *weights, const fw_hit *hits, const float *surface, float *sums, int on_device, void *stream_) {
    if (!codes || !picks || !weights || !hits || !surface || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    if (S == 0 || S > (1u << 20)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^20");
    if (n_entries == 0 || n_entries > (1u << 24)) return fail(FW_ERR_BAD_ARG, "n_entries must be in 1..2^24");
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((((uintptr_t)sums | (uintptr_t)hits | (uintptr_t)surface) & 15u) || (((uintptr_t)weights | (uintptr_t)picks | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums, hits and surface must be 16-byte aligned, device picks, weights and ids 4-byte aligned");
    if ((uint64_t)n * S >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x samples must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t entries = (size_t)n * S;
    Staged st(device, stream, on_device != 0);
    const int i_codes = st.add(Staged::IN, codes, (size_t)n_entries * 8, true), i_p = st.add(Staged::IN, picks, entries * 4), i_w = st.add(Staged::IN, weights, entries * 4),
              i_hits = st.add(Staged::IN, hits, entries * sizeof(fw_hit)), i_surf = st.add(Staged::IN, surface, entries * 64),
              i_sums = st.add(Staged::INOUT, sums, on_device ? 0 : (size_t)ao_extent(n, ids) * 16), i_ids = st.add(Staged::IN, ids, (size_t)n * 4);
    if (int rc = st.up()) return rc;
    fw::launch_emitters_reduce(stream, device_cus(device), 0, n, S, st.ptr<const uint32_t>(i_ids), st.ptr<const uint32_t>(i_codes), n_entries,
                               st.ptr<const uint32_t>(i_p), st.ptr<const float>(i_w), st.ptr<const fw_hit>(i_hits), st.ptr<const float>(i_surf), st.ptr<float>(i_sums));
    return st.finish();
}

// fw_bake_emitters: fw_bake_area's shape — k_emitters_rays as trace_rounds' generator over the scene's own records and cdf where they lie,
// which fills the chunk's weights and picks beside its rays; the reducer is k_hit_surface and k_emitters_reduce
int bake_emitters_impl(fw_scene *sc, const fw_emitters *ep, const fw_trace_params *tp, uint32_t N, const float *positions, const float *normals,
                       uint32_t stride, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    if (!sc || !ep || !tp || !positions || !normals) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = emitters_check(ep)) return rc;
    if (N == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (tp->on_device && ((((uintptr_t)sums | (uintptr_t)out) & 15u) || (((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)ids) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and out must be 16-byte aligned, device positions, normals and ids 4-byte aligned");
    if (int rc = need_device()) return rc;
    if (int rc = ensure_emitters_surface(sc)) return rc;
    const uint32_t S = ep->samples;
    if ((uint64_t)N * S >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n x samples must be below 2^31");
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)tp->stream;
    const bool on_device = tp->on_device != 0;
    uint64_t extent;
    if (int rc = points_extent(stream, N, ids, on_device, sums, extent)) return rc;
    const uint32_t chunk = std::min<uint32_t>(N, ep->chunk_points ? ep->chunk_points : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)S * 144)));
    const size_t rec_bytes = (size_t)extent * 16, cm = (size_t)chunk * S;
    Staged st(dev, stream, on_device);
    const AoSlots slots = ao_points_stage(st, N, positions, normals, stride, ids, extent);
    const int i_rays = st.add(Staged::WORK, nullptr, cm * 24), i_hits = st.add(Staged::WORK, nullptr, cm * sizeof(fw_hit)),
              i_w = st.add(Staged::WORK, nullptr, cm * 4), i_p = st.add(Staged::WORK, nullptr, cm * 4), i_surf = st.add(Staged::WORK, nullptr, cm * 64);
    const int i_sums = st.add_sums(sums, rec_bytes), i_out = st.add(ids ? Staged::INOUT : Staged::OUT, out, rec_bytes);      // (with ids, entries outside the list stay)
    if (int rc = st.up()) return rc;
    const fw::DAoPoints pts = ao_points_device(st, slots, stride);
    float *d_sums = st.ptr<float>(i_sums), *d_w = st.ptr<float>(i_w), *d_surf = st.ptr<float>(i_surf);
    uint32_t *d_p = st.ptr<uint32_t>(i_p);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    const uint32_t Ne = (uint32_t)sc->es_cdf.size();
    if (Ne > 0 && sc->es_total > 0.0) {
        const TraceRounds b{N, S, chunk, st.ptr<float>(i_rays), st.ptr<fw_hit>(i_hits)};
        if (int rc = trace_rounds(sc, tp, b, first_round, rounds, stats ? &total : nullptr,
                [&](uint32_t r, uint32_t q0, uint32_t k, float *rays) {
                    fw::launch_emitters_rays(stream, n_cus, emitters_rays_device(ep, r, pts, emitters_surface_records(sc), emitters_surface_cdf(sc), Ne, q0), k, rays, d_w, d_p);
                },
                [&](uint32_t q0, uint32_t k, const float *rays, const fw_hit *hits) {
                    const uint32_t km = k * S;
                    fw::launch_hit_surface(stream, sc->n_cus, sc->d, sc->n_mat, rays, (const float4 *)hits, km, (float4 *)d_surf);
                    fw::launch_emitters_reduce(stream, n_cus, q0, k, S, pts.ids, emitters_surface_codes(sc), Ne, d_p, d_w, hits, d_surf, d_sums);
                }))
            return rc;
    }
    if (int rc = st.download(i_sums)) return rc;
    if (out) fw::launch_area_resolve(stream, N, (double)((uint64_t)first_round + rounds), pts.ids, d_sums, st.ptr<float>(i_out));
    if (int rc = st.finish()) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// ---- probe radiance maps (include/firework_hip.h) ------------------------------------------------------------------
// A radiance description's own argument checks (FW_ERR_BAD_ARG only) and what the kernels need of it
int probe_radiance_check(const fw_probe_radiance *pr, fw::DProbeRadiance &d) {
    if (pr->resolution != 4 && pr->resolution != 8 && pr->resolution != 16 && pr->resolution != 32)
        return fail(FW_ERR_BAD_ARG, "a probe radiance map's resolution must be 4, 8, 16 or 32");
    if (pr->sharpness_log2 > 8) return fail(FW_ERR_BAD_ARG, "sharpness_log2 must be in 0..8");
    if (pr->levels == 0 || pr->levels > FW_PROBE_RADIANCE_MAX_LEVELS || (pr->resolution >> (pr->levels - 1)) < 4)
        return fail(FW_ERR_BAD_ARG, "levels must be >= 1 and the last level's resolution at least 4");
    for (uint32_t l = 0; l < pr->levels; l++) {
        const float rho = pr->roughness[l];
        if (!(rho >= 0.f && rho <= 1.f)) return fail(FW_ERR_BAD_ARG, "every level's roughness must be in [0, 1]");
        if (l > 0 && !(rho > pr->roughness[l - 1])) return fail(FW_ERR_BAD_ARG, "the levels' roughness must ascend strictly");
    }
    d = fw::DProbeRadiance{};
    d.R = pr->resolution; d.k = pr->sharpness_log2; d.levels = pr->levels;
    for (uint32_t l = 0; l < pr->levels; l++) { d.texels += (d.R >> l) * (d.R >> l); d.rho[l] = (double)pr->roughness[l]; }
    return FW_OK;
}

// fw_probe_radiance_reduce: fw_probe_depth_reduce's shape
int probe_radiance_reduce_impl(int device, const fw_probe_radiance *pr, uint32_t n_probes, uint32_t directions, uint32_t samples, const float *rays,
                               const float *accum, float *sums, int on_device, void *stream_) {
    if (!pr || !rays || !accum || !sums) return fail(FW_ERR_BAD_ARG, "null argument");
    fw::DProbeRadiance d{};
    if (int rc = probe_radiance_check(pr, d)) return rc;
    if (n_probes == 0) return fail(FW_ERR_BAD_ARG, "n_probes must be > 0");
    if (directions == 0 || directions > (1u << 20)) return fail(FW_ERR_BAD_ARG, "directions must be in 1..2^20");
    if (samples == 0 || samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    if (on_device && ((((uintptr_t)sums | (uintptr_t)accum) & 15u) || ((uintptr_t)rays & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and accum must be 16-byte aligned, device rays 4-byte aligned");
    const uint32_t R = d.R;
    if ((uint64_t)n_probes * directions >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if ((uint64_t)n_probes * R * R >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x resolution^2 must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)n_probes * directions;
    Staged st(device, stream, on_device != 0);
    const int i_rays = st.add(Staged::IN, rays, n * 24), i_acc = st.add(Staged::IN, accum, n * 16),
              i_sums = st.add(Staged::INOUT, sums, (size_t)n_probes * R * R * 16);
    if (int rc = st.up()) return rc;
    fw::launch_probe_radiance_reduce(stream, n_probes, directions, d, samples, st.ptr<const float>(i_rays), st.ptr<const float>(i_acc), st.ptr<float>(i_sums));
    return st.finish();
}

// fw_probe_radiance_prefilter: the maps are overwritten, so a host caller's are not uploaded
int probe_radiance_prefilter_impl(int device, const fw_probe_radiance *pr, uint32_t n_probes, const float *sums, float *maps, int on_device,
                                  void *stream_) {
    if (!pr || !sums || !maps) return fail(FW_ERR_BAD_ARG, "null argument");
    fw::DProbeRadiance d{};
    if (int rc = probe_radiance_check(pr, d)) return rc;
    if (n_probes == 0) return fail(FW_ERR_BAD_ARG, "n_probes must be > 0");
    if (on_device && (((uintptr_t)sums | (uintptr_t)maps) & 15u)) return fail(FW_ERR_BAD_ARG, "device sums and maps must be 16-byte aligned");
    if ((uint64_t)n_probes * d.texels >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x texels must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Staged st(device, stream, on_device != 0);
    const int i_sums = st.add(Staged::IN, sums, (size_t)n_probes * d.R * d.R * 16), i_maps = st.add(Staged::OUT, maps, (size_t)n_probes * d.texels * 16);
    if (int rc = st.up()) return rc;
    fw::launch_probe_radiance_prefilter(stream, device_cus(device), n_probes, d, st.ptr<const float>(i_sums), st.ptr<float>(i_maps));
    return st.finish();
}

// fw_bake_probe_radiance: bake_probes_impl with k_probe_radiance_reduce as bake_rounds' reducer — and, with sh_sums or sh, k_probe_project
// beside it on the same rendered accum — and one prefilter of the final sums.  Its own are the argument checks, the Staged arrays
// (positions, a chunk's rays and accum, and whichever running sums and maps the caller's device memory does not hold) and sh, divided on
// the host.
int bake_probe_radiance_impl(fw_scene *sc, const fw_probe_set *s, const fw_probe_radiance *pr, const fw_render_rays_params *rp, uint32_t first_round,
                             uint32_t rounds, float *sums, float *maps, float *sh_sums, float *sh, fw_stats *stats) {
    if (!sc || !s || !pr || !rp) return fail(FW_ERR_BAD_ARG, "null argument");
    bool too_large = false;
    if (int rc = probe_set_check(s, too_large)) return rc;
    fw::DProbeRadiance d{};
    if (int rc = probe_radiance_check(pr, d)) return rc;
    if (rounds == 0) return fail(FW_ERR_BAD_ARG, "rounds must be > 0");
    if ((uint64_t)first_round + rounds > 0xffffffffull) return fail(FW_ERR_BAD_ARG, "first_round + rounds overflows");
    if (rp->samples == 0 || rp->samples > (1u << 24)) return fail(FW_ERR_BAD_ARG, "samples must be in 1..2^24");
    const bool with_sh = sh_sums || sh;
    if (!sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sums of the rounds before it");
    if (with_sh && !sh_sums && first_round > 0) return fail(FW_ERR_BAD_ARG, "first_round > 0 needs the sh_sums of the rounds before it");
    if (rp->on_device && ((((uintptr_t)sums | (uintptr_t)maps) & 15u) || (((uintptr_t)sh_sums | (uintptr_t)sh) & 3u)))
        return fail(FW_ERR_BAD_ARG, "device sums and maps must be 16-byte aligned, device sh_sums and sh 4-byte aligned");
    const uint32_t N = s->n_probes, D = s->directions, S = rp->samples, R = d.R;
    if (too_large) return fail(FW_ERR_UNSUPPORTED, "n_probes x directions must be below 2^31");
    if ((uint64_t)N * d.texels >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "n_probes x texels must be below 2^31");
    if (int rc = need_device()) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int dev = sc->device;
    HIPCHK(hipSetDevice(dev));
    hipStream_t stream = (hipStream_t)rp->stream;
    const uint32_t chunk = std::min<uint32_t>(N, s->chunk_probes ? s->chunk_probes : (uint32_t)std::max<uint64_t>(1, CALL_SCRATCH_BYTES / ((uint64_t)D * 40)));
    Staged st(dev, stream, rp->on_device != 0);
    const int i_pos = st.add(Staged::IN, s->positions, (size_t)N * 12, true), i_rays = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 24),
              i_acc = st.add(Staged::WORK, nullptr, (size_t)chunk * D * 16), i_sums = st.add_sums(sums, (size_t)N * R * R * 16),
              i_sh = with_sh ? st.add_sums(sh_sums, (size_t)N * 108) : st.add(Staged::IN, nullptr, 0),
              i_maps = st.add(Staged::OUT, maps, (size_t)N * d.texels * 16);
    if (int rc = st.up()) return rc;
    const float *d_pos = st.ptr<const float>(i_pos);
    float *d_sums = st.ptr<float>(i_sums), *d_sh = st.ptr<float>(i_sh);
    const int n_cus = device_cus(dev);
    fw_stats total{};
    // (the reducers' loads and their sums: 40 B per ray and 32 B per texel; the projection's 40 B per ray and 216 B per probe)
    const BakeRounds b{first_round, rounds, N, D, chunk, st.ptr<float>(i_rays), st.ptr<float>(i_acc), 0, with_sh ? 80u : 40u, R * R * 32u + (with_sh ? 216u : 0u)};
    if (int rc = bake_rounds(sc, rp, b, stats ? &total : nullptr,
            [&](uint32_t r, uint32_t p0, uint32_t k, float *rays) { fw::launch_probe_rays(stream, n_cus, probes_device(s, r, p0, d_pos + (size_t)p0 * 3), k, rays); },
            [&](uint32_t p0, uint32_t k, const float *rays, const float *acc) {
                fw::launch_probe_radiance_reduce(stream, k, D, d, S, rays, acc, d_sums + (size_t)p0 * R * R * 4);
                if (with_sh) fw::launch_probe_project(stream, n_cus, k, D, S, rays, acc, d_sh + (size_t)p0 * 27);
            }))
        return rc;
    if (maps) {
        CallEvents<2> ev;                                 // around the prefilter: its time joins the reducers'
        if (stats) { for (hipEvent_t &e : ev.e) HIPCHK(hipEventCreate(&e)); HIPCHK(hipEventRecord(ev.e[0], stream)); }
        fw::launch_probe_radiance_prefilter(stream, n_cus, N, d, d_sums, st.ptr<float>(i_maps));
        if (stats) {
            HIPCHK(hipEventRecord(ev.e[1], stream));
            HIPCHK(hipEventSynchronize(ev.e[1]));
            float pf_ms = 0.f;
            HIPCHK(hipEventElapsedTime(&pf_ms, ev.e[0], ev.e[1]));
            total.ms_render += pf_ms;
            if (rp->flags & FW_FLAG_TIME_KERNELS) total.ms_accumulate += pf_ms;
            total.bytes_accumulate += (uint64_t)N * ((uint64_t)R * R + d.texels) * 16;
        }
    }
    // the outputs: sums, maps and sh_sums where the caller keeps them, and sh = sh_sums / rounds so far
    std::vector<float> keep;
    const float *h_sh = nullptr;
    if (int rc = st.download(i_sums)) return rc;
    if (int rc = st.download(i_maps)) return rc;
    if (with_sh) if (int rc = st.fetch(i_sh, sh != nullptr, keep, h_sh)) return rc;
    if (int rc = st.finish()) return rc;
    if (sh) if (int rc = sh_from_sums(stream, h_sh, (size_t)N * 27, first_round, rounds, sh, rp->on_device != 0)) return rc;
    stats_finish(stats, total, wall0);
    return FW_OK;
}

// fw_probe_radiance_lookup: probe_irradiance_impl's shape; a host call's slab holds 40 B in and 12 B out per point
int probe_radiance_lookup_impl(const fw_probe_grid *grid, const ProbeLookupArgs &a, int device, uint32_t n, const float *positions,
                               const float *normals, uint32_t stride, const float *dirs, const float *roughness, float *radiance, int on_device,
                               void *stream_) {
    ProbeLookup L;
    if (int rc = probe_lookup_check(grid, a, !a.pr || !a.maps || !positions || !normals || !dirs || !roughness || !radiance, false, L)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (device < 0) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (on_device && ((((uintptr_t)positions | (uintptr_t)normals | (uintptr_t)dirs | (uintptr_t)roughness | (uintptr_t)radiance | (uintptr_t)a.moments |
                        (uintptr_t)a.placement) & 3u) || ((uintptr_t)a.maps & 15u)))
        return fail(FW_ERR_BAD_ARG, "device maps must be 16-byte aligned, the other device arrays 4-byte aligned");
    if (int rc = probe_lookup_sizes(a, L)) return rc;
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Staged st(device, stream, on_device != 0);
    const ProbeTables t = probe_tables_stage(st, a, L);
    HostSlabs sl(st, n, 52);
    const int a_pts = sl.in(positions, 24, stride, normals), a_dir = sl.in(dirs, 12), a_rough = sl.in(roughness, 4), a_out = sl.out(radiance, 12);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) {
        const fw::DProbeVis v = probe_vis_device(a, st.ptr<const float>(t.mom));
        fw::launch_probe_radiance_lookup(stream, L.g, a.vis ? &v : nullptr, L.d, st.ptr<const float>(t.maps), st.ptr<const float>(t.pl), k,
                                         sl.ptr<const float>(a_pts), sl.with(a_pts), sl.stride(a_pts), sl.ptr<const float>(a_dir), sl.ptr<const float>(a_rough),
                                         sl.ptr<float>(a_out));
    });
}

// ---- SunSky: fw_check_sky, fw_sky_map, fw_sky_radiance, fw_sky_sun --------------------------------------------------------
int sky_check(const fw_sky *s) {
    if (!s) return fail(FW_ERR_BAD_ARG, "null argument");
    const float half_pi = 1.5707964f;                                                 // float(pi / 2): the largest elevation a float can ask for
    if (!(s->sun_elevation >= -half_pi && s->sun_elevation <= half_pi)) return fail(FW_ERR_BAD_ARG, "sun_elevation must be in [-pi/2, pi/2]");
    if (!std::isfinite(s->sun_azimuth)) return fail(FW_ERR_BAD_ARG, "sun_azimuth must be finite");
    if (!(s->turbidity >= 0.f && s->turbidity <= 64.f)) return fail(FW_ERR_BAD_ARG, "turbidity must be in [0, 64]");
    for (float v : {s->sun_irradiance.x, s->sun_irradiance.y, s->sun_irradiance.z})
        if (!(v >= 0.f && std::isfinite(v))) return fail(FW_ERR_BAD_ARG, "sun_irradiance must be finite and >= 0");
    if (!(s->sun_radius > 0.f && s->sun_radius <= 0.1f)) return fail(FW_ERR_BAD_ARG, "sun_radius must be in (0, 0.1]");
    if (!(s->altitude >= 1.f && s->altitude <= 50000.f)) return fail(FW_ERR_BAD_ARG, "altitude must be in [1, 50000]");
    for (float v : {s->ground_albedo.x, s->ground_albedo.y, s->ground_albedo.z})
        if (!(v >= 0.f && v <= 1.f)) return fail(FW_ERR_BAD_ARG, "ground_albedo must be in [0, 1]");
    if (s->view_steps < 1 || s->view_steps > 64) return fail(FW_ERR_BAD_ARG, "view_steps must be in 1..64");
    if (s->light_steps < 1 || s->light_steps > 32) return fail(FW_ERR_BAD_ARG, "light_steps must be in 1..32");
    if (s->sun_samples < 1 || s->sun_samples > 16) return fail(FW_ERR_BAD_ARG, "sun_samples must be in 1..16");
    if (s->flags & ~FW_SKY_DISC) return fail(FW_ERR_BAD_ARG, "flags has an unknown bit");
    return FW_OK;
}

// the sky as the kernels read it; `below`: the sun is under the observer's horizon (no disc, no light)
fw::DSky sky_device(const fw_sky *s, bool &below) {
    fw::DSky K{};
    const double el = (double)s->sun_elevation, az = (double)s->sun_azimuth, ce = std::cos(el);
    K.s[0] = ce * std::cos(az); K.s[1] = std::sin(el); K.s[2] = ce * std::sin(az);
    K.oy = fw::SKY_RG + (double)s->altitude;
    K.beta_r[0] = 5.8e-6; K.beta_r[1] = 13.5e-6; K.beta_r[2] = 33.1e-6;
    K.beta_m = 21e-6 * (double)s->turbidity; K.beta_me = 1.1 * K.beta_m;
    const double e0[3] = {s->sun_irradiance.x, s->sun_irradiance.y, s->sun_irradiance.z};
    const double al[3] = {s->ground_albedo.x, s->ground_albedo.y, s->ground_albedo.z};
    K.cos_sr = std::cos((double)s->sun_radius);
    K.nv = s->view_steps; K.nl = s->light_steps; K.ss = s->sun_samples; K.flags = s->flags;
    double T[3], b, disc;
    fw::sky_sun_transmittance(K, 0.0, K.oy, 0.0, T);
    below = fw::sky_ground(0.0, K.oy, 0.0, K.s[0], K.s[1], K.s[2], b, disc);
    for (int c = 0; c < 3; c++) {
        K.e0[c] = e0[c]; K.albedo_pi[c] = al[c] / fw::SKY_PI;
        K.et[c] = e0[c] * T[c];
        K.disc_l[c] = K.et[c] / ((2.0 * fw::SKY_PI) * (1.0 - K.cos_sr));
    }
    return K;
}

// the rows k_sky_sun visits, its rejection bound, and the texel the FW_ENV_HDR lookup reads for s (env_sample's float32 arithmetic)
fw::DSkyDisc sky_disc(const fw_sky *s, const fw::DSky &K, uint32_t W, uint32_t H) {
    fw::DSkyDisc D{};
    const double PI = fw::SKY_PI, el = (double)s->sun_elevation, reach = (double)s->sun_radius + PI / (double)H;
    const double top = (double)H * (0.5 - (el + reach) / PI) - 0.5, bottom = (double)H * (0.5 - (el - reach) / PI) - 0.5;
    D.row_lo = (uint32_t)std::min<double>(std::max(std::floor(top) - 1.0, 0.0), (double)H - 1.0);
    D.row_hi = (uint32_t)std::min<double>(std::max(std::ceil(bottom) + 1.0, 0.0), (double)H - 1.0);
    D.cos_reject = std::cos(std::min(PI, reach + 2.0 * PI / (double)W));
    const float dx = (float)K.s[0], dy = (float)K.s[1], dz = (float)K.s[2], pi_f = (float)PI, two_pi_f = (float)(2.0 * PI), half_pi_f = (float)(PI / 2.0);
    const float phi = std::atan2(dz, dx), theta = std::asin(std::min(std::max(dy, -1.f), 1.f));
    const float u = 1.f - (phi + pi_f) / two_pi_f, v = (theta + half_pi_f) / pi_f;
    const double x = std::floor((double)std::max(u * (float)W, 0.f)), y = std::floor((double)std::max((1.f - v) * (float)H, 0.f));
    const double idx = std::floor((double)((float)y * (float)W)) + x;
    D.fallback = (uint32_t)std::min(idx, (double)W * (double)H - 1.0);
    return D;
}

// fw_sky_map: fw_model_rays' shape — device output: the launches into the caller's memory; host output — host_slabs of rows
int sky_map_impl(const fw_sky *s, int device, uint32_t W, uint32_t H, float *rgb, int on_device, void *stream_) {
    if (!s || !rgb) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = sky_check(s)) return rc;
    if (W < 2 || H < 2) return fail(FW_ERR_BAD_ARG, "width and height must be >= 2");
    if (on_device && ((uintptr_t)rgb & 3u)) return fail(FW_ERR_BAD_ARG, "rgb must be 4-byte aligned");
    if ((uint64_t)W * H >= (1ull << 31)) return fail(FW_ERR_UNSUPPORTED, "W x H must be below 2^31");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    bool below = false;
    const fw::DSky K = sky_device(s, below);
    const fw::DSkyDisc D = sky_disc(s, K, W, H);
    const bool disc = (s->flags & FW_SKY_DISC) && !below;
    auto launch = [&](uint32_t first_row, uint32_t k, float *d_rgb) {
        fw::launch_sky_map(stream, n_cus, K, W, H, first_row, k, d_rgb);
        if (disc) fw::launch_sky_sun(stream, K, D, W, H, first_row, k, d_rgb);
    };
    if (on_device) {
        launch(0u, H, rgb);
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipGetLastError());
        return FW_OK;
    }
    return host_slabs(stream, device, H, (size_t)W * 12, rgb, launch);
}

// fw_sky_radiance: fw_ao_rays' shape — device arrays: one launch over the caller's memory; host arrays: slabs of directions, packed
int sky_radiance_impl(const fw_sky *s, int device, uint32_t n, const float *dirs, uint32_t stride, float *rgb, int on_device, void *stream_) {
    if (!s || !dirs || !rgb) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = sky_check(s)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (stride < 3) return fail(FW_ERR_BAD_ARG, "stride_floats must be >= 3");
    if (on_device && (((uintptr_t)dirs | (uintptr_t)rgb) & 3u)) return fail(FW_ERR_BAD_ARG, "device arrays must be 4-byte aligned");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    bool below = false;
    const fw::DSky K = sky_device(s, below);
    Staged st(device, stream, on_device != 0);
    HostSlabs sl(st, n, 24);
    const int a_dirs = sl.in(dirs, 12, stride), a_rgb = sl.out(rgb, 12);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) { fw::launch_sky_dirs(stream, n_cus, K, k, sl.ptr<const float>(a_dirs), sl.stride(a_dirs), sl.ptr<float>(a_rgb)); });
}

int sky_sun_impl(const fw_sky *s, fw_light *out) {
    if (!s || !out) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = sky_check(s)) return rc;
    bool below = false;
    const fw::DSky K = sky_device(s, below);
    *out = fw_light{};
    out->kind = FW_LIGHT_DIRECTIONAL;
    out->direction = fw_vec3{(float)-K.s[0], (float)-K.s[1], (float)-K.s[2]};
    out->intensity = fw_vec3{(float)K.et[0], (float)K.et[1], (float)K.et[2]};
    return FW_OK;
}

// ---- the GGX albedo table: fw_check_ggx_quad, fw_ggx_terms, fw_ggx_table, fw_ggx_table_lookup, fw_probe_shade_split -------
int ggx_quad_check(const fw_ggx_quad *q) {
    if (!q) return fail(FW_ERR_BAD_ARG, "null argument");
    if (q->m1 < 1 || q->m1 > fw::GGX_MAX_M) return fail(FW_ERR_BAD_ARG, "m1 must be in 1..1024");
    if (q->m2 < 1 || q->m2 > fw::GGX_MAX_M) return fail(FW_ERR_BAD_ARG, "m2 must be in 1..1024");
    return FW_OK;
}
int ggx_table_sizes(uint32_t n_mu, uint32_t n_rho) {
    if (n_mu < fw::GGX_MIN_N || n_mu > fw::GGX_MAX_N || n_rho < fw::GGX_MIN_N || n_rho > fw::GGX_MAX_N) return fail(FW_ERR_BAD_ARG, "n_mu and n_rho must be in 2..256");
    return FW_OK;
}

// fw_ggx_terms: fw_sky_radiance's shape — device arrays: one launch over the caller's memory; host arrays: slabs of pairs
int ggx_terms_impl(const fw_ggx_quad *q, int device, uint32_t n, const float *mu, const float *rho, float *terms, int on_device, void *stream_) {
    if (!q || !mu || !rho || !terms) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = ggx_quad_check(q)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((((uintptr_t)mu | (uintptr_t)rho) & 3u) || ((uintptr_t)terms & 7u)))
        return fail(FW_ERR_BAD_ARG, "device terms must be 8-byte aligned, device mu and rho 4-byte aligned");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    Staged st(device, stream, on_device != 0);
    HostSlabs sl(st, n, 16);
    const int a_mu = sl.in(mu, 4), a_rho = sl.in(rho, 4), a_out = sl.out(terms, 8);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) {
        fw::launch_ggx_terms(stream, n_cus, q->m1, q->m2, k, sl.ptr<const float>(a_mu), sl.ptr<const float>(a_rho), 0u, 0u, 0u, sl.ptr<float>(a_out));
    });
}

// fw_ggx_table: fw_sky_map's shape — device output: one launch into the caller's memory; host output: host_slabs of texels
int ggx_table_impl(const fw_ggx_quad *q, int device, uint32_t n_mu, uint32_t n_rho, float *table, int on_device, void *stream_) {
    if (!q || !table) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = ggx_quad_check(q)) return rc;
    if (int rc = ggx_table_sizes(n_mu, n_rho)) return rc;
    if (on_device && ((uintptr_t)table & 7u)) return fail(FW_ERR_BAD_ARG, "device table must be 8-byte aligned");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int n_cus = device_cus(device);
    auto launch = [&](uint32_t first, uint32_t k, float *d_terms) {
        fw::launch_ggx_terms(stream, n_cus, q->m1, q->m2, k, nullptr, nullptr, first, n_mu, n_rho, d_terms);
    };
    if (on_device) {
        launch(0u, n_mu * n_rho, table);
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipGetLastError());
        return FW_OK;
    }
    return host_slabs(stream, device, n_mu * n_rho, 8, table, launch);
}

// fw_ggx_table_lookup: fw_ggx_terms' shape with the table as a staged input
int ggx_table_lookup_impl(int device, uint32_t n_mu, uint32_t n_rho, const float *table, uint32_t n, const float *mu, const float *rho, float *terms,
                          int on_device, void *stream_) {
    if (!table || !mu || !rho || !terms) return fail(FW_ERR_BAD_ARG, "null argument");
    if (int rc = ggx_table_sizes(n_mu, n_rho)) return rc;
    if (n == 0) return fail(FW_ERR_BAD_ARG, "n must be > 0");
    if (on_device && ((((uintptr_t)mu | (uintptr_t)rho) & 3u) || (((uintptr_t)terms | (uintptr_t)table) & 7u)))
        return fail(FW_ERR_BAD_ARG, "device table and terms must be 8-byte aligned, device mu and rho 4-byte aligned");
    if (int rc = use_device(device)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Staged st(device, stream, on_device != 0);
    const int a_tab = st.add(Staged::IN, table, (size_t)n_mu * n_rho * 8);
    HostSlabs sl(st, n, 16);
    const int a_mu = sl.in(mu, 4), a_rho = sl.in(rho, 4), a_out = sl.out(terms, 8);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) {
        fw::launch_ggx_table_lookup(stream, n_mu, n_rho, st.ptr<const float>(a_tab), k, sl.ptr<const float>(a_mu), sl.ptr<const float>(a_rho), sl.ptr<float>(a_out));
    });
}

// fw_probe_shade_glossy (split false: Schlick's term; table, n_mu, n_rho and flags are not looked at) and fw_probe_shade_split (split true:
// the table is one more staged input): probe_shade_impl's shape; a host call's slab holds 48 B of record, 16 B of spec, 12 B of view and
// up to 27 B of outputs per pixel
int probe_shade_glossy_impl(const fw_probe_grid *grid, const ProbeLookupArgs &a, const fw_probe_shade_params *p, const float *aov, const float *spec,
                            const float *view, uint32_t view_stride, bool split, const float *table, uint32_t n_mu, uint32_t n_rho, uint32_t flags,
                            float *linear_rgb, float *gamma_rgb, uint8_t *rgb8) {
    ProbeLookup L;
    if (!split) table = nullptr;
    if (!grid || !a.sh || !a.pr || !a.maps || !p || !aov || !spec || !view || (split && !table) || (a.vis && (!a.pd || !a.moments)) ||
        (a.placed && !a.placement))
        return fail(FW_ERR_BAD_ARG, "null argument");
    if (split) {
        if (int rc = ggx_table_sizes(n_mu, n_rho)) return rc;
        if (flags & ~FW_SPLIT_ENERGY) return fail(FW_ERR_BAD_ARG, "flags has an unknown bit");
    }
    if (int rc = probe_lookup_check(grid, a, false, !linear_rgb && !gamma_rgb && !rgb8, L)) return rc;
    if (p->width == 0 || p->height == 0) return fail(FW_ERR_BAD_ARG, "width and height must be > 0");
    if (!std::isfinite(p->gamma) || !(p->gamma > 0.f)) return fail(FW_ERR_BAD_ARG, "gamma must be finite and > 0");
    if (view_stride < 3) return fail(FW_ERR_BAD_ARG, "view_stride_floats must be >= 3");
    if (p->device < 0) return fail(FW_ERR_BAD_ARG, "device index out of range");
    if (p->on_device && ((((uintptr_t)aov | (uintptr_t)spec | (uintptr_t)a.maps) & 15u) || ((uintptr_t)table & 7u) ||
                         (((uintptr_t)a.sh | (uintptr_t)view | (uintptr_t)linear_rgb | (uintptr_t)gamma_rgb | (uintptr_t)a.moments | (uintptr_t)a.placement) & 3u)))
        return fail(FW_ERR_BAD_ARG, split ? "device aov, spec and maps must be 16-byte aligned, device table 8-byte aligned, the other device arrays 4-byte aligned"
                                          : "device aov, spec and maps must be 16-byte aligned, the other device arrays 4-byte aligned");
    const uint64_t full = (uint64_t)p->width * p->height;
    if (int rc = probe_lookup_sizes(a, L)) return rc;
    if (full > 0xffffffffull) return fail(FW_ERR_UNSUPPORTED, "image too large");
    const int dev = p->device;
    if (int rc = use_device(dev)) return rc;
    hipStream_t stream = (hipStream_t)p->stream;
    Staged st(dev, stream, p->on_device != 0);
    const ProbeTables t = probe_tables_stage(st, a, L);
    const int a_tab = st.add(Staged::IN, table, split ? (size_t)n_mu * n_rho * 8 : 0);      // (no table: no slot, NULL)
    HostSlabs sl(st, (uint32_t)full, 103);
    const int a_aov = sl.in(aov, 48), a_spec = sl.in(spec, 16), a_view = sl.in(view, 12, view_stride);
    const int a_lin = sl.out(linear_rgb, 12), a_gam = sl.out(gamma_rgb, 12), a_8 = sl.out(rgb8, 3);
    if (int rc = st.up()) return rc;
    return sl.run([&](uint32_t, uint32_t k) {
        const fw::DProbeVis v = probe_vis_device(a, st.ptr<const float>(t.mom));
        const float *d_sh = st.ptr<const float>(t.sh), *d_maps = st.ptr<const float>(t.maps), *d_pl = st.ptr<const float>(t.pl);
        const float *d_aov = sl.ptr<const float>(a_aov), *d_spec = sl.ptr<const float>(a_spec), *d_view = sl.ptr<const float>(a_view);
        uint8_t *o8 = sl.ptr<uint8_t>(a_8);
        float *og = sl.ptr<float>(a_gam), *ol = sl.ptr<float>(a_lin);
        if (split) fw::launch_probe_split_shade(stream, L.g, a.vis ? &v : nullptr, L.d, d_sh, d_maps, d_pl, k, d_aov, d_spec, d_view, sl.stride(a_view),
                                                st.ptr<const float>(a_tab), n_mu, n_rho, flags, p->gamma, o8, og, ol);
        else fw::launch_probe_shade_glossy(stream, L.g, a.vis ? &v : nullptr, L.d, d_sh, d_maps, d_pl, k, d_aov, d_spec, d_view, sl.stride(a_view), p->gamma,
                                           o8, og, ol);
    });
}

} // namespace

// =========================================================================================================
extern "C" {

int fw_abi_version(void) { return FW_ABI_VERSION; }

const char *fw_strerror(int s) {
    switch (s) {
    case FW_OK: return "ok";
    case FW_ERR_BAD_ARG: return "bad argument";
    case FW_ERR_EMPTY_SCENE: return "No render objects added to scene!";
    case FW_ERR_NAN_BBOX: return "Float comparison failed in BVH constructor";
    case FW_ERR_MESH_NORMALS: return "TriangleMesh::new() -- normals.len() must equal verts.len()";
    case FW_ERR_MESH_UVS: return "TriangleMesh::new() -- uvs.len() must equal verts.len()";
    case FW_ERR_UNSUPPORTED: return "unsupported on the HIP path";
    case FW_ERR_HIP: return "HIP runtime error";
    case FW_ERR_NO_DEVICE: return "no HIP device (no CPU fallback exists)";
    case FW_ERR_BVH_DEPTH: return "BVH deeper than the traversal stack";
    case FW_ERR_OOM: return "out of memory";
    default: return "unknown error";
    }
}

const char *fw_last_error(void) { return g_last_error.c_str(); }

int fw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fw_selftest_arith(int device, uint32_t n, uint32_t seed, int mode, uint64_t *div_mismatches, uint64_t *sqrt_mismatches) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FW_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev || !div_mismatches || !sqrt_mismatches) return fail(FW_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(device));
    unsigned long long *d = nullptr, h[2] = {0, 0};
    HIPCHK(hipMalloc(&d, sizeof h));
    HIPCHK(hipMemset(d, 0, sizeof h));
    fw::launch_selftest_arith(nullptr, n, seed, mode, d);
    hipError_t e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(FW_ERR_HIP, hipGetErrorString(e));
    *div_mismatches = h[0]; *sqrt_mismatches = h[1];
    return FW_OK;
}

int fw_selftest_libm(int device, int fn, uint32_t n, const float *x, const float *y, float *out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FW_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev || fn < 0 || fn > 7 || !x || !out || n == 0 || ((fn == 6 || fn == 7) && !y)) return fail(FW_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(device));
    DevBuf dx, dy, dout;
    int rc = dx.alloc((size_t)n * 4);
    if (!rc && y) rc = dy.alloc((size_t)n * 4);
    if (!rc) rc = dout.alloc((size_t)n * 4);
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpy(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && y) e = hipMemcpy(dy.p, y, (size_t)n * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            fw::launch_selftest_libm(nullptr, fn, n, (const float *)dx.p, y ? (const float *)dy.p : nullptr, (float *)dout.p);
            e = hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost);
        }
    }
    dx.release(); dy.release(); dout.release();
    if (rc) return rc;
    if (e != hipSuccess) return fail(FW_ERR_HIP, hipGetErrorString(e));
    return FW_OK;
}

// n GgxMat vertices through the shade kernels' own device functions (k_ggx_test)
int fw_selftest_ggx(int device, uint32_t n, const float *in, float *out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FW_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev || !in || !out || n == 0 || n > (1u << 24)) return fail(FW_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(device));
    DevBuf din, dout;
    int rc = din.alloc((size_t)n * FW_GGX_IN_FLOATS * 4);
    if (!rc) rc = dout.alloc((size_t)n * FW_GGX_OUT_FLOATS * 4);
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpy(din.p, in, (size_t)n * FW_GGX_IN_FLOATS * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            fw::launch_ggx_test(nullptr, n, (const float *)din.p, (float *)dout.p);
            e = hipMemcpy(out, dout.p, (size_t)n * FW_GGX_OUT_FLOATS * 4, hipMemcpyDeviceToHost);
        }
    }
    din.release(); dout.release();
    if (rc) return rc;
    if (e != hipSuccess) return fail(FW_ERR_HIP, hipGetErrorString(e));
    return FW_OK;
}

int fw_set_option(const char *name, const char *value) {
    std::lock_guard<std::mutex> g(g_opt_mu);
    if (!name) { g_opt = options_from_env(); return FW_OK; }          // back to what the environment said
    const char *n = std::strncmp(name, "FIREWORK_", 9) == 0 ? name + 9 : name;
    if (!option_apply(g_opt, n, value)) {
        bool known = false;
        for (int k = 0; OPTION_NAMES[k] && !known; k++) known = std::strcmp(OPTION_NAMES[k], n) == 0;
        return fail(FW_ERR_BAD_ARG, std::string(known ? "bad value for option " : "unknown option ") + name);
    }
    return FW_OK;
}

// CPU-only diagnostic: the WIDE-node builder (wide_convert) on a caller's item boxes, its invariants checked on the finished tree
// (every item exactly once, every decoded child box a superset of the exact one, free slots unhittable, f32 item boxes bit for bit).
// boxes: n x 6 floats (min.xyz max.xyz); format: FW_WIDE_F32 (1) or FW_WIDE_Q8 (2); stats: nodes, leaves, free slots, depth.
int fw_selftest_wide_bvh(const float *boxes, uint32_t n, int format, uint32_t *violations, uint32_t stats[4]) {
    if (!boxes || n == 0 || !violations || !stats || (format != fw::WIDE_F32 && format != fw::WIDE_Q8)) return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        std::vector<Box> b(n);
        for (uint32_t i = 0; i < n; i++) b[i] = Box{{boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2]}, {boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5]}};
        FlatBvh sah; sah_build(sah, b);
        WideBvh w; w.fmt = format;
        const uint32_t root = wide_convert(sah, b, w);
        if (root == 0xffffffffu) return fail(FW_ERR_UNSUPPORTED, "tree not encodable as wide nodes (more than 32767 items or nodes, or a box that is not finite)");
        *violations = wide_check(w, root, b, stats);
        return FW_OK;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_selftest_wide_bvh"); }
}

// CPU-only diagnostic (ABI v7): the host builders — the reference's median-split tree (bvh.rs:21-71) and the binned-SAH tree that is walked —
// over n item boxes with `threads` host threads (1 = the sequential recursion); hashes[0..1] = FNV-1a of the two node arrays, stats = nodes and
// depth of each.  The parallel builds must reproduce the sequential ones bit for bit (tests/test_host_build_cpu.py).
int fw_selftest_lights(const fw_scene_desc *desc, float *out, uint32_t cap, uint32_t *n) {
    if (!desc || !n || (!out && cap > 0) || (desc->n_objects && !desc->objects) || (desc->n_shapes && !desc->shapes) || (desc->n_materials && !desc->materials))
        return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        const std::vector<LightRec> L = scene_lights(desc);
        *n = (uint32_t)L.size();
        for (uint32_t i = 0; i < cap && i < *n; i++) light_record_floats(L[i], out + (size_t)i * FW_LIGHT_RECORD_FLOATS);
        return FW_OK;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
}

// Diagnostics: the environment table of a caller's w x h RGB map built on GPU `device` as a render builds it, and n samples of it
// as k_shade_env draws them.  EnvTest holds the map (16-byte texels, as a scene uploads it) and the table.
struct EnvTest {
    DevBuf map, dist, p;          // p: the per-texel probabilities (with_p)
    fw::DEnv env{}; double total = 0;
    int make(int device, const float *rgb, uint32_t w, uint32_t h, bool with_p) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(FW_ERR_NO_DEVICE, "no HIP device visible"); }
        if (device >= ndev) return fail(FW_ERR_BAD_ARG, "device index out of range");
        HIPCHK(hipSetDevice(device));
        const size_t n = (size_t)w * h;
        std::vector<float> px(n * 4, 0.f);
        for (size_t k = 0; k < n; k++) { px[4 * k] = rgb[3 * k]; px[4 * k + 1] = rgb[3 * k + 1]; px[4 * k + 2] = rgb[3 * k + 2]; }
        if (int rc = map.upload(px.data(), px.size() * 4)) return rc;
        if (with_p) if (int rc = p.alloc(n * 4)) return rc;
        env.kind = FW_ENV_HDR; env.hdr = (const float *)map.p; env.hdr_w = w; env.hdr_h = h;
        return build_env_table(env, dist, with_p ? (float *)p.p : nullptr, total);
    }
    ~EnvTest() { map.release(); dist.release(); p.release(); }
};
static bool env_test_args(int device, const float *rgb, uint32_t w, uint32_t h) {
    return device >= 0 && rgb && w > 0 && h > 0 && (uint64_t)w * h <= (1ull << 24);
}
int fw_selftest_env_dist(int device, const float *rgb, uint32_t w, uint32_t h, float *p, double *total) {
    if (!env_test_args(device, rgb, w, h) || !p || !total) return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        EnvTest t;
        if (int rc = t.make(device, rgb, w, h, true)) return rc;
        if (hipMemcpy(p, t.p.p, (size_t)w * h * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(FW_ERR_HIP, "copy failed");
        *total = t.total;
        return FW_OK;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
}
int fw_selftest_env_sample(int device, const float *rgb, uint32_t w, uint32_t h, uint32_t n, uint32_t seed, float *out) {
    if (!env_test_args(device, rgb, w, h) || n == 0 || n > (1u << 26) || !out) return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        EnvTest t;
        if (int rc = t.make(device, rgb, w, h, false)) return rc;
        if (!(t.total > 0)) return fail(FW_ERR_BAD_ARG, "the map has no positive weight");
        DevBuf o;
        if (int rc = o.alloc((size_t)n * FW_ENV_SAMPLE_FLOATS * 4)) return rc;
        fw::launch_env_sample_test(nullptr, t.env, env_dist_of(t.dist, t.env, 1.f), n, seed, (float *)o.p);
        int rc = FW_OK;
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, o.p, (size_t)n * FW_ENV_SAMPLE_FLOATS * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FW_ERR_HIP, "sampling failed");
        o.release();
        return rc;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
}

// Diagnostic: the entries of a description, their areas in float64 (a mesh's triangles from its vertices) and weights
int fw_selftest_emitters(const fw_scene_desc *desc, float *out, uint32_t cap, uint32_t *n) {
    if (!desc || !n || (!out && cap > 0)) return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        uint64_t total = 0;
        const std::vector<EmitterObj> E = scene_emitters(desc, total);
        *n = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
        uint64_t i = 0;
        for (const EmitterObj &e : E) {
            const fw_shape &s = desc->shapes[desc->objects[e.obj].shape];
            const double power = emitter_power(desc, desc->materials[s.material]);
            double area[6] = {0, 0, 0, 0, 0, 0};
            if (e.kind != FW_SHAPE_TRIANGLE_MESH) emitter_areas(s, area);
            for (uint32_t k = 0; k < e.count && i < cap; k++, i++) {
                double a = area[e.kind == FW_SHAPE_TRIANGLE_MESH ? 0 : k];
                if (e.kind == FW_SHAPE_TRIANGLE_MESH) {
                    double v[3][3];
                    for (int c = 0; c < 3; c++) { const uint32_t vi = s.indices[3 * k + c]; for (int j = 0; j < 3; j++) v[c][j] = vi < s.n_verts ? (double)s.verts[3 * vi + j] : 0.0; }
                    const double e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]}, e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
                    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
                    a = 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
                }
                float *r = out + (size_t)i * FW_EMITTER_RECORD_FLOATS;
                r[0] = (float)e.obj; r[1] = (float)k; r[2] = (float)e.kind; r[3] = (float)a; r[4] = (float)emitter_weight(a * power);
            }
        }
        return FW_OK;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
}
int fw_selftest_emitter_sample(fw_scene *sc, const float *x, uint32_t n, uint32_t seed, float *out) {
    if (!sc || !x || n == 0 || n > (1u << 26) || !out) return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        HIPCHK(hipSetDevice(sc->device));
        Workspace *ws = workspace_for(sc->device);
        if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
        std::lock_guard<std::mutex> ws_guard(ws->mu);
        if (int rc = init_device_locked(ws, sc->device)) return rc;
        if (sc->n_entries > fw::EMITTER_MAX_ENTRIES) return fail(FW_ERR_UNSUPPORTED, "more than 2^26 emitter entries");
        if (sc->emit_state == 0) {
            if (sc->n_entries == 0) sc->emit_state = 2;
            else if (int rc = build_emitter_table(sc, ws->ev_upload)) return rc;
        }
        if (sc->emit_state != 1) return fail(FW_ERR_UNSUPPORTED, "no emitter entry of positive weight");
        DevBuf o;
        if (int rc = o.alloc((size_t)n * FW_EMITTER_SAMPLE_FLOATS * 4)) return rc;
        fw::launch_emitter_sample_test(nullptr, sc->d, emitters_of(sc, 0.f), x[0], x[1], x[2], n, seed, (float *)o.p);
        int rc = FW_OK;
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, o.p, (size_t)n * FW_EMITTER_SAMPLE_FLOATS * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FW_ERR_HIP, "sampling failed");
        o.release();
        return rc;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
}

int fw_selftest_bvh_build(const float *boxes, uint32_t n, int threads, uint64_t hashes[2], uint32_t stats[4]) {
    if (!boxes || n == 0 || threads < 1 || !hashes || !stats) return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        std::vector<Box> b(n);
        for (uint32_t i = 0; i < n; i++) b[i] = Box{{boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2]}, {boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5]}};
        auto fnv = [](const std::vector<float> &v) { uint64_t h = 1469598103934665603ull; const uint8_t *p = (const uint8_t *)v.data(); for (size_t i = 0; i < v.size() * 4; i++) { h ^= p[i]; h *= 1099511628211ull; } return h; };
        FlatBvh ref, sah;
        { BuildPool pool(threads - 1); try { (void)bvh_build(ref, b, &pool); } catch (NanError &) { return fail(FW_ERR_NAN_BBOX, "Float comparison failed in BVH constructor"); } }
        { BuildPool pool(threads - 1); sah_build(sah, b, &pool); }
        hashes[0] = fnv(ref.nodes); hashes[1] = fnv(sah.nodes);
        stats[0] = ref.count(); stats[1] = ref.depth; stats[2] = sah.count(); stats[3] = sah.depth;
        return FW_OK;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_selftest_bvh_build"); }
}

// Diagnostic: both trees over n item boxes, built on GPU `device` (fw_build.hip) or, for device = -1, by the host builders; the node arrays
// (8 floats per node, up to 2n - 1 nodes each) are written to ref_nodes / sah_nodes, stats = nodes and depth of each.  The device build
// must equal the host's bit for bit (tests/test_gpu_device_build.py).
int fw_selftest_bvh_trees(int device, const float *boxes, uint32_t n, float *ref_nodes, float *sah_nodes, uint32_t stats[4]) {
    if (!boxes || n == 0 || !ref_nodes || !sah_nodes || !stats || device < -1 || n > fw::NODE_MASK) return fail(FW_ERR_BAD_ARG, "bad argument");
    try {
        FlatBvh ref, sah;
        if (device >= 0) {
            int ndev = 0;
            if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(FW_ERR_NO_DEVICE, "no HIP device visible"); }
            if (device >= ndev) return fail(FW_ERR_BAD_ARG, "device index out of range");
            HIPCHK(hipSetDevice(device));
            std::string msg;
            int rc = fw::device_build_tree(device, fw::BUILD_MEDIAN, boxes, n, ref.nodes, ref.depth, nullptr, msg);
            if (!rc) rc = fw::device_build_tree(device, fw::BUILD_SAH, boxes, n, sah.nodes, sah.depth, nullptr, msg);
            if (rc) return fail(rc, msg);
        } else {
            std::vector<Box> b(n);
            for (uint32_t i = 0; i < n; i++) b[i] = Box{{boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2]}, {boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5]}};
            if (int rc = build_tree(-1, fw::BUILD_MEDIAN, b, ref, nullptr, nullptr)) return rc;
            if (int rc = build_tree(-1, fw::BUILD_SAH, b, sah, nullptr, nullptr)) return rc;
        }
        if (ref.count() > 2 * (size_t)n - 1 || sah.count() > 2 * (size_t)n - 1) return fail(FW_ERR_HIP, "tree larger than 2n - 1 nodes");
        std::memcpy(ref_nodes, ref.nodes.data(), ref.nodes.size() * 4);
        std::memcpy(sah_nodes, sah.nodes.data(), sah.nodes.size() * 4);
        stats[0] = ref.count(); stats[1] = ref.depth; stats[2] = sah.count(); stats[3] = sah.depth;
        return FW_OK;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_selftest_bvh_trees"); }
}

#if FW_AB
int fw_debug_ab(void) { return 1; }      // present only in the A/B build: tests of the alternative kernels look for it
#endif

int fw_debug_kernels(int device, char *buf, uint32_t cap) {
    try {
        if (device < -1 || device >= MAX_DEVICES) return fail(FW_ERR_BAD_ARG, "fw_debug_kernels: device out of range");
        if (!buf && cap > 0) return fail(FW_ERR_BAD_ARG, "fw_debug_kernels: null buffer with cap > 0");
        std::vector<std::string> names;
        if (device < 0) for (uint32_t i = 0; i < fw::KID_COUNT; i++) names.push_back(fw::KERNEL_NAMES[i]);
        else {
            Workspace *ws = workspace_for(device);
            if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
            fw::KernelLog log;
            { std::lock_guard<std::mutex> g(ws->mu); log = ws->kernels; }
            for (uint32_t i = 0; i < fw::KID_COUNT; i++) {
                if (!log.has(i)) continue;
                if (fw::KERNEL_FAMILY[i] < 0) { names.push_back(fw::KERNEL_NAMES[i]); continue; }
                const uint32_t waves[3] = {16u, 12u, 8u};
                for (int b = 0; b < 3; b++) if (log.waves[i] & (1u << b)) names.push_back(std::string(fw::KERNEL_NAMES[i]) + "@" + std::to_string(waves[b]));
            }
            // a fused launch (FUSE_SEGMENTS): beside the two kernels whose text it ran, its own name.  Names of a call only: the table of
            // device -1 lists kernel texts, and this one has none of its own
            for (int b = 0; b < 4; b++) if (log.fused & (1u << b)) names.push_back(fw::FUSED_KERNEL_NAMES[b]);
        }
        std::sort(names.begin(), names.end());
        std::string all;
        for (const std::string &n : names) { if (!all.empty()) all += ','; all += n; }
        if (cap > 0) { const size_t k = std::min<size_t>(all.size(), (size_t)cap - 1); std::memcpy(buf, all.data(), k); buf[k] = 0; }
        return (int)all.size();
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_debug_kernels"); }
}

int fw_init(int device, uint64_t arena_bytes) {
    try {
        if (int rc = use_device(device)) return rc;
        Workspace *ws = workspace_for(device);
        if (!ws) return fail(FW_ERR_OOM, "no workspace for this device");
        std::lock_guard<std::mutex> g(ws->mu);
        int rc = init_device_locked(ws, device);
        if (rc) return rc;
        size_t want = arena_bytes == FW_INIT_NO_ARENA ? 0 : (arena_bytes ? (size_t)arena_bytes : default_arena_bytes(ws));
        want = (want + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
        if (want > ws->arena.bytes) {
            const auto ta = std::chrono::steady_clock::now();
            rc = arena_reserve_locked(ws, device, want);
            if (options().trace) fprintf(stderr, "[firework] fw_init: path arena of %.1f GiB in %.2f ms\n", (double)want / (double)(1 << 30),
                                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count());
        }
        return rc;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_init"); }
}

int fw_scene_create(const fw_scene_desc *desc, int device, fw_scene **out) {
    try { return create_scene_impl(desc, device, out); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_scene_create"); }
}

int fw_scene_update(fw_scene *scene, const fw_scene_desc *desc) {
    try { return update_scene_impl(scene, desc); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_scene_update"); }
}

int fw_scene_set_lights(fw_scene *scene, const fw_light *lights, uint32_t n) {
    try { return set_lights_impl(scene, lights, n); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_scene_set_lights"); }
}

int fw_check_lights(const fw_light *lights, uint32_t n) {
    try { return check_lights_impl(lights, n); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_check_lights"); }
}

void fw_release_workspace(int device) {
    Workspace *ws = workspace_for(device);
    if (!ws) return;
    std::lock_guard<std::mutex> g(ws->mu);
    if (hipSetDevice(device) == hipSuccess) { ws->release(); fw::device_build_release(device); }
}

void fw_scene_destroy(fw_scene *scene) {
    if (!scene) return;
    (void)hipSetDevice(scene->device);
    if (Workspace *ws = workspace_for(scene->device)) {   // keep the allocation for the next scene (one-shot renders)
        std::lock_guard<std::mutex> g(ws->mu);
        if (scene->data.p && scene->data.bytes > ws->scene_cache.bytes) { ws->scene_cache.release(); ws->scene_cache = scene->data; scene->data = DevBuf{}; }
    }
    delete scene;
}

int fw_render(fw_scene *scene, const fw_render_params *params, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats) {
    try { return render_impl(scene, params, rgb8, gamma_rgb, linear_rgb, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render"); }
}

int fw_trace_rays(fw_scene *scene, const fw_trace_params *params, const float *rays, uint32_t n_rays, fw_hit *hits, fw_stats *stats) {
    try { return trace_impl(scene, params, rays, n_rays, hits, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_trace_rays"); }
}

int fw_camera_rays(const fw_render_params *params, int device, uint32_t sample, float *rays) {
    try { return camera_rays_impl(params, device, sample, rays); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_camera_rays"); }
}

int fw_render_aovs(fw_scene *scene, const fw_render_params *params, float *aov, fw_stats *stats) {
    try { return aovs_impl(scene, params, aov, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_aovs"); }
}

int fw_model_rays(const fw_camera_model *model, int device, uint32_t first_sample, uint32_t n_samples, float *rays, int on_device, void *stream) {
    try { return model_rays_impl(model, device, first_sample, n_samples, rays, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_model_rays"); }
}

int fw_render_model(fw_scene *scene, const fw_camera_model *model, const fw_render_rays_params *rp, float *accum, uint8_t *rgb8,
                    float *gamma_rgb, float *linear_rgb, fw_stats *stats) {
    try { return render_model_impl(scene, model, rp, accum, rgb8, gamma_rgb, linear_rgb, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_model"); }
}

int fw_render_model_aovs(fw_scene *scene, const fw_camera_model *model, const fw_render_params *params, float *aov, fw_stats *stats) {
    try { return model_aovs_impl(scene, model, params, aov, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_model_aovs"); }
}

int fw_probe_rays(const fw_probe_set *set, int device, uint32_t round, uint32_t first_probe, uint32_t n, float *rays, int on_device, void *stream) {
    try { return probe_rays_impl(set, device, round, first_probe, n, rays, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_rays"); }
}

int fw_probe_project(int device, uint32_t n_probes, uint32_t directions, uint32_t samples, const float *rays, const float *accum, float *sums,
                     int on_device, void *stream) {
    try { return probe_project_impl(device, n_probes, directions, samples, rays, accum, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_project"); }
}

int fw_bake_probes(fw_scene *scene, const fw_probe_set *set, const fw_render_rays_params *rp, uint32_t first_round, uint32_t rounds, float *sums,
                   float *sh, fw_stats *stats) {
    try { return bake_probes_impl(scene, set, rp, first_round, rounds, sums, sh, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_probes"); }
}

int fw_probe_irradiance(const fw_probe_grid *grid, const float *sh, int device, uint32_t n, const float *positions, const float *normals,
                        uint32_t stride_floats, float *irradiance, int on_device, void *stream) {
    try { return probe_irradiance_impl(grid, ProbeLookupArgs{sh}, device, n, positions, normals, stride_floats, irradiance, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_irradiance"); }
}

int fw_probe_shade(const fw_probe_grid *grid, const float *sh, const fw_probe_shade_params *p, const float *aov, float *linear_rgb,
                   float *gamma_rgb, uint8_t *rgb8) {
    try { return probe_shade_impl(grid, ProbeLookupArgs{sh}, p, aov, linear_rgb, gamma_rgb, rgb8); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_shade"); }
}

int fw_probe_depth_reduce(int device, const fw_probe_depth *pd, uint32_t n_probes, uint32_t directions, const float *rays, const fw_hit *hits,
                          float *sums, int on_device, void *stream) {
    try { return probe_depth_reduce_impl(device, pd, n_probes, directions, rays, hits, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_depth_reduce"); }
}

int fw_bake_probe_depth(fw_scene *scene, const fw_probe_set *set, const fw_probe_depth *pd, const fw_trace_params *tp, uint32_t first_round,
                        uint32_t rounds, float *sums, float *moments, fw_stats *stats) {
    try { return bake_probe_depth_impl(scene, set, pd, tp, first_round, rounds, sums, moments, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_probe_depth"); }
}

int fw_ao_rays(const fw_ao *ao, int device, uint32_t round, uint32_t n, const float *positions, const float *normals, uint32_t stride_floats,
               const uint32_t *ids, float *rays, int on_device, void *stream) {
    try { return ao_rays_impl(ao, device, round, n, positions, normals, stride_floats, ids, rays, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_ao_rays"); }
}

int fw_ao_reduce(int device, const fw_ao *ao, uint32_t n, const uint32_t *ids, const float *rays, const fw_hit *hits, float *sums, int on_device,
                 void *stream) {
    try { return ao_reduce_impl(device, ao, n, ids, rays, hits, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_ao_reduce"); }
}

int fw_bake_ao(fw_scene *scene, const fw_ao *ao, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
               uint32_t stride_floats, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    try { return bake_ao_impl(scene, ao, tp, n, positions, normals, stride_floats, ids, first_round, rounds, sums, out, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_ao"); }
}

int fw_direct_rays(const fw_direct *direct, const fw_light *lights, uint32_t n_lights, int device, uint32_t n, const float *positions,
                   const float *normals, uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats,
                   const float *spec, float *rays, int on_device, void *stream) {
    try { return direct_rays_impl(direct, lights, n_lights, device, n, positions, normals, stride_floats, ids, view, view_stride_floats, spec, rays, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_direct_rays"); }
}

int fw_direct_reduce(int device, const fw_direct *direct, const fw_light *lights, uint32_t n_lights, uint32_t n, const float *positions,
                     const float *normals, uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats,
                     const float *spec, const float *rays, const fw_hit *hits, float *sums, int on_device, void *stream) {
    try {
        return direct_reduce_impl(device, direct, lights, n_lights, n, positions, normals, stride_floats, ids, view, view_stride_floats, spec, rays, hits, sums,
                                  on_device, stream);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_direct_reduce"); }
}

int fw_bake_direct(fw_scene *scene, const fw_direct *direct, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
                   uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats, const float *spec,
                   uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    try { return bake_direct_impl(scene, direct, tp, n, positions, normals, stride_floats, ids, view, view_stride_floats, spec, first_round, rounds, sums, out, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_direct"); }
}

int fw_hit_surface(fw_scene *scene, const float *rays, const fw_hit *hits, uint32_t n, float *surface, int on_device, void *stream) {
    try { return hit_surface_impl(scene, rays, hits, n, surface, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_hit_surface"); }
}

int fw_gather_reduce(int device, uint32_t directions, uint32_t n, const uint32_t *ids, const float *surface, const float *irradiance,
                     const float *direct, float *sums, int on_device, void *stream) {
    try { return gather_reduce_impl(device, directions, n, ids, surface, irradiance, direct, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_gather_reduce"); }
}

int fw_bake_gather(fw_scene *scene, const fw_gather *g, const fw_trace_params *tp, const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd,
                   const float *moments, float normal_bias, const float *placement, uint32_t n, const float *positions, const float *normals,
                   uint32_t stride_floats, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    try {
        return bake_gather_impl(scene, g, tp, grid, sh, pd, moments, normal_bias, placement, n, positions, normals, stride_floats, ids, first_round, rounds,
                                sums, out, stats);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_gather"); }
}

int fw_scene_area_lights(fw_scene *scene, float *out, uint32_t cap, uint32_t *n) {
    try { return scene_area_lights_impl(scene, out, cap, n); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_scene_area_lights"); }
}

int fw_area_rays(const fw_area *area, const float *lights, uint32_t n_lights, int device, uint32_t round, uint32_t n, const float *positions,
                 const float *normals, uint32_t stride_floats, const uint32_t *ids, float *rays, float *weights, int on_device, void *stream) {
    try { return area_rays_impl(area, lights, n_lights, device, round, n, positions, normals, stride_floats, ids, rays, weights, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_area_rays"); }
}

int fw_area_reduce(int device, uint32_t samples, const uint32_t *objects, uint32_t n_objects, uint32_t n, const uint32_t *ids, const float *weights,
                   const fw_hit *hits, const float *surface, float *sums, int on_device, void *stream) {
    try { return area_reduce_impl(device, samples, objects, n_objects, n, ids, weights, hits, surface, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_area_reduce"); }
}

int fw_area_mask(int device, const uint32_t *objects, uint32_t n_objects, uint32_t n, const fw_hit *hits, float *surface, int on_device, void *stream) {
    try { return area_mask_impl(device, objects, n_objects, n, hits, surface, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_area_mask"); }
}

int fw_bake_area(fw_scene *scene, const fw_area *area, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
                 uint32_t stride_floats, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    try { return bake_area_impl(scene, area, tp, n, positions, normals, stride_floats, ids, first_round, rounds, sums, out, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_area"); }
}

int fw_selftest_emitters_records(const fw_scene_desc *desc, float *records, uint32_t *codes, uint32_t cap, uint32_t *n) {
    try { return selftest_emitters_records_impl(desc, records, codes, cap, n); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_selftest_emitters_records"); }
}

int fw_scene_emitters(fw_scene *scene, float *records, uint32_t *codes, uint32_t cap, uint32_t *n) {
    try { return scene_emitters_impl(scene, records, codes, cap, n); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_scene_emitters"); }
}

int fw_emitters_cdf(const float *weights, uint32_t n, double *cdf, double *total) {
    try { return emitters_cdf_impl(weights, n, cdf, total); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_emitters_cdf"); }
}

int fw_emitters_rays(const fw_emitters *emitters, const float *records, const double *cdf, uint32_t n_entries, int device, uint32_t round, uint32_t n,
                     const float *positions, const float *normals, uint32_t stride_floats, const uint32_t *ids, float *rays, float *weights,
                     uint32_t *picks, int on_device, void *stream) {
    try { return emitters_rays_impl(emitters, records, cdf, n_entries, device, round, n, positions, normals, stride_floats, ids, rays, weights, picks, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_emitters_rays"); }
}

int fw_emitters_reduce(int device, uint32_t samples, const uint32_t *codes, uint32_t n_entries, uint32_t n, const uint32_t *ids, const uint32_t *picks,
                       const float *weights, const fw_hit *hits, const float *surface, float *sums, int on_device, void *stream) {
    try { return emitters_reduce_impl(device, samples, codes, n_entries, n, ids, picks, weights, hits, surface, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_emitters_reduce"); }
}

int fw_bake_emitters(fw_scene *scene, const fw_emitters *emitters, const fw_trace_params *tp, uint32_t n, const float *positions, const float *normals,
                     uint32_t stride_floats, const uint32_t *ids, uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    try { return bake_emitters_impl(scene, emitters, tp, n, positions, normals, stride_floats, ids, first_round, rounds, sums, out, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_emitters"); }
}

int fw_reflect_rays(const fw_reflect *reflect, int device, uint32_t round, uint32_t n, const float *positions, const float *normals,
                    uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats, const float *spec, float *rays,
                    float *weights, int on_device, void *stream) {
    try { return reflect_rays_impl(reflect, device, round, n, positions, normals, stride_floats, ids, view, view_stride_floats, spec, rays, weights, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_reflect_rays"); }
}

int fw_reflect_reduce(int device, uint32_t directions, uint32_t n, const uint32_t *ids, const float *surface, const float *irradiance,
                      const float *direct, const float *weights, float *sums, int on_device, void *stream) {
    try { return reflect_reduce_impl(device, directions, n, ids, surface, irradiance, direct, weights, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_reflect_reduce"); }
}

int fw_bake_reflect(fw_scene *scene, const fw_reflect *reflect, const fw_trace_params *tp, const fw_probe_grid *grid, const float *sh,
                    const fw_probe_depth *pd, const float *moments, float normal_bias, const float *placement, uint32_t n, const float *positions,
                    const float *normals, uint32_t stride_floats, const uint32_t *ids, const float *view, uint32_t view_stride_floats, const float *spec,
                    uint32_t first_round, uint32_t rounds, float *sums, float *out, fw_stats *stats) {
    try {
        return bake_reflect_impl(scene, reflect, tp, grid, sh, pd, moments, normal_bias, placement, n, positions, normals, stride_floats, ids, view,
                                 view_stride_floats, spec, first_round, rounds, sums, out, stats);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_reflect"); }
}

int fw_check_sky(const fw_sky *sky) {
    try { return sky_check(sky); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_check_sky"); }
}

int fw_sky_map(const fw_sky *sky, int device, uint32_t width, uint32_t height, float *rgb, int on_device, void *stream) {
    try { return sky_map_impl(sky, device, width, height, rgb, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_sky_map"); }
}

int fw_sky_radiance(const fw_sky *sky, int device, uint32_t n, const float *dirs, uint32_t stride_floats, float *rgb, int on_device, void *stream) {
    try { return sky_radiance_impl(sky, device, n, dirs, stride_floats, rgb, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_sky_radiance"); }
}

int fw_sky_sun(const fw_sky *sky, fw_light *out) {
    try { return sky_sun_impl(sky, out); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_sky_sun"); }
}

int fw_check_ggx_quad(const fw_ggx_quad *quad) {
    try { return ggx_quad_check(quad); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_check_ggx_quad"); }
}

int fw_ggx_terms(const fw_ggx_quad *quad, int device, uint32_t n, const float *mu, const float *rho, float *terms, int on_device, void *stream) {
    try { return ggx_terms_impl(quad, device, n, mu, rho, terms, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_ggx_terms"); }
}

int fw_ggx_table(const fw_ggx_quad *quad, int device, uint32_t n_mu, uint32_t n_rho, float *table, int on_device, void *stream) {
    try { return ggx_table_impl(quad, device, n_mu, n_rho, table, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_ggx_table"); }
}

int fw_ggx_table_lookup(int device, uint32_t n_mu, uint32_t n_rho, const float *table, uint32_t n, const float *mu, const float *rho, float *terms,
                        int on_device, void *stream) {
    try { return ggx_table_lookup_impl(device, n_mu, n_rho, table, n, mu, rho, terms, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_ggx_table_lookup"); }
}

int fw_probe_shade_split(const fw_probe_grid *grid, const float *sh, const fw_probe_radiance *pr, const float *maps, const fw_probe_depth *pd,
                         const float *moments, float normal_bias, const float *placement, const fw_probe_shade_params *p, const float *aov,
                         const float *spec, const float *view, uint32_t view_stride_floats, const float *table, uint32_t n_mu, uint32_t n_rho,
                         uint32_t flags, float *linear_rgb, float *gamma_rgb, uint8_t *rgb8) {
    try {
        const ProbeLookupArgs a{sh, pr, maps, pd, moments, normal_bias, placement, pd || moments, placement != nullptr};
        return probe_shade_glossy_impl(grid, a, p, aov, spec, view, view_stride_floats, true, table, n_mu, n_rho, flags, linear_rgb, gamma_rgb, rgb8);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_shade_split"); }
}

int fw_probe_irradiance_vis(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias, int device,
                            uint32_t n, const float *positions, const float *normals, uint32_t stride_floats, float *irradiance, int on_device,
                            void *stream) {
    try {
        const ProbeLookupArgs a{sh, nullptr, nullptr, pd, moments, normal_bias, nullptr, true, false};
        return probe_irradiance_impl(grid, a, device, n, positions, normals, stride_floats, irradiance, on_device, stream);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_irradiance_vis"); }
}

int fw_probe_shade_vis(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias,
                       const fw_probe_shade_params *p, const float *aov, float *linear_rgb, float *gamma_rgb, uint8_t *rgb8) {
    try {
        const ProbeLookupArgs a{sh, nullptr, nullptr, pd, moments, normal_bias, nullptr, true, false};
        return probe_shade_impl(grid, a, p, aov, linear_rgb, gamma_rgb, rgb8);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_shade_vis"); }
}

int fw_probe_survey(int device, uint32_t n_probes, uint32_t directions, const float *rays, const fw_hit *hits, float *survey, int on_device,
                    void *stream) {
    try { return probe_survey_impl(device, n_probes, directions, rays, hits, survey, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_survey"); }
}

int fw_probe_relocate_step(int device, const fw_probe_relocate *rl, uint32_t n_probes, uint32_t directions, const float *survey, float *placement,
                           int move, int on_device, void *stream) {
    try { return probe_relocate_step_impl(device, rl, n_probes, directions, survey, placement, move, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_relocate_step"); }
}

int fw_relocate_probes(fw_scene *scene, const fw_probe_set *set, const fw_probe_relocate *rl, const fw_trace_params *tp, uint32_t first_step,
                       uint32_t steps, float *placement, float *survey, fw_stats *stats) {
    try { return relocate_probes_impl(scene, set, rl, tp, first_step, steps, placement, survey, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_relocate_probes"); }
}

// pd and moments both NULL: a placed lookup without visibility; one of them NULL is the counterpart's null argument
int fw_probe_irradiance_placed(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias,
                               const float *placement, int device, uint32_t n, const float *positions, const float *normals, uint32_t stride_floats,
                               float *irradiance, int on_device, void *stream) {
    try {
        const ProbeLookupArgs a{sh, nullptr, nullptr, pd, moments, normal_bias, placement, pd || moments, true};
        return probe_irradiance_impl(grid, a, device, n, positions, normals, stride_floats, irradiance, on_device, stream);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_irradiance_placed"); }
}

int fw_probe_shade_placed(const fw_probe_grid *grid, const float *sh, const fw_probe_depth *pd, const float *moments, float normal_bias,
                          const float *placement, const fw_probe_shade_params *p, const float *aov, float *linear_rgb, float *gamma_rgb,
                          uint8_t *rgb8) {
    try {
        const ProbeLookupArgs a{sh, nullptr, nullptr, pd, moments, normal_bias, placement, pd || moments, true};
        return probe_shade_impl(grid, a, p, aov, linear_rgb, gamma_rgb, rgb8);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_shade_placed"); }
}

int fw_probe_radiance_reduce(int device, const fw_probe_radiance *pr, uint32_t n_probes, uint32_t directions, uint32_t samples, const float *rays,
                             const float *accum, float *sums, int on_device, void *stream) {
    try { return probe_radiance_reduce_impl(device, pr, n_probes, directions, samples, rays, accum, sums, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_radiance_reduce"); }
}

int fw_probe_radiance_prefilter(int device, const fw_probe_radiance *pr, uint32_t n_probes, const float *sums, float *maps, int on_device,
                                void *stream) {
    try { return probe_radiance_prefilter_impl(device, pr, n_probes, sums, maps, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_radiance_prefilter"); }
}

int fw_bake_probe_radiance(fw_scene *scene, const fw_probe_set *set, const fw_probe_radiance *pr, const fw_render_rays_params *rp,
                           uint32_t first_round, uint32_t rounds, float *sums, float *maps, float *sh_sums, float *sh, fw_stats *stats) {
    try { return bake_probe_radiance_impl(scene, set, pr, rp, first_round, rounds, sums, maps, sh_sums, sh, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_probe_radiance"); }
}

int fw_probe_radiance_lookup(const fw_probe_grid *grid, const fw_probe_radiance *pr, const float *maps, const fw_probe_depth *pd, const float *moments,
                             float normal_bias, const float *placement, int device, uint32_t n, const float *positions, const float *normals,
                             uint32_t stride_floats, const float *dirs, const float *roughness, float *radiance, int on_device, void *stream) {
    try {
        const ProbeLookupArgs a{nullptr, pr, maps, pd, moments, normal_bias, placement, pd || moments, placement != nullptr};
        return probe_radiance_lookup_impl(grid, a, device, n, positions, normals, stride_floats, dirs, roughness, radiance, on_device, stream);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_radiance_lookup"); }
}

int fw_probe_shade_glossy(const fw_probe_grid *grid, const float *sh, const fw_probe_radiance *pr, const float *maps, const fw_probe_depth *pd,
                          const float *moments, float normal_bias, const float *placement, const fw_probe_shade_params *p, const float *aov,
                          const float *spec, const float *view, uint32_t view_stride_floats, float *linear_rgb, float *gamma_rgb, uint8_t *rgb8) {
    try {
        const ProbeLookupArgs a{sh, pr, maps, pd, moments, normal_bias, placement, pd || moments, placement != nullptr};
        return probe_shade_glossy_impl(grid, a, p, aov, spec, view, view_stride_floats, false, nullptr, 0, 0, 0, linear_rgb, gamma_rgb, rgb8);
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_probe_shade_glossy"); }
}

int fw_lightmap_texels(const fw_lightmap *lm, int device, float *records, uint32_t *owner, uint32_t *n_covered, int on_device, void *stream) {
    try { return lightmap_texels_impl(lm, device, records, owner, n_covered, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_lightmap_texels"); }
}

int fw_lightmap_rays(const fw_lightmap *lm, int device, uint32_t round, uint32_t first, uint32_t n, float *rays, int on_device, void *stream) {
    try { return lightmap_rays_impl(lm, device, round, first, n, rays, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_lightmap_rays"); }
}

int fw_lightmap_reduce(int device, uint32_t n, uint32_t directions, uint32_t samples, const uint32_t *texel_ids, const float *accum, float *sums,
                       uint32_t n_texels, int on_device, void *stream) {
    try { return lightmap_reduce_impl(device, n, directions, samples, texel_ids, accum, sums, n_texels, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_lightmap_reduce"); }
}

int fw_lightmap_dilate(int device, uint32_t width, uint32_t height, uint32_t passes, float *image, int on_device, void *stream) {
    try { return lightmap_dilate_impl(device, width, height, passes, image, on_device, stream); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_lightmap_dilate"); }
}

int fw_bake_lightmap(fw_scene *scene, const fw_lightmap *lm, const fw_render_rays_params *rp, uint32_t first_round, uint32_t rounds, uint32_t dilate,
                     float *sums, float *irradiance, fw_stats *stats) {
    try { return bake_lightmap_impl(scene, lm, rp, first_round, rounds, dilate, sums, irradiance, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_bake_lightmap"); }
}

int fw_denoise(const fw_denoise_params *p, const float *color, const float *aov, const float *moments, float *linear_rgb, float *gamma_rgb,
               uint8_t *rgb8) {
    try { return denoise_impl(p, color, aov, moments, linear_rgb, gamma_rgb, rgb8); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_denoise"); }
}


// ---- single-process multi-GPU: one host thread per device, 16x16 tiles dealt diagonally (the scheme of firework_amd/tiles.py),
// each device renders its pixels with the keys one GPU would use, results are scattered into the caller's buffers.
int fw_temporal(const fw_temporal_params *p, const float *color, const float *moments, const float *aov, const float *hist_color,
                const float *hist_moments, const float *hist_aov, const float *prev_position, float *out_color, float *out_moments,
                float *out_history) {
    try { return temporal_impl(p, color, moments, aov, hist_color, hist_moments, hist_aov, prev_position, out_color, out_moments, out_history); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_temporal"); }
}

int fw_render_scene_tiled(const fw_scene_desc *desc, const fw_render_params *params, const int *devices, int n_devices,
                          uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats) {
    if (!desc || !params || !devices || n_devices <= 0) return fail(FW_ERR_BAD_ARG, "null argument");
    if (params->pixel_ids || params->outputs_on_device) return fail(FW_ERR_BAD_ARG, "fw_render_scene_tiled renders whole frames into host buffers");
    if (params->width == 0 || params->height == 0) return fail(FW_ERR_BAD_ARG, "width, height and samples must be > 0");
    const auto call0 = std::chrono::steady_clock::now();
    try {
        const uint32_t W = params->width, H = params->height, TILE = 16, tx = (W + TILE - 1) / TILE, ty = (H + TILE - 1) / TILE;
        const int N = n_devices;
        std::vector<std::vector<uint32_t>> ids(N);
        for (uint32_t t = 0; t < tx * ty; t++) {
            const uint32_t owner = (t % tx + t / tx) % (uint32_t)N, y0 = (t / tx) * TILE, x0 = (t % tx) * TILE;
            for (uint32_t y = y0; y < std::min(y0 + TILE, H); y++) for (uint32_t x = x0; x < std::min(x0 + TILE, W); x++) ids[owner].push_back(y * W + x);
        }
        // Device-side gather (round 2): every device renders its tiles into its OWN memory, copies them peer-to-peer
        // (hipMemcpyPeer: over xGMI where the devices are linked) into one buffer on the first device, which scatters them to
        // their pixels and sends the finished frames to the host once — instead of one D2H per device and a host-side scatter.
        struct Part { int rc = FW_OK; std::string err; fw_stats st{}; double ms_scene = 0; };
        std::vector<Part> parts(N);
        std::vector<size_t> first(N + 1, 0);                       // part r holds the concatenated entries [first[r], first[r+1])
        for (int r = 0; r < N; r++) first[r + 1] = first[r] + ids[r].size();
        const size_t n_total = first[N];
        const int dev0 = devices[0];
        HIPCHK(hipSetDevice(dev0));
        // on the first device: [ids | gathered rgb8 | gamma | linear | frame rgb8 | gamma | linear], 256-byte aligned sections
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t b8 = rgb8 ? n_total * 3 : 0, bg = gamma_rgb ? n_total * 12 : 0, bl = linear_rgb ? n_total * 12 : 0;
        const size_t o_ids = 0, o_g8 = al(n_total * 4), o_gg = o_g8 + al(b8), o_gl = o_gg + al(bg), o_f8 = o_gl + al(bl), o_fg = o_f8 + al(b8),
                     o_fl = o_fg + al(bg), dev_bytes = o_fl + al(bl) + 256;
        struct GatherBuf : DevBuf { int dev; explicit GatherBuf(int d) : dev(d) {} ~GatherBuf() { if (p) { (void)hipSetDevice(dev); release(); } } };
        GatherBuf gather(dev0);                                    // released on every way out of this function, exceptions included
        int grc = gather.alloc(dev_bytes);
        if (grc) return grc;
        uint8_t *gb = (uint8_t *)gather.p;
        {
            std::vector<uint32_t> all_ids; all_ids.reserve(n_total);
            for (int r = 0; r < N; r++) all_ids.insert(all_ids.end(), ids[r].begin(), ids[r].end());
            if (hipMemcpy(gb + o_ids, all_ids.data(), n_total * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(FW_ERR_HIP, "tile id upload failed");
        }
        // Peer access to the first device, asked for once per pair (hipMemcpyPeer works without it, staged through the host by the
        // runtime; with it the copy goes over the xGMI link).  Where a pair has no peer path the tiles are staged through pinned
        // host memory here, and fw_last_error() says so after a successful call.
        std::vector<char> peer_ok(N, 1);
        std::string peer_note;
        for (int r = 0; r < N; r++) {
            if (devices[r] == dev0) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[r], dev0) != hipSuccess) can = 0;
            if (can) {
                (void)hipSetDevice(devices[r]);
                const hipError_t pe = hipDeviceEnablePeerAccess(dev0, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) can = 0;
                (void)hipGetLastError();
            }
            if (!can) { peer_ok[r] = 0; peer_note += (peer_note.empty() ? "no peer access to device " : ", ") + std::to_string(devices[r]); }
        }
        (void)hipSetDevice(dev0);
        if (!peer_note.empty()) peer_note = peer_note + " from device " + std::to_string(dev0) + ": those tiles were staged through host memory";
        std::vector<std::thread> threads;
        struct Joiner { std::vector<std::thread> &t; ~Joiner() { for (auto &x : t) if (x.joinable()) x.join(); } } joiner{threads};   // a failed emplace_back must not destroy joinable threads
        threads.reserve((size_t)N);
        for (int r = 0; r < N; r++) threads.emplace_back([&, r] {
            Part &pt = parts[r];
            const size_t n = ids[r].size();
            if (n == 0) return;
            try {
                auto t0 = std::chrono::steady_clock::now();
                fw_scene *sc = nullptr;
                pt.rc = fw_scene_create(desc, devices[r], &sc);
                if (pt.rc) { pt.err = g_last_error; return; }
                pt.ms_scene = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                DevBuf part;                                            // this device's tiles, in its own HBM
                const size_t p8 = rgb8 ? n * 3 : 0, pg = gamma_rgb ? n * 12 : 0, pl = linear_rgb ? n * 12 : 0;
                const size_t q8 = 0, qg = al(p8), ql = qg + al(pg);
                (void)hipSetDevice(devices[r]);
                pt.rc = part.alloc(ql + al(pl) + 256);
                if (!pt.rc) {
                    uint8_t *pb = (uint8_t *)part.p;
                    fw_render_params p = *params;
                    p.pixel_ids = ids[r].data(); p.n_pixels = (uint32_t)n; p.stream = nullptr; p.outputs_on_device = 1;
                    pt.rc = fw_render(sc, &p, rgb8 ? pb + q8 : nullptr, gamma_rgb ? (float *)(pb + qg) : nullptr, linear_rgb ? (float *)(pb + ql) : nullptr, &pt.st);
                    if (pt.rc) pt.err = g_last_error;
                    auto peer = [&](size_t dst_off, size_t src_off, size_t bytes) {
                        if (pt.rc || !bytes) return;
                        if (peer_ok[r]) {
                            if (hipMemcpyPeer(gb + dst_off, dev0, pb + src_off, devices[r], bytes) != hipSuccess) { pt.rc = FW_ERR_HIP; pt.err = "hipMemcpyPeer of a device's tiles failed"; }
                            return;
                        }
                        void *host = nullptr;                            // no peer path: device -> pinned host -> first device
                        if (hipHostMalloc(&host, bytes, hipHostMallocDefault) != hipSuccess) { pt.rc = FW_ERR_OOM; pt.err = "pinned staging for a device's tiles failed"; return; }
                        hipError_t e = hipMemcpy(host, pb + src_off, bytes, hipMemcpyDeviceToHost);
                        if (e == hipSuccess) { (void)hipSetDevice(dev0); e = hipMemcpy(gb + dst_off, host, bytes, hipMemcpyHostToDevice); (void)hipSetDevice(devices[r]); }
                        (void)hipHostFree(host);
                        if (e != hipSuccess) { pt.rc = FW_ERR_HIP; pt.err = "host-staged copy of a device's tiles failed"; }
                    };
                    peer(o_g8 + first[r] * 3, q8, p8); peer(o_gg + first[r] * 12, qg, pg); peer(o_gl + first[r] * 12, ql, pl);
                } else pt.err = g_last_error;
                part.release();
                fw_scene_destroy(sc);
            } catch (...) { pt.rc = FW_ERR_OOM; pt.err = "host allocation failed in a tile worker"; }
        });
        for (auto &t : threads) t.join();
        for (int r = 0; r < N; r++) if (parts[r].rc) return fail(parts[r].rc, parts[r].err);
        // the one scatter and the one device -> host transfer
        (void)hipSetDevice(dev0);
        fw::launch_scatter_tiles(nullptr, (const uint32_t *)(gb + o_ids), (uint32_t)n_total, rgb8 ? gb + o_g8 : nullptr, gamma_rgb ? (const float *)(gb + o_gg) : nullptr,
                                 linear_rgb ? (const float *)(gb + o_gl) : nullptr, gb + o_f8, (float *)(gb + o_fg), (float *)(gb + o_fl));
        hipError_t ce = hipGetLastError();                          // the scatter launch itself
        if (rgb8 && ce == hipSuccess) ce = hipMemcpy(rgb8, gb + o_f8, b8, hipMemcpyDeviceToHost);
        if (gamma_rgb && ce == hipSuccess) ce = hipMemcpy(gamma_rgb, gb + o_fg, bg, hipMemcpyDeviceToHost);
        if (linear_rgb && ce == hipSuccess) ce = hipMemcpy(linear_rgb, gb + o_fl, bl, hipMemcpyDeviceToHost);
        if (ce != hipSuccess) return fail(FW_ERR_HIP, hipGetErrorString(ce));
        if (!peer_note.empty()) g_last_error = peer_note;          // informational: the call succeeded
        if (stats) std::memset(stats, 0, sizeof *stats);
        for (int r = 0; r < N; r++) {
            const Part &pt = parts[r];
            if (stats && !ids[r].empty()) {
                stats->samples += pt.st.samples; stats->rays += pt.st.rays; stats->algorithmic_bytes += pt.st.algorithmic_bytes;
                stats->bytes_raygen += pt.st.bytes_raygen; stats->bytes_extend += pt.st.bytes_extend; stats->bytes_shade += pt.st.bytes_shade;
                stats->bytes_accumulate += pt.st.bytes_accumulate; stats->deposits += pt.st.deposits; stats->parked_rays += pt.st.parked_rays;
                stats->ms_d2h = std::max(stats->ms_d2h, pt.st.ms_d2h);
                for (int k = 0; k < FW_MAX_SEGMENTS; k++) stats->rays_per_depth[k] += pt.st.rays_per_depth[k];
                stats->ms_render = std::max(stats->ms_render, pt.st.ms_render); stats->ms_scene = std::max(stats->ms_scene, pt.ms_scene);
                stats->n_batches = std::max(stats->n_batches, pt.st.n_batches);
                stats->tlas_nodes = pt.st.tlas_nodes; stats->blas_nodes = pt.st.blas_nodes; stats->reserved = pt.st.reserved;
            }
        }
        if (stats) stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - call0).count();
        return FW_OK;
    }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_scene_tiled"); }
}

int fw_render_progressive(fw_scene *scene, const fw_render_params *params, uint32_t first_sample, float *accum,
                          uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats) {
    if (!accum) return fail(FW_ERR_BAD_ARG, "fw_render_progressive needs an accumulation buffer");
    try { return render_impl(scene, params, rgb8, gamma_rgb, linear_rgb, stats, first_sample, accum); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_progressive"); }
}

int fw_render_adaptive(fw_scene *scene, const fw_render_params *params, float tolerance, uint32_t min_samples, float *accum, float *moments,
                       uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, uint32_t *round_pixels, fw_stats *stats) {
    try { return adaptive_impl(scene, params, tolerance, min_samples, accum, moments, rgb8, gamma_rgb, linear_rgb, round_pixels, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_adaptive"); }
}

int fw_render_views(fw_scene *scene, const fw_render_params *params, const fw_camera_settings *cameras, uint32_t n_views,
                    uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats) {
    try { return views_impl(scene, params, cameras, n_views, rgb8, gamma_rgb, linear_rgb, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_views"); }
}

int fw_render_rays(fw_scene *scene, const fw_render_rays_params *p, const float *rays, float *accum,
                   uint8_t *rgb8, float *gamma_rgb, float *linear_rgb, fw_stats *stats) {
    try { return rays_impl(scene, p, rays, accum, rgb8, gamma_rgb, linear_rgb, stats); }
    catch (std::bad_alloc &) { return fail(FW_ERR_OOM, "host allocation failed"); }
    catch (...) { return fail(FW_ERR_BAD_ARG, "unexpected exception in fw_render_rays"); }
}

int fw_render_scene(const fw_scene_desc *desc, const fw_render_params *params, int device, uint8_t *rgb8, float *gamma_rgb,
                    float *linear_rgb, fw_stats *stats) {
    auto t0 = std::chrono::steady_clock::now();
    fw_scene *sc = nullptr;
    int rc = fw_scene_create(desc, device, &sc);
    if (rc) return rc;
    double ms_scene = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    rc = fw_render(sc, params, rgb8, gamma_rgb, linear_rgb, stats);
    fw_scene_destroy(sc);
    if (!rc && stats) {
        stats->ms_scene = ms_scene;
        stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();   // main.rs:40-44's region
    }
    return rc;
}

} // extern "C"
