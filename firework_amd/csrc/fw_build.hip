// fw_build.hip — the two host tree builders of fw_runtime.cpp (bvh_build: the reference's median-split tree, sah_build: the binned-SAH tree)
// restated on the device, level by level, with every decision taken on the same values in the same way, so that the node arrays are the
// host's bit for bit.
//
// A level is every node of one depth, each a contiguous segment [start, start + count) of the item order `idx`.  Per level:
//   median  every node's segment is sorted stably by the centre on axis depth % 3 (leaves of one or two items too: bvh.rs sorts before it
//           looks at the count); an inner node splits at count / 2.
//   SAH     per inner node (count > 2): the centroids' bounds, 3 x 16 bins (box unions and counts), one lane's 16-bin sweep with the host's
//           expressions in the host's order, then a stable partition; where no split is found (or past SAH_MAX_DEPTH) the segment is
//           sorted stably on the axis of largest centroid extent and split at count / 2.
// A stable segmented sort is one global sort by (segment start, centre key, position): segments keep their places, equal keys keep their
// order.  A stable partition is a scan of the "goes left" flags.  Nodes are kept in level (BFS) order while the levels are built; then the
// subtree sizes and boxes go bottom-up (box_union(left, right), as the host unites them), the depth-first indices top-down, and every node
// is written to its depth-first slot.
//
// Where the host's result rests on x86 rather than C++: fmin / fmax (minss / maxss: for equal operands, ±0, the FIRST operand; a NaN
// first operand gives the second) and (int) of a float (cvttss2si: NaN and out of range give INT_MIN).  Bins and centroid bounds are
// reduced with atomics on order-preserving integers, so their zeros may carry the other sign than the host's sequential fmin gives; no
// decision reads the sign of a zero (bins from (key - lo) / ext, areas and costs compared with <), and no output box comes from them.
#include "fw_build.h"
#include "fw_device.h"
#include "../../include/firework_hip.h"

#include <chrono>
#include <climits>
#include <cstring>
#include <mutex>

namespace {

constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t SAH_MAX_DEPTH = 40;      // fw_runtime.cpp
constexpr int NB = 16;                      // bins per axis (fw_runtime.cpp sah_build_rec)
constexpr int BIN_W = 7;                    // per bin: min.xyz max.xyz (ordered ints), count
constexpr int TILE = 1024;                  // the bitonic sort's LDS tile
constexpr int SCAN_B = 1024;                // elements per block of the scan (256 threads x 4)
constexpr uint32_t BIN_CHUNK = 16384;       // SAH inner nodes binned per pass: 22 MB of bins, whatever the tree's size

struct SortKey { uint32_t a, b, c, v; };    // (segment start, centre key, position) and the item

__device__ __forceinline__ float hmin(float a, float b) { return a != a ? b : (b < a ? b : a); }   // x86 fminf as compiled: minss
__device__ __forceinline__ float hmax(float a, float b) { return a != a ? b : (b > a ? b : a); }
__device__ __forceinline__ int host_int(float f) { return (f != f || f >= 2147483648.f || f < -2147483648.f) ? INT_MIN : (int)f; }   // cvttss2si
__device__ __forceinline__ uint32_t ord(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float unord(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ uint32_t sort_key(float f) { return ord(f == 0.f ? 0.f : f); }   // -0 folded into +0: the host compares with <
__device__ __forceinline__ bool key_less(const SortKey &x, const SortKey &y) { return x.a != y.a ? x.a < y.a : (x.b != y.b ? x.b < y.b : x.c < y.c); }
__device__ __forceinline__ int bin_of(float key, float lo, float ext) { return min(NB - 1, max(0, host_int((key - lo) / ext * NB))); }
__device__ __forceinline__ float box_area(const float *mn, const float *mx) {
    const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
    return 2.f * (dx * dy + dy * dz + dz * dx);
}

// ---- exclusive scan of m u32 into out[0..m] (out[m] = the total) ----
__global__ void k_scan_blocks(const uint32_t *in, uint32_t *out, uint32_t m, uint32_t *bsum) {
    __shared__ uint32_t s[256];
    const uint32_t t = threadIdx.x, base = blockIdx.x * SCAN_B + t * 4;
    uint32_t v[4], sum = 0;
    for (int k = 0; k < 4; k++) { v[k] = base + k < m ? in[base + k] : 0u; sum += v[k]; }
    s[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t x = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    uint32_t run = s[t] - sum;
    for (int k = 0; k < 4; k++) { if (base + k < m) out[base + k] = run; run += v[k]; }
    if (t == 255) bsum[blockIdx.x] = s[255];
}
__global__ void k_scan_sums(uint32_t *bsum, uint32_t nb) {       // one block: exclusive scan of the block sums, bsum[nb] = total
    __shared__ uint32_t s[1024];
    __shared__ uint32_t carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < nb; c0 += 1024) {
        const uint32_t v = c0 + t < nb ? bsum[c0 + t] : 0u;
        s[t] = v;
        __syncthreads();
        for (uint32_t off = 1; off < 1024; off <<= 1) {
            const uint32_t x = t >= off ? s[t - off] : 0u;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (c0 + t < nb) bsum[c0 + t] = carry + s[t] - v;
        __syncthreads();
        if (t == 0) carry += s[1023];
        __syncthreads();
    }
    if (t == 0) bsum[nb] = carry;
}
__global__ void k_scan_add(uint32_t *out, uint32_t m, const uint32_t *bsum, uint32_t nb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] += bsum[i / SCAN_B];
    if (i == 0) out[m] = bsum[nb];
}

// ---- bitonic sort of SortKey[N], N a power of two >= TILE ----
__global__ void k_bitonic_global(SortKey *key, uint32_t N, uint32_t k, uint32_t j) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t l = i ^ j;
    if (l <= i) return;
    const SortKey x = key[i], y = key[l];
    const bool asc = (i & k) == 0;
    if (asc ? key_less(y, x) : key_less(x, y)) { key[i] = y; key[l] = x; }
}
// every step of the sizes k_lo..k_hi whose stride is below TILE, inside one tile (k_lo = k_hi > TILE: the tail of one merge)
__global__ void __launch_bounds__(TILE / 2) k_bitonic_tile(SortKey *key, uint32_t k_lo, uint32_t k_hi) {
    __shared__ SortKey s[TILE];
    const uint32_t t = threadIdx.x, base = blockIdx.x * TILE;
    s[t] = key[base + t]; s[t + TILE / 2] = key[base + t + TILE / 2];
    __syncthreads();
    for (uint32_t k = k_lo; k <= k_hi; k <<= 1) {
        for (uint32_t j = (k > TILE ? TILE : k) / 2; j > 0; j >>= 1) {
            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const SortKey x = s[i], y = s[l];
            const bool asc = ((base + i) & k) == 0;
            if (asc ? key_less(y, x) : key_less(x, y)) { s[i] = y; s[l] = x; }
            __syncthreads();
        }
    }
    key[base + t] = s[t]; key[base + t + TILE / 2] = s[t + TILE / 2];
}

// ---- setup ----
__global__ void k_setup(const float *box, float *cen, uint32_t *idx, uint32_t n, uint32_t *nstart, uint32_t *ncount) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { nstart[0] = 0; ncount[0] = n; }
    if (i >= n) return;
    for (int a = 0; a < 3; a++) cen[(size_t)a * n + i] = 0.5f * box[(size_t)i * 6 + a] + 0.5f * box[(size_t)i * 6 + 3 + a];   // aabb.rs:59-61
    idx[i] = i;
}

// ---- one level: nodes [b, b + m) ----
__global__ void k_level_flags(const uint32_t *ncount, uint32_t b, uint32_t m, uint32_t *lflag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) lflag[j] = ncount[b + j] > 2u ? 1u : 0u;
}
__global__ void k_level_compact(const uint32_t *lflag, const uint32_t *lscan, uint32_t b, uint32_t m, uint32_t *inl) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m && lflag[j]) inl[lscan[j]] = b + j;
}
// pseg[p] = the node of this level whose segment holds position p (median: every node; SAH: inner nodes), else NONE.  The level's
// segments are in increasing order of start.
__global__ void k_pseg(uint32_t n, const uint32_t *nstart, const uint32_t *ncount, uint32_t b, uint32_t m, int all, uint32_t *pseg) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t lo = 0, hi = m;                  // first node with start > p
    while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (nstart[b + mid] <= p) lo = mid + 1; else hi = mid; }
    uint32_t r = NONE;
    if (lo > 0) {
        const uint32_t j = b + lo - 1;
        if (p - nstart[j] < ncount[j] && (all || ncount[j] > 2u)) r = j;
    }
    pseg[p] = r;
}
__global__ void k_median_nodes(uint32_t b, uint32_t m, uint32_t depth, const uint32_t *ncount, uint32_t *naxis, uint32_t *nhalf, uint32_t *nfb) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    naxis[b + j] = depth % 3; nhalf[b + j] = ncount[b + j] / 2; nfb[b + j] = 1;
}
__global__ void k_nan_check(uint32_t n, const uint32_t *pseg, const uint32_t *idx, const float *key, uint32_t *cnt) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || pseg[p] == NONE) return;
    const float c = key[idx[p]];
    if (c != c) atomicOr(&cnt[2], 1u);
}

// SAH: the inner nodes of a level are binned in passes of `cap` (<= BIN_CHUNK) nodes: pass r0 holds the nodes of inner rank (in the level's
// inner list inl) r0 <= r < r0 + cap, node r's centroid bounds at cb[(r - r0) * 6], its bins at bins[(r - r0) * 3 * NB * BIN_W].
__device__ __forceinline__ uint32_t chunk_rank(uint32_t r, uint32_t r0, uint32_t cap) { return r != NONE && r >= r0 && r - r0 < cap ? r - r0 : NONE; }
__global__ void k_sah_init(const uint32_t *lscan, uint32_t m, uint32_t r0, uint32_t cap, uint32_t *cb, uint32_t *bins) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, M = lscan[m];
    if (i >= cap * 3 * NB) return;
    const uint32_t r = i / (3 * NB), q = i % (3 * NB);
    if (r0 + r >= M) return;
    uint32_t *bq = bins + ((size_t)r * 3 * NB + q) * BIN_W;
    for (int c = 0; c < 3; c++) { bq[c] = ord(1e30f); bq[3 + c] = ord(-1e30f); }     // EMPTY (fw_runtime.cpp)
    bq[6] = 0;
    if (q == 0) for (int c = 0; c < 3; c++) { cb[(size_t)r * 6 + c] = ord(1e30f); cb[(size_t)r * 6 + 3 + c] = ord(-1e30f); }
}
// A wave whose positions all lie in one node (every wave of the big nodes near the root) reduces its 64 centres first and sends one lane's
// atomics: per-lane atomics on the same six words of the root serialise (300 ms of a million-item build).
__global__ void k_sah_bounds(uint32_t n, const uint32_t *pseg, const uint32_t *idx, const float *cen, const uint32_t *lscan, uint32_t b, uint32_t r0, uint32_t cap, uint32_t *cb) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t r = p < n && pseg[p] != NONE ? chunk_rank(lscan[pseg[p] - b], r0, cap) : NONE;
    const bool active = r != NONE;
    uint32_t v[6] = {NONE, NONE, NONE, 0u, 0u, 0u};    // min keys, max keys; NONE / 0 = nothing (a NaN centre adds nothing: fmin(acc, NaN) = acc)
    if (active) {
        const uint32_t it = idx[p];
        for (int a = 0; a < 3; a++) {
            const float c = cen[(size_t)a * n + it];
            if (c == c) { v[a] = ord(c); v[3 + a] = ord(c); }
        }
    }
    uint32_t rmin = r;
    for (int off = 32; off > 0; off >>= 1) rmin = min(rmin, (uint32_t)__shfl_xor((int)rmin, off));
    if (__all(r == rmin || r == NONE)) {
        if (rmin == NONE) return;
        for (int off = 32; off > 0; off >>= 1)
            for (int c = 0; c < 6; c++) {
                const uint32_t o = (uint32_t)__shfl_xor((int)v[c], off);
                v[c] = c < 3 ? min(v[c], o) : max(v[c], o);
            }
        if ((threadIdx.x & 63) != 0) return;
        r = rmin;                              // lane 0 writes for the wave, whether or not its own position is in the node
    } else if (!active) return;
    for (int a = 0; a < 3; a++) {
        if (v[a] != NONE) atomicMin(&cb[(size_t)r * 6 + a], v[a]);
        if (v[3 + a] != 0u) atomicMax(&cb[(size_t)r * 6 + 3 + a], v[3 + a]);
    }
}
__global__ void k_sah_bins(uint32_t n, const uint32_t *pseg, const uint32_t *idx, const float *cen, const float *box, const uint32_t *lscan, uint32_t b,
                           uint32_t r0, uint32_t cap, const uint32_t *cb, uint32_t *bins) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || pseg[p] == NONE) return;
    const uint32_t r = chunk_rank(lscan[pseg[p] - b], r0, cap);
    if (r == NONE) return;
    const uint32_t it = idx[p];
    float bx[6];
    for (int c = 0; c < 6; c++) bx[c] = box[(size_t)it * 6 + c];
    for (int a = 0; a < 3; a++) {
        const float lo = unord(cb[(size_t)r * 6 + a]), ext = unord(cb[(size_t)r * 6 + 3 + a]) - lo;
        if (!(ext > 0.f)) continue;
        const int q = bin_of(cen[(size_t)a * n + it], lo, ext);
        uint32_t *bq = bins + ((size_t)r * 3 * NB + (size_t)a * NB + q) * BIN_W;
        for (int c = 0; c < 3; c++) {
            if (bx[c] == bx[c]) atomicMin(&bq[c], ord(bx[c]));
            if (bx[3 + c] == bx[3 + c]) atomicMax(&bq[3 + c], ord(bx[3 + c]));
        }
        atomicAdd(&bq[6], 1u);
    }
}
// one lane per inner node: fw_runtime.cpp sah_build_rec's sweep and decision, expression for expression
__global__ void k_sah_sweep(const uint32_t *lscan, uint32_t m, uint32_t r0, uint32_t cap, const uint32_t *inl, uint32_t depth, const uint32_t *ncount, const uint32_t *cb,
                            const uint32_t *bins, uint32_t *naxis, uint32_t *nhalf, uint32_t *nsplit, uint32_t *nfb, float *nlo, float *next, uint32_t *cnt) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;      // rank in this pass
    if (r >= cap || r0 + r >= lscan[m]) return;
    const uint32_t j = inl[r0 + r], n = ncount[j];
    float cmn[3], cmx[3];
    for (int a = 0; a < 3; a++) { cmn[a] = unord(cb[(size_t)r * 6 + a]); cmx[a] = unord(cb[(size_t)r * 6 + 3 + a]); }
    int best_axis = -1; uint32_t best_split = 0, best_left = 0; float best_cost = 1e38f;
    if (depth < SAH_MAX_DEPTH) {
        for (int axis = 0; axis < 3; axis++) {
            const float lo = cmn[axis], ext = cmx[axis] - lo;
            if (!(ext > 0.f)) continue;
            const uint32_t *bq = bins + ((size_t)r * 3 + axis) * NB * BIN_W;
            float la[NB], ra[NB]; uint32_t lc[NB], rc[NB];
            float amn[3] = {1e30f, 1e30f, 1e30f}, amx[3] = {-1e30f, -1e30f, -1e30f};
            uint32_t cnt_acc = 0;
            for (int k = 0; k < NB; k++) {
                const uint32_t *x = bq + k * BIN_W;
                if (x[6]) for (int c = 0; c < 3; c++) { amn[c] = hmin(amn[c], unord(x[c])); amx[c] = hmax(amx[c], unord(x[3 + c])); }
                cnt_acc += x[6];
                la[k] = cnt_acc ? box_area(amn, amx) : 0.f; lc[k] = cnt_acc;
            }
            for (int c = 0; c < 3; c++) { amn[c] = 1e30f; amx[c] = -1e30f; }
            cnt_acc = 0;
            for (int k = NB - 1; k >= 0; k--) {
                const uint32_t *x = bq + k * BIN_W;
                if (x[6]) for (int c = 0; c < 3; c++) { amn[c] = hmin(amn[c], unord(x[c])); amx[c] = hmax(amx[c], unord(x[3 + c])); }
                cnt_acc += x[6];
                ra[k] = cnt_acc ? box_area(amn, amx) : 0.f; rc[k] = cnt_acc;
            }
            for (int k = 0; k + 1 < NB; k++) {
                if (lc[k] == 0 || rc[k + 1] == 0) continue;
                const float cost = la[k] * (float)lc[k] + ra[k + 1] * (float)rc[k + 1];
                if (cost < best_cost) { best_cost = cost; best_axis = axis; best_split = (uint32_t)k; best_left = lc[k]; }
            }
        }
    }
    uint32_t half, axis;
    if (best_axis >= 0) {
        axis = (uint32_t)best_axis; half = best_left; nfb[j] = 0;
        nlo[j] = cmn[axis]; next[j] = cmx[axis] - cmn[axis];
    } else {               // all centroids coincide (or depth cap): median split on the axis of the largest extent
        const float ex = cmx[0] - cmn[0], ey = cmx[1] - cmn[1], ez = cmx[2] - cmn[2];
        axis = ex >= ey ? (ex >= ez ? 0u : 2u) : (ey >= ez ? 1u : 2u);
        half = n / 2; nfb[j] = 1;
        atomicAdd(&cnt[1], 1u);
    }
    if (half == 0 || half == n) half = n / 2;
    naxis[j] = axis; nhalf[j] = half; nsplit[j] = best_split;
}

// the sort keys of a level: the positions of every node that sorts (nfb) by (start, centre key, position), every other position by itself
__global__ void k_keys(uint32_t N, uint32_t n, const uint32_t *pseg, const uint32_t *idx, const float *cen, const uint32_t *nstart, const uint32_t *naxis,
                       const uint32_t *nfb, SortKey *key) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    if (p >= n) { key[p] = SortKey{NONE, NONE, NONE, NONE}; return; }
    const uint32_t j = pseg[p], it = idx[p];
    if (j != NONE && nfb[j]) key[p] = SortKey{nstart[j], sort_key(cen[(size_t)naxis[j] * n + it]), p, it};
    else key[p] = SortKey{p, 0u, p, it};
}
__global__ void k_unkeys(uint32_t n, const SortKey *key, uint32_t *idx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) idx[p] = key[p].v;
}
// 1 = the item at p goes to the left child (or stays: a position of no inner node of this level)
__global__ void k_split_flags(uint32_t n, const uint32_t *pseg, const uint32_t *idx, const float *cen, const uint32_t *nstart, const uint32_t *ncount,
                              const uint32_t *naxis, const uint32_t *nhalf, const uint32_t *nsplit, const uint32_t *nfb, const float *nlo, const float *next, uint32_t *flag) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t j = pseg[p];
    uint32_t f = 1;
    if (j != NONE && ncount[j] > 2u) {
        if (nfb[j]) f = p - nstart[j] < nhalf[j] ? 1u : 0u;
        else f = (uint32_t)bin_of(cen[(size_t)naxis[j] * n + idx[p]], nlo[j], next[j]) <= nsplit[j] ? 1u : 0u;
    }
    flag[p] = f;
}
__global__ void k_scatter(uint32_t n, const uint32_t *pseg, const uint32_t *idx, const uint32_t *flag, const uint32_t *scan, const uint32_t *nstart,
                          const uint32_t *ncount, const uint32_t *nhalf, uint32_t *idx_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t j = pseg[p];
    uint32_t dst = p;
    if (j != NONE && ncount[j] > 2u) {
        const uint32_t s = nstart[j], left_before = scan[p] - scan[s];
        dst = flag[p] ? s + left_before : s + nhalf[j] + (p - s - left_before);
    }
    idx_out[dst] = idx[p];
}
__global__ void k_emit(uint32_t b, uint32_t m, const uint32_t *lflag, const uint32_t *lscan, uint32_t e, uint32_t *nstart, uint32_t *ncount,
                       const uint32_t *nhalf, uint32_t *nchild) {
    const uint32_t jj = blockIdx.x * blockDim.x + threadIdx.x;
    if (jj >= m) return;
    const uint32_t j = b + jj;
    if (!lflag[jj]) { nchild[j] = NONE; return; }
    const uint32_t c = e + 2 * lscan[jj], s = nstart[j], n = ncount[j], h = nhalf[j];
    nstart[c] = s; ncount[c] = h; nstart[c + 1] = s + h; ncount[c + 1] = n - h;
    nchild[j] = c;
}

// ---- assembly ----
__global__ void k_up(uint32_t b, uint32_t m, const uint32_t *nstart, const uint32_t *ncount, const uint32_t *nchild, const uint32_t *idx, const float *box,
                     uint32_t *nsize, float *nbox) {
    const uint32_t j = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b + m) return;
    float *o = nbox + (size_t)j * 6;
    const uint32_t c = nchild[j];
    if (c == NONE) {
        const float *x = box + (size_t)idx[nstart[j]] * 6;
        if (ncount[j] == 1) for (int k = 0; k < 6; k++) o[k] = x[k];
        else {
            const float *y = box + (size_t)idx[nstart[j] + 1] * 6;
            for (int k = 0; k < 3; k++) { o[k] = hmin(x[k], y[k]); o[3 + k] = hmax(x[3 + k], y[3 + k]); }   // box_union(a, b)
        }
        nsize[j] = 1;
    } else {
        const float *x = nbox + (size_t)c * 6, *y = nbox + (size_t)(c + 1) * 6;
        for (int k = 0; k < 3; k++) { o[k] = hmin(x[k], y[k]); o[3 + k] = hmax(x[3 + k], y[3 + k]); }
        nsize[j] = 1 + nsize[c] + nsize[c + 1];
    }
}
__global__ void k_down(uint32_t b, uint32_t m, const uint32_t *nstart, const uint32_t *ncount, const uint32_t *nchild, const uint32_t *naxis, const uint32_t *idx,
                       const uint32_t *nsize, const float *nbox, uint32_t *ndfs, uint32_t total, float *out) {
    const uint32_t j = b + blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b + m) return;
    const uint32_t me = j == 0 ? 0u : ndfs[j], c = nchild[j];
    if (me >= total) return;
    uint32_t A, B = 0;
    if (c == NONE) {
        const uint32_t s = nstart[j];
        if (ncount[j] == 1) A = (fw::NODE_LEAF << 30) | idx[s];
        else { A = (fw::NODE_DOUBLE << 30) | idx[s]; B = idx[s + 1]; }
    } else {
        ndfs[c] = me + 1;
        ndfs[c + 1] = me + 1 + nsize[c];
        A = me + 1 + nsize[c];
        B = naxis[j];
    }
    const float *x = nbox + (size_t)j * 6;
    float *o = out + (size_t)me * 8;
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = __uint_as_float(A);
    o[4] = x[3]; o[5] = x[4]; o[6] = x[5]; o[7] = __uint_as_float(B);
}

inline uint32_t grid(size_t n, uint32_t block = 256) { return (uint32_t)std::max<size_t>(1, (n + block - 1) / block); }

// ---- the builder's own memory: one allocation per device, grown on demand, and a stream ----
struct Scratch {
    std::mutex mu;
    void *dev = nullptr; size_t bytes = 0;
    uint32_t *host_cnt = nullptr;             // pinned: the level's counters
    hipStream_t stream = nullptr;
};
constexpr int MAX_DEV = 64;
Scratch g_scratch[MAX_DEV];

struct Layout {
    size_t off = 0;
    template <class T> T *take(char *base, size_t count) { T *p = reinterpret_cast<T *>(base + off); off += (count * sizeof(T) + 255) & ~(size_t)255; return p; }
};

int hip_fail(hipError_t e, const char *what, std::string &msg) {
    (void)hipGetLastError();
    msg = std::string("device tree build: ") + what + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? FW_ERR_OOM : FW_ERR_HIP;
}

} // namespace

namespace fw {

int device_build_tree(int device, BuildTree tree, const float *boxes, uint32_t n, std::vector<float> &nodes, uint32_t &depth_out,
                      DeviceBuildTimes *times, std::string &msg) {
    if (device < 0 || device >= MAX_DEV || !boxes || n == 0 || n > NODE_MASK) { msg = "device tree build: bad argument"; return FW_ERR_BAD_ARG; }
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    Scratch &S = g_scratch[device];
    std::lock_guard<std::mutex> guard(S.mu);
    hipError_t e;
#define BCHK(expr, what) do { if ((e = (expr)) != hipSuccess) return hip_fail(e, what, msg); } while (0)
    // this device's stream and memory, whichever device the calling thread has current (a helper thread of scene creation has the
    // default one); the caller's current device is given back on return
    int prev_device = -1;
    BCHK(hipGetDevice(&prev_device), "current device");
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{prev_device};
    BCHK(hipSetDevice(device), "set device");
    if (!S.stream) BCHK(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking), "stream");
    if (!S.host_cnt) BCHK(hipHostMalloc((void **)&S.host_cnt, 64, hipHostMallocDefault), "pinned counters");
    const hipStream_t st = S.stream;
    const bool sah = tree == BUILD_SAH;
    const size_t NC = 2 * (size_t)n;                       // nodes: at most 2n - 1
    size_t N2 = TILE; while (N2 < n) N2 <<= 1;             // the sort's power of two
    const size_t IC = sah ? std::min<size_t>(BIN_CHUNK, n / 3 + 1) : 1;   // inner nodes binned per pass (each holds 3 items or more)
    const size_t NBS = std::max(NC, (size_t)n) / SCAN_B + 2;
    auto carve = [&](char *base, Layout &L) {
        struct P {
            float *box, *cen, *nbox, *nlo, *next, *out; uint32_t *idx, *idx2, *pseg, *flag, *scan, *nstart, *ncount, *nchild, *naxis, *nhalf, *nsplit, *nfb,
                *nsize, *ndfs, *lflag, *lscan, *inl, *cb, *bins, *bsum, *cnt; SortKey *key;
        } p;
        p.box = L.take<float>(base, (size_t)n * 6); p.cen = L.take<float>(base, (size_t)n * 3);
        p.idx = L.take<uint32_t>(base, n); p.idx2 = L.take<uint32_t>(base, n); p.pseg = L.take<uint32_t>(base, n); p.flag = L.take<uint32_t>(base, n);
        p.scan = L.take<uint32_t>(base, (size_t)n + 1);
        p.nstart = L.take<uint32_t>(base, NC); p.ncount = L.take<uint32_t>(base, NC); p.nchild = L.take<uint32_t>(base, NC); p.naxis = L.take<uint32_t>(base, NC);
        p.nhalf = L.take<uint32_t>(base, NC); p.nsplit = L.take<uint32_t>(base, NC); p.nfb = L.take<uint32_t>(base, NC); p.nsize = L.take<uint32_t>(base, NC);
        p.ndfs = L.take<uint32_t>(base, NC); p.nlo = L.take<float>(base, NC); p.next = L.take<float>(base, NC); p.nbox = L.take<float>(base, NC * 6);
        p.lflag = L.take<uint32_t>(base, NC); p.lscan = L.take<uint32_t>(base, NC + 1); p.inl = L.take<uint32_t>(base, NC);
        p.cb = L.take<uint32_t>(base, IC * 6); p.bins = L.take<uint32_t>(base, IC * 3 * NB * BIN_W);
        p.bsum = L.take<uint32_t>(base, NBS + 1); p.cnt = L.take<uint32_t>(base, 16);
        p.key = L.take<SortKey>(base, N2); p.out = L.take<float>(base, NC * 8);
        return p;
    };
    Layout probe; (void)carve(nullptr, probe);
    if (S.bytes < probe.off) {
        if (S.dev) { (void)hipFree(S.dev); S.dev = nullptr; S.bytes = 0; }
        BCHK(hipMalloc(&S.dev, probe.off), "scratch allocation");
        S.bytes = probe.off;
    }
    Layout lay; auto P = carve((char *)S.dev, lay);

    auto scan = [&](const uint32_t *in, uint32_t *out, uint32_t m) {
        const uint32_t nb = (m + SCAN_B - 1) / SCAN_B;
        if (nb) k_scan_blocks<<<nb, 256, 0, st>>>(in, out, m, P.bsum);
        k_scan_sums<<<1, 1024, 0, st>>>(P.bsum, nb);
        k_scan_add<<<grid(m), 256, 0, st>>>(out, m, P.bsum, nb);
    };
    auto sort = [&]() {
        const uint32_t tiles = (uint32_t)(N2 / TILE);
        k_bitonic_tile<<<tiles, TILE / 2, 0, st>>>(P.key, 2, TILE);
        for (size_t k = 2 * TILE; k <= N2; k <<= 1) {
            for (size_t j = k / 2; j >= TILE; j >>= 1) k_bitonic_global<<<grid(N2), 256, 0, st>>>(P.key, (uint32_t)N2, (uint32_t)k, (uint32_t)j);
            k_bitonic_tile<<<tiles, TILE / 2, 0, st>>>(P.key, (uint32_t)k, (uint32_t)k);
        }
    };

    const auto t0 = clk::now();
    BCHK(hipMemcpyAsync(P.box, boxes, (size_t)n * 24, hipMemcpyHostToDevice, st), "upload");
    BCHK(hipStreamSynchronize(st), "upload");
    const auto t1 = clk::now();
    k_setup<<<grid(n), 256, 0, st>>>(P.box, P.cen, P.idx, n, P.nstart, P.ncount);
    std::vector<uint32_t> level_base{0u};
    uint32_t b = 0, m = 1, depth = 0;
    while (true) {
        const uint32_t e_ = b + m;
        level_base.push_back(e_);
        BCHK(hipMemsetAsync(P.cnt, 0, 16 * 4, st), "memset");
        k_level_flags<<<grid(m), 256, 0, st>>>(P.ncount, b, m, P.lflag);
        scan(P.lflag, P.lscan, m);
        k_level_compact<<<grid(m), 256, 0, st>>>(P.lflag, P.lscan, b, m, P.inl);
        k_pseg<<<grid(n), 256, 0, st>>>(n, P.nstart, P.ncount, b, m, sah ? 0 : 1, P.pseg);
        if (sah) {
            const size_t most_inner = std::min<size_t>(m, n / 3 + 1);       // the level's inner count is on the device: a pass past it does nothing
            for (uint32_t r0 = 0; r0 < most_inner; r0 += (uint32_t)IC) {
                const uint32_t cap = (uint32_t)IC;
                k_sah_init<<<grid(IC * 3 * NB), 256, 0, st>>>(P.lscan, m, r0, cap, P.cb, P.bins);
                k_sah_bounds<<<grid(n), 256, 0, st>>>(n, P.pseg, P.idx, P.cen, P.lscan, b, r0, cap, P.cb);
                if (depth < SAH_MAX_DEPTH) k_sah_bins<<<grid(n), 256, 0, st>>>(n, P.pseg, P.idx, P.cen, P.box, P.lscan, b, r0, cap, P.cb, P.bins);
                k_sah_sweep<<<grid(IC, 64), 64, 0, st>>>(P.lscan, m, r0, cap, P.inl, depth, P.ncount, P.cb, P.bins, P.naxis, P.nhalf, P.nsplit, P.nfb, P.nlo, P.next, P.cnt);
            }
        } else {
            k_median_nodes<<<grid(m), 256, 0, st>>>(b, m, depth, P.ncount, P.naxis, P.nhalf, P.nfb);
            k_nan_check<<<grid(n), 256, 0, st>>>(n, P.pseg, P.idx, P.cen + (size_t)(depth % 3) * n, P.cnt);
        }
        BCHK(hipMemcpyAsync(P.cnt, P.lscan + m, 4, hipMemcpyDeviceToDevice, st), "level count");
        BCHK(hipMemcpyAsync(S.host_cnt, P.cnt, 16, hipMemcpyDeviceToHost, st), "level counters");
        BCHK(hipStreamSynchronize(st), "level");
        const uint32_t inner = S.host_cnt[0], fallbacks = sah ? S.host_cnt[1] : m;
        if (S.host_cnt[2]) { msg = "Float comparison failed in BVH constructor"; return FW_ERR_NAN_BBOX; }
        if (fallbacks) {
            k_keys<<<grid(N2), 256, 0, st>>>((uint32_t)N2, n, P.pseg, P.idx, P.cen, P.nstart, P.naxis, P.nfb, P.key);
            sort();
            k_unkeys<<<grid(n), 256, 0, st>>>(n, P.key, P.idx);
        }
        if (inner) {
            k_split_flags<<<grid(n), 256, 0, st>>>(n, P.pseg, P.idx, P.cen, P.nstart, P.ncount, P.naxis, P.nhalf, P.nsplit, P.nfb, P.nlo, P.next, P.flag);
            scan(P.flag, P.scan, n);
            k_scatter<<<grid(n), 256, 0, st>>>(n, P.pseg, P.idx, P.flag, P.scan, P.nstart, P.ncount, P.nhalf, P.idx2);
            std::swap(P.idx, P.idx2);
        }
        k_emit<<<grid(m), 256, 0, st>>>(b, m, P.lflag, P.lscan, e_, P.nstart, P.ncount, P.nhalf, P.nchild);
        if (!inner) break;
        if ((size_t)e_ + 2 * (size_t)inner > NC) { msg = "device tree build: node count overflow"; return FW_ERR_HIP; }   // cannot happen: 2n - 1 nodes
        b = e_; m = 2 * inner; depth++;
    }
    const uint32_t total = level_base.back(), levels = (uint32_t)level_base.size() - 1;
    for (int l = (int)levels - 1; l >= 0; l--)
        k_up<<<grid(level_base[l + 1] - level_base[l]), 256, 0, st>>>(level_base[l], level_base[l + 1] - level_base[l], P.nstart, P.ncount, P.nchild, P.idx, P.box, P.nsize, P.nbox);
    for (uint32_t l = 0; l < levels; l++)
        k_down<<<grid(level_base[l + 1] - level_base[l]), 256, 0, st>>>(level_base[l], level_base[l + 1] - level_base[l], P.nstart, P.ncount, P.nchild, P.naxis, P.idx,
                                                                       P.nsize, P.nbox, P.ndfs, total, P.out);
    BCHK(hipGetLastError(), "launch");
    BCHK(hipStreamSynchronize(st), "build");
    const auto t2 = clk::now();
    try { nodes.resize((size_t)total * 8); } catch (...) { msg = "host allocation failed"; return FW_ERR_OOM; }
    BCHK(hipMemcpyAsync(nodes.data(), P.out, (size_t)total * 32, hipMemcpyDeviceToHost, st), "copy back");
    BCHK(hipStreamSynchronize(st), "copy back");
#undef BCHK
    depth_out = depth;
    if (times) { times->upload_ms += ms(t0, t1); times->kernel_ms += ms(t1, t2); times->copy_ms += ms(t2, clk::now()); }
    return FW_OK;
}

void device_build_release(int device) {
    if (device < 0 || device >= MAX_DEV) return;
    Scratch &S = g_scratch[device];
    std::lock_guard<std::mutex> guard(S.mu);
    if (S.stream) (void)hipStreamSynchronize(S.stream);
    if (S.dev) (void)hipFree(S.dev);
    if (S.stream) (void)hipStreamDestroy(S.stream);
    if (S.host_cnt) (void)hipHostFree(S.host_cnt);
    S.dev = nullptr; S.bytes = 0; S.stream = nullptr; S.host_cnt = nullptr;
}

} // namespace fw
