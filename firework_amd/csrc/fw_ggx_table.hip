// fw_ggx_table.hip — the split sum's BRDF term for gfx950: GgxMat's directional albedo as the two terms (A, B) of F0 A + B, integrated
// over the visible-normal square by a midpoint rule, as a table over (mu, rho), its bilinear lookup, and the probe shade that uses it
// (include/firework_hip.h has the statement, DESIGN.md §9y the design).
//
//   k_ggx_terms          one workgroup of 256 lanes per (mu, rho) pair — an entry of a list or a texel of a table — grid-stride over the
//                        pairs.  What a sample owes to the quadrature alone is staged once per workgroup in LDS as float64: sqrt(xi1) for
//                        the m1 rows (8 KB at 1024) and (cos, sin)(2 pi xi2) for the m2 columns (16 KB at 1024), so the software float64
//                        sine and cosine are paid m2 times per workgroup, not m1 m2 times per pair.  Lane l takes the samples l, l + 256,
//                        ... in ascending order, id = a m2 + b, everything else of a sample in registers; the trip count is
//                        ceil(m1 m2 / 256) for every lane — a lane past the end adds 0.0, which is exact — and `wi.z > 0` is a select
//                        around arithmetic that every lane runs.  Two float64 accumulators per lane, then a fixed tree: __shfl_xor at 32,
//                        16, 8, 4, 2, 1 within a wave, the four waves' partials through LDS added in wave order by lane 0.  8 B stored
//                        per pair.  Every barrier is reached by all 256 lanes: whether a pair is in range is workgroup-uniform.
//   k_ggx_table_lookup   one lane per pair: four 8-byte loads at indices clamped to the table, a bilinear blend in float64.
//   k_probe_split_shade  one lane per pixel: k_probe_shade_glossy's pixel (shade_glossy_pixel) with the table lookup as its specular term.
//
// No atomics, no inline assembly.  Every table index is formed from i0 in [0, n_mu - 2] and j0 in [0, n_rho - 2] plus 0 or 1, whatever
// mu and rho hold, so no load leaves the table; the maps are read through fw_probe_radiance_fetch.h, whose indices are clamped likewise.
// A pair's terms depend on nothing but the pair and the quadrature: not on the batch, the launch geometry or the run.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.ggx_terms / api.ggx_table_lookup /
// api.probe_split_ref; fmin, fmax and the int conversions are exact; sqrt, sin and cos are the device library's float64 functions.
#include "fw_ggx_table.h"
#include "fw_probe_corners.h"
#include "fw_probe_radiance_fetch.h"

namespace fw {
namespace {

constexpr int GT_BLOCK = 256;
constexpr int GL_BLOCK = 256;                   // the lookup and the shade

__global__ __launch_bounds__(GT_BLOCK) void k_ggx_terms(uint32_t m1, uint32_t m2, uint32_t n_pairs, const float *__restrict__ mu,
                                                        const float *__restrict__ rho, uint32_t first, uint32_t n_mu, uint32_t n_rho,
                                                        float2 *__restrict__ out) {
    __shared__ double s_r[GGX_MAX_M];                                                   // sqrt(xi1) of row a
    __shared__ double s_cs[GGX_MAX_M * 2];                                              // (cos, sin)(2 pi xi2) of column b
    __shared__ double s_part[2 * (GT_BLOCK / 64)];
    const uint32_t lane = threadIdx.x;
    const double PI = 3.141592653589793;
    for (uint32_t a = lane; a < m1; a += GT_BLOCK) s_r[a] = sqrt(((double)a + 0.5) / (double)m1);            // m1, m2 <= GGX_MAX_M
    for (uint32_t b = lane; b < m2; b += GT_BLOCK) {
        const double phi = (2.0 * PI) * (((double)b + 0.5) / (double)m2);
        s_cs[2u * b] = cos(phi); s_cs[2u * b + 1u] = sin(phi);
    }
    __syncthreads();
    const uint32_t total = m1 * m2;                                                     // <= 2^20
    const uint32_t trips = (total + GT_BLOCK - 1u) / GT_BLOCK;
    const double count = (double)m1 * (double)m2;
    for (uint32_t q = blockIdx.x; q < n_pairs; q += gridDim.x) {                        // q is workgroup-uniform
        float muf, rhof;
        if (mu) { muf = mu[q]; rhof = rho[q]; }
        else {
            const uint32_t t = first + q, j = t / n_mu, i = t - j * n_mu;
            muf = (float)(((double)i + 0.5) / (double)n_mu); rhof = (float)(((double)j + 0.5) / (double)n_rho);
        }
        double accA = 0.0, accB = 0.0;
        if (muf > 0.f && muf <= 1.f && rhof >= 0.f && rhof <= 1.f) {                    // false for a NaN; workgroup-uniform
            const double alpha = (double)(rhof * rhof), a2 = alpha * alpha;
            const double cm = (double)muf;
            const double sx = sqrt(fmax(1.0 - cm * cm, 0.0));
            const double vx = alpha * sx;
            const double vl = sqrt(vx * vx + cm * cm);
            const double vhx = vx / vl, vhz = cm / vl;
            const double s = 0.5 * (1.0 + vhz), s1 = 1.0 - s;
            const double lo1 = 1.0 + 0.5 * (sqrt(1.0 + a2 * ((sx * sx) / (cm * cm))) - 1.0);                 // 1 + Lambda(wo)
            for (uint32_t it = 0; it < trips; it++) {
                const uint32_t id_raw = it * GT_BLOCK + lane;
                const bool valid = id_raw < total;
                const uint32_t id = valid ? id_raw : total - 1u;
                const uint32_t a = id / m2, b = id - a * m2;                            // a < m1, b < m2
                const double r = s_r[a], cphi = s_cs[2u * b], sphi = s_cs[2u * b + 1u];
                const double p1 = r * cphi;
                const double q1 = 1.0 - p1 * p1;
                const double p2 = s1 * sqrt(fmax(q1, 0.0)) + s * (r * sphi);
                const double nz = sqrt(fmax(q1 - p2 * p2, 0.0));
                const double nhx = nz * vhx - p2 * vhz, nhz = p2 * vhx + nz * vhz;      // nh = p1 T1 + p2 T2 + nz Vh, T1 = (0, 1, 0)
                const double gx = alpha * nhx, gy = alpha * p1, gz = fmax(nhz, 0.0);
                const double hl = sqrt((gx * gx + gy * gy) + gz * gz);
                const double hx = gx / hl, hy = gy / hl, hz = gz / hl;
                const double oh = sx * hx + cm * hz;
                const double t2 = 2.0 * oh;
                const double wx = t2 * hx - sx, wy = t2 * hy, wz = t2 * hz - cm;
                const bool alive = wz > 0.0;
                const double zz = alive ? wz : 1.0, xy = alive ? wx * wx + wy * wy : 0.0;
                const double li = 0.5 * (sqrt(1.0 + a2 * (xy / (zz * zz))) - 1.0);
                const double k = (alive && valid) ? lo1 / (lo1 + li) : 0.0;
                const double m = fmax(1.0 - oh, 0.0);
                const double fc = ((m * m) * (m * m)) * m;
                accA = accA + k * (1.0 - fc);
                accB = accB + k * fc;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            accA = accA + __shfl_xor(accA, off, 64);
            accB = accB + __shfl_xor(accB, off, 64);
        }
        if ((lane & 63u) == 0u) { s_part[2u * (lane >> 6)] = accA; s_part[2u * (lane >> 6) + 1u] = accB; }
        __syncthreads();
        if (lane == 0u) {
            const double A = ((s_part[0] + s_part[2]) + s_part[4]) + s_part[6], B = ((s_part[1] + s_part[3]) + s_part[5]) + s_part[7];
            out[q] = make_float2((float)(A / count), (float)(B / count));
        }
        __syncthreads();                                                                // the partials are overwritten by the next pair
    }
}

// (A, B) of the n_rho x n_mu table at (mu, rho): bilinear over the four texel centres around it, edges clamped; zeros for a non-finite
// mu or rho.  i0 <= n_mu - 2 and j0 <= n_rho - 2 whatever the inputs are.
__device__ __forceinline__ void ggx_table_fetch(const float2 *__restrict__ table, uint32_t n_mu, uint32_t n_rho, float muf, float rhof, float &A,
                                                float &B) {
    A = 0.f; B = 0.f;
    if (!(finite_f(muf) && finite_f(rhof))) return;
    const double x = fmin(fmax((double)muf * (double)n_mu - 0.5, 0.0), (double)n_mu - 1.0);
    const double y = fmin(fmax((double)rhof * (double)n_rho - 0.5, 0.0), (double)n_rho - 1.0);
    const uint32_t i0 = min((uint32_t)(int)x, n_mu - 2u), j0 = min((uint32_t)(int)y, n_rho - 2u);          // x, y >= 0; n_mu, n_rho >= 2
    const double tx = x - (double)i0, ty = y - (double)j0, ux = 1.0 - tx, uy = 1.0 - ty;
    const float2 *__restrict__ r0 = table + (size_t)(j0 * n_mu + i0);
    const float2 *__restrict__ r1 = r0 + n_mu;
    const float2 t00 = r0[0], t10 = r0[1], t01 = r1[0], t11 = r1[1];
    A = (float)((((double)t00.x * ux + (double)t10.x * tx) * uy) + (((double)t01.x * ux + (double)t11.x * tx) * ty));
    B = (float)((((double)t00.y * ux + (double)t10.y * tx) * uy) + (((double)t01.y * ux + (double)t11.y * tx) * ty));
}

__global__ __launch_bounds__(GL_BLOCK) void k_ggx_table_lookup(uint32_t n_mu, uint32_t n_rho, const float2 *__restrict__ table, uint32_t n,
                                                               const float *__restrict__ mu, const float *__restrict__ rho, float2 *__restrict__ out) {
    const uint32_t q = blockIdx.x * GL_BLOCK + threadIdx.x;                            // one pair per lane: the grid covers n
    if (q < n) {
        float A, B;
        ggx_table_fetch(table, n_mu, n_rho, mu[q], rho[q], A, B);
        out[q] = make_float2(A, B);
    }
}

// the split sum's term F0 A + B with (A, B) from the table at (cos, rho), times 1 + F0 (1 / (A + B) - 1) under FW_SPLIT_ENERGY; where
// nothing is seen the table is read at cos = 0
struct TableTerm {
    const float2 *__restrict__ table; uint32_t n_mu, n_rho, flags;
    static constexpr double UNSEEN = 0.0;
    __device__ __forceinline__ void operator()(double cost, const float4 &sp, float &s0, float &s1, float &s2) const {
        float A, B;
        ggx_table_fetch(table, n_mu, n_rho, (float)cost, sp.w, A, B);
        s0 = sp.x * A + B; s1 = sp.y * A + B; s2 = sp.z * A + B;
        if (flags & 1u) {                                                              // FW_SPLIT_ENERGY
            const float e1 = A + B;
            const float g = e1 > 0.f ? 1.f / e1 - 1.f : 0.f;
            s0 = s0 * (1.f + sp.x * g); s1 = s1 * (1.f + sp.y * g); s2 = s2 * (1.f + sp.z * g);
        }
    }
};

template <bool DEPTH>
__global__ __launch_bounds__(GL_BLOCK) void k_probe_split_shade(DProbeGrid G, DProbeVis V, DProbeRadiance pr, ShLookupConst K, const float *__restrict__ sh,
                                                                const float4 *__restrict__ maps, const float *__restrict__ placement, uint32_t n,
                                                                const float4 *__restrict__ aov, const float4 *__restrict__ spec,
                                                                const float *__restrict__ view, uint32_t view_stride,
                                                                const float2 *__restrict__ table, uint32_t n_mu, uint32_t n_rho, uint32_t flags,
                                                                float gamma, uint8_t *rgb8, float *gamma_rgb, float *linear_rgb) {
    const uint32_t p = blockIdx.x * GL_BLOCK + threadIdx.x;                            // one pixel per lane: the grid covers n
    if (p < n) shade_glossy_pixel<DEPTH>(G, V, pr, K, sh, maps, placement, p, aov, spec, view, view_stride, gamma, rgb8, gamma_rgb, linear_rgb,
                                         TableTerm{table, n_mu, n_rho, flags});
}

uint32_t gl_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + GL_BLOCK - 1) / GL_BLOCK); }          // n > 0; at most 2^24 blocks

} // namespace

void launch_ggx_terms(hipStream_t stream, int n_cus, uint32_t m1, uint32_t m2, uint32_t k, const float *mu, const float *rho, uint32_t first,
                      uint32_t n_mu, uint32_t n_rho, float *terms) {
    hipLaunchKernelGGL(k_ggx_terms, dim3(grid_for(k, 1u, n_cus, 4u)), dim3(GT_BLOCK), 0, stream, m1, m2, k, mu, rho, first, n_mu, n_rho,
                       (float2 *)terms);                                                // 24 KB of LDS: six per CU would fit
}

void launch_ggx_table_lookup(hipStream_t stream, uint32_t n_mu, uint32_t n_rho, const float *table, uint32_t k, const float *mu, const float *rho,
                             float *terms) {
    hipLaunchKernelGGL(k_ggx_table_lookup, dim3(gl_blocks(k)), dim3(GL_BLOCK), 0, stream, n_mu, n_rho, (const float2 *)table, k, mu, rho, (float2 *)terms);
}

void launch_probe_split_shade(hipStream_t stream, const DProbeGrid &g, const DProbeVis *v, const DProbeRadiance &pr, const float *sh, const float *maps,
                              const float *placement, uint32_t n, const float *aov, const float *spec, const float *view, uint32_t view_stride,
                              const float *table, uint32_t n_mu, uint32_t n_rho, uint32_t flags, float gamma, uint8_t *rgb8, float *gamma_rgb,
                              float *linear_rgb) {
    if (v) hipLaunchKernelGGL(k_probe_split_shade<true>, dim3(gl_blocks(n)), dim3(GL_BLOCK), 0, stream, g, *v, pr, sh_lookup_const(), sh,
                              (const float4 *)maps, placement, n, (const float4 *)aov, (const float4 *)spec, view, view_stride, (const float2 *)table,
                              n_mu, n_rho, flags, gamma, rgb8, gamma_rgb, linear_rgb);
    else hipLaunchKernelGGL(k_probe_split_shade<false>, dim3(gl_blocks(n)), dim3(GL_BLOCK), 0, stream, g, DProbeVis{nullptr, 0.0, 0u}, pr,
                            sh_lookup_const(), sh, (const float4 *)maps, placement, n, (const float4 *)aov, (const float4 *)spec, view, view_stride,
                            (const float2 *)table, n_mu, n_rho, flags, gamma, rgb8, gamma_rgb, linear_rgb);
}

} // namespace fw
