// fw_temporal.hip — fw_temporal's kernel for gfx950 (include/firework_hip.h has the statement, DESIGN.md §9j the design).
//
//   k_tp_reproject   one thread per current pixel: reads its record (colour, moments, guides: 76 B), projects its previous world position
//                    with the previous camera, gathers up to four bilinear taps of the history (76 B each, shared between neighbours
//                    through L2), tests each tap geometrically and merges by sample counts; writes 32 B.
//
// 16 x 16 tiles, thread t = pixel (t & 15, t >> 4) of its tile: a wave is a 16 x 4 block of pixels, so under a coherent camera motion
// its taps fall into a compact region of the previous frame.  No atomics, no LDS, no inline assembly: every output is one thread's.
//
// Numerics: -ffp-contract=off, + - * IEEE as written; division is fw_shared.h's fdiv and the square root fw_kernels.hip's fsqrt, written
// out below (the same correctly rounded bits).
#include "../../include/firework_hip.h"     // FW_DENOISE_EPS, FW_TEMPORAL_*
#include "fw_temporal.h"
#include "fw_shared.h"          // fdiv, finite_f

namespace fw {
namespace {

constexpr uint32_t TP_TILE = 16;
constexpr int TP_BLOCK = 256;

// fw_kernels.hip's fsqrt (see there for why): v_sqrt_f32 corrected by the exact residuals of its neighbours.
__device__ __forceinline__ float fsqrt(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
    float vd = fmaf(-sd, s, x), vu = fmaf(-su, s, x);
    s = (vd <= 0.f) ? sd : s;
    s = (vu > 0.f) ? su : s;
    return s;
}
__device__ __forceinline__ bool finite3(float x, float y, float z) { return finite_f(x) && finite_f(y) && finite_f(z); }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__global__ __launch_bounds__(TP_BLOCK) void k_tp_reproject(uint32_t W, uint32_t H, uint32_t tiles_x, TpCamera cam, float samples, float max_history,
                                                           const float *color, const float4 *moments, const float4 *aov,
                                                           const float *__restrict__ hist_color, const float4 *__restrict__ hist_moments,
                                                           const float4 *__restrict__ hist_aov, const float *prev_pos, float *out_color,
                                                           float4 *out_moments, float *out_history) {
    const uint32_t px = (blockIdx.x % tiles_x) * TP_TILE + (threadIdx.x & 15u), py = (blockIdx.x / tiles_x) * TP_TILE + (threadIdx.x >> 4);
    if (px >= W || py >= H) return;
    const size_t p = (size_t)py * W + px;
    const float eps = FW_DENOISE_EPS;
    const float cr = color[3 * p], cg = color[3 * p + 1], cb = color[3 * p + 2];
    float4 cur;                                                  // (Q_c, n_c)
    if (moments) cur = moments[p];
    else cur = make_float4(samples * (cr * cr), samples * (cg * cg), samples * (cb * cb), samples);
    float o_r = cr, o_g = cg, o_b = cb, n_h = 0.f;
    float4 o_m = cur;
    if (hist_color) {
        const float4 a = aov[3 * p], nd = aov[3 * p + 1], xa = aov[3 * p + 2];
        float X0 = xa.x, X1 = xa.y, X2 = xa.z;
        if (prev_pos) { X0 = prev_pos[3 * p]; X1 = prev_pos[3 * p + 1]; X2 = prev_pos[3 * p + 2]; }
        const float nl = fsqrt(dot3(nd.x, nd.y, nd.z, nd.x, nd.y, nd.z));
        // 1: pass-through; a zero or non-finite normal fails every tap's normal test
        if (a.w != 0.f && finite3(cr, cg, cb) && finite3(X0, X1, X2) && nl > 0.f && finite_f(nl)) {
            const float n0 = fdiv(nd.x, nl), n1 = fdiv(nd.y, nl), n2 = fdiv(nd.z, nl);
            // 2: project X with the previous camera
            const float e0 = X0 - cam.pos[0], e1 = X1 - cam.pos[1], e2 = X2 - cam.pos[2];
            const float depth = -dot3(e0, e1, e2, cam.w[0], cam.w[1], cam.w[2]);
            const float Wf = (float)W, Hf = (float)H;
            float x = -2.f, row = -2.f;
            if (depth > 0.f) {
                const float u = 0.5f + fdiv(dot3(e0, e1, e2, cam.u[0], cam.u[1], cam.u[2]), (2.f * cam.half_width) * depth);
                const float v = 0.5f + fdiv(dot3(e0, e1, e2, cam.v[0], cam.v[1], cam.v[2]), (2.f * cam.half_height) * depth);
                x = u * Wf - 0.5f;
                row = Hf - (v * Hf - 0.5f);
            }
            // the range test first (false for NaN), the conversion to an integer only inside it: floor(x) is in [-1, W - 1]
            if (x > -1.f && x < Wf && row > -1.f && row < Hf) {
                const float fx = floorf(x), fy = floorf(row);
                const long long ix = (long long)fx, iy = (long long)fy;
                const float bx = x - fx, by = row - fy;
                const float plane_max = FW_TEMPORAL_PLANE * fsqrt(dot3(e0, e1, e2, e0, e1, e2));
                // 3: the taps.  b[k] = 0 marks a dropped tap; t_* hold a survivor's terms until the weights are renormalised
                float b[4], t_n[4], t_m[4][3], t_q[4][3];
                float sw = 0.f;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int dx = k & 1, dy = k >> 1;
                    b[k] = 0.f; t_n[k] = 0.f;
                    t_m[k][0] = t_m[k][1] = t_m[k][2] = 0.f; t_q[k][0] = t_q[k][1] = t_q[k][2] = 0.f;
                    const long long qx = ix + dx, qy = iy + dy;
                    if (qx < 0 || qy < 0 || qx >= (long long)W || qy >= (long long)H) continue;
                    const float wq = (dx ? bx : 1.f - bx) * (dy ? by : 1.f - by);
                    if (!(wq >= FW_TEMPORAL_MIN_TAP)) continue;
                    const size_t q = (size_t)qy * W + (size_t)qx;
                    const float4 hm = hist_moments[q];
                    if (!(finite3(hm.x, hm.y, hm.z) && finite_f(hm.w) && hm.w > 0.f)) continue;
                    const float4 ha = hist_aov[3 * q];
                    if (!(finite3(ha.x, ha.y, ha.z) && finite_f(ha.w) && ha.w != 0.f)) continue;
                    const float hr = hist_color[3 * q], hg = hist_color[3 * q + 1], hb = hist_color[3 * q + 2];
                    if (!finite3(hr, hg, hb)) continue;
                    const float4 hx = hist_aov[3 * q + 2];
                    if (!finite3(hx.x, hx.y, hx.z)) continue;
                    const float4 hn = hist_aov[3 * q + 1];
                    const float ql = fsqrt(dot3(hn.x, hn.y, hn.z, hn.x, hn.y, hn.z));
                    if (!(ql > 0.f && finite_f(ql))) continue;
                    const float cosq = dot3(n0, n1, n2, fdiv(hn.x, ql), fdiv(hn.y, ql), fdiv(hn.z, ql));
                    if (!(cosq >= FW_TEMPORAL_NORMAL_COS)) continue;
                    const float pd = fabsf(dot3(n0, n1, n2, hx.x - X0, hx.y - X1, hx.z - X2));
                    if (!(pd <= plane_max)) continue;
                    const float ar = ha.x + eps, ag = ha.y + eps, ab = ha.z + eps;
                    b[k] = wq; sw += wq; t_n[k] = hm.w;
                    t_m[k][0] = fdiv(hr, ar); t_m[k][1] = fdiv(hg, ag); t_m[k][2] = fdiv(hb, ab);
                    t_q[k][0] = fdiv(fdiv(hm.x, hm.w), ar * ar); t_q[k][1] = fdiv(fdiv(hm.y, hm.w), ag * ag); t_q[k][2] = fdiv(fdiv(hm.z, hm.w), ab * ab);
                }
                if (sw > 0.f) {
                    // 4: resample in demodulated space with the weights renormalised over the survivors (one survivor: exactly 1)
                    float sn = 0.f, sm[3] = {0.f, 0.f, 0.f}, sq[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float bk = fdiv(b[k], sw);
                        sn += bk * t_n[k];
#pragma unroll
                        for (int c = 0; c < 3; c++) { sm[c] += bk * t_m[k][c]; sq[c] += bk * t_q[k][c]; }
                    }
                    const float ar = a.x + eps, ag = a.y + eps, ab = a.z + eps;
                    const float nh = sn < max_history ? sn : max_history;
                    // 5: merge by sample counts
                    const float n = nh + cur.w;
                    const float m_r = fdiv(nh * (ar * sm[0]) + cur.w * cr, n), m_g = fdiv(nh * (ag * sm[1]) + cur.w * cg, n),
                                m_b = fdiv(nh * (ab * sm[2]) + cur.w * cb, n);
                    const float4 m_m = make_float4(nh * ((ar * ar) * sq[0]) + cur.x, nh * ((ag * ag) * sq[1]) + cur.y, nh * ((ab * ab) * sq[2]) + cur.z, n);
                    if (finite3(m_r, m_g, m_b) && finite3(m_m.x, m_m.y, m_m.z) && finite_f(n)) {
                        o_r = m_r; o_g = m_g; o_b = m_b; o_m = m_m; n_h = nh;
                    }
                }
            }
        }
    }
    if (out_color) { out_color[3 * p] = o_r; out_color[3 * p + 1] = o_g; out_color[3 * p + 2] = o_b; }
    if (out_moments) out_moments[p] = o_m;
    if (out_history) out_history[p] = n_h;
}

} // namespace

void launch_temporal(hipStream_t stream, uint32_t W, uint32_t H, const TpCamera &prev_cam, float samples, float max_history, const float *color,
                     const float4 *moments, const float4 *aov, const float *hist_color, const float4 *hist_moments, const float4 *hist_aov,
                     const float *prev_pos, float *out_color, float4 *out_moments, float *out_history) {
    const uint32_t tiles_x = (uint32_t)(((uint64_t)W + TP_TILE - 1) / TP_TILE);            // W x H < 2^32: the tile count fits
    const uint32_t tiles = tiles_x * (uint32_t)(((uint64_t)H + TP_TILE - 1) / TP_TILE);
    hipLaunchKernelGGL(k_tp_reproject, dim3(tiles), dim3(TP_BLOCK), 0, stream, W, H, tiles_x, prev_cam, samples, max_history, color, moments, aov,
                       hist_color, hist_moments, hist_aov, prev_pos, out_color, out_moments, out_history);
}

} // namespace fw
