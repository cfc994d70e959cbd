// fw_camera_models.hip — the ray generator of the camera models for gfx950 (include/firework_hip.h has the statement, DESIGN.md §9k the
// design).
//
//   k_model_rays   one lane per ray: the pixel's jitter (integer hashes), the model's formulas in float64, one rounding to float32; reads
//                  nothing, writes 24 B per ray.
//
// A wave takes 64 consecutive pixels of one sample — 1 536 contiguous bytes of the output.  Each lane puts its six floats into LDS, and the
// wave stores the block as six dword stores per lane at consecutive addresses (k_camera_rays' transposition in fw_kernels.hip): every store
// instruction covers 256 contiguous bytes instead of 64 lanes 24 bytes apart.  Dword stores, not wider ones: a sample's slab starts at
// s * W*H * 24 bytes, which is 16-byte aligned only for an even W*H.
// One wave per workgroup, so the barrier orders the LDS accesses only.  No atomics, no inline assembly.  The jitter draw and grid_for are
// fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.panorama_rays / orthographic_rays / fisheye_rays;
// sin, cos and sqrt are the device library's float64 functions, a few float64 ulps from the host's: after the rounding to float32 a
// component equals the host's or is its neighbour.
#include "../../include/firework_hip.h"     // FW_MODEL_*
#include "fw_camera_models.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int MR_BLOCK = 64;

__global__ __launch_bounds__(MR_BLOCK) void k_model_rays(DModel m, uint32_t first, uint32_t n_samples, uint32_t n_pix, uint32_t chunks_per_sample,
                                                         float *__restrict__ out) {
    __shared__ float tr[6 * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = (uint64_t)n_samples * chunks_per_sample;
    const double PI = 3.141592653589793;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t s = (uint32_t)(c / chunks_per_sample);
        const uint32_t id0 = (uint32_t)(c - (uint64_t)s * chunks_per_sample) * 64u;      // < n_pix < 2^31
        const uint32_t cnt = min(64u, n_pix - id0);
        if (lane < cnt) {
            const uint32_t p = id0 + lane;
            const uint32_t row = p / m.width, x = p - row * m.width;
            double xi_x = 0.5, xi_y = 0.5;
            if (m.jitter) { const Jitter xi = jitter_pair(m.seed32, first + s, p); xi_x = xi.u; xi_y = xi.v; }
            const double px = (double)x + xi_x, py = (double)row + xi_y;
            const double W = (double)m.width, H = (double)m.height;
            double o0 = m.pos[0], o1 = m.pos[1], o2 = m.pos[2], d0, d1, d2;
            if (m.kind == FW_MODEL_PANORAMA) {
                const double uu = px / W, vv = 1.0 - py / H;
                const double phi = PI - (2.0 * PI) * uu, theta = PI * vv - PI / 2.0;
                const double ct = cos(theta), st = sin(theta);
                d0 = ct * cos(phi); d1 = st; d2 = ct * sin(phi);
            } else if (m.kind == FW_MODEL_ORTHOGRAPHIC) {
                const double a = (px / W - 0.5) * m.view_w, b = ((1.0 - py / H) - 0.5) * m.view_h;
                o0 = (m.pos[0] + a * m.u[0]) + b * m.v[0];
                o1 = (m.pos[1] + a * m.u[1]) + b * m.v[1];
                o2 = (m.pos[2] + a * m.u[2]) + b * m.v[2];
                d0 = m.dir[0]; d1 = m.dir[1]; d2 = m.dir[2];
            } else {                                                       // FW_MODEL_FISHEYE
                const double a = 2.0 * px - W, b = H - 2.0 * py;
                const double rho = sqrt(a * a + b * b);
                d0 = -m.w[0]; d1 = -m.w[1]; d2 = -m.w[2];
                if (rho > 0.0) {
                    const double theta = (rho / m.diag) * m.half_fov;
                    const double st = sin(theta), ct = cos(theta);
                    d0 = st * ((a * m.u[0] + b * m.v[0]) / rho) - ct * m.w[0];
                    d1 = st * ((a * m.u[1] + b * m.v[1]) / rho) - ct * m.w[1];
                    d2 = st * ((a * m.u[2] + b * m.v[2]) / rho) - ct * m.w[2];
                }
            }
            float *d = tr + lane * 6u;
            d[0] = (float)o0; d[1] = (float)o1; d[2] = (float)o2; d[3] = (float)d0; d[4] = (float)d1; d[5] = (float)d2;
        }
        __syncthreads();
        float *dst = out + ((size_t)s * n_pix + id0) * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * 64u + lane; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

} // namespace

void launch_model_rays(hipStream_t stream, int n_cus, const DModel &m, uint32_t first, uint32_t n, float *out) {
    const uint32_t n_pix = m.width * m.height;                               // < 2^31
    const uint32_t cps = (n_pix + 63u) / 64u;
    const uint64_t chunks = (uint64_t)n * cps;
    hipLaunchKernelGGL(k_model_rays, dim3(grid_for(chunks, 1u, n_cus, 128u)), dim3(MR_BLOCK), 0, stream, m, first, n, n_pix, cps, out);
}

} // namespace fw
