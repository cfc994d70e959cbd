// fw_sky.hip — the analytic sun-and-sky environment for gfx950: single scattering through a Rayleigh and Mie atmosphere, baked into an
// equirectangular map or evaluated along given directions (include/firework_hip.h has the statement, DESIGN.md §9x the design).
//
//   k_sky_map    one lane per texel, a wave = 64 consecutive x of one row (256 x per block, blockIdx.y strides the rows).  The trip counts
//                are NV and NL for every lane, whether or not its ray meets the ground, so the loops are wave-uniform; only the ground's
//                own term (one more D of NL steps) is taken by the lanes that hit.  Accumulators are float64; 12 B go out per texel.
//   k_sky_sun    one workgroup of 256.  It visits the rows within sun_radius + pi / H of the sun's, in ascending order; the lanes stride
//                over x.  A texel is rejected without sampling only when its centre is farther from s than sun_radius + pi / H + 2 pi / W
//                (every sample of a texel lies within pi / (2 H) + pi / W of its centre, so the bound is conservative and no part of the
//                statement).  Pass 1 counts each row's covered samples — integers, added through LDS, so the order of the lanes does not
//                matter — and lane 0 adds (n_j / S^2) Omega_j to A row by row; pass 2 counts again and overwrites each covered texel of
//                the launch's rows with float(L(centre) + E0 T(O) c / A): one rounding, as everywhere else.
//   k_sky_dirs   one lane per direction.
//
// All three evaluate fw_sky.h's sky_radiance.  No atomics, no inline assembly; k_sky_sun alone uses LDS (1 KiB) and barriers, and every
// one of its barriers is reached by all 256 lanes.  Every index is formed from x < W, j < H, q < n.  A texel's value depends on no other
// texel and not on the launch geometry; two runs are bit-equal.
#include "fw_sky.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int SKY_BLOCK = 256;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(SKY_BLOCK) void k_sky_map(DSky K, uint32_t W, uint32_t H, uint32_t first_row, uint32_t n_rows, float *__restrict__ out) {
    const uint32_t x = blockIdx.x * SKY_BLOCK + threadIdx.x;
    if (x >= W) return;
    const double wd = (double)W, hd = (double)H;
    for (uint32_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const uint32_t j = first_row + r;                                              // j < H
        double dx, dy, dz, L[3];
        sky_map_dir((double)x + 0.5, (double)j + 0.5, wd, hd, dx, dy, dz);
        sky_radiance(K, dx, dy, dz, L);
        float *o = out + ((size_t)r * W + x) * 3u;
        o[0] = (float)L[0]; o[1] = (float)L[1]; o[2] = (float)L[2];
    }
}

// the samples of texel (x, j) inside the disc: of the S x S directions at the offsets ((a + 1/2) / S, (b + 1/2) / S)
__device__ __forceinline__ uint32_t disc_count(const DSky &K, double cos_reject, uint32_t x, uint32_t j, double wd, double hd) {
    double dx, dy, dz;
    sky_map_dir((double)x + 0.5, (double)j + 0.5, wd, hd, dx, dy, dz);
    if (sky_dot(dx, dy, dz, K.s[0], K.s[1], K.s[2]) < cos_reject) return 0u;
    const double sd = (double)K.ss;
    uint32_t cnt = 0;
    for (uint32_t b = 0; b < K.ss; b++)
        for (uint32_t a = 0; a < K.ss; a++) {
            sky_map_dir((double)x + ((double)a + 0.5) / sd, (double)j + ((double)b + 0.5) / sd, wd, hd, dx, dy, dz);
            if (sky_dot(dx, dy, dz, K.s[0], K.s[1], K.s[2]) >= K.cos_sr) cnt++;
        }
    return cnt;
}

// Omega_j: the solid angle of one texel of row j (tests/env_dist_ref.omega_row)
__device__ __forceinline__ double omega_row(uint32_t j, double wd, double hd) {
    const double hi = cos(((double)j * SKY_PI) / hd), lo = cos(((double)(j + 1u) * SKY_PI) / hd);
    return ((2.0 * SKY_PI) / wd) * (hi - lo);
}

__device__ __forceinline__ void disc_store(const DSky &K, uint32_t x, uint32_t j, double wd, double hd, double c, double A, float *o) {
    double dx, dy, dz, L[3];
    sky_map_dir((double)x + 0.5, (double)j + 0.5, wd, hd, dx, dy, dz);
    sky_radiance(K, dx, dy, dz, L);
    o[0] = (float)(L[0] + (K.et[0] * c) / A); o[1] = (float)(L[1] + (K.et[1] * c) / A); o[2] = (float)(L[2] + (K.et[2] * c) / A);
}

__global__ __launch_bounds__(SKY_BLOCK) void k_sky_sun(DSky K, DSkyDisc D, uint32_t W, uint32_t H, uint32_t first_row, uint32_t n_rows,
                                                       float *__restrict__ out) {
    __shared__ uint32_t part[SKY_BLOCK];
    __shared__ double area;
    const uint32_t t = threadIdx.x;
    const double wd = (double)W, hd = (double)H, s2 = (double)(K.ss * K.ss);
    double A = 0.0;                                                                    // lane 0's
    for (uint32_t j = D.row_lo; j <= D.row_hi; j++) {                                  // block-uniform bounds, row_hi < H
        uint32_t cnt = 0;
        for (uint32_t x = t; x < W; x += SKY_BLOCK) cnt += disc_count(K, D.cos_reject, x, j, wd, hd);
        part[t] = cnt;
        __syncthreads();
        for (uint32_t m = SKY_BLOCK / 2; m >= 1u; m >>= 1) {
            if (t < m) part[t] += part[t + m];
            __syncthreads();
        }
        if (t == 0u) A = A + ((double)part[0] / s2) * omega_row(j, wd, hd);
        __syncthreads();
    }
    if (t == 0u) area = A;
    __syncthreads();
    A = area;
    if (A == 0.0) {                                                                    // no sample of any texel lies inside the disc
        const uint32_t j = D.fallback / W, x = D.fallback - j * W;                     // fallback < W H
        if (t == 0u && j >= first_row && j - first_row < n_rows)
            disc_store(K, x, j, wd, hd, 1.0, omega_row(j, wd, hd), out + ((size_t)(j - first_row) * W + x) * 3u);
        return;
    }
    const uint32_t lo = max(D.row_lo, first_row), end = min(D.row_hi + 1u, first_row + n_rows);
    for (uint32_t j = lo; j < end; j++)
        for (uint32_t x = t; x < W; x += SKY_BLOCK) {
            const uint32_t cnt = disc_count(K, D.cos_reject, x, j, wd, hd);
            if (cnt) disc_store(K, x, j, wd, hd, (double)cnt / s2, A, out + ((size_t)(j - first_row) * W + x) * 3u);
        }
}

__global__ __launch_bounds__(SKY_BLOCK) void k_sky_dirs(DSky K, uint32_t n, const float *__restrict__ dirs, uint32_t stride, float *__restrict__ out) {
    for (uint32_t q = blockIdx.x * SKY_BLOCK + threadIdx.x; q < n; q += gridDim.x * SKY_BLOCK) {
        const float *p = dirs + (size_t)q * stride;
        const double rx = (double)p[0], ry = (double)p[1], rz = (double)p[2];
        const double l2 = sky_dot(rx, ry, rz, rx, ry, rz);
        double L[3] = {0.0, 0.0, 0.0};
        if (l2 > 0.0 && finite_d(l2)) {                                                // false for a NaN component too
            const double l = sqrt(l2);
            const double dx = rx / l, dy = ry / l, dz = rz / l;
            sky_radiance(K, dx, dy, dz, L);
            if ((K.flags & 1u) && sky_dot(dx, dy, dz, K.s[0], K.s[1], K.s[2]) >= K.cos_sr)
                for (int c = 0; c < 3; c++) L[c] = L[c] + K.disc_l[c];
        }
        float *o = out + (size_t)q * 3u;
        o[0] = (float)L[0]; o[1] = (float)L[1]; o[2] = (float)L[2];
    }
}

} // namespace

void launch_sky_map(hipStream_t stream, int n_cus, const DSky &sky, uint32_t width, uint32_t height, uint32_t first_row, uint32_t n_rows, float *out) {
    const uint32_t gx = (width + (uint32_t)SKY_BLOCK - 1u) / (uint32_t)SKY_BLOCK;
    const uint32_t gy = std::min<uint32_t>(n_rows, 65535u);
    (void)n_cus;
    hipLaunchKernelGGL(k_sky_map, dim3(gx, gy), dim3(SKY_BLOCK), 0, stream, sky, width, height, first_row, n_rows, out);
}

void launch_sky_sun(hipStream_t stream, const DSky &sky, const DSkyDisc &disc, uint32_t width, uint32_t height, uint32_t first_row, uint32_t n_rows,
                    float *out) {
    hipLaunchKernelGGL(k_sky_sun, dim3(1), dim3(SKY_BLOCK), 0, stream, sky, disc, width, height, first_row, n_rows, out);
}

void launch_sky_dirs(hipStream_t stream, int n_cus, const DSky &sky, uint32_t n, const float *dirs, uint32_t stride, float *out) {
    hipLaunchKernelGGL(k_sky_dirs, dim3(grid_for(n, SKY_BLOCK, n_cus, 32u)), dim3(SKY_BLOCK), 0, stream, sky, n, dirs, stride, out);
}

} // namespace fw
