// fw_probes.hip — the two kernels of the irradiance-probe baker for gfx950 (include/firework_hip.h has the statement, DESIGN.md §9n the
// design).
//
//   k_probe_rays      one lane per entry (probe p, direction j): the (round, probe) shift (integer hashes), the spherical Fibonacci
//                     direction in float64, one rounding to float32; reads 12 B of position per lane (64 consecutive entries share one
//                     or two probes: the loads hit one or two cache lines), writes 24 B per entry.  Stores are k_model_rays': the six
//                     floats of a lane go through LDS and leave as six dword stores per lane at consecutive addresses.
//   k_probe_project   one wave per probe: lane l takes the entries j = l, l + 64, ... in ascending order, reads the stored float32
//                     direction (12 of the entry's 24 B; the lines are fetched whole) and the entry's 16 B of sums, and keeps 27
//                     float64 partial sums (9 coefficients x 3 channels).  The lanes are then combined by one fixed tree of
//                     __shfl_xor steps (below), the result is rounded to float32 once and added to the probe's 27 running sums.
//                     No atomics, no LDS, no barrier; the result is a pure function of the inputs.
//
// The hashes and the jitter draw are fw_shared.h's.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.ProbeSet.rays / api.sh_project; sin, cos and sqrt are
// the device library's float64 functions, a few float64 ulps from the host's.
#include "fw_probes.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int PR_BLOCK = 64;
constexpr int PP_WAVES = 4;

__global__ __launch_bounds__(PR_BLOCK) void k_probe_rays(DProbes P, uint32_t n_entries, float *__restrict__ out) {
    __shared__ float tr[6 * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = (n_entries + 63u) / 64u;                                    // n_entries < 2^31
    const double PI = 3.141592653589793, G = 0.6180339887498949;                        // G = (sqrt(5) - 1) / 2
    const double Dd = (double)P.directions;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t id0 = c * 64u;
        const uint32_t cnt = min(64u, n_entries - id0);
        if (lane < cnt) {
            const uint32_t i = id0 + lane;
            const uint32_t pl = i / P.directions, j = i - pl * P.directions;
            double xi_u = 0.5, xi_v = 0.5;
            if (P.jitter) { const Jitter xi = jitter_pair(P.seed32, P.round, P.first_probe + pl); xi_u = xi.u; xi_v = xi.v; }     // 2 p + 1 < 2^32
            const double u = ((double)j + xi_u) / Dd;
            const double ct = 1.0 - 2.0 * u;
            const double rad = sqrt(fmax(0.0, 1.0 - ct * ct));
            const double t = (double)j * G + xi_v;
            const double v = t - floor(t);
            const double phi = (2.0 * PI) * v;
            const float *pos = P.positions + (size_t)pl * 3u;
            float *d = tr + lane * 6u;
            d[0] = pos[0]; d[1] = pos[1]; d[2] = pos[2];
            d[3] = (float)(rad * cos(phi)); d[4] = (float)ct; d[5] = (float)(rad * sin(phi));
        }
        __syncthreads();
        float *dst = out + (size_t)id0 * 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) { const uint32_t e = k * 64u + lane; if (e < 6u * cnt) dst[e] = tr[e]; }
        __syncthreads();
    }
}

// the constants of the real orthonormal SH basis up to l = 2, formed in double on the host
struct ShConst { double y0, c1, c2, c6, c8, four_pi; };

__global__ __launch_bounds__(PP_WAVES * 64) void k_probe_project(ShConst K, uint32_t n_probes, uint32_t directions, uint32_t samples,
                                                                 const float *__restrict__ rays, const float4 *__restrict__ accum,
                                                                 float *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * PP_WAVES + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * PP_WAVES;
    const double Sd = (double)samples;
    const double scale = K.four_pi / (double)directions;
    for (uint32_t p = wave; p < n_probes; p += n_waves) {
        const size_t base = (size_t)p * directions;
        double v[32];
#pragma unroll
        for (int i = 0; i < 32; i++) v[i] = 0.0;
        for (uint32_t j = lane; j < directions; j += 64u) {
            const float *r = rays + (base + j) * 6u + 3u;
            const float4 a4 = accum[base + j];
            const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
            const double a[3] = {(double)a4.x / Sd, (double)a4.y / Sd, (double)a4.z / Sd};
            const double Y[9] = {K.y0, K.c1 * y, K.c1 * z, K.c1 * x, (K.c2 * x) * y, (K.c2 * y) * z, K.c6 * (3.0 * (z * z) - 1.0),
                                 (K.c2 * x) * z, K.c8 * (x * x - y * y)};
#pragma unroll
            for (int k = 0; k < 9; k++) {
#pragma unroll
                for (int c = 0; c < 3; c++) v[k * 3 + c] = v[k * 3 + c] + Y[k] * a[c];
            }
        }
        // The tree: five exchange steps with the lanes 32, 16, 8, 4 and 2 away.  At each step a lane keeps one half of its slots and
        // adds the partner's partial sums of that half (the slots 27..31 are zero padding): 16 + 8 + 4 + 2 + 1 = 31 exchanges instead
        // of 27 x 6.  After them lane l holds slot l >> 1 summed over the 32 lanes of its parity; the last step adds the two parities.
        // Every slot's sum is one fixed binary tree over the 64 lanes.
#pragma unroll
        for (int h = 16, m = 32; h >= 1; h >>= 1, m >>= 1) {
            const bool upper = (lane & (uint32_t)m) != 0u;
#pragma unroll
            for (int i = 0; i < h; i++) {
                const double send = upper ? v[i] : v[i + h];
                const double keep = upper ? v[i + h] : v[i];
                v[i] = keep + __shfl_xor(send, m, 64);
            }
        }
        const double total = v[0] + __shfl_xor(v[0], 1, 64);
        const uint32_t slot = lane >> 1;
        if ((lane & 1u) == 0u && slot < 27u) {
            const float proj = (float)(scale * total);
            float *s = sums + (size_t)p * 27u + slot;
            *s = *s + proj;
        }
    }
}

} // namespace

void launch_probe_rays(hipStream_t stream, int n_cus, const DProbes &p, uint32_t n, float *out) {
    const uint32_t n_entries = n * p.directions;                              // < 2^31
    hipLaunchKernelGGL(k_probe_rays, dim3(grid_for(n_entries, 64u, n_cus, 128u)), dim3(PR_BLOCK), 0, stream, p, n_entries, out);
}

void launch_probe_project(hipStream_t stream, int n_cus, uint32_t n, uint32_t directions, uint32_t samples, const float *rays,
                          const float *accum, float *sums) {
    const double PI = 3.141592653589793;
    const ShConst K{0.5 * std::sqrt(1.0 / PI), std::sqrt(3.0 / (4.0 * PI)), 0.5 * std::sqrt(15.0 / PI), 0.25 * std::sqrt(5.0 / PI),
                    0.25 * std::sqrt(15.0 / PI), 4.0 * PI};
    hipLaunchKernelGGL(k_probe_project, dim3(grid_for(n, PP_WAVES, n_cus, 32u)), dim3(PP_WAVES * 64), 0, stream, K, n, directions, samples, rays,
                       (const float4 *)accum, sums);
}

} // namespace fw
