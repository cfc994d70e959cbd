// fw_probe_depth.hip — probe visibility for gfx950: the reduction of traced distances into per-probe depth moments (include/firework_hip.h
// has the statement, DESIGN.md §9s the design).  The lookups that weight a probe by these moments are fw_probe_lookup.hip's, over
// fw_probe_corners.h; the texel centres are fw_shared.h's.
//
//   k_probe_depth           one workgroup of 256 lanes per probe.  256 directions at a time, lane l turns ray and hit c0 + l (12 B of
//                           direction, 4 B of t and 4 B of object) into (d.xyz, dist) in float64 and stages the 32 B in LDS; after the
//                           barrier every lane walks the staged chunk in ascending j for its texels t = lane, lane + 256, ... (at most
//                           four, R = 32).  All lanes read the same LDS address at once: a broadcast, no bank conflict.  A texel's three
//                           float64 accumulators stay in registers across the chunks; at the end each is rounded to float32 once and
//                           added to the texel's running sums with one float32 addition (.w is neither read nor written).  A texel is
//                           one lane's and its sum is sequential in j, so the result is a pure function of the inputs: no atomics, and
//                           no dependence on the launch geometry.  With R = 4 only 16 lanes of a workgroup have a texel; that is accepted
//                           (the trace beside it is the cost of a bake).
//
// No inline assembly.
//
// Numerics: -ffp-contract=off, so + - * / round as written and in the order of api.probe_depth_reduce; min, max and fabs are exact; sqrt
// is the device library's float64 function.
#include "fw_probe_depth.h"
#include "fw_shared.h"

namespace fw {
namespace {

constexpr int PD_BLOCK = 256;
constexpr int PD_MAXT = 4;                      // texels per lane at R = 32

__global__ __launch_bounds__(PD_BLOCK) void k_probe_depth(uint32_t n_probes, uint32_t directions, uint32_t R, uint32_t k, double r_max,
                                                          const float *__restrict__ rays, const uint32_t *__restrict__ hits,
                                                          float *__restrict__ sums) {
    __shared__ double st[PD_BLOCK * 4];                                                 // (dx, dy, dz, dist) of the staged directions
    const uint32_t lane = threadIdx.x;
    const uint32_t n_tex = R * R;
    const uint32_t nq = (n_tex + PD_BLOCK - 1u) / PD_BLOCK;                             // wave-uniform: 1, or 4 at R = 32
    double T[PD_MAXT][3];
#pragma unroll
    for (int q = 0; q < PD_MAXT; q++) {
        T[q][0] = T[q][1] = T[q][2] = 0.0;
        const uint32_t t = lane + (uint32_t)q * PD_BLOCK;
        if (t < n_tex) texel_dir(t, R, T[q]);
    }
    for (uint32_t p = blockIdx.x; p < n_probes; p += gridDim.x) {
        const size_t base = (size_t)p * directions;                                    // < 2^31
        double A[PD_MAXT], B[PD_MAXT], W[PD_MAXT];
#pragma unroll
        for (int q = 0; q < PD_MAXT; q++) { A[q] = 0.0; B[q] = 0.0; W[q] = 0.0; }
        for (uint32_t c0 = 0; c0 < directions; c0 += PD_BLOCK) {
            const uint32_t cnt = min((uint32_t)PD_BLOCK, directions - c0);
            if (lane < cnt) {
                const size_t e = base + c0 + lane;
                const float *r = rays + e * 6u + 3u;
                const uint32_t *h = hits + e * 12u;
                const double dx = (double)r[0], dy = (double)r[1], dz = (double)r[2];
                double dist = r_max;
                if (h[10] != 0xFFFFFFFFu) dist = fmin((double)__uint_as_float(h[0]) * sqrt((dx * dx + dy * dy) + dz * dz), r_max);
                double *s = st + lane * 4u;
                s[0] = dx; s[1] = dy; s[2] = dz; s[3] = dist;
            }
            __syncthreads();
            for (uint32_t j = 0; j < cnt; j++) {
                const double dx = st[j * 4u], dy = st[j * 4u + 1u], dz = st[j * 4u + 2u], dist = st[j * 4u + 3u];
#pragma unroll
                for (int q = 0; q < PD_MAXT; q++) {
                    if ((uint32_t)q < nq && lane + (uint32_t)q * PD_BLOCK < n_tex) {
                        double w = fmax(0.0, (T[q][0] * dx + T[q][1] * dy) + T[q][2] * dz);
                        for (uint32_t s = 0; s < k; s++) w = w * w;
                        const double wd = w * dist;
                        A[q] = A[q] + wd;
                        B[q] = B[q] + wd * dist;
                        W[q] = W[q] + w;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < PD_MAXT; q++) {
            const uint32_t t = lane + (uint32_t)q * PD_BLOCK;
            if (t < n_tex) {
                float *s = sums + ((size_t)p * n_tex + t) * 4u;                         // < 2^33 floats
                s[0] = s[0] + (float)A[q]; s[1] = s[1] + (float)B[q]; s[2] = s[2] + (float)W[q];
            }
        }
    }
}

} // namespace

void launch_probe_depth(hipStream_t stream, uint32_t n, uint32_t directions, uint32_t R, uint32_t sharpness_log2, float max_distance,
                        const float *rays, const void *hits, float *sums) {
    hipLaunchKernelGGL(k_probe_depth, dim3(n), dim3(PD_BLOCK), 0, stream, n, directions, R, sharpness_log2, (double)max_distance, rays,
                       (const uint32_t *)hits, sums);                                   // n < 2^27: one workgroup per probe
}

} // namespace fw
