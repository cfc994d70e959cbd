// fw_probes.h — what the host runtime (fw_runtime.cpp) and the probe kernels (fw_probes.hip) share.  Kept out of fw_device.h so that the
// translation units of fw_kernels.hip, fw_build.hip, fw_temporal.hip and fw_camera_models.hip read exactly what they read before
// (DESIGN.md §9n).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// A probe set as k_probe_rays needs it (include/firework_hip.h has the statement).
struct DProbes {
    uint32_t directions;        // D
    uint32_t seed32;            // the folded 64-bit seed of the shifts
    uint32_t jitter;            // 0: the shift (1/2, 1/2)
    uint32_t round;
    uint32_t first_probe;       // the absolute index of the first probe written (the shift's `pixel` word)
    const float *positions;     // device memory: the positions of the probes [first_probe, first_probe + n), n x 3
};

// The rays of round `p.round` of the probes [first_probe, first_probe + n): n x D x 6 floats at `out` (device memory), one launch on
// `stream`.  (first_probe + n) x D < 2^31 (the runtime checks it).
void launch_probe_rays(hipStream_t stream, int n_cus, const DProbes &p, uint32_t n, float *out);

// sums[p][k][c] += float((4 pi / D) sum_j Y_k(d_pj) (double)accum[p D + j].c / S) for n probes: rays n x D x 6, accum n x D x 4 (16-byte
// aligned), sums n x 27, all device memory; one launch on `stream`.  n x D < 2^31.
void launch_probe_project(hipStream_t stream, int n_cus, uint32_t n, uint32_t directions, uint32_t samples, const float *rays,
                          const float *accum, float *sums);

} // namespace fw
