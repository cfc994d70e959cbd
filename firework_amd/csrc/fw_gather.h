// fw_gather.h — what the host runtime (fw_runtime.cpp) and the final-gather kernels (fw_gather.hip) share.  A header of its own, so that
// the translation units of the other .hip files read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// sums[id(first + q)] += float(scale x accumulator) for q < n and the four accumulators (L.rgb, sky), id(q) = ids ? ids[q] : q.  surface
// n x D records of 64 B (16-byte aligned) as k_hit_surface writes them, irradiance n x D x 3 floats, direct n x D records of 8 floats
// (floats 0..2 are read) or NULL, all three starting at point `first`; sums 16-byte records indexed by id.  n x D < 2^31.
void launch_gather_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t directions, const uint32_t *ids, const float *surface,
                          const float *irradiance, const float *direct, float *sums);
// out[id(q)] = float(sums[id(q)] / rounds) for q < n and the four floats
void launch_gather_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out);

} // namespace fw
