// fw_probe_depth.h — what the host runtime (fw_runtime.cpp) and the probe-visibility reduction (fw_probe_depth.hip) share (DESIGN.md
// §9s).  The lookups that weight a probe by the depth maps, and DProbeVis, are fw_probe_lookup.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// sums[p][b][a].xyz += float(A), float(B), float(W) of one round's rays and hits of n probes: rays n x D x 6 floats, hits n x D records
// of 48 B (16-byte aligned), sums n x R x R x 4 floats (16-byte aligned; .w is left alone), all device memory; one launch on `stream`.
// n x D < 2^31 and n x R x R < 2^31 (the runtime checks both).
void launch_probe_depth(hipStream_t stream, uint32_t n, uint32_t directions, uint32_t R, uint32_t sharpness_log2, float max_distance,
                        const float *rays, const void *hits, float *sums);

} // namespace fw
