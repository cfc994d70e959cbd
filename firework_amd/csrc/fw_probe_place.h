// fw_probe_place.h — what the host runtime (fw_runtime.cpp) and the probe-placement kernels (fw_probe_place.hip) share.
// The lookups over placed probes are fw_probe_lookup.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// The checked fw_probe_relocate, widened once on the host.
struct DRelocate {
    double min_front;           // > 0
    double back_fraction;       // in [0, 1]
    double max_offset[3];       // >= 0, world units per axis
};

// survey[p] = the three float4s of include/firework_hip.h from one round's rays and hits of n probes: rays n x D x 6 floats, hits n x D
// records of 48 B (16-byte aligned), survey n x 12 floats (16-byte aligned, overwritten), all device memory; one launch on `stream`.
// n x D < 2^31 (the runtime checks it).
void launch_probe_survey(hipStream_t stream, int n_cus, uint32_t n, uint32_t directions, const float *rays, const void *hits, float *survey);

// One relocation step of n probes: survey n x 12 floats and placement n x 4 floats, both device memory and 16-byte aligned.  move == 0
// writes placement[p].w only.
void launch_probe_relocate_step(hipStream_t stream, const DRelocate &rl, uint32_t n, uint32_t directions, const float *survey, float *placement,
                                int move);

} // namespace fw
