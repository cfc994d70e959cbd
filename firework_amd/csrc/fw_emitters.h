// fw_emitters.h — what the host runtime (fw_runtime.cpp) and the kernels that sample every emitter at surface points (fw_emitters.hip)
// share.  A header of its own, so that the translation units of the other .hip files read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fw_ao.h"

namespace fw {

// The shadow rays of one round as k_emitters_rays needs them.  records: n_entries records of four float4 (FW_EMITTERS_RECORD_FLOATS = 16
// floats: object, kind, 12 geometry floats, area, weight) in device memory, 16-byte aligned; cdf: n_entries float64, non-decreasing, in
// [0, 1], the last one 1 (fw_emitters_cdf's), 8-byte aligned.
struct DEmittersRays {
    DAoPoints pts;
    const float4 *records;
    const double *cdf;
    uint32_t n_entries;         // N >= 1, <= 2^24
    uint32_t samples;           // S >= 1
    uint32_t first;             // the launch covers the points [first, first + n) of the call
    uint32_t seed32;            // the folded 64-bit seed of the shifts
    uint32_t jitter;            // 0: the shift (1/2, 1/2)
    uint32_t round;
    float bias;
};

// n x S x 6 floats at `rays`, as many floats at `weights` and as many words at `picks`: entry q S + s is sample s from point first + q,
// picks its entry index; a dead entry is six zeros, the weight 0 and the pick 0xffffffff.  n x S < 2^31.
void launch_emitters_rays(hipStream_t stream, int n_cus, const DEmittersRays &r, uint32_t n, float *rays, float *weights, uint32_t *picks);
// sums[id(first + q)] += float((1 / S) E.rgb, (1 / S) V) over the S entries of point q < n.  picks and weights n x S words, hits n x S
// records of 48 B, surface n x S records of 64 B (16-byte aligned), all four starting at point `first`; codes: (object, prim) of each of
// the n_entries entries; sums 16-byte records indexed by id.  n x S < 2^31.
void launch_emitters_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t samples, const uint32_t *ids, const uint32_t *codes,
                            uint32_t n_entries, const uint32_t *picks, const float *weights, const void *hits, const float *surface, float *sums);

} // namespace fw
