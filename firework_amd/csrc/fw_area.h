// fw_area.h — what the host runtime (fw_runtime.cpp) and the area-light kernels (fw_area.hip) share.  A header of its own, so that the
// translation units of the other .hip files read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fw_ao.h"

namespace fw {

// The shadow rays of one round as k_area_rays needs them.  lights: n_lights records of four float4 (FW_LIGHT_RECORD_FLOATS = 16 floats:
// object, kind, 12 geometry floats, area, p_pick) in device memory, 16-byte aligned.
struct DAreaRays {
    DAoPoints pts;
    const float4 *lights;
    uint32_t n_lights;          // Ln >= 1
    uint32_t samples;           // S >= 1
    uint32_t first;             // the launch covers the points [first, first + n) of the call
    uint32_t seed32;            // the folded 64-bit seed of the shifts
    uint32_t jitter;            // 0: the shift (1/2, 1/2)
    uint32_t round;
    float bias;
};

// n x Ln x S x 6 floats at `rays` and as many floats at `weights`: entry (q Ln + i) S + s is sample s of light i seen from point
// first + q; a dead entry is six zeros and the weight 0.  n x Ln x S < 2^31.
void launch_area_rays(hipStream_t stream, int n_cus, const DAreaRays &r, uint32_t n, float *rays, float *weights);
// sums[id(first + q)] += float((1 / S) E.rgb, (1 / M) V) over the M = Ln x S entries of point q < n.  weights n x M floats, hits n x M
// records of 48 B, surface n x M records of 64 B (16-byte aligned), all three starting at point `first`; objects: the Ln lights' object
// indices; sums 16-byte records indexed by id.  n x M < 2^31.
void launch_area_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t n_lights, uint32_t samples, const uint32_t *ids,
                        const uint32_t *objects, const float *weights, const void *hits, const float *surface, float *sums);
// out[id(q)] = float(sums[id(q)] / rounds) for q < n and the four floats
void launch_area_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out);
// surface record e < n becomes (kind -2, every other float 0) where its kind is 3 and hit e's object is one of the n_objects ascending
// `objects`; every other record keeps its bits
void launch_area_mask(hipStream_t stream, int n_cus, uint32_t n, const uint32_t *objects, uint32_t n_objects, const void *hits, float *surface);

} // namespace fw
