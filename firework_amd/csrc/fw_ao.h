// fw_ao.h — what the host runtime (fw_runtime.cpp) and the ambient-occlusion kernels (fw_ao.hip) share.  A header of its own, so that the
// translation units of the other .hip files read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// The surface points of a call as the three kernels address them (include/firework_hip.h has the statement): point q of the call is
// id = ids ? ids[q] : q, its position and normal three floats each at id x stride.
struct DAoPoints {
    const float *positions;     // device memory, 4-byte aligned
    const float *normals;       // device memory, 4-byte aligned
    const uint32_t *ids;        // device memory, distinct entries, or nullptr
    uint32_t stride;            // floats, >= 3
};

// The rays of one round as k_ao_rays needs them.
struct DAoRays {
    DAoPoints pts;
    uint32_t first;             // the launch covers the points [first, first + n) of the call
    uint32_t directions;        // D
    uint32_t seed32;            // the folded 64-bit seed of the shifts
    uint32_t jitter;            // 0: the shift (1/2, 1/2)
    uint32_t round;
    float bias;
};

// n x D x 6 floats at `out`: entry q D + j is direction j of point first + q; D zero rays for an unusable point.  n x D < 2^31.
void launch_ao_rays(hipStream_t stream, int n_cus, const DAoRays &r, uint32_t n, float *out);
// sums[id(first + q)] += float((1 / D) sum_j term_j) for q < n, per accumulator (Bx, By, Bz, O).  rays n x D x 6 floats, hits n x D records
// of 48 B (16-byte aligned), both starting at point `first`; sums 16-byte aligned records indexed by id.
void launch_ao_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t directions, uint32_t falloff, float radius,
                      const uint32_t *ids, const float *rays, const void *hits, float *sums);
// out[id(q)] = (bent.xyz, ao) from sums[id(q)] after `rounds` rounds in all, for q < n
void launch_ao_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out);

} // namespace fw
