// fw_reflect.h — what the host runtime (fw_runtime.cpp) and the reflection-gather kernels (fw_reflect.hip) share.  A header of its own, so
// that the translation units of the other .hip files read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// The glossy receivers of a call as the kernels address them (include/firework_hip.h has the statement): point q of the call is
// id = ids ? ids[q] : q, its position and normal three floats each at id x stride, its view three floats at id x view_stride, its
// (F0.rgb, rho) the float4 spec[id].
struct DReflectPoints {
    const float *positions;     // device memory, 4-byte aligned
    const float *normals;       // device memory, 4-byte aligned
    const uint32_t *ids;        // device memory, distinct entries, or nullptr
    const float *view;          // device memory, 4-byte aligned
    const float4 *spec;         // device memory, 16-byte aligned
    uint32_t stride;            // floats, >= 3
    uint32_t view_stride;       // floats, >= 3
};

// The rays of one round as k_reflect_rays needs them.
struct DReflectRays {
    DReflectPoints pts;
    uint32_t first;             // the launch covers the points [first, first + n) of the call
    uint32_t directions;        // D
    uint32_t seed32;            // the folded 64-bit seed of the shifts
    uint32_t jitter;            // 0: the shift (1/2, 1/2)
    uint32_t round;
    float bias;
};

// n x D x 6 floats at `rays` and n x D x 2 floats (g, s) at `weights` (8-byte aligned): entry q D + j is ray j of point first + q; zeros
// for a dead ray and for every ray of an unusable point.  n x D < 2^31.
void launch_reflect_rays(hipStream_t stream, int n_cus, const DReflectRays &r, uint32_t n, float *rays, float *weights);
// sums[id(first + q)] += float((1 / D) x accumulator) for q < n and the eight accumulators (P.rgb, alive, Q.rgb, sky).  surface n x D
// records of 64 B (16-byte aligned), irradiance n x D x 3 floats, direct n x D records of 8 floats (floats 0..2 are read) or NULL,
// weights n x D x 2 floats (8-byte aligned), all four starting at point `first`; sums 32-byte records indexed by id.  n x D < 2^31.
void launch_reflect_reduce(hipStream_t stream, int n_cus, uint32_t first, uint32_t n, uint32_t directions, const uint32_t *ids, const float *surface,
                           const float *irradiance, const float *direct, const float *weights, float *sums);
// out[id(q)] = (float((f0_c P_c + Q_c) / rounds), float(alive / rounds)) for q < n, f0 = spec[id(q)].xyz
void launch_reflect_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *spec, const float *sums, float *out);

} // namespace fw
