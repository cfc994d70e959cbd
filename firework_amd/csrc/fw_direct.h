// fw_direct.h — what the host runtime (fw_runtime.cpp) and the direct-light kernels (fw_direct.hip) share.  A header of its own, so that
// the translation units of the other .hip files read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// The surface points of a call as the three kernels address them (include/firework_hip.h has the statement): point q of the call is
// id = ids ? ids[q] : q, its position and normal three floats each at id x stride, its view direction three floats at id x view_stride,
// its (F0.rgb, rho) four floats at id x 4.
struct DDirectPoints {
    const float *positions;     // device memory, 4-byte aligned
    const float *normals;       // device memory, 4-byte aligned
    const uint32_t *ids;        // device memory, distinct entries, or nullptr
    const float *view;          // device memory, 4-byte aligned, or nullptr
    const float4 *spec;         // device memory, 16-byte aligned, or nullptr
    uint32_t stride;            // floats, >= 3
    uint32_t view_stride;       // floats, >= 3 (read only with view)
};

// One call's description: the points, the light records (DDeltaLights.rec's three float4 per light) and fw_direct's fields.
struct DDirect {
    DDirectPoints pts;
    const float4 *lights;       // device memory, 3 x n_lights records of 16 B
    uint32_t n_lights;          // Ln >= 1
    uint32_t first;             // the launch covers the points [first, first + n) of the call
    uint32_t lobe;              // 0: c, 1: 2 c^3
    uint32_t face_view;         // 0 / 1; without view it changes nothing
    float bias;
};

// n x Ln x 6 floats at `out`: entry q Ln + i is the shadow ray of point first + q towards light i, or six zeros.  n x Ln < 2^31.
void launch_direct_rays(hipStream_t stream, int n_cus, const DDirect &d, uint32_t n, float *out);
// sums[id(first + q)] += float(accumulator) for q < n and the seven accumulators (E.rgb, N, S.rgb): floats 0..6 of the 32-byte record, the
// eighth is never written.  rays n x Ln x 6 floats, hits n x Ln records of 48 B (16-byte aligned), both starting at point `first`.
void launch_direct_reduce(hipStream_t stream, int n_cus, const DDirect &d, uint32_t n, const float *rays, const void *hits, float *sums);
// out[id(q)] = float(sums[id(q)] / rounds) for q < n: seven floats, the eighth 0
void launch_direct_resolve(hipStream_t stream, uint32_t n, double rounds, const uint32_t *ids, const float *sums, float *out);

} // namespace fw
