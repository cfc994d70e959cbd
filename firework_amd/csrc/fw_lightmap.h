// fw_lightmap.h — what the host runtime (fw_runtime.cpp) and the lightmap kernels (fw_lightmap.hip) share.  Kept out of fw_device.h so
// that the translation units of fw_kernels.hip, fw_build.hip, fw_temporal.hip, fw_camera_models.hip and fw_probes.hip read exactly what
// they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

constexpr uint32_t LM_NO_OWNER = 0xffffffffu;      // FW_NO_HIT

// One mesh placement and a texture size as k_lm_cover and k_lm_texels need them (include/firework_hip.h has the statement).
struct DLightmapMesh {
    const float *verts;         // device memory, n_verts x 3
    const uint32_t *indices;    // device memory, n_tris x 3, every index < n_verts (the runtime checks it)
    const float *normals;       // device memory, n_verts x 3, or nullptr: the geometric normal
    const float *uvs;           // device memory, n_verts x 2
    uint32_t n_tris;
    uint32_t width, height;
    uint32_t rotated;           // 1/2 (tr R - 1) < 0.999: rows is applied; otherwise only the translation
    uint32_t negate;            // flip_normals xor flip
    float rows[3][3];           // rotor_rows of the placement
    float position[3];
};

// The rays of one round as k_lm_rays needs them.
struct DLightmapRays {
    uint32_t directions;        // D
    uint32_t seed32;            // the folded 64-bit seed of the shifts
    uint32_t jitter;            // 0: the shift (1/2, 1/2)
    uint32_t round;
    float bias;
    const uint32_t *texel_ids;  // device memory: the covered list's entries [first, first + n)
    const float4 *records;      // device memory: W x H records of two float4 each, indexed by texel id
};

// owner[texel] = min(owner[texel], t) for every texel whose centre lies in UV triangle t; owner (W x H) starts as LM_NO_OWNER.
void launch_lm_cover(hipStream_t stream, int n_cus, const DLightmapMesh &m, uint32_t *owner);
// records[texel] = (position.xyz, owner bits), (normal.xyz, 0); a texel without a usable position or normal loses its owner.
void launch_lm_texels(hipStream_t stream, int n_cus, const DLightmapMesh &m, uint32_t *owner, float4 *records);
// n x D x 6 floats at `out`: entry q D + j is direction j of texel texel_ids[q].  n x D < 2^31.
void launch_lm_rays(hipStream_t stream, int n_cus, const DLightmapRays &r, uint32_t n, float *out);
// sums[tid(q)].c += float((pi / D) sum_j (double)accum[q D + j].c / S) for q < n; tid(q) = texel_ids ? texel_ids[q] : q, all distinct.
void launch_lm_reduce(hipStream_t stream, int n_cus, uint32_t n, uint32_t directions, uint32_t samples, const uint32_t *texel_ids,
                      const float *accum, float *sums);
// out[texel] = owner[texel] != LM_NO_OWNER ? (float(sums.xyz / rounds), 1) : 0
void launch_lm_resolve(hipStream_t stream, uint32_t n_texels, double rounds, const uint32_t *owner, const float *sums, float *out);
// one dilation pass from `in` to `out` (W x H x 4 floats each, distinct buffers)
void launch_lm_dilate(hipStream_t stream, uint32_t width, uint32_t height, const float *in, float *out);

} // namespace fw
