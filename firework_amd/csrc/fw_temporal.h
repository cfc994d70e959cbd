// fw_temporal.h — what the host runtime (fw_runtime.cpp) and fw_temporal's kernel (fw_temporal.hip) share.  Kept out of fw_device.h so
// that the translation units of fw_kernels.hip and fw_build.hip read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// the previous camera as the projection needs it: make_camera's basis (camera.rs:74-107) and the half extents of its image plane
struct TpCamera {
    float pos[3], u[3], v[3], w[3];
    float half_width, half_height;
};

// fw_temporal on device arrays (include/firework_hip.h has the statement): one launch of k_tp_reproject on `stream`.  moments, prev_pos and
// every output may be nullptr; hist_color / hist_moments / hist_aov are all nullptr for a first frame.
void launch_temporal(hipStream_t stream, uint32_t W, uint32_t H, const TpCamera &prev_cam, float samples, float max_history, const float *color,
                     const float4 *moments, const float4 *aov, const float *hist_color, const float4 *hist_moments, const float4 *hist_aov,
                     const float *prev_pos, float *out_color, float4 *out_moments, float *out_history);

} // namespace fw
