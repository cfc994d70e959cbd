// fw_camera_models.h — what the host runtime (fw_runtime.cpp) and the camera-model ray generator (fw_camera_models.hip) share.  Kept out of
// fw_device.h so that the translation units of fw_kernels.hip and fw_build.hip read exactly what they read before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fw {

// A camera model as k_model_rays needs it (include/firework_hip.h has the statement): everything that does not depend on the pixel is
// formed on the host in float64.
struct DModel {
    int32_t kind;               // fw_model_kind
    uint32_t width, height;
    uint32_t seed32;            // the folded 64-bit jitter seed
    uint32_t jitter;            // 0: pixel centres
    double pos[3];              // cam_pos
    double u[3], v[3], w[3];    // camera.rs's basis (orthographic, fisheye)
    double dir[3];              // orthographic: look_at - cam_pos
    double view_w, view_h;      // orthographic: the view plane
    double half_fov;            // fisheye: fov / 2 in radians
    double diag;                // fisheye: sqrt(W W + H H)
};

// The rays of the absolute samples [first, first + n) of `m`: n x W*H x 6 floats at `out` (device memory), one launch on `stream`.
// W x H < 2^31 and first + n <= 2^32 (the runtime checks both).
void launch_model_rays(hipStream_t stream, int n_cus, const DModel &m, uint32_t first, uint32_t n, float *out);

} // namespace fw
