// fw_build.h — the device tree builders (fw_build.hip), called by fw_runtime.cpp.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace fw {

enum BuildTree { BUILD_MEDIAN = 0, BUILD_SAH = 1 };

struct DeviceBuildTimes { double upload_ms = 0, kernel_ms = 0, copy_ms = 0; };

// Builds one tree over n item boxes (host memory, n x 6 floats: min.xyz max.xyz) on `device` and copies its FlatBvh node array
// (8 floats per node, depth-first order) back into `nodes`, its depth into `depth`:
//   BUILD_MEDIAN  the reference's median-split tree (fw_runtime.cpp bvh_build: bvh.rs:21-71),
//   BUILD_SAH     the binned-SAH tree (fw_runtime.cpp sah_build),
// bit for bit what the host builders give.  Returns FW_OK, FW_ERR_NAN_BBOX (a centre the median tree compares is NaN), FW_ERR_OOM
// or FW_ERR_HIP; `msg` says what failed.  Thread-safe: builds on one device run one at a time, on the builder's own stream and
// scratch memory, so a render in flight on the device is never touched.  It makes `device` current for its own calls and gives the
// calling thread's current device back.
int device_build_tree(int device, BuildTree tree, const float *boxes, uint32_t n, std::vector<float> &nodes, uint32_t &depth,
                      DeviceBuildTimes *times, std::string &msg);

// Frees the builder's memory and stream on `device` (fw_release_workspace).  The caller has made `device` current.
void device_build_release(int device);

} // namespace fw
