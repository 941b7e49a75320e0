// What pointcloud.hip and tsdf.hip share: the depth rule and keep predicate of a CloudSel (edv_cloud_selection) and its checks.
// Everything here is internal to the translation unit that includes it.
// Contraction is off from here to the end of that unit: every fp32 and fp64 operation is numpy's, in the order written.
#pragma once
#include "ops.hpp"

#pragma clang fp contract(off)

namespace edv {
namespace {

__device__ __forceinline__ float depth_value(const CloudSel &s, float x) {
    if (s.mode == 0) return x * s.gain;
    const float scaled = s.lo + s.span * x;
    const float z = 1.0f / scaled;
    return z * s.gain;
}

// NaN fails both comparisons, +Inf fails z < far even for far = +Inf
__device__ __forceinline__ bool kept(const CloudSel &s, float x, unsigned m, float &z) {
    z = depth_value(s, x);
    return m != 0 && z > s.near_z && z < s.far_z;
}

inline int check_selection(const CloudSel &s) {
    EDV_CHECK(s.x, "null depth");
    EDV_CHECK(s.n >= 1 && s.n <= 65535, "n must be in 1..65535");
    EDV_CHECK(s.h >= 1 && s.w >= 1 && s.step >= 1, "h, w and step must be at least 1");
    EDV_CHECK((long long)s.h * s.w < (1ll << 31), "a frame beyond 2^31 pixels");
    EDV_CHECK(s.mode == 0 || s.mode == 1, "mode: 0 depth, 1 disparity");
    EDV_CHECK(s.mask_stride == 0 || s.mask_stride == (long long)s.h * s.w, "mask_stride: 0 (one mask for all frames) or h * w (a mask per frame)");
    EDV_CHECK(aligned_to(s.x, 4), "depth not 4-byte aligned");
    return 0;
}

}  // namespace
}  // namespace edv
