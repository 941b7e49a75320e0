// What pointcloud.hip, tsdf.hip and tsdf_track.hip share: the depth rule and keep predicate of a CloudSel (edv_cloud_selection), the source pixel
// of an output pixel of its subsampled grid, and its checks.
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

// output pixel q = oy * ow + ox of the subsampled grid -> the source pixel that holds the grid position ((ox + 0.5) * step, (oy + 0.5) * step)
__device__ __forceinline__ int source_pixel(const CloudSel &s, int ow, unsigned q, int &ox, int &oy) {
    oy = (int)(q / (unsigned)ow), ox = (int)(q - (unsigned)oy * (unsigned)ow);
    const long long sy = min((long long)oy * s.step + s.step / 2, (long long)s.h - 1);
    const long long sx = min((long long)ox * s.step + s.step / 2, (long long)s.w - 1);
    return (int)(sy * s.w + sx);  // h * w < 2^31
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
