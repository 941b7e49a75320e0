// What pointcloud.hip and tsdf.hip share: the depth rule and keep predicate of a CloudSel (edv_cloud_selection), its checks, and the one-workgroup
// 64-bit exclusive scan behind both order-preserving compactions.  Everything here is internal to the translation unit that includes it.
// Contraction is off from here to the end of that unit: every fp32 and fp64 operation is numpy's, in the order written.
#pragma once
#include "ops.hpp"

#pragma clang fp contract(off)

namespace edv {
namespace {

using u64 = unsigned long long;

constexpr int SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / WAVE, SCAN_ITEMS = 4;

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

// one workgroup: ws[i] = sum of ws[0 .. i) for the `tiles` counts, offsets[n] = the total; with tiles_per_frame > 0 also
// offsets[f] = ws[f * tiles_per_frame] after the scan (tiles_per_frame == 0, n == 0: the total alone, in offsets[0])
__global__ __launch_bounds__(SCAN_THREADS) void cloud_scan_kernel(u64 *__restrict__ ws, long long tiles, long long tiles_per_frame, long long *__restrict__ offsets,
                                                                  long long n) {
    __shared__ u64 wave_sum_s[SCAN_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    u64 carry = 0;
    for (long long base = 0; base < tiles; base += (long long)SCAN_THREADS * SCAN_ITEMS) {
        const long long i0 = base + (long long)threadIdx.x * SCAN_ITEMS;
        u64 v[SCAN_ITEMS], mine = 0;
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            v[j] = i0 + j < tiles ? ws[i0 + j] : 0;
            mine += v[j];
        }
        u64 inc = mine;  // inclusive over the lanes of the wave
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const u64 up = __shfl_up(inc, o, WAVE);
            if (lane >= o) inc += up;
        }
        if (lane == WAVE - 1) wave_sum_s[wave] = inc;
        __syncthreads();
        u64 before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < SCAN_WAVES; ++k) {
            const u64 t = wave_sum_s[k];
            before += k < wave ? t : 0;
            total += t;
        }
        u64 ex = carry + before + (inc - mine);
#pragma unroll
        for (int j = 0; j < SCAN_ITEMS; ++j) {
            const long long i = i0 + j;
            if (i < tiles) {
                ws[i] = ex;
                if (tiles_per_frame > 0 && i % tiles_per_frame == 0) offsets[i / tiles_per_frame] = (long long)ex;
                ex += v[j];
            }
        }
        carry += total;
        __syncthreads();  // wave_sum_s is rewritten by the next round
    }
    if (threadIdx.x == 0) offsets[n] = (long long)carry;
}

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

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
