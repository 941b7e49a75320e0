// Source coordinates and the four-tap blend of F.interpolate(mode="bilinear", align_corners=True), shared by the kernels that must agree
// bit for bit on an upsampled value (resample.hip: bilinear; stitch.hip: the on-the-fly upsample of the video stitch).
// The index arithmetic follows ATen's upsample kernels: ratio = (in-1)/(out-1) in float, src = ratio*dst, i0 = int(src),
// lambda = src - i0, i1 = i0 + (i0 < in-1).
// Every file that includes this header switches FMA contraction off (#pragma clang fp contract(off)) BEFORE the include: the blend below
// is then the same sequence of rounded products and sums everywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace edv {

__device__ __forceinline__ void lin_coord(int dst, int in, int out, float ratio, int &i0, int &i1, float &l1) {
    if (in == out) {
        i0 = i1 = dst;
        l1 = 0.f;
        return;
    }
    const float src = __fmul_rn(ratio, (float)dst);  // rounded product, as ATen computes it (no FMA into src - i0)
    i0 = (int)src;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}
inline float lin_ratio(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// one output pixel of a single-channel plane pl [H, W]
__device__ __forceinline__ float bilinear_tap(const float *__restrict__ pl, int W, int y0, int y1, int x0, int x1, float ly, float lx) {
    const float v00 = pl[(long long)y0 * W + x0], v01 = pl[(long long)y0 * W + x1];
    const float v10 = pl[(long long)y1 * W + x0], v11 = pl[(long long)y1 * W + x1];
    return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

}  // namespace edv
