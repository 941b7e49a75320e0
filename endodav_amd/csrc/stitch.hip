// Whole-video stitching on the device (reference models/endodav/endodav.py:213-254 with utils/util.py:40-74; host counterpart
// video.stitch_windows):
//   stitch_fit    least-squares (s, t) with s*p + t ~ tail over the 8 overlap frames of a window, p = window slots 2..9 upsampled on the fly
//   stitch_apply  max(p*s + t, 0) for slots 10..31 as new frames, and the linear cross-fade of slots 2..9 in place over the tail
// Both read the window's NETWORK-size disparity [32, ih, iw] (8 MB at 224 x 280: it stays in L2 / MALL) and upsample it to the frame size
// with the arithmetic of resample.hip's bilinear kernel (resample_coord.hpp), so the 32 frame-size maps are never written and re-read: the
// only HBM traffic is the tail (read for the fit, read + written by the fade) and the new frames (written once).
// Layout: a thread owns 4 consecutive pixels of a frame (one 16-byte load / store) when the frame's pixel count is a multiple of 4 and the
// buffers are 16-byte aligned -- a group may wrap from one row into the next, never into the next frame -- and one pixel otherwise.
// The sums are fp64 from the first addition on (products of two floats are exact in fp64) and are reduced in a fixed order: per-thread
// partials over a grid-stride loop whose grid depends on the shape alone, a wave butterfly, the block's four waves in order, then ONE block
// over the per-block partials.  No atomics: the same input gives the same bits on every call.
#include <algorithm>

#include "ops.hpp"

// same reason as in resample.hip: an upsampled value must not depend on which products the compiler fuses
#pragma clang fp contract(off)
#include "resample_coord.hpp"
#include "select_common.hpp"  // load_group

namespace edv {
namespace {

constexpr int W_LEN = 32, W_OVERLAP = 10, W_INTERP = 8;  // INFER_LEN, OVERLAP, INTERP_LEN of the reference's endodav.py
constexpr int W_ALIGN = W_OVERLAP - W_INTERP;            // the first overlap slot that is fitted and faded
constexpr int FIT_MAX_BLOCKS = 1024;                     // 4 workgroups per CU; 640 blocks already at 8 x 256 x 320 (one group per thread)

struct Upsample {
    const float *disp;  // [32, ih, iw]
    int ih, iw, fh, fw;
    float rh, rw;
};

__device__ __forceinline__ float up_at(const Upsample &u, int slot, int oy, int ox) {
    int y0, y1, x0, x1;
    float ly, lx;
    lin_coord(oy, u.ih, u.fh, u.rh, y0, y1, ly);
    lin_coord(ox, u.iw, u.fw, u.rw, x0, x1, lx);
    return bilinear_tap(u.disp + (long long)slot * u.ih * u.iw, u.iw, y0, y1, x0, x1, ly, lx);
}

// partials [gridDim.x][4]: sum p*p, sum p, sum p*t, sum t of the pixels this block visited
template <int VW>
__global__ __launch_bounds__(256) void stitch_fit_kernel(Upsample u, const float *__restrict__ tail, double *__restrict__ partials) {
    const long long E = (long long)u.fh * u.fw;
    const long long groups = (long long)W_INTERP * E / VW;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long e0 = g * VW;
        const int fr = (int)(e0 / E);
        const int r = (int)(e0 - fr * E);
        int oy = r / u.fw, ox = r - oy * u.fw;
        float t[VW];
        load_group<VW>(tail, g, t);
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            const double p = (double)up_at(u, W_ALIGN + fr, oy, ox), tt = (double)t[j];
            a[0] += p * p;
            a[1] += p;
            a[2] += p * tt;
            a[3] += tt;
            if (++ox == u.fw) ox = 0, ++oy;
        }
    }
    block_sum_store<4>(a, partials + (long long)blockIdx.x * 4);
}

// one block: the per-block partials in a fixed order, then the 2x2 normal equations of utils/util.py:40-63 (mask = 1) in fp64
__global__ __launch_bounds__(256) void stitch_solve_kernel(const double *__restrict__ partials, int nblocks, double count, float *__restrict__ st) {
    __shared__ double red[256][4];
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += partials[(long long)b * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; ++q) red[threadIdx.x][q] = a[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[threadIdx.x][q] += red[threadIdx.x + o][q];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a00 = red[0][0], a01 = red[0][1], b0 = red[0][2], b1 = red[0][3], a11 = count;
        const double det = a00 * a11 - a01 * a01;
        double s = 1.0, t = 0.0;  // det == 0: the reference returns (1, 0)
        if (det != 0.0) {
            s = (a11 * b0 - a01 * b1) / det;
            t = (-a01 * b0 + a00 * b1) / det;
        }
        st[0] = (float)s;
        st[1] = (float)t;
    }
}

struct Fade {
    float keep[W_INTERP], take[W_INTERP];  // fp32(1 - f_i), fp32(f_i)
};

// st == nullptr: window 0, every slot is the plain upsample.  Otherwise slots 2..9 fade into tail[0..7] and slots 10..31 go to out_new[0..21].
template <int VW>
__global__ __launch_bounds__(256) void stitch_apply_kernel(Upsample u, const float *__restrict__ st, float *__restrict__ tail, float *__restrict__ out_new,
                                                            Fade fade) {
    const bool first = st == nullptr;
    const long long E = (long long)u.fh * u.fw;
    const long long groups = (long long)(first ? W_LEN : W_LEN - W_ALIGN) * E / VW;
    const float s = first ? 1.f : st[0], t = first ? 0.f : st[1];
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long e0 = g * VW;
        const int si = (int)(e0 / E);
        const int r = (int)(e0 - si * E);
        const int slot = first ? si : si + W_ALIGN;
        int oy = r / u.fw, ox = r - oy * u.fw;
        float v[VW];
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            float p = up_at(u, slot, oy, ox);
            if (!first) {
                p = p * s + t;
                p = p < 0.f ? 0.f : p;  // d[d < 0] = 0
            }
            v[j] = p;
            if (++ox == u.fw) ox = 0, ++oy;
        }
        float *dst;
        if (!first && slot < W_OVERLAP) {
            const int i = slot - W_ALIGN;
            dst = tail + i * E + r;
            const float keep = fade.keep[i], take = fade.take[i];
            if constexpr (VW == 4) {
                const f32x4 pre = *reinterpret_cast<const f32x4 *>(dst);
                v[0] = pre.x * keep + v[0] * take, v[1] = pre.y * keep + v[1] * take;
                v[2] = pre.z * keep + v[2] * take, v[3] = pre.w * keep + v[3] * take;
            } else {
                v[0] = dst[0] * keep + v[0] * take;
            }
        } else {
            dst = out_new + (long long)(first ? slot : slot - W_OVERLAP) * E + r;
        }
        if constexpr (VW == 4) {
            f32x4 o;
            o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
            *reinterpret_cast<f32x4 *>(dst) = o;
        } else {
            dst[0] = v[0];
        }
    }
}

inline int check_shapes(int ih, int iw, int fh, int fw) {
    EDV_CHECK(ih > 0 && iw > 0 && fh > 0 && fw > 0, "empty problem");
    EDV_CHECK((long long)W_LEN * ih * iw < (1ll << 31) && (long long)fh * fw < (1ll << 31), "a map beyond 2^31 pixels");
    return 0;
}

}  // namespace

size_t stitch_workspace() { return (size_t)FIT_MAX_BLOCKS * 4 * sizeof(double); }

int stitch_fit(const float *disp, int ih, int iw, const float *tail, int fh, int fw, float *st, void *ws, size_t ws_bytes, hipStream_t stream) {
    EDV_CHECK(disp && tail && st && ws, "null operand");
    EDV_TRY(check_shapes(ih, iw, fh, fw));
    EDV_CHECK(ws_bytes >= stitch_workspace() && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, "workspace too small or not 8-byte aligned (edv_stitch_workspace)");
    const Upsample u{disp, ih, iw, fh, fw, lin_ratio(ih, fh), lin_ratio(iw, fw)};
    const long long E = (long long)fh * fw;
    const bool vec = E % 4 == 0 && aligned_to(tail, 16);
    const long long groups = W_INTERP * E / (vec ? 4 : 1);
    const int blocks = blocks_for(groups, FIT_MAX_BLOCKS);
    double *partials = static_cast<double *>(ws);
    if (vec)
        EDV_LAUNCH(stitch_fit_kernel<4>, dim3(blocks), dim3(256), 0, stream, u, tail, partials);
    else
        EDV_LAUNCH(stitch_fit_kernel<1>, dim3(blocks), dim3(256), 0, stream, u, tail, partials);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(stitch_solve_kernel, dim3(1), dim3(256), 0, stream, partials, blocks, (double)(W_INTERP * E), st);
    EDV_LAUNCH_OK();
    return 0;
}

int stitch_apply(const float *disp, int ih, int iw, const float *st, float *tail, float *out_new, int fh, int fw, hipStream_t stream) {
    EDV_CHECK(disp && out_new, "null operand");
    EDV_CHECK((st == nullptr) == (tail == nullptr), "window 0 takes neither (s, t) nor a tail; every later window takes both");
    EDV_TRY(check_shapes(ih, iw, fh, fw));
    const Upsample u{disp, ih, iw, fh, fw, lin_ratio(ih, fh), lin_ratio(iw, fw)};
    const long long E = (long long)fh * fw;
    // get_interpolate_frames (utils/util.py:66-74): python floats 0, 1/7, ..., 1; numpy rounds (1 - f) and f to fp32 when it multiplies a
    // float32 map by them (video.stitch_windows)
    Fade fade;
    const double step = 1.0 / (W_INTERP - 1);
    for (int i = 0; i < W_INTERP; ++i) {
        const double f = i == 0 ? 0.0 : (i == W_INTERP - 1 ? 1.0 : i * step);
        fade.keep[i] = (float)(1.0 - f);
        fade.take[i] = (float)f;
    }
    const bool vec = E % 4 == 0 && aligned_to(out_new, 16) && (!tail || aligned_to(tail, 16));
    const long long groups = (st ? W_LEN - W_ALIGN : W_LEN) * E / (vec ? 4 : 1);
    const int blocks = blocks_for(groups, 16384);
    if (vec)
        EDV_LAUNCH(stitch_apply_kernel<4>, dim3(blocks), dim3(256), 0, stream, u, st, tail, out_new, fade);
    else
        EDV_LAUNCH(stitch_apply_kernel<1>, dim3(blocks), dim3(256), 0, stream, u, st, tail, out_new, fade);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace edv
