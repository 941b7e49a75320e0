// Colour-mapped depth on the device: the numpy of the reference's three renderers (utils/eval_utils.py:284-295 save_video,
// evaluate_depth_video.py:32-36 render_depth, test_simple.py:156-167), as two steps over a clip [n, h, w] fp32.
//   render_range     (lo, hi) per frame: the frame's or the whole clip's minimum and maximum, or two order statistics per frame.  All of them
//                    compare the order-preserving integer image of the float bits (select_common.hpp's order_key), so they are exact,
//                    independent of the order of the reduction, and use integer atomics only: the same input gives the same bits on every call.
//                    The order statistics are the radix select of select_common.hpp, ungated, with the frames of a chunk as its batch: every
//                    frame has a select state of its own in the workspace, so a pass is one launch for all frames of a chunk.
//   render_colorize  idx = trunc((x - lo) / ((hi - lo) + eps) * 255) -> lut[idx], 3 bytes a pixel.  The table lives in LDS as one dword per
//                    entry.  A sub-dword global store costs several times a dword store per byte on this part, so where the shape allows it
//                    a thread owns four pixels: one 16-byte load, twelve output bytes assembled in registers and stored as three whole dwords
//                    (the lanes of a wave write 768 contiguous bytes).  Any other shape or alignment takes the byte-per-store kernel.
// Contraction is off for the whole file and the division is IEEE's: every fp32 operation is numpy's, in numpy's order.
#include <algorithm>

#include "ops.hpp"

#pragma clang fp contract(off)

#include "select_common.hpp"  // SelState, select_hist_kernel, select_narrow, order_key, key_value, load_group: shared with metrics.hip

namespace edv {
namespace {

constexpr int RANGE_CHUNK = 64;        // frames per launch of the range kernels: the workspace stops growing there
constexpr int FRAME_BLOCKS = 128;      // blocks per frame at most (1024 x 1280 in groups of 4: 10 groups per thread)
constexpr int FLAT_MAX_BLOCKS = 2048;  // blocks of the whole-clip reduction
constexpr int COLOR_BLOCKS = 1024;     // blocks per frame of the colouring at most
constexpr int COLOR_FRAMES = 32768;    // frames per launch of the colouring (blockIdx.y)

// maxima of key and of ~key: zero is the identity of both, so a memset initialises them
struct MinMax {
    unsigned hi_key, lo_inv;
};
static_assert(sizeof(MinMax) * RANGE_CHUNK <= sizeof(SelState));

// ---- minimum and maximum ------------------------------------------------------------------------------------------------------------------
// grid (blocks, frames): frame blockIdx.y is x[blockIdx.y * elems ..), its extremes go to mm[blockIdx.y]
template <int VW>
__global__ __launch_bounds__(256) void minmax_kernel(const float *__restrict__ x, long long elems, MinMax *__restrict__ mm) {
    __shared__ unsigned red[4][2];
    const float *xf = x + (long long)blockIdx.y * elems;
    const long long groups = elems / VW;
    unsigned hi = 0, lo = 0;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        float v[VW];
        load_group<VW>(xf, g, v);
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            const unsigned k = order_key(v[j]);
            hi = max(hi, k), lo = max(lo, ~k);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
        lo = max(lo, (unsigned)__shfl_xor((int)lo, o, 64));
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) red[wave][0] = hi, red[wave][1] = lo;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(&mm[blockIdx.y].hi_key, max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0])));
        atomicMax(&mm[blockIdx.y].lo_inv, max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1])));
    }
}

// range[r] = the extremes of mm[r * mm_stride] (mm_stride 0: one pair for every row)
__global__ __launch_bounds__(256) void minmax_final_kernel(const MinMax *__restrict__ mm, int mm_stride, float *__restrict__ range, long long rows) {
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
        const MinMax m = mm[r * mm_stride];
        range[2 * r] = key_value(~m.lo_inv);
        range[2 * r + 1] = key_value(m.hi_key);
    }
}

// ---- two order statistics per frame ---------------------------------------------------------------------------------------------------------
// one block per frame: takes the two ranks before the first narrowing, narrows, clears the counters, and after the last pass writes (lo, hi)
__global__ __launch_bounds__(256) void select_step_kernel(SelState *states, int shift, u64 rank_lo, u64 rank_hi, float *__restrict__ range) {
    SelState *s = states + blockIdx.x;
    if (threadIdx.x == 0) {
        if (shift == 24) s->rank[0] = rank_lo, s->rank[1] = rank_hi;  // the state was zeroed: both prefixes are empty
        select_narrow(s, shift);
        if (shift == 0) {
            range[2 * blockIdx.x] = key_value(s->prefix[0]);
            range[2 * blockIdx.x + 1] = key_value(s->prefix[1]);
        }
    }
    __syncthreads();
    s->hist[0][threadIdx.x] = 0, s->hist[1][threadIdx.x] = 0;
}

// ---- colour ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned lut_index(float x, float lo, float den, int clip) {
    float t = (x - lo) / den;
    if (clip) t = fminf(fmaxf(t, 0.0f), 1.0f);
    const int i = (int)(t * 255.0f);  // truncation towards zero, as .astype(np.uint8) of a value in [0, 256)
    return den == 0.0f ? 0u : (unsigned)min(max(i, 0), 255);
}

// the table as one dword per entry (channel 0 in the low byte), staged by the block's 256 threads
__device__ __forceinline__ void stage_lut(const uint8_t *__restrict__ lut, unsigned (&lut_s)[256]) {
    const int t = threadIdx.x;
    lut_s[t] = (unsigned)lut[3 * t] | ((unsigned)lut[3 * t + 1] << 8) | ((unsigned)lut[3 * t + 2] << 16);
    __syncthreads();
}

struct Dwords3 {
    unsigned a, b, c;
};

// grid (blocks, frames); w % 4 == 0, x 16-byte, out and beside 4-byte aligned.  A thread owns pixels 4 g .. 4 g + 3 of its frame: they lie in
// one row, and their 12 output bytes start at a multiple of 12 from the 4-byte aligned base.
__global__ __launch_bounds__(256) void colorize4_kernel(const float *__restrict__ x, int E, int w, const float *__restrict__ range, int range_stride, float eps, int clip,
                                                        const uint8_t *__restrict__ lut, const uint8_t *__restrict__ beside, uint8_t *__restrict__ out) {
    __shared__ unsigned lut_s[256];
    stage_lut(lut, lut_s);
    const long long f = blockIdx.y;
    const float lo = range[f * range_stride], hi = range[f * range_stride + 1];
    const float den = (hi - lo) + eps;
    const int groups = E / 4;
    const f32x4 *xf = reinterpret_cast<const f32x4 *>(x + f * E);
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const f32x4 v = xf[g];
        const unsigned c0 = lut_s[lut_index(v.x, lo, den, clip)], c1 = lut_s[lut_index(v.y, lo, den, clip)];
        const unsigned c2 = lut_s[lut_index(v.z, lo, den, clip)], c3 = lut_s[lut_index(v.w, lo, den, clip)];
        const Dwords3 d = {c0 | (c1 << 24), (c1 >> 8) | (c2 << 16), (c2 >> 16) | (c3 << 8)};
        const int p = 4 * g;
        if (beside) {
            const int row = p / w, col = p - row * w;
            const long long q = (f * 2 * E + (long long)row * 2 * w + col) * 3;  // the byte at which this run of the frame row starts
            *reinterpret_cast<Dwords3 *>(out + q) = *reinterpret_cast<const Dwords3 *>(beside + (f * E + p) * 3);
            *reinterpret_cast<Dwords3 *>(out + q + (long long)w * 3) = d;
        } else {
            *reinterpret_cast<Dwords3 *>(out + (f * E + p) * 3) = d;
        }
    }
}

// any shape and alignment: one pixel per thread, one byte per store
__global__ __launch_bounds__(256) void colorize1_kernel(const float *__restrict__ x, int E, int w, const float *__restrict__ range, int range_stride, float eps, int clip,
                                                        const uint8_t *__restrict__ lut, const uint8_t *__restrict__ beside, uint8_t *__restrict__ out) {
    __shared__ unsigned lut_s[256];
    stage_lut(lut, lut_s);
    const long long f = blockIdx.y;
    const float lo = range[f * range_stride], hi = range[f * range_stride + 1];
    const float den = (hi - lo) + eps;
    const float *xf = x + f * E;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < E; p += gridDim.x * 256) {
        const unsigned c = lut_s[lut_index(xf[p], lo, den, clip)];
        uint8_t *o;
        if (beside) {
            const int row = p / w, col = p - row * w;
            uint8_t *left = out + (f * 2 * E + (long long)row * 2 * w + col) * 3;
            const uint8_t *b = beside + (f * E + p) * 3;
            left[0] = b[0], left[1] = b[1], left[2] = b[2];
            o = left + (long long)w * 3;
        } else {
            o = out + (f * E + p) * 3;
        }
        o[0] = (uint8_t)c, o[1] = (uint8_t)(c >> 8), o[2] = (uint8_t)(c >> 16);
    }
}

inline int check_clip(long long n, int h, int w) {
    EDV_CHECK(n >= 1 && h >= 1 && w >= 1, "empty clip");
    EDV_CHECK((long long)h * w < (1ll << 31) - 256ll * COLOR_BLOCKS, "a frame beyond 2^31 pixels");
    EDV_CHECK(n < (1ll << 31) && n * h * w < (1ll << 40), "clip too large");
    return 0;
}

}  // namespace

size_t render_workspace(long long n) { return (size_t)std::max<long long>(1, std::min<long long>(n, RANGE_CHUNK)) * sizeof(SelState); }

int render_range(const float *x, long long n, int h, int w, int mode, long long rank_lo, long long rank_hi, float *range, void *ws, size_t ws_bytes, hipStream_t stream) {
    EDV_CHECK(x && range, "null operand");
    EDV_CHECK(mode >= 0 && mode <= 2, "mode: 0 frame, 1 video, 2 quantile");
    EDV_TRY(check_clip(n, h, w));
    const int E = h * w;
    EDV_CHECK(mode != 2 || (rank_lo >= 0 && rank_lo <= rank_hi && rank_hi < E), "ranks must satisfy 0 <= rank_lo <= rank_hi < h * w");
    EDV_CHECK(aligned_to(range, 4), "range not 4-byte aligned");
    EDV_CHECK(ws && aligned_to(ws, 16) && ws_bytes >= render_workspace(n), "workspace missing, too small or not 16-byte aligned (edv_render_workspace)");
    MinMax *mm = static_cast<MinMax *>(ws);
    if (mode == 1) {
        const long long count = n * E;
        const bool vec = count % 4 == 0 && aligned_to(x, 16);
        EDV_HIP(hipMemsetAsync(mm, 0, sizeof(MinMax), stream));
        if (vec)
            EDV_LAUNCH(minmax_kernel<4>, dim3(blocks_for(count / 4, FLAT_MAX_BLOCKS)), dim3(256), 0, stream, x, count, mm);
        else
            EDV_LAUNCH(minmax_kernel<1>, dim3(blocks_for(count, FLAT_MAX_BLOCKS)), dim3(256), 0, stream, x, count, mm);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(minmax_final_kernel, dim3(blocks_for(n, 64)), dim3(256), 0, stream, mm, 0, range, n);
        EDV_LAUNCH_OK();
        return 0;
    }
    const bool vec = E % 4 == 0 && aligned_to(x, 16);  // then every frame starts 16-byte aligned
    const int blocks = blocks_for(E / (vec ? 4 : 1), FRAME_BLOCKS);
    SelState *states = static_cast<SelState *>(ws);
    for (long long f0 = 0; f0 < n; f0 += RANGE_CHUNK) {
        const int frames = (int)std::min<long long>(RANGE_CHUNK, n - f0);
        const float *xc = x + f0 * E;
        float *rc = range + f0 * 2;
        if (mode == 0) {
            EDV_HIP(hipMemsetAsync(mm, 0, sizeof(MinMax) * frames, stream));
            if (vec)
                EDV_LAUNCH(minmax_kernel<4>, dim3(blocks, frames), dim3(256), 0, stream, xc, (long long)E, mm);
            else
                EDV_LAUNCH(minmax_kernel<1>, dim3(blocks, frames), dim3(256), 0, stream, xc, (long long)E, mm);
            EDV_LAUNCH_OK();
            EDV_LAUNCH(minmax_final_kernel, dim3(1), dim3(256), 0, stream, mm, 1, rc, (long long)frames);
            EDV_LAUNCH_OK();
            continue;
        }
        EDV_HIP(hipMemsetAsync(states, 0, sizeof(SelState) * frames, stream));
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (vec)
                EDV_LAUNCH((select_hist_kernel<4, false>), dim3(blocks, frames), dim3(256), 0, stream, xc, (const float *)nullptr, (long long)E, 0.f, 0.f, shift, states);
            else
                EDV_LAUNCH((select_hist_kernel<1, false>), dim3(blocks, frames), dim3(256), 0, stream, xc, (const float *)nullptr, (long long)E, 0.f, 0.f, shift, states);
            EDV_LAUNCH_OK();
            EDV_LAUNCH(select_step_kernel, dim3(frames), dim3(256), 0, stream, states, shift, (u64)rank_lo, (u64)rank_hi, rc);
            EDV_LAUNCH_OK();
        }
    }
    return 0;
}

int render_colorize(const float *x, long long n, int h, int w, const float *range, int range_stride, float eps, int clip, const uint8_t *lut, const uint8_t *beside,
                    uint8_t *out, hipStream_t stream) {
    EDV_CHECK(x && range && lut && out, "null operand");
    EDV_CHECK(range_stride == 0 || range_stride == 2, "range_stride: 2 (a pair per frame) or 0 (one pair for all frames)");
    EDV_TRY(check_clip(n, h, w));
    EDV_CHECK(aligned_to(x, 4) && aligned_to(range, 4), "x / range not 4-byte aligned");
    const int E = h * w;
    const bool fast = w % 4 == 0 && aligned_to(x, 16) && aligned_to(out, 4) && (!beside || aligned_to(beside, 4));
    const int blocks = blocks_for(fast ? E / 4 : E, COLOR_BLOCKS);
    const long long out_frame = (long long)E * 3 * (beside ? 2 : 1);
    for (long long f0 = 0; f0 < n; f0 += COLOR_FRAMES) {
        const int frames = (int)std::min<long long>(COLOR_FRAMES, n - f0);
        const float *xc = x + f0 * E, *rc = range + f0 * range_stride;
        const uint8_t *bc = beside ? beside + f0 * E * 3 : nullptr;
        uint8_t *oc = out + f0 * out_frame;
        if (fast)
            EDV_LAUNCH(colorize4_kernel, dim3(blocks, frames), dim3(256), 0, stream, xc, E, w, rc, range_stride, eps, clip, lut, bc, oc);
        else
            EDV_LAUNCH(colorize1_kernel, dim3(blocks, frames), dim3(256), 0, stream, xc, E, w, rc, range_stride, eps, clip, lut, bc, oc);
        EDV_LAUNCH_OK();
    }
    return 0;
}

}  // namespace edv
