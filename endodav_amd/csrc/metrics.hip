// Video-depth evaluation on the device (reference evaluate_depth_video.py:163-215 with utils/utils.py:112-133, utils/layers.py:11-20 and
// utils/eval_utils.py:63-143,265-282; host counterpart evaluate.clip_metrics_host).  A clip is [n, h, w] fp32.
//   masked_median     the exact radix select of select_common.hpp over the elements with lo < gate < hi, as a batch of one.  Both middle
//                     order statistics are followed at once, so an even count costs no extra pass.  np.median's bits.
//   metrics_pred      disparity -> depth, the alignment ("scale": ratio of medians; "scale_shift": medians and mean absolute deviations),
//                     the scale factor and the clip.  Every fp32 operation is the host's, in the host's order; the alignment scalars stay in
//                     device memory (doubles that hold fp32 values exactly, and the count).
//   metrics_errors    per frame: the valid count and the seven numbers of compute_errors.  fp32 terms as the host forms them, fp64 sums.
//   metrics_temporal  per consecutive pair: lift-and-splat in both directions, TAE and TAS.  fp64 geometry in a fixed left-to-right FMA chain;
//                     the splat is a 64-bit atomic maximum of (source index + 1) << 32 | bits(float(z)): the largest row-major source index
//                     wins a target pixel, which is numpy's "later points overwrite earlier ones", whatever the order of arrival.
// Contraction is off for the whole file: numpy never fuses a product into a sum (the one place that fuses, dot4, says so with fma()).
// Sums are reduced in a fixed order (per-thread partials over a grid whose size depends on the shape alone, a wave butterfly, the block's four waves in order, one thread over the per-block partials); the
// only atomics are integer ones, so the same input gives the same bits on every call.
#include <algorithm>
#include <cmath>
#include <limits>

#include "ops.hpp"

#pragma clang fp contract(off)

#include "select_common.hpp"  // SelState, select_hist_kernel, select_narrow, order_key, key_value, in_gate, load_group: shared with render.hip

namespace edv {
namespace {

constexpr int RED_BLOCKS = 128;      // blocks per frame of the per-frame reductions (1024 x 1280: 40 pixels per thread)
constexpr int FRAME_CHUNK = 8;       // frames per launch of the error kernel
constexpr int PAIR_CHUNK = 4;        // pairs per launch of the temporal kernels: the key images of one chunk are all the memory they need
constexpr int FLAT_MAX_BLOCKS = 2048;
constexpr int ERR_Q = 8, TMP_Q = 3;
constexpr float MIN_DEPTH = 1e-3f, ALIGN_MAX_DEPTH = 150.0f, SPLAT_EPS_F = 1e-6f;
constexpr double SPLAT_EPS = 1e-6;

constexpr size_t WS_STATE = 8192;                                                  // SelState, padded
constexpr size_t WS_PARTIALS = (size_t)FRAME_CHUNK * RED_BLOCKS * ERR_Q * 8;       // the largest of the partial arrays (64 KiB)
constexpr size_t WS_HEAD = WS_STATE + WS_PARTIALS;
static_assert(sizeof(SelState) <= WS_STATE);
static_assert((size_t)FLAT_MAX_BLOCKS * 8 <= WS_PARTIALS && (size_t)2 * PAIR_CHUNK * RED_BLOCKS * TMP_Q * 8 <= WS_PARTIALS);

// ---- masked median (the select itself is select_common.hpp) --------------------------------------------------------------------------------
// one block: after the first pass the total and from it the two middle ranks; narrows, clears the counters, and after the last pass writes the
// median and the count
__global__ __launch_bounds__(256) void select_step_kernel(SelState *s, int shift, double *out_median, double *out_count) {
    if (threadIdx.x == 0) {
        if (shift == 24) {
            u64 total = 0;
            for (int b = 0; b < 256; ++b) total += s->hist[0][b];
            s->total = total;
            s->rank[0] = total ? (total - 1) / 2 : 0;
            s->rank[1] = total / 2;
        }
        if (s->total != 0) select_narrow(s, shift);
        if (shift == 0) {
            float med = std::numeric_limits<float>::quiet_NaN();
            if (s->total != 0) {
                const float a = key_value(s->prefix[0]), b = key_value(s->prefix[1]);
                med = (s->total & 1) ? a : (a + b) / 2.0f;  // np.median: the fp32 mean of the two middle values
            }
            *out_median = (double)med;
            *out_count = (double)s->total;
        }
    }
    __syncthreads();
    s->hist[0][threadIdx.x] = 0, s->hist[1][threadIdx.x] = 0;
}

// a batch of one
int median_into(const float *x, const float *gate, long long count, float lo, float hi, double *out_median, double *out_count, void *ws, hipStream_t stream) {
    SelState *s = static_cast<SelState *>(ws);
    EDV_HIP(hipMemsetAsync(s, 0, sizeof(SelState), stream));
    const bool vec = count % 4 == 0 && aligned_to(x, 16) && aligned_to(gate, 16);
    const int blocks = blocks_for(count / (vec ? 4 : 1), FLAT_MAX_BLOCKS);
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (vec)
            EDV_LAUNCH((select_hist_kernel<4, true>), dim3(blocks), dim3(256), 0, stream, x, gate, count, lo, hi, shift, s);
        else
            EDV_LAUNCH((select_hist_kernel<1, true>), dim3(blocks), dim3(256), 0, stream, x, gate, count, lo, hi, shift, s);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(select_step_kernel, dim3(1), dim3(256), 0, stream, s, shift, out_median, out_count);
        EDV_LAUNCH_OK();
    }
    return 0;
}

// ---- prediction -------------------------------------------------------------------------------------------------------------------------
// scal (doubles; fp32 values are held exactly): 0 ratio, 1 t_gt (median of gt), 2 s_gt, 3 t_pred (median of pred), 4 s_pred, 5 selected count
enum { S_RATIO = 0, S_TGT = 1, S_SGT = 2, S_TPRED = 3, S_SPRED = 4, S_COUNT = 5, S_SPARE = 6, S_LEN = 8 };

template <int VW>
__global__ __launch_bounds__(256) void depth_kernel(const float *__restrict__ disp, float *__restrict__ pred, long long count, float lo, float span) {
    const long long groups = count / VW;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        if constexpr (VW == 4) {
            const f32x4 d = reinterpret_cast<const f32x4 *>(disp)[g];
            f32x4 o;
            o.x = 1.0f / (lo + span * d.x), o.y = 1.0f / (lo + span * d.y), o.z = 1.0f / (lo + span * d.z), o.w = 1.0f / (lo + span * d.w);
            reinterpret_cast<f32x4 *>(pred)[g] = o;
        } else {
            pred[g] = 1.0f / (lo + span * disp[g]);
        }
    }
}

// partials[block] = sum |x - t| over the gated elements, t = (float)scal[t_slot]; the fp32 difference is the host's, the sum is fp64
template <int VW>
__global__ __launch_bounds__(256) void absdev_kernel(const float *__restrict__ x, const float *__restrict__ gate, long long count, const double *__restrict__ scal,
                                                      int t_slot, double *__restrict__ partials) {
    const float t = (float)scal[t_slot];
    const long long groups = count / VW;
    double a[1] = {0.0};
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        float xv[VW], gv[VW];
        load_group<VW>(x, g, xv), load_group<VW>(gate, g, gv);
#pragma unroll
        for (int j = 0; j < VW; ++j)
            if (in_gate(gv[j], MIN_DEPTH, ALIGN_MAX_DEPTH)) a[0] += (double)fabsf(xv[j] - t);
    }
    block_sum_store<1>(a, partials + blockIdx.x);
}

// one thread: the per-block partials in order, the mean in fp64, ONE rounding to fp32
__global__ void absdev_final_kernel(const double *__restrict__ partials, int nblocks, double *__restrict__ scal, int s_slot) {
    double sum = 0.0;
    for (int b = 0; b < nblocks; ++b) sum += partials[b];
    scal[s_slot] = (double)(float)(sum / scal[S_COUNT]);
}

__global__ void ratio_kernel(double *__restrict__ scal) { scal[S_RATIO] = (double)((float)scal[S_TGT] / (float)scal[S_TPRED]); }

// mode 0: none; 1: p * ratio; 2: (p - t_pred) * (s_gt / s_pred) + t_gt.  Then clip(p * factor, MIN_DEPTH, cap); a NaN stays a NaN, as in np.clip.
template <int VW>
__global__ __launch_bounds__(256) void apply_kernel(float *__restrict__ pred, long long count, int mode, const double *__restrict__ scal, float factor, float cap) {
    const float ratio = (float)scal[S_RATIO], t_gt = (float)scal[S_TGT], t_pred = (float)scal[S_TPRED];
    const float q = mode == 2 ? (float)scal[S_SGT] / (float)scal[S_SPRED] : 0.f;
    const long long groups = count / VW;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        float v[VW];
        load_group<VW>(pred, g, v);
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            float p = v[j];
            if (mode == 1) p = p * ratio;
            if (mode == 2) p = (p - t_pred) * q + t_gt;
            p = p * factor;
            v[j] = p < MIN_DEPTH ? MIN_DEPTH : (p > cap ? cap : p);
        }
        if constexpr (VW == 4) {
            f32x4 o;
            o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
            reinterpret_cast<f32x4 *>(pred)[g] = o;
        } else {
            pred[g] = v[0];
        }
    }
}

// ---- per-frame errors -------------------------------------------------------------------------------------------------------------------
// grid (RED_BLOCKS, frames of the chunk); partials [frame][block][8]: count, abs_rel, sq_rel, squared error, squared log error, a1, a2, a3
__global__ __launch_bounds__(256) void errors_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int E, float cap, double *__restrict__ partials) {
    const float *p_ = pred + (long long)blockIdx.y * E, *g_ = gt + (long long)blockIdx.y * E;
    double a[ERR_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < E; i += RED_BLOCKS * 256) {
        const float g = g_[i];
        if (!in_gate(g, MIN_DEPTH, cap)) continue;
        const float p = p_[i];
        const float r0 = g / p, r1 = p / g;
        const float ratio = r0 > r1 ? r0 : r1;
        const float d = g - p;
        const float sq = d * d;
        const float lg = logf(g) - logf(p);
        a[0] += 1.0;
        a[1] += (double)(fabsf(d) / g);
        a[2] += (double)(sq / g);
        a[3] += (double)sq;
        a[4] += (double)(lg * lg);
        a[5] += ratio < 1.25f ? 1.0 : 0.0;
        a[6] += ratio < 1.5625f ? 1.0 : 0.0;
        a[7] += ratio < 1.953125f ? 1.0 : 0.0;
    }
    block_sum_store<ERR_Q>(a, partials + ((long long)blockIdx.y * RED_BLOCKS + blockIdx.x) * ERR_Q);
}

// one block per frame, thread q sums quantity q over the blocks in order; out [frame][8]: count, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3
__global__ __launch_bounds__(64) void errors_final_kernel(const double *__restrict__ partials, double *__restrict__ out) {
    __shared__ double sums[ERR_Q];
    if (threadIdx.x < ERR_Q) {
        double s = 0.0;
        for (int b = 0; b < RED_BLOCKS; ++b) s += partials[((long long)blockIdx.x * RED_BLOCKS + b) * ERR_Q + threadIdx.x];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < ERR_Q) {
        const int q = threadIdx.x;
        const double cnt = sums[0];  // 0: every mean is 0 / 0 = NaN, which the caller skips as the reference does
        double v = q == 0 ? cnt : sums[q] / cnt;
        if (q == 3 || q == 4) v = sqrt(v);
        out[(long long)blockIdx.x * ERR_Q + q] = v;
    }
}

// ---- temporal ---------------------------------------------------------------------------------------------------------------------------
// Row m of a 4x4 matrix times (X, Y, Z, 1): left to right, one EXPLICIT fused multiply-add per term (the compiler fuses nothing by itself
// in this file).  This is the accumulation of the dgemm kernels behind the host's `pts @ M.T` (the first product rounded, then one FMA per
// term in k order), so a coordinate that sits on a rounding tie -- a camera that moves along x alone projects every point to y + 0.5 up to
// this arithmetic's noise -- falls to the side it falls to on the host.
__device__ __forceinline__ double dot4(const double *m, double X, double Y, double Z) { return fma(1.0, m[3], fma(Z, m[2], fma(Y, m[1], X * m[0]))); }

// mats [n][2][16]: per frame img2world = inv(K @ pose) and its inverse, row-major 4x4 fp64, made on the host.
// grid (RED_BLOCKS, 2 * pairs of the chunk): slot = blockIdx.y; pair = slot / 2; direction 0 lifts frame `pair` into frame `pair + 1`, 1 the reverse.
__global__ __launch_bounds__(256) void splat_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int h, int w, float cap, const double *__restrict__ mats,
                                                     u64 *__restrict__ keys) {
    const int E = h * w;
    const int slot = blockIdx.y, pair = slot >> 1, dir = slot & 1;
    const int src = pair + dir, dst = pair + 1 - dir;
    const double *A = mats + (long long)src * 32;        // img2world of the source
    const double *B = mats + (long long)dst * 32 + 16;   // inverse of the target's img2world
    double a[12], b[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) a[i] = A[i], b[i] = B[i];
    const float *p_ = pred + (long long)src * E, *g_ = gt + (long long)src * E;
    u64 *k_ = keys + (long long)slot * E;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < E; i += RED_BLOCKS * 256) {
        if (!in_gate(g_[i], MIN_DEPTH, cap)) continue;
        const double d = (double)p_[i];
        const int y = i / w, x = i - y * w;
        const double X = ((double)x + 0.5) * d, Y = ((double)y + 0.5) * d;
        const double wx = dot4(a + 0, X, Y, d), wy = dot4(a + 4, X, Y, d), wz = dot4(a + 8, X, Y, d);
        const double qx = dot4(b + 0, wx, wy, wz), qy = dot4(b + 4, wx, wy, wz), z = dot4(b + 8, wx, wy, wz);
        if (!(z > SPLAT_EPS)) continue;
        const double u = rint(qx / z), v = rint(qy / z);  // z > eps: the host's clip to eps leaves it alone; rint is round-half-even like np.round
        if (!(u >= 0.0 && u < (double)w && v >= 0.0 && v < (double)h)) continue;  // in fp64, before any conversion to int
        const int t = (int)v * w + (int)u;
        atomicMax(&k_[t], ((u64)(unsigned)(i + 1) << 32) | (u64)__float_as_uint((float)z));
    }
}

// resolves a key image to z * target mask and reduces the target's depth against it under (warp > 1e-6) & mask.
// partials [slot][block][3]: sum |t - w| / t, count of max(t / w, w / t) < 1.25, count
__global__ __launch_bounds__(256) void resolve_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int E, float cap, const u64 *__restrict__ keys,
                                                       float *__restrict__ warp, double *__restrict__ partials) {
    const int slot = blockIdx.y, pair = slot >> 1, dir = slot & 1;
    const int dst = pair + 1 - dir;
    const float *p_ = pred + (long long)dst * E, *g_ = gt + (long long)dst * E;
    const u64 *k_ = keys + (long long)slot * E;
    float *w_ = warp ? warp + (long long)slot * E : nullptr;
    double a[TMP_Q] = {0.0, 0.0, 0.0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < E; i += RED_BLOCKS * 256) {
        const bool m = in_gate(g_[i], MIN_DEPTH, cap);
        const float wp = __uint_as_float((unsigned)k_[i]) * (m ? 1.0f : 0.0f);  // an untouched key is 0: bits of +0.0f
        if (w_) w_[i] = wp;
        if (wp > SPLAT_EPS_F && m) {
            const float t = p_[i];
            const float r0 = t / wp, r1 = wp / t;
            a[0] += (double)(fabsf(t - wp) / t);
            a[1] += (r0 > r1 ? r0 : r1) < 1.25f ? 1.0 : 0.0;
            a[2] += 1.0;
        }
    }
    block_sum_store<TMP_Q>(a, partials + ((long long)slot * RED_BLOCKS + blockIdx.x) * TMP_Q);
}

// thread = pair of the chunk: out [pair][2] = (tae, tas), each 0.5 * (a->b + b->a); an empty overlap is 0 / 0 = NaN, the host's mean of nothing
__global__ void pairs_final_kernel(const double *__restrict__ partials, int pairs, double *__restrict__ out) {
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= pairs) return;
    double e[2][2];
    for (int dir = 0; dir < 2; ++dir) {
        double s[TMP_Q] = {0.0, 0.0, 0.0};
        const double *p = partials + (long long)(pair * 2 + dir) * RED_BLOCKS * TMP_Q;
        for (int b = 0; b < RED_BLOCKS; ++b)
            for (int q = 0; q < TMP_Q; ++q) s[q] += p[b * TMP_Q + q];
        e[dir][0] = s[0] / s[2];
        e[dir][1] = s[1] / s[2];
    }
    out[pair * 2 + 0] = 0.5 * (e[0][0] + e[1][0]);
    out[pair * 2 + 1] = 0.5 * (e[0][1] + e[1][1]);
}

inline int check_clip(long long n, int h, int w) {
    EDV_CHECK(n > 0 && h > 0 && w > 0, "empty clip");
    EDV_CHECK((long long)h * w < (1ll << 31) - 256ll * RED_BLOCKS, "a frame beyond 2^31 pixels");
    EDV_CHECK(n < (1ll << 31) && n * h * w < (1ll << 40), "clip too large");
    return 0;
}
inline int check_ws(const void *ws, size_t ws_bytes, size_t need) {
    EDV_CHECK(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && ws_bytes >= need, "workspace missing, too small or not 16-byte aligned (edv_metrics_workspace)");
    return 0;
}

}  // namespace

size_t metrics_workspace(long long n, int h, int w) {
    (void)n;  // the temporal pass works through the pairs in chunks: nothing here grows with the length of the clip
    return WS_HEAD + (h > 0 && w > 0 ? (size_t)2 * PAIR_CHUNK * h * w * sizeof(u64) : 0);
}

int masked_median(const float *x, const float *gate, long long count, float lo, float hi, double *out, void *ws, size_t ws_bytes, hipStream_t stream) {
    EDV_CHECK(x && gate && out, "null operand");
    EDV_CHECK(count > 0 && count < (1ll << 40), "count out of range");
    EDV_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0, "out not 8-byte aligned");
    EDV_TRY(check_ws(ws, ws_bytes, WS_HEAD));
    return median_into(x, gate, count, lo, hi, out, out + 1, ws, stream);
}

int metrics_pred(const float *disp, const float *gt, float *pred, long long n, int h, int w, double min_depth, double max_depth, int align, float factor, float cap,
                 double *scal, void *ws, size_t ws_bytes, hipStream_t stream) {
    EDV_CHECK(disp && gt && pred && scal, "null operand");
    EDV_CHECK(align >= 0 && align <= 2, "align: 0 none, 1 scale, 2 scale_shift");
    EDV_CHECK(min_depth > 0 && max_depth > min_depth, "depth range");
    EDV_CHECK((reinterpret_cast<uintptr_t>(scal) & 7) == 0, "scalars not 8-byte aligned");
    EDV_TRY(check_clip(n, h, w));
    EDV_TRY(check_ws(ws, ws_bytes, WS_HEAD));
    const long long count = n * h * w;
    // disp_to_depth: python floats lo = 1 / max, hi = 1 / min; numpy rounds lo and (hi - lo) to fp32 when they meet the float32 map
    const double lo = 1.0 / max_depth, hi = 1.0 / min_depth;
    const bool vec = count % 4 == 0 && aligned_to(disp, 16) && aligned_to(gt, 16) && aligned_to(pred, 16);
    const int blocks = blocks_for(count / (vec ? 4 : 1), FLAT_MAX_BLOCKS);
    double *partials = reinterpret_cast<double *>(static_cast<char *>(ws) + WS_STATE);
    EDV_HIP(hipMemsetAsync(scal, 0, S_LEN * sizeof(double), stream));
    if (vec)
        EDV_LAUNCH(depth_kernel<4>, dim3(blocks), dim3(256), 0, stream, disp, pred, count, (float)lo, (float)(hi - lo));
    else
        EDV_LAUNCH(depth_kernel<1>, dim3(blocks), dim3(256), 0, stream, disp, pred, count, (float)lo, (float)(hi - lo));
    EDV_LAUNCH_OK();
    if (align != 0) {
        EDV_TRY(median_into(gt, gt, count, MIN_DEPTH, ALIGN_MAX_DEPTH, scal + S_TGT, scal + S_COUNT, ws, stream));
        EDV_TRY(median_into(pred, gt, count, MIN_DEPTH, ALIGN_MAX_DEPTH, scal + S_TPRED, scal + S_COUNT, ws, stream));
    }
    if (align == 1) {
        EDV_LAUNCH(ratio_kernel, dim3(1), dim3(1), 0, stream, scal);
        EDV_LAUNCH_OK();
    }
    if (align == 2) {
        for (int which = 0; which < 2; ++which) {
            const float *x = which == 0 ? gt : pred;
            const int t_slot = which == 0 ? S_TGT : S_TPRED, s_slot = which == 0 ? S_SGT : S_SPRED;
            if (vec)
                EDV_LAUNCH(absdev_kernel<4>, dim3(blocks), dim3(256), 0, stream, x, gt, count, scal, t_slot, partials);
            else
                EDV_LAUNCH(absdev_kernel<1>, dim3(blocks), dim3(256), 0, stream, x, gt, count, scal, t_slot, partials);
            EDV_LAUNCH_OK();
            EDV_LAUNCH(absdev_final_kernel, dim3(1), dim3(1), 0, stream, partials, blocks, scal, s_slot);
            EDV_LAUNCH_OK();
        }
    }
    if (vec)
        EDV_LAUNCH(apply_kernel<4>, dim3(blocks), dim3(256), 0, stream, pred, count, align, scal, factor, cap);
    else
        EDV_LAUNCH(apply_kernel<1>, dim3(blocks), dim3(256), 0, stream, pred, count, align, scal, factor, cap);
    EDV_LAUNCH_OK();
    return 0;
}

int metrics_errors(const float *pred, const float *gt, long long n, int h, int w, float cap, double *out, void *ws, size_t ws_bytes, hipStream_t stream) {
    EDV_CHECK(pred && gt && out, "null operand");
    EDV_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0, "out not 8-byte aligned");
    EDV_TRY(check_clip(n, h, w));
    EDV_TRY(check_ws(ws, ws_bytes, WS_HEAD));
    const int E = h * w;
    double *partials = reinterpret_cast<double *>(static_cast<char *>(ws) + WS_STATE);
    for (long long f0 = 0; f0 < n; f0 += FRAME_CHUNK) {
        const int frames = (int)std::min<long long>(FRAME_CHUNK, n - f0);
        EDV_LAUNCH(errors_kernel, dim3(RED_BLOCKS, frames), dim3(256), 0, stream, pred + f0 * E, gt + f0 * E, E, cap, partials);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(errors_final_kernel, dim3(frames), dim3(64), 0, stream, partials, out + f0 * ERR_Q);
        EDV_LAUNCH_OK();
    }
    return 0;
}

int metrics_temporal(const float *pred, const float *gt, long long n, int h, int w, float cap, const double *mats, double *out, float *warp, void *ws,
                     size_t ws_bytes, hipStream_t stream) {
    EDV_CHECK(pred && gt && mats && (out || n < 2), "null operand");
    EDV_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(mats) & 7) == 0, "out / mats not 8-byte aligned");
    EDV_TRY(check_clip(n, h, w));
    EDV_TRY(check_ws(ws, ws_bytes, metrics_workspace(n, h, w)));
    const int E = h * w;
    double *partials = reinterpret_cast<double *>(static_cast<char *>(ws) + WS_STATE);
    u64 *keys = reinterpret_cast<u64 *>(static_cast<char *>(ws) + WS_HEAD);
    for (long long p0 = 0; p0 + 1 < n; p0 += PAIR_CHUNK) {
        const int pairs = (int)std::min<long long>(PAIR_CHUNK, n - 1 - p0);
        EDV_HIP(hipMemsetAsync(keys, 0, (size_t)2 * pairs * E * sizeof(u64), stream));
        EDV_LAUNCH(splat_kernel, dim3(RED_BLOCKS, 2 * pairs), dim3(256), 0, stream, pred + p0 * E, gt + p0 * E, h, w, cap, mats + p0 * 32, keys);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(resolve_kernel, dim3(RED_BLOCKS, 2 * pairs), dim3(256), 0, stream, pred + p0 * E, gt + p0 * E, E, cap, keys,
                   warp ? warp + p0 * 2 * E : nullptr, partials);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(pairs_final_kernel, dim3(1), dim3(64), 0, stream, partials, pairs, out + p0 * 2);
        EDV_LAUNCH_OK();
    }
    return 0;
}

}  // namespace edv
