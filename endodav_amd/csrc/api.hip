// extern "C" per-kernel entry points declared in include/endodav_hip.h (unit tests, micro-benchmarks).
#include "../../include/endodav_hip.h"
#include <algorithm>
#include <vector>

#include "ops.hpp"

using namespace edv;

extern "C" {

int edv_layernorm(const float *x_dev, const float *w_dev, const float *b_dev, float *y_dev, int64_t rows, int32_t dim, float eps,
                  const float *pe_dev, int32_t rows_per_frame, int32_t T, void *stream) {
    return layernorm(x_dev, identity_map(), w_dev, b_dev, y_dev, identity_map(), rows, dim, eps, pe_dev, rows_per_frame, T, (hipStream_t)stream);
}

size_t edv_gemm_workspace(void) { return gemm_workspace() * sizeof(float); }
int edv_gemm(const float *A_dev, const float *W_dev, float *C_dev, int64_t M, int32_t N, int32_t K, const float *bias_dev, int32_t act,
             const float *gamma_dev, const float *R_dev, float *workspace_dev, size_t workspace_bytes, void *stream) {
    GemmDesc g;
    g.A = A_dev; g.lda = K; g.W = W_dev; g.ldw = K; g.C = C_dev; g.ldc = N; g.M = M; g.N = N; g.K = K;
    g.bias = bias_dev; g.act = act; g.gamma = gamma_dev; g.R1 = R_dev; g.ldr1 = N;
    g.ws = workspace_dev; g.ws_floats = workspace_bytes / sizeof(float);
    EDV_CHECK(act >= ACT_NONE && act <= ACT_RELU, "act must be 0, 1 or 2");
    return gemm(g, (hipStream_t)stream);
}

size_t edv_gemm_x6_planes_bytes(int32_t N, int32_t K) { return N > 0 && K > 0 ? gemm_x6_planes_bytes(N, K) : 0; }

int edv_gemm_x6_split(const float *W_dev, void *planes_dev, int32_t N, int32_t K, void *stream) {
    return gemm_x6_split(W_dev, planes_dev, N, K, (hipStream_t)stream);
}

int edv_gemm_x6(const float *A_dev, const void *planes_dev, float *C_dev, int64_t M, int32_t N, int32_t K, const float *bias_dev, int32_t act,
                const float *gamma_dev, const float *R_dev, float *workspace_dev, size_t workspace_bytes, void *stream) {
    GemmDesc g;
    g.A = A_dev; g.lda = K; g.W = reinterpret_cast<const float *>(planes_dev); g.ldw = K; g.C = C_dev; g.ldc = N; g.M = M; g.N = N; g.K = K;
    g.bias = bias_dev; g.act = act; g.gamma = gamma_dev; g.R1 = R_dev; g.ldr1 = N;
    g.ws = workspace_dev; g.ws_floats = workspace_bytes / sizeof(float);
    g.Wx6 = planes_dev;
    EDV_CHECK(act >= ACT_NONE && act <= ACT_RELU, "act must be 0, 1 or 2");
    EDV_CHECK(M > 0 && N >= 64 && K > 0 && K % 16 == 0, "edv_gemm_x6: K % 16 == 0, N >= 64");
    return gemm_x6(g, (hipStream_t)stream);
}

int edv_pack_geglu(const float *w_dev, const float *b_dev, float *wi_dev, float *bi_dev, int32_t N, int32_t K, void *stream) {
    return pack_geglu(w_dev, b_dev, wi_dev, bi_dev, N, K, (hipStream_t)stream);
}

int edv_gemm_geglu(const float *A_dev, const float *Wi_dev, const float *bi_dev, float *C_dev, int64_t M, int32_t N, int32_t K, void *stream) {
    GemmDesc g;
    g.A = A_dev; g.lda = K; g.W = Wi_dev; g.ldw = K; g.C = C_dev; g.ldc = N / 2; g.M = M; g.N = N; g.K = K;
    g.bias = bi_dev; g.geglu = 1;
    EDV_CHECK(A_dev && Wi_dev && bi_dev && C_dev && M > 0, "null operand");
    EDV_CHECK(gemm_geglu_supported(g), "edv_gemm_geglu: K % 32 == 0, N % 64 == 0, output below 4 GB");
    return gemm(g, (hipStream_t)stream);
}

static int conv3x3_impl(const float *x_dev, const float *wpacked_dev, const float *bias_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t Cin,
                        int32_t Cout, int32_t stride, int32_t pre_relu, int32_t post_relu, const float *R1_dev, const float *R2_dev, float *ws,
                        size_t ws_bytes, void *stream) {
    EDV_CHECK(F > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "empty problem");
    EDV_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2");
    GemmDesc g;
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    g.A = x_dev; g.W = wpacked_dev; g.ldw = 9 * Cin; g.C = y_dev; g.ldc = Cout; g.M = (long long)F * OH * OW; g.N = Cout; g.K = 9 * Cin;
    g.bias = bias_dev; g.act = post_relu ? ACT_RELU : ACT_NONE; g.R1 = R1_dev; g.ldr1 = Cout; g.R2 = R2_dev; g.ldr2 = Cout;
    g.loader = LOAD_CONV3; g.cH = H; g.cW = W; g.cC = Cin; g.cOH = OH; g.cOW = OW; g.cS = stride; g.pre_relu = pre_relu ? 1 : 0;
    g.ws = ws; g.ws_floats = ws_bytes / sizeof(float);
    return gemm(g, (hipStream_t)stream);
}

int edv_conv3x3(const float *x_dev, const float *wpacked_dev, const float *bias_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t Cin,
                int32_t Cout, int32_t stride, int32_t pre_relu, int32_t post_relu, const float *R1_dev, const float *R2_dev, void *stream) {
    return conv3x3_impl(x_dev, wpacked_dev, bias_dev, y_dev, F, H, W, Cin, Cout, stride, pre_relu, post_relu, R1_dev, R2_dev, nullptr, 0, stream);
}

int edv_conv3x3_ws(const float *x_dev, const float *wpacked_dev, const float *bias_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t Cin,
                   int32_t Cout, int32_t stride, int32_t pre_relu, int32_t post_relu, const float *R1_dev, const float *R2_dev, float *workspace_dev,
                   size_t workspace_bytes, void *stream) {
    return conv3x3_impl(x_dev, wpacked_dev, bias_dev, y_dev, F, H, W, Cin, Cout, stride, pre_relu, post_relu, R1_dev, R2_dev, workspace_dev,
                        workspace_bytes, stream);
}

int edv_set_conv_impl(int32_t mode) {
    EDV_CHECK(mode >= 0 && mode <= 2, "edv_set_conv_impl: mode 0 (automatic), 1 (never fused) or 2 (fused wherever supported)");
    set_conv_impl(mode);
    return 0;
}

int edv_set_x6_remainder(int32_t mode, int32_t cus) {
    EDV_CHECK(mode >= 0 && mode <= 2 && cus >= 0, "edv_set_x6_remainder: mode 0 (off), 1 (by policy) or 2 (wherever supported); cus 0 = the device's count");
    set_x6_remainder(mode, cus);
    return 0;
}

int edv_conv3x3_dot(const float *x_dev, const float *wpacked_dev, const float *bias_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t Cin,
                    int32_t Cout, int32_t stride, int32_t pre_relu, int32_t post_relu, const float *w2_dev, const float *b2_dev, int32_t act2, void *stream) {
    EDV_CHECK(F > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "empty problem");
    EDV_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2");
    EDV_CHECK(conv_dot_enabled(), "edv_conv3x3_dot: the fused epilogue is switched off (edv_set_conv_impl(1) or EDV_CONV_DOT=0)");
    GemmDesc g;
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    g.A = x_dev; g.W = wpacked_dev; g.ldw = 9 * Cin; g.ldc = Cout; g.M = (long long)F * OH * OW; g.N = Cout; g.K = 9 * Cin;
    g.bias = bias_dev; g.act = post_relu ? ACT_RELU : ACT_NONE;
    g.loader = LOAD_CONV3; g.cH = H; g.cW = W; g.cC = Cin; g.cOH = OH; g.cOW = OW; g.cS = stride; g.pre_relu = pre_relu ? 1 : 0;
    g.w2 = w2_dev; g.b2 = b2_dev; g.act2 = act2; g.dot_out = y_dev;
    return conv_dot(g, (hipStream_t)stream);
}

int edv_pack_conv3x3(const float *w_dev, float *wpacked_dev, int32_t Cout, int32_t Cin, void *stream) {
    return pack_conv3x3(w_dev, wpacked_dev, Cout, Cin, (hipStream_t)stream);
}

int edv_conv_transpose(const float *x_dev, const float *w_dev, const float *b_dev, float *wpack_dev, float *bpack_dev, float *y_dev, int32_t F, int32_t h,
              int32_t w, int32_t C, int32_t s, void *stream) {
    EDV_CHECK(F > 0 && h > 0 && w > 0 && C > 0 && s > 0, "empty problem");
    EDV_TRY(pack_convT(w_dev, wpack_dev, b_dev, bpack_dev, C, C, s, (hipStream_t)stream));
    GemmDesc g;
    g.A = x_dev; g.lda = C; g.W = wpack_dev; g.ldw = C; g.C = y_dev; g.ldc = C; g.M = (long long)F * h * w; g.N = s * s * C; g.K = C;
    g.bias = bpack_dev; g.store = STORE_SHUFFLE; g.ps_s = s; g.ps_C = C; g.ps_h = h; g.ps_w = w;
    return gemm(g, (hipStream_t)stream);
}

size_t edv_attn_spatial_workspace(int32_t F, int32_t N, int32_t heads) { return attn_spatial_workspace(F, N, heads) * sizeof(float); }
int edv_attn_spatial(const float *qkv_dev, float *out_dev, int32_t F, int32_t N, int32_t heads, float *workspace_dev, size_t workspace_bytes,
                     float *lse_dev, void *stream) {
    return attn_spatial(qkv_dev, out_dev, F, N, heads, workspace_dev, workspace_bytes / sizeof(float), (hipStream_t)stream, lse_dev);
}
size_t edv_attn_spatial_x6_workspace(int32_t F, int32_t N, int32_t heads) { return attn_spatial_workspace(F, N, heads, true) * sizeof(float); }
int edv_attn_spatial_x6(const float *qkv_dev, float *out_dev, int32_t F, int32_t N, int32_t heads, float *workspace_dev, size_t workspace_bytes, void *stream) {
    return attn_spatial(qkv_dev, out_dev, F, N, heads, workspace_dev, workspace_bytes / sizeof(float), (hipStream_t)stream, nullptr, true);
}

size_t edv_attn_spatial_bwd_workspace(int32_t F, int32_t N, int32_t heads) { return attn_spatial_bwd_workspace(F, N, heads) * sizeof(float); }
int edv_attn_spatial_bwd(const float *qkv_dev, const float *out_dev, const float *dout_dev, const float *lse_dev, float *delta_dev, float *dqkv_dev,
                         int32_t F, int32_t N, int32_t heads, float *workspace_dev, size_t workspace_bytes, void *stream) {
    return attn_spatial_bwd(qkv_dev, out_dev, dout_dev, lse_dev, delta_dev, dqkv_dev, F, N, heads, workspace_dev, workspace_bytes / sizeof(float),
                            (hipStream_t)stream);
}
int edv_layernorm_bwd(const float *x_dev, const float *w_dev, const float *dy_dev, float *dx_dev, int64_t rows, int32_t dim, float eps, int32_t accumulate,
                      void *stream) {
    return layernorm_bwd(x_dev, identity_map(), w_dev, dy_dev, identity_map(), dx_dev, identity_map(), rows, dim, eps, accumulate != 0, (hipStream_t)stream);
}
int edv_ew_bwd(const float *d_dev, const float *src_dev, const float *add_dev, float *out_dev, int64_t n, int32_t mode, void *stream) {
    return ew_bwd(d_dev, src_dev, add_dev, out_dev, n, mode, (hipStream_t)stream);
}
int edv_geglu_bwd(const float *x_dev, const float *dy_dev, float *dx_dev, int64_t M, int32_t inner, void *stream) {
    return geglu_bwd(x_dev, dy_dev, dx_dev, M, inner, (hipStream_t)stream);
}
int edv_transpose_scale(const float *W_dev, const float *gamma_dev, float *Wt_dev, int32_t N, int32_t K, void *stream) {
    return transpose_scale(W_dev, K, gamma_dev, Wt_dev, N, K, (hipStream_t)stream);
}
size_t edv_lora_grads_workspace(int64_t M, int32_t nin, int32_t nout, int32_t r) { return lora_grads_workspace(M, nin, nout, r) * sizeof(float); }
int edv_lora_grads(const float *x_dev, const float *g_dev, int64_t M, int32_t nin, int32_t nout, int32_t r, const float *A_dev, const float *B_dev,
                   const float *U_dev, const float *V_dev, float s, const float *gamma_dev, float *workspace_dev, size_t workspace_bytes, float *dA_dev,
                   float *dB_dev, float *dU_dev, float *dV_dev, void *stream) {
    EDV_CHECK(M > 0 && nin > 0 && nout > 0 && nin % 4 == 0 && nout % 4 == 0, "shape");
    return lora_grads(x_dev, nin, g_dev, nout, M, nin, nout, r, A_dev, B_dev, U_dev, V_dev, s, gamma_dev, workspace_dev, workspace_bytes / sizeof(float),
                      dA_dev, dB_dev, dU_dev, dV_dev, (hipStream_t)stream);
}
int edv_bilinear_bwd(const float *dy_dev, float *dx_dev, int32_t F, int32_t ih, int32_t iw, int32_t C, int32_t oh, int32_t ow, int32_t accumulate,
                     void *stream) {
    return bilinear_bwd(dy_dev, dx_dev, F, ih, iw, C, oh, ow, accumulate != 0, (hipStream_t)stream);
}
int edv_dot_channels_bwd(const float *g_dev, const float *disp_dev, const float *w_dev, const float *o2_dev, float *d_o2_dev, float *gz_out_dev,
                         int64_t npix, int32_t C, int32_t mode, void *stream) {
    return dot_channels_bwd(g_dev, disp_dev, w_dev, o2_dev, d_o2_dev, gz_out_dev, npix, C, mode, (hipStream_t)stream);
}
size_t edv_conv3x3_wgrad_workspace(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout) {
    return conv3_wgrad_workspace(F, H, W, Cin, Cout) * sizeof(float);
}
int edv_conv3x3_wgrad(const float *x_dev, const float *dy_dev, float *dw_dev, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                      float *workspace_dev, size_t workspace_bytes, int32_t accumulate, void *stream) {
    return conv3_wgrad(x_dev, dy_dev, dw_dev, F, H, W, Cin, Cout, workspace_dev, workspace_bytes / sizeof(float), accumulate != 0, (hipStream_t)stream);
}
size_t edv_colsum_workspace(int32_t N) { return colsum_workspace(N) * sizeof(float); }
int edv_colsum_rows(const float *P_dev, const float *rowscale_dev, int64_t M, int32_t N, float *workspace_dev, size_t workspace_bytes, float *out_dev,
                    int32_t accumulate, void *stream) {
    return colsum_rows(P_dev, rowscale_dev, M, N, workspace_dev, workspace_bytes / sizeof(float), out_dev, accumulate != 0, (hipStream_t)stream);
}
size_t edv_colsum_batch_workspace(int32_t n, const int64_t *rows, const int32_t *cols) {
    std::vector<long long> r(rows, rows + n);
    std::vector<int> c(cols, cols + n);
    return colsum_batch_workspace(n, r.data(), c.data()) * sizeof(float);
}
int edv_colsum_batch(int32_t n, const float *const *src_dev, const int64_t *ld, const int64_t *rows, const int32_t *row_map, const int32_t *cols,
                     const float *const *scale_dev, float *const *dst_dev, const int32_t *accumulate, float *workspace_dev, size_t workspace_bytes, void *stream) {
    EDV_CHECK(n >= 0 && (n == 0 || (src_dev && ld && rows && cols && dst_dev)), "null argument");
    std::vector<long long> l(ld, ld + n), r(rows, rows + n);
    std::vector<int> c(cols, cols + n), acc(n, 0);
    std::vector<RowMap> maps(n, identity_map());
    for (int k = 0; k < n; ++k) {
        if (row_map) maps[k] = RowMap{row_map[3 * k], row_map[3 * k + 1], row_map[3 * k + 2]};
        if (accumulate) acc[k] = accumulate[k];
    }
    return colsum_batch(n, src_dev, l.data(), r.data(), maps.data(), c.data(), scale_dev, dst_dev, acc.data(), workspace_dev, workspace_bytes / sizeof(float),
                        (hipStream_t)stream);
}
int edv_groupnorm_bwd(const float *x_dev, const float *stats_dev, const float *w_dev, const float *dy_dev, float *sums_dev, float *dx_dev, int32_t F,
                      int32_t P, int32_t C, int32_t groups, int32_t accumulate, void *stream) {
    return groupnorm_bwd(x_dev, stats_dev, w_dev, dy_dev, sums_dev, dx_dev, F, P, C, groups, accumulate != 0, (hipStream_t)stream);
}
int edv_attn_temporal_bwd(const float *qkv_dev, const float *dout_dev, float *dqkv_dev, int32_t B, int32_t T, int32_t P, int32_t C, int32_t heads,
                          void *stream) {
    return attn_temporal_bwd(qkv_dev, dout_dev, dqkv_dev, B, T, P, C, heads, (hipStream_t)stream);
}
int edv_pack_conv3x3_bwd(const float *w_dev, float *wpacked_dev, int32_t Cout, int32_t Cin, void *stream) {
    return pack_conv3x3_bwd(w_dev, wpacked_dev, Cout, Cin, (hipStream_t)stream);
}
int edv_conv3x3_s2_bwd(const float *dy_dev, const float *wpacked_dev, float *dx_dev, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                       void *stream) {
    return conv3x3_s2_bwd(dy_dev, wpacked_dev, dx_dev, F, H, W, Cin, Cout, (hipStream_t)stream);
}
int edv_dilate2(const float *dy_dev, float *z_dev, int32_t F, int32_t H, int32_t W, int32_t C, void *stream) {
    return dilate2(dy_dev, z_dev, F, H, W, C, (hipStream_t)stream);
}
int edv_pixel_unshuffle(const float *dy_dev, float *A_dev, int32_t F, int32_t h, int32_t w, int32_t C, int32_t s, void *stream) {
    return pixel_unshuffle(dy_dev, A_dev, F, h, w, C, s, (hipStream_t)stream);
}

int edv_attn_temporal(const float *qkv_dev, float *out_dev, int32_t B, int32_t T, int32_t P, int32_t C, int32_t heads, void *stream) {
    return attn_temporal(qkv_dev, out_dev, B, T, P, C, heads, (hipStream_t)stream);
}

int edv_rope_qk(float *qkv_dev, const float *table_dev, int32_t B, int32_t T, int32_t P, int32_t C, int32_t transpose, void *stream) {
    return rope_qk(qkv_dev, table_dev, B, T, P, C, transpose != 0, (hipStream_t)stream);
}

size_t edv_groupnorm_workspace(int32_t F, int32_t P, int32_t C) { return groupnorm_workspace(F, P, C) * sizeof(float); }

int edv_groupnorm(const float *x_dev, const float *w_dev, const float *b_dev, float *y_dev, float *stats_dev, int32_t F, int32_t P, int32_t C,
                  int32_t groups, float eps, float *workspace_dev, size_t workspace_bytes, void *stream) {
    return groupnorm(x_dev, w_dev, b_dev, y_dev, stats_dev, F, P, C, groups, eps, (hipStream_t)stream, workspace_dev, workspace_bytes / sizeof(float));
}

// Test hook: every CU's whole LDS (160 KB) filled with `value` -- LDS keeps its contents between kernels, so a kernel that reads LDS bytes it never
// wrote (or relies on the DMA writing something it does not write) sees the poison.  tests/test_kernels_gpu.py::test_attention_on_poisoned_lds.
namespace edv {
namespace {
__global__ __launch_bounds__(256) void fill_lds_kernel(float value, float *sink) {
    extern __shared__ float lds_all[];
    for (int i = threadIdx.x; i < 160 * 256; i += 256) lds_all[i] = value;
    __syncthreads();
    if (sink && lds_all[(threadIdx.x * 97) % (160 * 256)] != value) *sink = 1.f;  // keeps the stores alive
}
}  // namespace
}  // namespace edv
int edv_debug_fill_lds(float value, void *stream) {
    int dev = 0, cus = 0;
    EDV_HIP(hipGetDevice(&dev));
    EDV_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    EDV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(edv::fill_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    EDV_LAUNCH(edv::fill_lds_kernel, dim3((unsigned)(8 * cus)), dim3(256), 160 * 1024, (hipStream_t)stream, value, (float *)nullptr);
    EDV_LAUNCH_OK();
    return 0;
}

int edv_geglu(const float *x_dev, float *y_dev, int64_t M, int32_t inner, void *stream) { return geglu(x_dev, y_dev, M, inner, (hipStream_t)stream); }

int edv_bilinear(const float *x_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void *stream) {
    return bilinear(x_dev, y_dev, F, H, W, C, OH, OW, ACT_NONE, (hipStream_t)stream);
}

int edv_dot_channels(const float *x_dev, const float *w_dev, const float *b_dev, float *y_dev, int64_t M, int32_t C, int32_t act, void *stream) {
    EDV_CHECK(act == ACT_NONE || act == ACT_RELU || act == ACT_SIGMOID || act == ACT_SIGMOID_NEG, "act must be 0, 2, 3 or 4");
    return dot_channels(x_dev, w_dev, b_dev, y_dev, M, C, act, (hipStream_t)stream);
}

int edv_patchify(const float *x_dev, float *cols_dev, int32_t F, int32_t H, int32_t W, int32_t ih, int32_t iw, void *stream) {
    return patchify(x_dev, cols_dev, F, H, W, ih, iw, (hipStream_t)stream);
}

int edv_bicubic_pos(const float *grid_dev, float *out_dev, int32_t S, int32_t D, int32_t oh, int32_t ow, double scale_h, double scale_w, void *stream) {
    EDV_CHECK(scale_h > 0 && scale_w > 0, "scale factors must be positive");
    return bicubic_pos(grid_dev, out_dev, S, D, oh, ow, (float)(1.0 / scale_h), (float)(1.0 / scale_w), (hipStream_t)stream);
}

int edv_resize_bicubic(const float *x_dev, float *y_dev, int32_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, void *stream) {
    return resize_bicubic(x_dev, y_dev, planes, H, W, OH, OW, (hipStream_t)stream);
}

int edv_ingest_u8(const uint8_t *src_dev, int32_t src_frames, const int32_t *slots_host, int32_t n, float *out_dev, int32_t H, int32_t W, int32_t OH, int32_t OW,
                  void *stream) {
    return ingest_u8(src_dev, src_frames, slots_host, n, out_dev, H, W, OH, OW, (hipStream_t)stream);
}

size_t edv_render_workspace(int64_t n) { return render_workspace(n); }
int edv_render_range(const float *x_dev, int64_t n, int32_t h, int32_t w, int32_t mode, int64_t rank_lo, int64_t rank_hi, float *range_dev, void *workspace_dev,
                     size_t workspace_bytes, void *stream) {
    return render_range(x_dev, n, h, w, mode, rank_lo, rank_hi, range_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int edv_render_colorize(const float *x_dev, int64_t n, int32_t h, int32_t w, const float *range_dev, int32_t range_stride, float eps, int32_t clip,
                        const uint8_t *lut_dev, const uint8_t *beside_dev, uint8_t *out_dev, void *stream) {
    return render_colorize(x_dev, n, h, w, range_dev, range_stride, eps, clip, lut_dev, beside_dev, out_dev, (hipStream_t)stream);
}

namespace {
CloudSel cloud_sel(const edv_cloud_selection &s) {
    return CloudSel{s.x_dev, s.n, s.h, s.w, s.step, s.mode, s.lo, s.span, s.gain, s.near_z, s.far_z, s.mask_dev, s.mask_stride};
}
}  // namespace
int32_t edv_cloud_tile_pixels(void) { return cloud_tile_pixels(); }
size_t edv_cloud_workspace(int64_t n, int32_t h, int32_t w, int32_t step) { return cloud_workspace(n, h, w, step); }
int edv_cloud_count(const edv_cloud_selection *sel, int64_t *offsets_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    EDV_CHECK(sel, "null selection");
    return cloud_count(cloud_sel(*sel), reinterpret_cast<long long *>(offsets_dev), workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int edv_cloud_scatter(const edv_cloud_selection *sel, const double *cams_dev, int32_t cam_stride, const uint8_t *frames_dev, const int64_t *offsets_dev,
                      const void *workspace_dev, size_t workspace_bytes, float *points_dev, uint8_t *colors_dev, int64_t capacity, void *stream) {
    EDV_CHECK(sel, "null selection");
    return cloud_scatter(cloud_sel(*sel), cams_dev, cam_stride, frames_dev, reinterpret_cast<const long long *>(offsets_dev), workspace_dev, workspace_bytes,
                         points_dev, colors_dev, capacity, (hipStream_t)stream);
}

namespace {
TsdfVol tsdf_vol(const edv_tsdf_volume &v) {
    return TsdfVol{v.tsdf_dev, v.weight_dev, v.color_dev, v.nx, v.ny, v.nz, {v.origin[0], v.origin[1], v.origin[2]}, v.voxel, v.trunc, v.max_weight};
}
}  // namespace
int32_t edv_tsdf_tile_voxels(void) { return tsdf_tile_voxels(); }
size_t edv_tsdf_workspace(int32_t nx, int32_t ny, int32_t nz) { return tsdf_workspace(nx, ny, nz); }
int edv_tsdf_integrate(const edv_tsdf_volume *vol, const edv_cloud_selection *sel, const double *cams_dev, int32_t cam_stride, const uint8_t *frames_dev,
                       void *stream) {
    EDV_CHECK(vol, "null volume");
    EDV_CHECK(sel, "null selection");
    return tsdf_integrate(tsdf_vol(*vol), cloud_sel(*sel), cams_dev, cam_stride, frames_dev, (hipStream_t)stream);
}
int edv_tsdf_count(const edv_tsdf_volume *vol, float min_weight, int64_t *total_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    EDV_CHECK(vol, "null volume");
    return tsdf_count(tsdf_vol(*vol), min_weight, reinterpret_cast<long long *>(total_dev), workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int edv_tsdf_extract(const edv_tsdf_volume *vol, float min_weight, const void *workspace_dev, size_t workspace_bytes, float *points_dev, uint8_t *colors_dev,
                     int64_t capacity, void *stream) {
    EDV_CHECK(vol, "null volume");
    return tsdf_extract(tsdf_vol(*vol), min_weight, workspace_dev, workspace_bytes, points_dev, colors_dev, capacity, (hipStream_t)stream);
}

size_t edv_tsdf_mesh_workspace(int32_t nx, int32_t ny, int32_t nz) { return tsdf_mesh_workspace(nx, ny, nz); }
int edv_tsdf_mesh_count(const edv_tsdf_volume *vol, float min_weight, int64_t *totals_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    EDV_CHECK(vol, "null volume");
    return tsdf_mesh_count(tsdf_vol(*vol), min_weight, reinterpret_cast<long long *>(totals_dev), workspace_dev, workspace_bytes, (hipStream_t)stream);
}
// min_weight is not read again: the flags edv_tsdf_mesh_count left in the workspace hold every comparison with it
int edv_tsdf_mesh_extract(const edv_tsdf_volume *vol, float /*min_weight*/, const void *workspace_dev, size_t workspace_bytes, float *vertices_dev,
                          float *normals_dev, uint8_t *colors_dev, int64_t vertex_capacity, int32_t *triangles_dev, int64_t triangle_capacity, void *stream) {
    EDV_CHECK(vol, "null volume");
    return tsdf_mesh_extract(tsdf_vol(*vol), workspace_dev, workspace_bytes, vertices_dev, normals_dev, colors_dev, vertex_capacity, triangles_dev,
                             triangle_capacity, (hipStream_t)stream);
}

int edv_tsdf_raycast(const edv_tsdf_volume *vol, const double *cams_dev, int32_t views, int32_t h, int32_t w, double near, double step, int32_t steps,
                     float min_weight, float *depth_dev, float *normals_dev, uint8_t *colors_dev, void *stream) {
    EDV_CHECK(vol, "null volume");
    return tsdf_raycast(tsdf_vol(*vol), cams_dev, views, h, w, near, step, steps, min_weight, depth_dev, normals_dev, colors_dev, (hipStream_t)stream);
}

int32_t edv_icp_tile_pixels(void) { return icp_tile_pixels(); }
size_t edv_icp_workspace(int32_t h, int32_t w, int32_t step) { return icp_workspace(h, w, step); }
int edv_icp_sums(const edv_cloud_selection *sel, int64_t frame, const double *live_cam_host, const double *model_cam_host, const float *model_depth_dev,
                 const float *model_normals_dev, int32_t mh, int32_t mw, double max_dist2, double *sums_dev, void *workspace_dev, size_t workspace_bytes,
                 void *stream) {
    EDV_CHECK(sel, "null selection");
    return icp_sums(cloud_sel(*sel), frame, live_cam_host, model_cam_host, model_depth_dev, model_normals_dev, mh, mw, max_dist2, sums_dev, workspace_dev,
                    workspace_bytes, (hipStream_t)stream);
}
size_t edv_icp_scaled_workspace(int32_t h, int32_t w, int32_t step) { return icp_scaled_workspace(h, w, step); }
int edv_icp_scaled_sums(const edv_cloud_selection *sel, int64_t frame, const double *live_cam_host, const double *model_cam_host, const float *model_depth_dev,
                        const float *model_normals_dev, int32_t mh, int32_t mw, double max_dist2, double *sums_dev, void *workspace_dev, size_t workspace_bytes,
                        void *stream) {
    EDV_CHECK(sel, "null selection");
    return icp_scaled_sums(cloud_sel(*sel), frame, live_cam_host, model_cam_host, model_depth_dev, model_normals_dev, mh, mw, max_dist2, sums_dev, workspace_dev,
                           workspace_bytes, (hipStream_t)stream);
}
size_t edv_icp_colour_workspace(int32_t h, int32_t w, int32_t step, int32_t cols) { return icp_colour_workspace(h, w, step, cols); }
int edv_icp_colour_sums(const edv_cloud_selection *sel, int64_t frame, const uint8_t *frames_dev, const double *live_cam_host, const double *model_cam_host,
                        const float *model_depth_dev, const float *model_normals_dev, const uint8_t *model_colors_dev, int32_t mh, int32_t mw, double max_dist2,
                        int32_t cols, double *sums_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    EDV_CHECK(sel, "null selection");
    return icp_colour_sums(cloud_sel(*sel), frame, frames_dev, live_cam_host, model_cam_host, model_depth_dev, model_normals_dev, model_colors_dev, mh, mw, max_dist2,
                           cols, sums_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int edv_frame_normals(const edv_cloud_selection *sel, const double *cams_dev, int32_t cam_stride, int64_t first, int64_t count, float *normals_dev, void *stream) {
    EDV_CHECK(sel, "null selection");
    return frame_normals(cloud_sel(*sel), cams_dev, cam_stride, first, count, normals_dev, (hipStream_t)stream);
}
size_t edv_icp_robust_workspace(int32_t h, int32_t w, int32_t step, int32_t cols, int32_t colour) { return icp_robust_workspace(h, w, step, cols, colour); }
int edv_icp_robust_sums(const edv_cloud_selection *sel, int64_t frame, const uint8_t *frames_dev, const double *live_cam_host, const double *model_cam_host,
                        const float *model_depth_dev, const float *model_normals_dev, const uint8_t *model_colors_dev, int32_t mh, int32_t mw, double max_dist2,
                        int32_t cols, const float *live_normals_dev, double min_cos, double huber, double huber_colour, double *sums_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream) {
    EDV_CHECK(sel, "null selection");
    return icp_robust_sums(cloud_sel(*sel), frame, frames_dev, live_cam_host, model_cam_host, model_depth_dev, model_normals_dev, model_colors_dev, mh, mw, max_dist2,
                           cols, live_normals_dev, min_cos, huber, huber_colour, sums_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int32_t edv_pyramid_max_levels(void) { return pyramid_max_levels(); }
size_t edv_pyramid_pixels(int32_t h, int32_t w, int32_t levels, int64_t *offsets_host) {
    return pyramid_pixels(h, w, levels, reinterpret_cast<long long *>(offsets_host));
}
int edv_depth_pyramid(const edv_cloud_selection *sel, int64_t frame, int32_t levels, float one_plus_jump, float *levels_dev, void *stream) {
    EDV_CHECK(sel, "null selection");
    return depth_pyramid(cloud_sel(*sel), frame, levels, one_plus_jump, levels_dev, (hipStream_t)stream);
}
int edv_rgb_pyramid(const uint8_t *frames_dev, int64_t n, int32_t h, int32_t w, int64_t frame, int32_t levels, uint8_t *levels_dev, void *stream) {
    return rgb_pyramid(frames_dev, n, h, w, frame, levels, levels_dev, (hipStream_t)stream);
}

size_t edv_stitch_workspace(void) { return stitch_workspace(); }
int edv_stitch_fit(const float *disp_dev, int32_t ih, int32_t iw, const float *tail_dev, int32_t fh, int32_t fw, float *st_dev, void *workspace_dev,
                   size_t workspace_bytes, void *stream) {
    return stitch_fit(disp_dev, ih, iw, tail_dev, fh, fw, st_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int edv_stitch_apply(const float *disp_dev, int32_t ih, int32_t iw, const float *st_dev, float *tail_dev, float *new_dev, int32_t fh, int32_t fw,
                     void *stream) {
    return stitch_apply(disp_dev, ih, iw, st_dev, tail_dev, new_dev, fh, fw, (hipStream_t)stream);
}

size_t edv_metrics_workspace(int64_t n, int32_t h, int32_t w) { return metrics_workspace(n, h, w); }
int edv_masked_median(const float *x_dev, const float *gate_dev, int64_t count, float lo, float hi, double *out_dev, void *workspace_dev, size_t workspace_bytes,
                      void *stream) {
    return masked_median(x_dev, gate_dev, count, lo, hi, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int edv_metrics_pred(const float *disp_dev, const float *gt_dev, float *pred_dev, int64_t n, int32_t h, int32_t w, double min_depth, double max_depth, int32_t align,
                     float pred_depth_scale_factor, float eval_max_depth, double *scalars_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return metrics_pred(disp_dev, gt_dev, pred_dev, n, h, w, min_depth, max_depth, align, pred_depth_scale_factor, eval_max_depth, scalars_dev, workspace_dev,
                        workspace_bytes, (hipStream_t)stream);
}
int edv_metrics_errors(const float *pred_dev, const float *gt_dev, int64_t n, int32_t h, int32_t w, float eval_max_depth, double *out_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream) {
    return metrics_errors(pred_dev, gt_dev, n, h, w, eval_max_depth, out_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}
int edv_metrics_temporal(const float *pred_dev, const float *gt_dev, int64_t n, int32_t h, int32_t w, float eval_max_depth, const double *mats_dev, double *out_dev,
                         float *warp_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return metrics_temporal(pred_dev, gt_dev, n, h, w, eval_max_depth, mats_dev, out_dev, warp_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int edv_fold_lora(const float *W_dev, const float *A_dev, const float *B_dev, const float *U_dev, const float *V_dev, float scale, float *out_dev,
                  int32_t nout, int32_t nin, int32_t r, void *stream) {
    return fold_lora(W_dev, A_dev, B_dev, U_dev, V_dev, scale, out_dev, nout, nin, r, (hipStream_t)stream);
}

// ---- test entry points (ABI 13): the descriptor forms only the engine reaches otherwise (tests/test_mapped_kernels_gpu.py) ----
namespace edv {
namespace {
// (period, stride, offset, inner) -> RowMap; a null pointer is the identity
bool row_map_from(const int32_t *m, RowMap *out) {
    *out = identity_map();
    if (!m) return true;
    if (m[0] < 0 || m[1] < 0 || m[2] < 0 || (m[3] != 0 && m[3] != 1)) return false;
    *out = RowMap{m[0], m[1], m[2], m[3]};
    return true;
}
}  // namespace
}  // namespace edv

int edv_gemm_desc(const edv_gemm_desc_t *d, void *stream) {
    EDV_CHECK(d, "null descriptor");
    GemmDesc g;
    g.A = d->A; g.lda = d->lda; g.W = d->W; g.ldw = d->ldw; g.C = d->C; g.ldc = d->ldc; g.M = d->M; g.N = d->N; g.K = d->K;
    g.bias = d->bias; g.act = d->act; g.gamma = d->gamma;
    g.R1 = d->R1; g.ldr1 = d->ldr1; g.R2 = d->R2; g.ldr2 = d->ldr2; g.P1 = d->P1; g.ldp1 = d->ldp1;
    g.ws = d->workspace; g.ws_floats = d->workspace_bytes / sizeof(float);
    g.Wx6 = d->x6_planes;
    EDV_CHECK(row_map_from(d->a_map, &g.a_map) && row_map_from(d->c_map, &g.c_map) && row_map_from(d->r1_map, &g.r1_map) &&
                  row_map_from(d->p1_map, &g.p1_map),
              "row map: period, stride, offset >= 0 and inner 0 or 1");
    EDV_CHECK(d->act >= ACT_NONE && d->act <= ACT_RELU, "act must be 0, 1 or 2");
    EDV_CHECK(d->N > 0 && d->ldc >= d->N, "ldc must be at least N");
    EDV_CHECK(!d->R1 || d->ldr1 >= d->N, "ldr1 must be at least N");
    EDV_CHECK(!d->R2 || d->ldr2 >= d->N, "ldr2 must be at least N");
    EDV_CHECK(!d->P1 || d->ldp1 >= d->N, "ldp1 must be at least N");
    return gemm(g, (hipStream_t)stream);
}

int edv_layernorm_mapped(const float *x_dev, const int32_t *in_map, const float *w_dev, const float *b_dev, float *y_dev, const int32_t *out_map,
                         int64_t rows, int32_t dim, float eps, const float *pe_dev, int32_t rows_per_frame, int32_t T, int32_t act, int32_t accumulate,
                         void *stream) {
    RowMap im, om;
    EDV_CHECK(row_map_from(in_map, &im) && row_map_from(out_map, &om), "row map: period, stride, offset >= 0 and inner 0 or 1");
    return layernorm(x_dev, im, w_dev, b_dev, y_dev, om, rows, dim, eps, pe_dev, rows_per_frame, T, (hipStream_t)stream, act, accumulate != 0);
}

int edv_layernorm_bwd_mapped(const float *x_dev, const int32_t *x_map, const float *w_dev, const float *dy_dev, const int32_t *dy_map, float *dx_dev,
                             const int32_t *dx_map, int64_t rows, int32_t dim, float eps, int32_t accumulate, void *stream) {
    RowMap xm, gm, dm;
    EDV_CHECK(row_map_from(x_map, &xm) && row_map_from(dy_map, &gm) && row_map_from(dx_map, &dm), "row map: period, stride, offset >= 0 and inner 0 or 1");
    return layernorm_bwd(x_dev, xm, w_dev, dy_dev, gm, dx_dev, dm, rows, dim, eps, accumulate != 0, (hipStream_t)stream);
}

int edv_fold_ssb(const float *W_dev, const float *a_dev, const float *b_dev, float *out_dev, int32_t nout, int32_t nin, void *stream) {
    return fold_ssb(W_dev, a_dev, b_dev, out_dev, nout, nin, (hipStream_t)stream);
}
int edv_fold_bn(float *w_dev, const float *b_dev, const float *gamma_dev, const float *beta_dev, const float *mean_dev, const float *var_dev, float eps,
                float *bout_dev, int32_t nout, int32_t K, void *stream) {
    return fold_bn(w_dev, b_dev, gamma_dev, beta_dev, mean_dev, var_dev, eps, bout_dev, nout, K, (hipStream_t)stream);
}
int edv_fold_dash(const float *Utop_dev, const float *idx_dev, const float *Vtop_dev, float *inout_dev, int32_t nout, int32_t nin, int32_t r, void *stream) {
    return fold_dash(Utop_dev, idx_dev, Vtop_dev, inout_dev, nout, nin, r, (hipStream_t)stream);
}
int edv_col_dot(const float *P_dev, const float *Q_dev, int64_t M, int32_t N, const float *scale_dev, float *part_dev, float *out_dev, void *stream) {
    return col_dot(P_dev, Q_dev, M, N, scale_dev, part_dev, out_dev, (hipStream_t)stream);
}
int edv_ssb_prep(const float *W_dev, const float *a_dev, const float *b_dev, const float *gamma_dev, float *Wa_dev, float *gb_dev, int32_t nout,
                 int32_t nin, void *stream) {
    return ssb_prep(W_dev, a_dev, b_dev, gamma_dev, Wa_dev, gb_dev, nout, nin, (hipStream_t)stream);
}
int edv_sigmoid_bwd(const float *g_dev, const float *s_dev, float *out_dev, int64_t n, void *stream) {
    return sigmoid_bwd(g_dev, s_dev, out_dev, n, (hipStream_t)stream);
}
int edv_bilinear_add(const float *x_dev, const float *add_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW,
                     void *stream) {
    EDV_CHECK(add_dev, "null addend");
    return bilinear(x_dev, y_dev, F, H, W, C, OH, OW, ACT_NONE, (hipStream_t)stream, add_dev);
}

// ---- test entry point (ABI 15): the launchers' planner and policies on a given slot count (tests/test_split_plan_cpu.py) ----
int edv_split_plan(int32_t kind, int64_t tiles_or_tasks, int32_t slots, int32_t k_tiles, int64_t out[8]) {
    if (kind == 5) {  // gemm_x6's remainder walk: the whole tile of raw block index `tiles_or_tasks` in a grid of `slots` workgroups, `k_tiles` of them run owners
        EDV_CHECK(out && slots > 0 && k_tiles >= 0 && k_tiles <= slots && tiles_or_tasks >= k_tiles && tiles_or_tasks < slots, "kind 5: nsplit <= block < grid");
        std::fill(out, out + 8, 0);
        out[0] = front_whole_tile((int)tiles_or_tasks, slots, k_tiles);
        return 0;
    }
    EDV_CHECK(out && kind >= 0 && kind <= 4 && tiles_or_tasks > 0 && tiles_or_tasks < (1ll << 31) && k_tiles > 0, "kind 0..5, a positive count below 2^31");
    if (kind == 4) {  // gemm_x6's remainder plan: slots = CUs; on entry out[0] = resident workgroups per CU, out[1] = 1 (by policy) or 2 (wherever supported)
        const int wgs = (int)out[0], mode = (int)out[1];
        EDV_CHECK(slots > 0 && wgs > 0 && wgs <= 64 && (mode == 1 || mode == 2), "kind 4: out[0] = workgroups per CU, out[1] = mode 1 or 2");
        const SplitPolicy &pol = gemm_x6_split_policy();
        GemmSplit sp{};
        long long grid;
        plan_plain(tiles_or_tasks, pol, &sp, &grid);
        const bool rem = gemm_x6_plan(tiles_or_tasks, k_tiles, slots * wgs, slots, wgs, mode, &sp, &grid) == 2;  // as launch_x6 decides
        const int64_t r[8] = {1, grid, sp.first_split, sp.chunk, sp.nsplit, tiles_or_tasks - sp.first_split, sp.units, (int64_t)split_ws_floats(sp, pol)};
        std::fill(out, out + 8, 0);  // another plan: all zero
        if (rem) std::copy(r, r + 8, out);
        return 0;
    }
    if (kind == 3) {
        const TaskSplit t = plan_tasks(tiles_or_tasks, k_tiles, slots, false);
        const int64_t r[8] = {t.nsplit > 0, t.grid, t.whole_rounds, t.chunk, t.nsplit, t.leftover, t.units, (int64_t)t.pieces()};
        std::copy(r, r + 8, out);
        return 0;
    }
    const SplitPolicy &pol = kind == 0 ? gemm_dma_split_policy() : kind == 1 ? gemm_x6_split_policy() : conv_dma_split_policy();
    GemmSplit sp{};
    long long grid;
    plan_plain(tiles_or_tasks, pol, &sp, &grid);
    const bool split = plan_split(tiles_or_tasks, slots, k_tiles, pol, &sp, &grid);
    const int64_t r[8] = {split, grid, sp.whole_rounds, sp.chunk, sp.nsplit, sp.stride, sp.units, split ? (int64_t)split_ws_floats(sp, pol) : 0};
    std::copy(r, r + 8, out);
    return 0;
}

size_t edv_trainer_loss_workspace(int32_t N, int32_t H, int32_t W) { return trainer_loss_workspace(N, H, W) * sizeof(float); }
int edv_trainer_loss(const edv_trainer_loss_inputs *in, int32_t N, int32_t H, int32_t W, const edv_trainer_loss_weights *weights, float *losses_dev,
                     const edv_trainer_loss_grads *grads, float *workspace_dev, size_t workspace_bytes, void *stream) {
    EDV_CHECK(in && weights && grads, "null argument");
    TrainerLossIn a{};
    TrainerLossGrads g{};
    for (int s = 0; s < 4; ++s) {
        a.color[s] = in->color[s];
        a.disp[s] = in->disp[s];
        a.disp_h[s] = in->disp_h[s];
        a.disp_w[s] = in->disp_w[s];
        g.disp[s] = grads->disp[s];
        for (int n = 0; n < 2; ++n) {
            a.refined[s][n] = in->refined[s][n];
            a.registration[s][n] = in->registration[s][n];
            a.transform[s][n] = in->transform[s][n];
            a.position[s][n] = in->position[s][n];
            g.refined[s][n] = grads->refined[s][n];
            g.transform[s][n] = grads->transform[s][n];
        }
    }
    for (int n = 0; n < 2; ++n) {
        a.color_nb[n] = in->color_nb[n];
        a.T[n] = in->T[n];
        a.mask[n] = in->mask[n];
        g.T[n] = grads->T[n];
    }
    a.K = in->K;
    a.invK = in->invK;
    g.K = grads->K;
    g.invK = grads->invK;
    const TrainerLossW w{weights->disparity_smoothness, weights->transform_constraint, weights->transform_smoothness, weights->depth_reproj, weights->depth_flow,
                         weights->tune_temporal, weights->min_depth, weights->max_depth};
    return trainer_loss(a, N, H, W, w, losses_dev, g, workspace_dev, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

size_t edv_photometric_loss_workspace(int32_t B, int32_t T, int32_t H, int32_t W) { return photometric_loss_workspace(B, T, H, W) * sizeof(float); }
int edv_photometric_loss(const float *frames_dev, const float *const disp_dev[4], const int32_t disp_h[4], const int32_t disp_w[4], int32_t B, int32_t T, int32_t H,
                         int32_t W, const float *K_dev, const float *invK_dev, const float *Tprev_dev, const float *Tnext_dev, float min_depth, float max_depth,
                         float disparity_smoothness, float *loss_dev, float *const grad_disp_dev[4], float *workspace_dev, size_t workspace_bytes, void *stream) {
    EDV_CHECK(disp_h && disp_w, "null argument");
    const int dh[4] = {disp_h[0], disp_h[1], disp_h[2], disp_h[3]}, dw[4] = {disp_w[0], disp_w[1], disp_w[2], disp_w[3]};
    return photometric_loss(frames_dev, disp_dev, dh, dw, B, T, H, W, K_dev, invK_dev, Tprev_dev, Tnext_dev, min_depth, max_depth, disparity_smoothness, loss_dev,
                            grad_disp_dev, workspace_dev, workspace_bytes / sizeof(float), (hipStream_t)stream);
}

}  // extern "C"
