// The fine-tune step's photometric loss and its gradient with respect to the four disparity maps, fused.
//
// What it restates (reference trainer_end_to_end_video.py:808-868 generate_images_pred, :899-911 compute_reprojection_loss, :927-951 the
// per-scale sum; utils/layers.py:11-20 disp_to_depth, :134-189 BackprojectDepth / Project3D, :222-236 get_smooth_loss, :276-306 SSIM), with
// the relative poses and intrinsics as inputs (the pose network is outside the hot path):
//
//   total = 1/4 sum_s [ 1/2 sum_{nb in {prev, next}} mean_{kept frames, pixels} (0.85 mean_c SSIM_c(warp_nb, frame) + 0.15 mean_c |frame - warp_nb|)
//                       + lambda / 2^s (mean |d_x norm| e^{-|d_x img|} + mean |d_y norm| e^{-|d_y img|}) ],   norm = D / (mean_frame D + 1e-7)
//   D = disp_s resized to the frame size (bilinear, align_corners), depth = 1 / (1/max + (1/min - 1/max) D),
//   warp_nb(p) = bilinear sample (border padding, align_corners) of the neighbouring frame at the projection of pixel p's 3-D point.
//
// Why it exists: as ~500 eager PyTorch kernels per step (every one a bandwidth-bound pass over [T, 3, 518, 518]) the loss was 36 % of the
// ViT-S fine-tune step (17.4 of 48.5 ms; profiles/r02_c_train_vits_T8_kernel_stats.csv) -- the condition SURVEY.md §8f rank 4 sets for
// building it.  Here a scale costs seven launches: every tensor is read a few times and the 3x3 SSIM windows are tiled through LDS.
//
// The loss value AND dL/d disp_s come out of one call (a training step always wants both): each kernel is a gather, no float atomics, every
// reduction is two-stage in a fixed order -- results are reproducible run to run.
//
// Kernels per scale (N = B*T frames, P = H*W pixels); the per-pixel warp, the SSIM tile and the sums are loss_common.hpp's:
//   bilinear (resample.hip)   D [N, P]                     (skipped when disp_s already has the frame size)
//   frame_sum_kernel x2       m[f] = mean_p D              (64 partials per frame, then one wave per frame)
//   smooth_kernel             g_sm [N, P] = dL_smooth / d norm, partial sums of the loss terms and of g_sm * D per frame
//   warp_kernel               x [2, N, 3, P] = the two warped neighbours (warp_pixel)
//   ssim_kernel<false>        LDS tile 32x32 + halo 2 per (neighbour, frame, channel): loss partials, g_x = dL / d x
//   finish_kernel             per-frame S_f = sum g_sm D; loss += this scale's terms
//   warp_bwd_kernel           gD [N, P]: g_x through the sampling coordinates, the projection and the depth map, + the smoothness term
//   bilinear_bwd (bwd.hip)    dL/d disp_s                  (skipped when no resize)
#include <cmath>

#include "loss_common.hpp"

namespace edv {
namespace {

// x[nb][f][c][p]: the neighbouring frame sampled where pixel p of frame f lands (trainer :853-857)
__global__ __launch_bounds__(256) void warp_kernel(const float *__restrict__ D, const float *__restrict__ img, const Cam *__restrict__ cams, float *__restrict__ xw, int N,
                                                   int T, int H, int W, float da, float db) {
    const long long P = (long long)H * W;
    const int f = blockIdx.y, nb = blockIdx.z, t = f % T;
    if ((nb == 0 && t == 0) || (nb == 1 && t == T - 1)) return;  // no such neighbour inside the clip
    const float *src = img + (long long)(nb ? f + 1 : f - 1) * 3 * P;
    const Cam c = cams[2 * f + nb];
    float *o = xw + ((long long)nb * N + f) * 3 * P;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        warp_pixel(c, D[(long long)f * P + p], x, y, src, o + p, P, H, W, da, db);
    }
}

// One workgroup: S[f] = sum of the per-block g_sm * D partials; loss += sum of the SSIM / L1 partials + w_sm (sum t_x / Nx + sum t_y / Ny)
__global__ __launch_bounds__(256) void finish_kernel(const float *__restrict__ ssim_part, long long n_ssim, const float *__restrict__ sm_part, int sm_blocks, int N,
                                                     float *__restrict__ S, float *__restrict__ loss, float w_sm, float inv_nx, float inv_ny) {
    __shared__ float t[3];
    float a = 0.f, tx, ty;
    for (long long i = threadIdx.x; i < n_ssim; i += 256) a += ssim_part[i];
    smooth_part_sums(sm_part, sm_blocks, N, S, tx, ty);
    block_sum_pairs_store({a, tx, ty}, t);
    __syncthreads();
    if (threadIdx.x == 0) loss[0] += t[0] + w_sm * (t[1] * inv_nx + t[2] * inv_ny);
}

// gD[f][p] = dL/dD: the warped neighbours' gradients through the sampling coordinates (grid_sampler backward), the projection
// (utils/layers.py:176-189) and the depth map (:11-20), plus the smoothness term through norm = D / (mean + 1e-7)
__global__ __launch_bounds__(256) void warp_bwd_kernel(const float *__restrict__ D, const float *__restrict__ img, const Cam *__restrict__ cams, const float *__restrict__ gx,
                                                       const float *__restrict__ gsm, const float *__restrict__ mean, const float *__restrict__ S, float *__restrict__ gD,
                                                       int N, int T, int H, int W, float da, float db, float w_sm) {
    const long long P = (long long)H * W;
    const int f = blockIdx.y, t = f % T;
    const float den = mean[f] + 1e-7f;
    const float sm_all = S[f] / (den * den) / (float)P;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const float depth = 1.0f / (da + db * D[(long long)f * P + p]);
        float gdepth = 0.f;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            if ((nb == 0 && t == 0) || (nb == 1 && t == T - 1)) continue;
            const float *src = img + (long long)(nb ? f + 1 : f - 1) * 3 * P;
            const Sample s = project_pixel(cams[2 * f + nb], depth, x, y, H, W);
            const float fx0 = floorf(s.ix), fy0 = floorf(s.iy);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const float wx = s.ix - fx0, wy = s.iy - fy0;
            const bool xin = x0 + 1 < W, yin = y0 + 1 < H;
            float gix = 0.f, giy = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float *sc = src + ch * P + (long long)y0 * W + x0;
                const float v00 = sc[0], v01 = xin ? sc[1] : 0.f, v10 = yin ? sc[W] : 0.f, v11 = (xin && yin) ? sc[W + 1] : 0.f;
                const float g = gx[(((long long)nb * N + f) * 3 + ch) * P + p];
                gix += g * ((v01 - v00) * (1.f - wy) + (v11 - v10) * wy);
                giy += g * ((v10 - v00) * (1.f - wx) + (v11 - v01) * wx);
            }
            gix *= s.mx;
            giy *= s.my;
            const float zi = s.Z + 1e-7f;
            // u = X / (Z + eps), d u / d depth = rx / zi - X rz / zi^2   (ix = u up to rounding: grid normalisation and un-normalisation cancel)
            gdepth += gix * (s.rx / zi - s.X * s.rz / (zi * zi)) + giy * (s.ry / zi - s.Y * s.rz / (zi * zi));
        }
        gD[(long long)f * P + p] = gdepth * (-db * depth * depth) + w_sm * (gsm[(long long)f * P + p] / den - sm_all);
    }
}

__global__ void kept_kernel(int *kept, int B, int T) {  // kept[k] = {frame with a previous neighbour, frame with a next neighbour}, k < B (T - 1)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B * (T - 1)) return;
    const int b = k / (T - 1), i = k - b * (T - 1);
    kept[2 * k] = b * T + i + 1;
    kept[2 * k + 1] = b * T + i;
}

struct LossWs {  // carve-up of the caller's workspace (floats)
    size_t cams, kept, D, mean, S, sum_part, sm_part, ssim_part, gsm, gD, xw, gx, total;
};
LossWs loss_layout(int B, int T, int H, int W) {
    const size_t N = (size_t)B * T, P = (size_t)H * W;
    LossWs w;
    Carve c;
    w.cams = c.take(2 * N * (sizeof(Cam) / sizeof(float)));
    w.kept = c.take(2 * (size_t)B * (T - 1));
    w.D = c.take(N * P);
    w.mean = c.take(N);
    w.S = c.take(N);
    w.sum_part = c.take(N * SUM_PARTS);
    w.sm_part = c.take(N * 64 * 3);
    w.ssim_part = c.take(2 * (size_t)B * (T - 1) * 3 * ssim_tiles(H, W));
    w.gsm = c.take(N * P);
    w.gD = c.take(N * P);
    w.xw = c.take(2 * N * 3 * P);
    w.gx = c.take(2 * N * 3 * P);
    w.total = c.o;
    return w;
}

}  // namespace

size_t photometric_loss_workspace(int B, int T, int H, int W) {
    if (B <= 0 || T < 2 || H < 3 || W < 3) return 0;
    return loss_layout(B, T, H, W).total;
}

int photometric_loss(const float *frames, const float *const disp[4], const int *dh, const int *dw, int B, int T, int H, int W, const float *K, const float *invK,
                     const float *Tprev, const float *Tnext, float min_depth, float max_depth, float smoothness, float *loss, float *const grad[4], float *ws,
                     size_t ws_floats, hipStream_t st) {
    EDV_CHECK(frames && disp && dh && dw && K && invK && Tprev && Tnext && loss && grad && ws, "null argument");
    EDV_CHECK(B > 0 && T >= 2, "the photometric loss needs clips of at least two frames");
    EDV_CHECK(H >= 3 && W >= 3, "frames smaller than the SSIM window");
    EDV_CHECK(min_depth > 0.f && max_depth > min_depth, "depth range");
    const LossWs L = loss_layout(B, T, H, W);
    EDV_CHECK(ws_floats >= L.total && (uintptr_t)ws % 16 == 0, "workspace too small (photometric_loss_workspace)");
    const int N = B * T;
    EDV_CHECK(N <= 65535, "too many frames");
    const long long P = (long long)H * W;
    const int kept_n = B * (T - 1);
    Cam *cams = reinterpret_cast<Cam *>(ws + L.cams);
    int *kept = reinterpret_cast<int *>(ws + L.kept);
    float *Dbuf = ws + L.D, *mean = ws + L.mean, *S = ws + L.S, *sum_part = ws + L.sum_part, *sm_part = ws + L.sm_part, *ssim_part = ws + L.ssim_part;
    float *gsm = ws + L.gsm, *gD = ws + L.gD, *xw = ws + L.xw, *gx = ws + L.gx;
    const auto [da, db] = depth_coef(min_depth, max_depth);
    const int tiles_x = ceil_div(W, TS), tiles = (int)ssim_tiles(H, W);
    const int pix_blocks = blocks_for(P, 1024);
    const int sm_blocks = 64;
    const float cnt = (float)((double)kept_n * (double)P);
    const float inv_nx = (float)(1.0 / ((double)N * H * (W - 1))), inv_ny = (float)(1.0 / ((double)N * (H - 1) * W));

    EDV_HIP(hipMemsetAsync(loss, 0, sizeof(float), st));
    EDV_LAUNCH(cam_kernel, dim3((2 * N + 63) / 64), dim3(64), 0, st, K, invK, Tprev, Tnext, cams, N);
    EDV_LAUNCH_OK();
    EDV_LAUNCH(kept_kernel, dim3((kept_n + 63) / 64), dim3(64), 0, st, kept, B, T);
    EDV_LAUNCH_OK();
    for (int s = 0; s < 4; ++s) {
        EDV_CHECK(disp[s] && grad[s] && dh[s] > 0 && dw[s] > 0, "bad disparity map");
        const bool same = dh[s] == H && dw[s] == W;
        const float *D = disp[s];
        if (!same) {  // F.interpolate(disp, [H, W], mode="bilinear", align_corners=True) (trainer :813-817, :931-933)
            EDV_TRY(bilinear(disp[s], Dbuf, N, dh[s], dw[s], 1, H, W, ACT_NONE, st));
            D = Dbuf;
        }
        // weights of this scale's terms in the total (trainer :948-966: / 2 per neighbour pair, smoothness / 2^s, mean over the 4 scales)
        const float w_rep = 0.25f * 0.5f / cnt, w_sm = 0.25f * smoothness / (float)(1 << s);
        EDV_LAUNCH(frame_sum_kernel, dim3(SUM_PARTS, N), dim3(256), 0, st, D, sum_part, P);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(frame_sum_finish_kernel, dim3(N), dim3(64), 0, st, sum_part, mean, (float)(1.0 / (double)P));
        EDV_LAUNCH_OK();
        EDV_LAUNCH(smooth_kernel, dim3(sm_blocks, N), dim3(256), 0, st, D, frames, mean, gsm, sm_part, H, W, inv_nx, inv_ny);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(warp_kernel, dim3(pix_blocks, N, 2), dim3(256), 0, st, D, frames, cams, xw, N, T, H, W, da, db);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(ssim_kernel<false>, dim3(tiles, 3, 2 * kept_n), dim3(256), 0, st, xw, frames, nullptr, nullptr, nullptr, gx, nullptr, ssim_part, kept, N, H, W, tiles_x,
                           w_rep, 0.f);
        EDV_LAUNCH_OK();
        EDV_LAUNCH(finish_kernel, dim3(1), dim3(256), 0, st, ssim_part, (long long)2 * kept_n * 3 * tiles, sm_part, sm_blocks, N, S, loss, w_sm, inv_nx, inv_ny);
        EDV_LAUNCH_OK();
        float *gdst = same ? grad[s] : gD;
        EDV_LAUNCH(warp_bwd_kernel, dim3(pix_blocks, N), dim3(256), 0, st, D, frames, cams, gx, gsm, mean, S, gdst, N, T, H, W, da, db, w_sm);
        EDV_LAUNCH_OK();
        if (!same) EDV_TRY(bilinear_bwd(gD, grad[s], N, dh[s], dw[s], 1, H, W, false, st));
    }
    return 0;
}

}  // namespace edv
