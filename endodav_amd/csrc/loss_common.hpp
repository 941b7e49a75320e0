// Pieces shared by the two fused losses (loss.hip: the round-2 photometric subset; loss_trainer.hip: the trainer's whole loss): the camera
// geometry of utils/layers.py:134-189, per-frame sums, the edge-aware smoothness kernel and its per-scale sums, the colour warp of one pixel
// (warp_pixel), the SSIM tile kernel in its plain and its mask-weighted form (ssim_kernel<WEIGHTED>), and on the host the workspace carve-up
// (Carve) and the disparity-to-depth coefficients.  NOT shared: the bilinear tap set-up and the colour gradient through the taps of
// warp_bwd_kernel (loss.hip) and geom_bwd_kernel (loss_trainer.hip).  Behind a __forceinline__ function, in every form tried, the compiler pairs
// and contracts geom_bwd_kernel's arithmetic differently and the trainer's gradients move in the last bit (profiles/loss_shared_notes.txt).
// Everything sits in an anonymous namespace: each translation unit gets its own copy of the kernels.
#pragma once
#include <cmath>

#include "ops.hpp"

namespace edv {
namespace {

constexpr int TS = 32;            // SSIM output tile (TS x TS pixels per workgroup)
constexpr int TI = TS + 4;        // input tile with halo 2
constexpr int TC = TS + 2;        // coefficient tile with halo 1
constexpr int SUM_PARTS = 64;     // partial sums per frame
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

struct Cam {  // per frame and neighbour: P = (K T)[:3, :] (row-major 3x4) and inv_K[:3, :3]
    float P[12];
    float iK[9];
};

// P[f][nb] = (K[f] @ T_nb[f])[:3, :], iK = inv_K[f][:3, :3]  (utils/layers.py:177, :168)
__global__ void cam_kernel(const float *__restrict__ K, const float *__restrict__ invK, const float *__restrict__ Tp, const float *__restrict__ Tn, Cam *cams, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * N) return;
    const int f = i >> 1, nb = i & 1;
    const float *k = K + (long long)f * 16, *t = (nb ? Tn : Tp) + (long long)f * 16, *ik = invK + (long long)f * 16;
    Cam c;
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) {
            float s = 0.f;
            for (int j = 0; j < 4; ++j) s += k[r * 4 + j] * t[j * 4 + col];
            c.P[r * 4 + col] = s;
        }
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 3; ++col) c.iK[r * 3 + col] = ik[r * 4 + col];
    cams[i] = c;
}

// partial[f][b] = sum of x[f][chunk b]; then out[f] = scale * sum_b partial[f][b]
__global__ __launch_bounds__(256) void frame_sum_kernel(const float *__restrict__ x, float *__restrict__ partial, long long P) {
    const int f = blockIdx.y, b = blockIdx.x;
    const long long per = (P + SUM_PARTS - 1) / SUM_PARTS, p0 = b * per, p1 = p0 + per < P ? p0 + per : P;
    float s = 0.f;
    for (long long p = p0 + threadIdx.x; p < p1; p += 256) s += x[(long long)f * P + p];
    block_sum_pairs_store({s}, partial + f * SUM_PARTS + b);
}
__global__ __launch_bounds__(64) void frame_sum_finish_kernel(const float *__restrict__ partial, float *__restrict__ out, float scale) {
    const int f = blockIdx.x;
    const float s = wave_sum(partial[f * SUM_PARTS + threadIdx.x]);
    if (threadIdx.x == 0) out[f] = s * scale;
}

// Edge-aware smoothness of the mean-normalised disparity (utils/layers.py:222-236 on norm = D / (mean + 1e-7), trainer :944-946).
// Thread = pixel p.  Loss terms: pairs (p, p + 1x), (p, p + 1y).  Gradient (a gather): d / d norm_p of the four pairs p is part of.
// part[f][b] = {sum t_x, sum t_y, sum g_p D_p} of the block's pixels; g_p = d (sum t_x / Nx + sum t_y / Ny) / d norm_p.
__global__ __launch_bounds__(256) void smooth_kernel(const float *__restrict__ D, const float *__restrict__ img, const float *__restrict__ mean, float *__restrict__ gsm,
                                                     float *__restrict__ part, int H, int W, float inv_nx, float inv_ny) {
    const int f = blockIdx.y;
    const long long P = (long long)H * W;
    const float *Df = D + (long long)f * P, *im = img + (long long)f * 3 * P;
    const float den = mean[f] + 1e-7f;
    float tx = 0.f, ty = 0.f, gd = 0.f;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const float n0 = Df[p] / den;
        const float c0 = im[p], c1 = im[P + p], c2 = im[2 * P + p];
        float g = 0.f;
        if (x + 1 < W) {
            const float w = expf(-((fabsf(c0 - im[p + 1]) + fabsf(c1 - im[P + p + 1]) + fabsf(c2 - im[2 * P + p + 1])) / 3.0f));
            const float d = n0 - Df[p + 1] / den;
            tx += fabsf(d) * w;
            g += (d > 0.f ? w : (d < 0.f ? -w : 0.f)) * inv_nx;
        }
        if (x > 0) {
            const float w = expf(-((fabsf(im[p - 1] - c0) + fabsf(im[P + p - 1] - c1) + fabsf(im[2 * P + p - 1] - c2)) / 3.0f));
            const float d = Df[p - 1] / den - n0;
            g -= (d > 0.f ? w : (d < 0.f ? -w : 0.f)) * inv_nx;
        }
        if (y + 1 < H) {
            const float w = expf(-((fabsf(c0 - im[p + W]) + fabsf(c1 - im[P + p + W]) + fabsf(c2 - im[2 * P + p + W])) / 3.0f));
            const float d = n0 - Df[p + W] / den;
            ty += fabsf(d) * w;
            g += (d > 0.f ? w : (d < 0.f ? -w : 0.f)) * inv_ny;
        }
        if (y > 0) {
            const float w = expf(-((fabsf(im[p - W] - c0) + fabsf(im[P + p - W] - c1) + fabsf(im[2 * P + p - W] - c2)) / 3.0f));
            const float d = Df[p - W] / den - n0;
            g -= (d > 0.f ? w : (d < 0.f ? -w : 0.f)) * inv_ny;
        }
        gsm[(long long)f * P + p] = g;  // d (t_x / Nx + t_y / Ny) / d norm_p
        gd += g * Df[p];
    }
    block_sum_pairs_store({tx, ty, gd}, part + ((long long)f * gridDim.x + blockIdx.x) * 3);
}

// The per-scale finish kernels' walk over smooth_kernel's partials (one workgroup of 256 threads): this thread's share of sum t_x and sum t_y
// over every frame and block, and S[f] = sum of frame f's g_sm * D partials in block order.
__device__ __forceinline__ void smooth_part_sums(const float *__restrict__ sm_part, int sm_blocks, int N, float *__restrict__ S, float &tx, float &ty) {
    tx = ty = 0.f;
    for (int i = threadIdx.x; i < N * sm_blocks; i += 256) {
        tx += sm_part[(long long)i * 3];
        ty += sm_part[(long long)i * 3 + 1];
    }
    for (int f = threadIdx.x; f < N; f += 256) {
        float s = 0.f;
        for (int b = 0; b < sm_blocks; ++b) s += sm_part[((long long)f * sm_blocks + b) * 3 + 2];
        S[f] = s;
    }
}

// Sampling geometry of pixel (x, y) of frame f towards neighbour nb (utils/layers.py:166-189 + F.grid_sample, border padding, align_corners).
struct Sample {
    float ix, iy;      // clipped source coordinates
    float mx, my;      // 1 where the coordinate was not clipped (d ix / d u), else 0
    float X, Y, Z;     // projected point (before the division)
    float rx, ry, rz;  // P3 . ray: d (X, Y, Z) / d depth
};
__device__ __forceinline__ Sample project_pixel(const Cam &c, float depth, int x, int y, int H, int W) {
    const float fx = (float)x, fy = (float)y;
    const float r0 = c.iK[0] * fx + c.iK[1] * fy + c.iK[2], r1 = c.iK[3] * fx + c.iK[4] * fy + c.iK[5], r2 = c.iK[6] * fx + c.iK[7] * fy + c.iK[8];
    const float c0 = depth * r0, c1 = depth * r1, c2 = depth * r2;
    Sample s;
    s.X = c.P[0] * c0 + c.P[1] * c1 + c.P[2] * c2 + c.P[3];
    s.Y = c.P[4] * c0 + c.P[5] * c1 + c.P[6] * c2 + c.P[7];
    s.Z = c.P[8] * c0 + c.P[9] * c1 + c.P[10] * c2 + c.P[11];
    s.rx = c.P[0] * r0 + c.P[1] * r1 + c.P[2] * r2;
    s.ry = c.P[4] * r0 + c.P[5] * r1 + c.P[6] * r2;
    s.rz = c.P[8] * r0 + c.P[9] * r1 + c.P[10] * r2;
    const float zi = s.Z + 1e-7f;
    float gx = (s.X / zi / (float)(W - 1) - 0.5f) * 2.0f, gy = (s.Y / zi / (float)(H - 1) - 0.5f) * 2.0f;
    float ix = (gx + 1.0f) / 2.0f * (float)(W - 1), iy = (gy + 1.0f) / 2.0f * (float)(H - 1);
    // clip_coordinates_set_grad (GridSampler.cuh): the gradient passes only strictly inside (0, size - 1)
    s.mx = (ix > 0.f && ix < (float)(W - 1)) ? 1.f : 0.f;
    s.my = (iy > 0.f && iy < (float)(H - 1)) ? 1.f : 0.f;
    s.ix = fminf((float)(W - 1), fmaxf(ix, 0.f));
    s.iy = fminf((float)(H - 1), fmaxf(iy, 0.f));
    return s;
}

// out[c * P] = channel c of the image `src` [3, P] sampled where pixel (x, y), of disparity-like value Dv, lands in camera c (trainer :853-857);
// out = the pixel's element of the output's first channel plane
__device__ __forceinline__ void warp_pixel(const Cam &c, float Dv, int x, int y, const float *__restrict__ src, float *__restrict__ out, long long P, int H, int W, float da,
                                           float db) {
    const float depth = 1.0f / (da + db * Dv);
    const Sample s = project_pixel(c, depth, x, y, H, W);
    const float fx0 = floorf(s.ix), fy0 = floorf(s.iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float wx = s.ix - fx0, wy = s.iy - fy0;
    const bool xin = x0 + 1 < W, yin = y0 + 1 < H;
    const float w00 = (1.f - wx) * (1.f - wy), w01 = wx * (1.f - wy), w10 = (1.f - wx) * wy, w11 = wx * wy;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float *sc = src + ch * P + (long long)y0 * W + x0;
        float v = sc[0] * w00;
        if (xin) v += sc[1] * w01;
        if (yin) v += sc[W] * w10;
        if (xin && yin) v += sc[W + 1] * w11;
        out[ch * P] = v;
    }
}

__device__ __forceinline__ int reflect1(int i, int n) {  // nn.ReflectionPad2d(1): -1 -> 1, n -> n - 2
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

// SSIM + L1 of a warped neighbour x against an image y through LDS, with dL/dx (a gather).  One workgroup = (tile, channel, blockIdx.z).
//   plain (loss.hip):            blockIdx.z = (kept frame, neighbour), f from `kept`; x = xw[nb][f], y = img[f]; every pixel weighs w_rep.
//                                part[(z * 3 + ch) * tiles + tile] = sum over the tile of w_ssim * SSIM + w_l1 * |y - x|.
//   WEIGHTED (loss_trainer.hip): blockIdx.z = f; x = xw[f], y = refined[f]; w_q = w_rep m_q / M is the per-pixel weight of the reprojection term and
//                                w_tr m_p / M that of |refined - registration_0|; also dL/dy into gy (may be null).
//                                part[((f * 3 + ch) * tiles + tile) * 2] = {reprojection partial, transform partial}.
// SSIM(q) depends on x AND y through the 3x3 window means mu, E[x^2], E[xy] (reflection-padded): A, B, C = w_q * dSSIM/d(mu_x, E[x^2], E[xy]) at q,
// A2 = w_q dSSIM/d mu_y (B serves E[y^2] too: the expression is symmetric in sigma_x + sigma_y), and
// dL/dx_p = 1/9 sum_{q : p in window(q)} mult(p, q) (A_q + 2 x_p B_q + y_p C_q); mult counts the padded taps of window q that reflect onto p.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ssim_kernel(const float *__restrict__ xw, const float *__restrict__ yimg, const float *__restrict__ reg0, const float *__restrict__ mask,
                                                   const float *__restrict__ msum, float *__restrict__ gx, float *__restrict__ gy, float *__restrict__ part,
                                                   const int *__restrict__ kept, int N, int H, int W, int tiles_x, float w_rep, float w_tr) {
    __shared__ float sx[TI * TI], sy[TI * TI], cA[TC * TC], cA2[WEIGHTED ? TC * TC : 1], cB[TC * TC], cC[TC * TC];
    const long long P = (long long)H * W;
    const int tile = blockIdx.x, ch = blockIdx.y;
    const int f = WEIGHTED ? blockIdx.z : kept[blockIdx.z];  // kept[(z >> 1) * 2 + nb], nb = z & 1
    const long long xplane = (WEIGHTED ? (long long)f : (long long)(blockIdx.z & 1) * N + f) * 3 + ch, yplane = (long long)f * 3 + ch;
    const int ty0 = (tile / tiles_x) * TS, tx0 = (tile % tiles_x) * TS;
    const float *xs = xw + xplane * P, *ys = yimg + yplane * P, *mf = WEIGHTED ? mask + (long long)f * P : nullptr;
    const float inv_m = WEIGHTED ? 1.0f / msum[0] : 1.0f;
    const float w_ssim = w_rep * 0.85f / 3.0f * inv_m, w_l1 = w_rep * 0.15f / 3.0f * inv_m, w_t = w_tr / 3.0f * inv_m;
    for (int i = threadIdx.x; i < TI * TI; i += 256) {
        const int r = i / TI, c = i - r * TI;
        int y = reflect1(ty0 - 2 + r, H), x = reflect1(tx0 - 2 + c, W);
        y = y < 0 ? 0 : (y >= H ? H - 1 : y);  // positions no window of an image pixel reaches (two rows out): any valid address
        x = x < 0 ? 0 : (x >= W ? W - 1 : x);
        sx[i] = xs[(long long)y * W + x];
        sy[i] = ys[(long long)y * W + x];
    }
    __syncthreads();
    float lrep = 0.f, ltr = 0.f;
    for (int i = threadIdx.x; i < TC * TC; i += 256) {
        const int r = i / TC, c = i - r * TC;
        const int qy = ty0 - 1 + r, qx = tx0 - 1 + c;
        float A = 0.f, A2 = 0.f, B = 0.f, C = 0.f;
        if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
            const float wq = WEIGHTED ? w_ssim * mf[(long long)qy * W + qx] : w_ssim;
            float s_x = 0.f, s_y = 0.f, s_xx = 0.f, s_yy = 0.f, s_xy = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float a = sx[(r + dy) * TI + c + dx], b = sy[(r + dy) * TI + c + dx];
                    s_x += a; s_y += b; s_xx += a * a; s_yy += b * b; s_xy += a * b;
                }
            const float mu_x = s_x / 9.0f, mu_y = s_y / 9.0f;
            const float sig_x = s_xx / 9.0f - mu_x * mu_x, sig_y = s_yy / 9.0f - mu_y * mu_y, sig_xy = s_xy / 9.0f - mu_x * mu_y;
            const float n1 = 2.0f * mu_x * mu_y + SSIM_C1, n2 = 2.0f * sig_xy + SSIM_C2;
            const float d1 = mu_x * mu_x + mu_y * mu_y + SSIM_C1, d2 = sig_x + sig_y + SSIM_C2;
            const float n = n1 * n2, d = d1 * d2;
            const float raw = (1.0f - n / d) / 2.0f;
            const bool inner = r >= 1 && r <= TS && c >= 1 && c <= TS;  // q belongs to this tile (not to its halo)
            if (inner) lrep += wq * fminf(1.0f, fmaxf(raw, 0.0f));
            if (raw >= 0.0f && raw <= 1.0f) {  // clamp passes the gradient on [0, 1]
                const float k = -0.5f * wq / (d * d);
                A = k * (2.0f * mu_y * (n2 - n1) * d - n * 2.0f * mu_x * (d2 - d1));
                A2 = k * (2.0f * mu_x * (n2 - n1) * d - n * 2.0f * mu_y * (d2 - d1));
                B = k * (-n * d1);
                C = k * (2.0f * n1 * d);
            }
        }
        cA[i] = A; cB[i] = B; cC[i] = C;
        if (WEIGHTED) cA2[i] = A2;
    }
    __syncthreads();
    float *gox = gx + xplane * P, *goy = WEIGHTED && gy ? gy + yplane * P : nullptr;
    for (int i = threadIdx.x; i < TS * TS; i += 256) {
        const int r = i / TS, c = i - r * TS;
        const int py = ty0 + r, px = tx0 + c;
        if (py >= H || px >= W) continue;
        float SA = 0.f, SA2 = 0.f, SB = 0.f, SC = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const float my = 1.0f + ((dy == 1 && py == H - 2) || (dy == -1 && py == 1) ? 1.0f : 0.0f);
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float m = my * (1.0f + ((dx == 1 && px == W - 2) || (dx == -1 && px == 1) ? 1.0f : 0.0f));
                const int j = (r + 1 + dy) * TC + c + 1 + dx;
                SA += m * cA[j]; SB += m * cB[j]; SC += m * cC[j];
                if (WEIGHTED) SA2 += m * cA2[j];
            }
        }
        const float xv = sx[(r + 2) * TI + c + 2], yv = sy[(r + 2) * TI + c + 2];
        const float mp = WEIGHTED ? mf[(long long)py * W + px] : 1.0f;
        const float diff = yv - xv;
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        lrep += w_l1 * mp * fabsf(diff);
        gox[(long long)py * W + px] = (SA + 2.0f * xv * SB + yv * SC) / 9.0f - w_l1 * mp * sgn;
        if (WEIGHTED) {
            const float dt = yv - reg0[yplane * P + (long long)py * W + px];
            ltr += w_t * mp * fabsf(dt);
            if (goy) goy[(long long)py * W + px] = (SA2 + 2.0f * yv * SB + xv * SC) / 9.0f + w_l1 * mp * sgn + w_t * mp * (dt > 0.f ? 1.f : (dt < 0.f ? -1.f : 0.f));
        }
    }
    const long long slot = ((long long)blockIdx.z * 3 + ch) * gridDim.x + tile;
    if constexpr (WEIGHTED) block_sum_pairs_store({lrep, ltr}, part + slot * 2);
    else block_sum_pairs_store({lrep}, part + slot);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------
struct Carve {  // carve-up of a caller's workspace: a cursor in floats, every piece rounded up to 4 floats (16 bytes)
    size_t o = 0;
    size_t take(size_t n) {
        const size_t at = o;
        o += (n + 3) & ~(size_t)3;
        return at;
    }
};
inline size_t ssim_tiles(int H, int W) { return (size_t)ceil_div(H, TS) * ceil_div(W, TS); }

struct DepthCoef {  // depth = 1 / (da + db D)   (utils/layers.py:16-18 disp_to_depth)
    float da, db;
};
inline DepthCoef depth_coef(float min_depth, float max_depth) {
    return {(float)(1.0 / (double)max_depth), (float)(1.0 / (double)min_depth - 1.0 / (double)max_depth)};
}

}  // namespace
}  // namespace edv
