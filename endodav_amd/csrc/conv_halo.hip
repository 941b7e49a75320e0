// 3x3 convolution (padding 1, stride 1, channels-last) on a 2-D output patch whose input halo is staged into LDS ONCE.
//
// Second implementation of the LOAD_CONV3 contract of conv_dma.hip, for Cout <= 32 and Cin = 32 or 64: same packed weight [Cout][3][3][Cin], same
// epilogues (bias, compile-time none / ReLU, gamma, R1 / R2, pre_relu on the A fragments; the fused 1x1 of gemm_common.hpp), and the SAME BITS: the
// k order (tap, then 32-channel block), the fragment-to-k mapping (chunk 2q + lh, element e -> mfma_f32_32x32x2f32, the (q, e) order of
// dma_tile.hpp's tile_multiply), the zero start of the accumulators and the epilogue arithmetic are conv3_dma_kernel's, so
// tests/test_conv_halo_gpu.py compares with torch.equal.
//
// What differs is the A side.  conv3_dma_kernel is an im2col GEMM over 128 consecutive rows of M: per k-tile it fetches the rows' 128-byte runs again,
// so every input pixel crosses the LDS-DMA path nine times (147 KB per 128x32 tile at Cin = 32, next to 36 KB of weights).  Here a workgroup owns an
// 8 x 16 patch of output pixels of ONE frame (4 waves x 32 pixels: wave w has image rows 2w and 2w + 1 of the patch, lane l31 = 16 * row + column), and
// its 10 x 18 input pixels go to LDS once (23 KB of payload); the k loop reads every tap's A fragments from that patch at per-lane base + an
// IMMEDIATE offset, and streams only W per k-tile, double-buffered, as conv3_dma_kernel does.
//
// LDS patch, per 32-channel block: [10 halo rows][192 chunks of 16 B]; a pixel is 9 chunks (8 of data + 1 of padding: stride 144 B), a row 18 x 9 = 162
// chunks rounded up to three LDS-DMA instructions of 64 lanes.  With a 144-byte pixel stride 16 pixels of an image row start 36 banks apart -- 9 p mod
// 16 is a bijection -- so they cover all 64 banks whatever the tap, and a halo row is a multiple of 256 B, so the wave's second image row falls on the
// first one's banks: each 16-lane group a ds_read_b128 is serviced in ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...) holds 16 distinct columns.
// Conflict-free without a swizzle, hence without any per-tap address arithmetic.  The row's three DMA instructions have compile-time lane patterns (lane -> halo column, chunk), computed once per
// tile; the halo row (frame, image row, in or outside the image) is wave-uniform and rides in the SCALAR offset.  Halo pixels outside the image --
// rows above 0 or below H - 1 included, which in memory are the neighbouring frame's -- and the padding chunks are lanes whose offset is sent past the
// descriptor: an out-of-range lane of a buffer LDS-DMA writes zeros (profiles/r03_notes.txt, "LDS-DMA out-of-range lanes"), so every byte the k loop
// reads was written by this tile.
//
// One tile per workgroup, everything drained (vmcnt(0), lgkmcnt(0)) at every barrier; overlap comes from the 4 (Cin = 32: 38 KB of LDS) or 2
// (Cin = 64: 68 KB) workgroups a CU holds.
#include <cstdlib>
#include <type_traits>

#include "dma_tile.hpp"

namespace edv {
namespace {

constexpr int HBK = TILE_BK;               // k-tile: one 32-channel block of one tap
constexpr int TH = 8, TW = 16;             // output patch
constexpr int ROW_BYTES = 3 * 64 * 16;     // one halo row of one channel block in LDS: three DMA instructions
constexpr int PIX_BYTES = 9 * 16;          // pixel stride inside a row
constexpr int PLANE_BYTES = (TH + 2) * ROW_BYTES;
constexpr int WSTAGE = 32 * HBK;           // floats of one W stage (32 output channels x 32 k)
constexpr unsigned LANE_OUT = 0x80000000u;  // per-lane offset of a lane that must not touch memory
constexpr unsigned ROW_OUT = 0x7ff00000u;   // scalar offset of a row that must not: beyond every descriptor here (< 2^31 - 2^20 bytes), and
                                            // LANE_OUT + ROW_OUT stays below 2^32

// NCB = Cin / 32.  ACT: ACT_NONE / ACT_RELU behind the bias.  DOT: the fused 1x1 (GemmDesc::w2) instead of the stored tile.
template <int NCB, int ACT, bool DOT>
__global__ __launch_bounds__(256, NCB == 1 ? 4 : 2) void conv3_halo_kernel(const GemmDesc g) {
    __shared__ __attribute__((aligned(16))) float smem[2 * WSTAGE + NCB * PLANE_BYTES / 4];
    constexpr int CIN = NCB * 32, NKT = 9 * NCB;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool prelu = g.pre_relu != 0;
    const int H = g.cH, W = g.cW;
    // tile decode, scalar, once: frame, patch row, patch column
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int f = bid / (tiles_x * tiles_y), tr = bid - f * (tiles_x * tiles_y);
    const int ty = tr / tiles_x, tx = tr - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int frames = (int)(g.M / ((long long)H * W));
    const unsigned a_bytes = (unsigned)((long long)frames * H * W * CIN * 4);
    const auto rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.A), 0, a_bytes, 0x00020000);
    const auto rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.W), 0, 0xffffffff, 0x00020000);
    float *const sW = smem;
    char *const patch = reinterpret_cast<char *>(smem + 2 * WSTAGE);

    // ---- the halo patch: wave w stages the (channel block, halo row) units w, w + 4, ..., three DMA instructions each ----
    unsigned pat[3];  // lane pattern of a row's k-th instruction: byte offset of (halo column, chunk) inside an image row, or LANE_OUT
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned ci = (unsigned)(k * 64 + lane);
        const unsigned hx = ci / 9u, c = ci - 9u * hx;
        const int ix = ox0 - 1 + (int)hx;
        pat[k] = (hx < (unsigned)(TW + 2) && c < 8u && ix >= 0 && ix < W) ? (unsigned)((ix * CIN + (int)c * 4) * 4) : LANE_OUT;
    }
#pragma unroll
    for (int t = 0; t < ((TH + 2) * NCB + 3) / 4; ++t) {
        const int u = wave_s + 4 * t;
        if (u < (TH + 2) * NCB) {
            const int cb = NCB == 1 ? 0 : u / (TH + 2), hy = u - cb * (TH + 2);
            const int iy = oy0 - 1 + hy;
            const unsigned so = (iy >= 0 && iy < H) ? (unsigned)((((f * H + iy) * W) * CIN + cb * 32) * 4) : ROW_OUT;
            char *dst = patch + cb * PLANE_BYTES + hy * ROW_BYTES;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void *)(dst + k * 1024), 16, (unsigned)pat[k], (int)so, 0, 0);
        }
    }
    // ---- W: k-tile kt = (tap, channel block) is columns 32 kt .. of the packed weight; LDS image and swizzle of conv3_dma_kernel (dma_tile.hpp) ----
    const int srow = lane >> 3, spos = lane & 7;
    unsigned vb;
    {
        const int r = 8 * wave_s + srow;
        const int c = tile_chunk(r, spos);
        const int n = tile_edge_row(r, g.N);
        vb = (unsigned)((n * g.ldw + c * 4) * 4);
    }
    auto issue_w = [&](int kt, int stg) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (__attribute__((address_space(3))) void *)(sW + stg * WSTAGE + 8 * wave_s * HBK), 16, (unsigned)vb, (int)(kt * HBK * 4),
                                                 0, 0);
    };
    const float *fpb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) fpb[q] = tile_frag_ptr(sW, l31, q, lh);
    // the lane's output pixel (patch row 2 w + l31 / 16, column l31 % 16): address of its window's top-left halo pixel, chunk lh
    const char *const a0 = patch + (2 * wave_s) * ROW_BYTES + (l31 >> 4) * ROW_BYTES + (l31 & 15) * PIX_BYTES + lh * 16;

    EpiCols<1> cols = gemm_epilogue_prefetch<1>(g, 0, 0, l31);
    float w2v = 0.f, b2v = 0.f;
    if constexpr (DOT) {
        w2v = g.w2[l31 < g.N ? l31 : g.N - 1];
        if (g.b2) b2v = g.b2[0];
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    issue_w(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        const int stg = kt & 1, tap = kt / NCB, cb = kt - tap * NCB, dy = tap / 3, dx = tap - 3 * dy;
        if (kt + 1 < NKT) issue_w(kt + 1, stg ^ 1);
        // tile_multiply of dma_tile.hpp (reads, fence, pre-ReLU, 16 MFMAs, fence, waits, barrier: explained there) with the A fragments from the
        // patch, written out: called as the shared function, the last k-tile schedules differently and the stored epilogue of Cin = 32 gains 16
        // v_mov (profiles/dma_tile_refactor_notes.txt)
        f32x4 fa[4], fb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            fa[q] = *reinterpret_cast<const f32x4 *>(a0 + cb * PLANE_BYTES + dy * ROW_BYTES + dx * PIX_BYTES + q * 32);
            fb[q] = *reinterpret_cast<const f32x4 *>(fpb[q] + stg * WSTAGE);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (prelu) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) fa[q][e] = __builtin_amdgcn_fmed3f(fa[q][e], 0.f, __builtin_inff());
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][e], fb[q][e], acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // ---- epilogue: register r of lane half lh is patch pixel (2 w + r / 8, (r & 3) + 8 * ((r >> 2) & 1) + 4 lh), channel l31 ----
    const int oyw = oy0 + 2 * wave_s;
    const unsigned mbase = (unsigned)((f * H + oyw) * W + ox0);  // row of M of the wave's first pixel
    if constexpr (DOT) {
        const float v = gemm_dot_reduce<ACT>(g, acc, cols, w2v, b2v, l31 < g.N, l31);
        const int i = l31 & 15, r = 2 * i + (l31 >> 4);  // the lane's sum is register r's row (gemm_dot_reduce)
        const int py = r >> 3, px = (r & 3) + 8 * ((r >> 2) & 1) + 4 * lh;
        const bool ok = i < 8 && oyw + py < H && ox0 + px < W;
        const auto ro = __builtin_amdgcn_make_buffer_rsrc(g.dot_out, 0, (int)(unsigned)(g.M * 4), 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, (int)(ok ? (unsigned)((py * W + px) * 4) : LANE_OUT), (int)(mbase * 4u), EDV_EPI_STORE_AUX);
    } else {
        // gemm_epilogue_buf's arithmetic -- (acc + bias), activation, * gamma + (R1 + R2) -- with the patch's row offsets: the part of a pixel's
        // offset that depends on r is uniform and rides in the scalar operand, a pixel right of the image is a per-lane offset switched out
        // (eight distinct columns), a row below it a scalar offset switched out.
        using f32x2 = __attribute__((ext_vector_type(2))) float;
        const int ld = g.ldc;
        const unsigned lane_off = l31 >= g.N ? LANE_OUT : (unsigned)((4 * lh * ld + l31) * 4);
        const int lim = W - ox0 - 4 * lh;  // register column xb is inside the image iff xb < lim
        unsigned vo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vo[j] = ((j & 3) + 8 * (j >> 2)) < lim ? lane_off : LANE_OUT;
        unsigned so[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            so[r] = oyw + (r >> 3) < H ? (mbase + (unsigned)((r >> 3) * W + (r & 3) + 8 * ((r >> 2) & 1))) * (unsigned)(ld * 4) : ROW_OUT;
        f32x2 res[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) res[i] = f32x2{0.f, 0.f};
        const int bytes = (int)(unsigned)(g.M * ld * 4);
        if (g.R1) {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.R1), 0, bytes, 0x00020000);
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r >> 1][r & 1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo[(r & 3) + 4 * ((r >> 2) & 1)], (int)so[r], 0));
        }
        if (g.R2) {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.R2), 0, bytes, 0x00020000);
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r >> 1][r & 1] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo[(r & 3) + 4 * ((r >> 2) & 1)], (int)so[r], 0));
        }
        const auto rc = __builtin_amdgcn_make_buffer_rsrc(g.C, 0, bytes, 0x00020000);
        const f32x2 bias = {cols.bias[0], cols.bias[0]}, gam = {cols.gam[0], cols.gam[0]};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x2 v = f32x2{acc[2 * i], acc[2 * i + 1]} + bias;
            if (ACT == ACT_RELU) v = f32x2{fmaxf(v[0], 0.0f), fmaxf(v[1], 0.0f)};
            v = v * gam + res[i];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int r = 2 * i + e;
                const float ve = e ? v[1] : v[0];
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ve), rc, (int)vo[(r & 3) + 4 * ((r >> 2) & 1)], (int)so[r], EDV_EPI_STORE_AUX);
            }
        }
    }
}

template <int NCB, int ACT>
int launch_halo(const GemmDesc &d, unsigned grid, hipStream_t st) {
    if (d.w2) EDV_LAUNCH((conv3_halo_kernel<NCB, ACT, true>), dim3(grid), dim3(256), 0, st, d);
    else EDV_LAUNCH((conv3_halo_kernel<NCB, ACT, false>), dim3(grid), dim3(256), 0, st, d);
    EDV_LAUNCH_OK();
    return 0;
}

long long halo_tiles(const GemmDesc &d) { return (d.M / ((long long)d.cH * d.cW)) * ((d.cH + TH - 1) / TH) * (long long)((d.cW + TW - 1) / TW); }

}  // namespace

// What the kernel covers; everything else stays with conv3_dma_kernel.  (d.w2 set: conv_dot_supported() is the caller's gate as well.)
bool conv_halo_supported(const GemmDesc &d) {
    if (!conv_dma_supported(d) || d.cS != 1 || d.N > 32 || (d.cC != 32 && d.cC != 64)) return false;
    if (d.M % ((long long)d.cH * d.cW) != 0 || halo_tiles(d) >= (1ll << 31)) return false;
    const long long lim = (1ll << 31) - (1 << 20);  // every operand below LANE_OUT / ROW_OUT
    if (d.M * d.cC * 4 >= lim || (long long)d.N * d.ldw * 4 >= lim) return false;
    if (d.w2) return d.M * 4 < lim;
    const int ep = epilogue_kind(d);
    if (ep != 1 + ACT_NONE && ep != 1 + ACT_RELU) return false;
    if ((d.R1 && d.ldr1 != d.ldc) || (d.R2 && d.ldr2 != d.ldc)) return false;
    return d.M * d.ldc * 4 < lim;
}

// The dispatch rule of automatic mode: a shape class goes to the halo kernel only where it measured faster than conv3_dma_kernel on the part
// (profiles/conv_halo_notes.txt; us per launch, conv3_dma_kernel / conv3_halo_kernel, T = 8 at the headline shapes).
//   Cin 32, Cout <= 32   output_conv2.0, 32 -> 32 at 8 x 518 x 518 (17 160 patches):  366.8 / 333.3 stored, 346.9 / 307.5 with the fused 1x1
//                        (conv3_dma_kernel + dot_channels_kernel, what the fused launch replaces: 366.8 + 51.0)
//   Cin 64, Cout <= 32   output_conv1, 64 -> 32 at 8 x 296 x 296 (5 624 patches):      235.9 / 209.2
//                        ViT-B output_conv2.0, 64 -> 32 at 16 x 518 x 518 (HIP events):   1303 / 1273 stored, 1295 / 1241 fused (+ dot_channels: 1408)
// Both were measured on grids of many rounds of the part; the kernel has no stream-K split, so a grid below 4096 patches (two rounds at four
// workgroups per CU: not measured) stays with conv3_dma_kernel.  Cout = 64 has no halo kernel yet.
bool conv_halo_pays(const GemmDesc &d) { return (d.cC == 32 || d.cC == 64) && d.N <= 32 && halo_tiles(d) >= 4096; }

bool conv_halo_wanted(const GemmDesc &d) {
    // EDV_CONV_HALO=0: never the halo kernel (A/B runs); read at every call like EDV_CONV_DOT (conv_dma.hip), so that a test reaches both kernels
    if (conv_impl() == 1 || !conv_halo_supported(d) || env_int("EDV_CONV_HALO", 1) == 0) return false;
    return conv_impl() == 2 || conv_halo_pays(d);
}

int conv_halo(const GemmDesc &d, hipStream_t st) {
    EDV_CHECK(d.A && d.W && (d.w2 ? (const void *)d.dot_out : (const void *)d.C), "null operand");
    EDV_CHECK(conv_halo_supported(d), "halo convolution: stride 1, Cin 32 or 64, Cout <= 32, operands below 2 GB");
    EDV_CHECK(((uintptr_t)d.A % 16 == 0) && ((uintptr_t)d.W % 16 == 0), "A/W must be 16-byte aligned");
    const unsigned grid = (unsigned)halo_tiles(d);
    const bool relu = d.act == ACT_RELU;
    if (d.cC == 32) return relu ? launch_halo<1, ACT_RELU>(d, grid, st) : launch_halo<1, ACT_NONE>(d, grid, st);
    return relu ? launch_halo<2, ACT_RELU>(d, grid, st) : launch_halo<2, ACT_NONE>(d, grid, st);
}

}  // namespace edv
