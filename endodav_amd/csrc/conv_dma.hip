// 3x3 convolution (padding 1, stride 1 or 2, channels-last) as an implicit GEMM with LDS-DMA staging.
//
// Same contract as the LOAD_CONV3 path of gemm.hip (util/blocks.py:20-32,68-91; dpt.py:86-90,117-124), for Cin % 32 == 0:
// then every 32-wide k-tile lies inside ONE tap (dy, dx) and is 128 contiguous bytes of one input pixel, which is exactly
// what a global_load_lds lane group moves.  The im2col gather happens in the per-lane SOURCE address; taps that fall into
// the zero padding read a 256-byte page of zeros instead.  No VGPR round trip, no address arithmetic per element, no
// ds_write: per k-tile a lane issues its DMAs with one 64-bit select each.  The pre-activation ReLU of the
// ResidualConvUnits is applied to the A fragments after the LDS read (4 v_max per 4 MFMAs).
//
// LDS image, swizzle and pipeline are those of gemm_dma.hip (dma_tile.hpp).  Tiles: 64x64 (2x2 waves) or, for Cout <= 32, 128x32 (4x1).
//
// Round 2 (BUF = true, operands within 4 GB): the k loop of gemm_dma.hip -- DMA through buffer descriptors with the tap / channel advance
// in the SCALAR offset, scalar wave index, loop unrolled by two so that the LDS stage is an immediate -- because the f32 MFMA and the
// VALU do not overlap on this part.  A padding tap is a lane whose byte offset is switched to one past the descriptor's range: an
// out-of-range lane of a buffer LDS-DMA writes zeros into LDS (checked on the part, scratch/ubench/README), so no zero page is read.
// What is left per k-tile: one compare + select per A-side DMA (is this lane's tap inside the image?) and, with pre_relu, the v_max of
// the A fragments.
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "dma_tile.hpp"

namespace edv {
namespace {

constexpr int CBK = TILE_BK;
__device__ __attribute__((aligned(256))) float g_zero_page[64];

// SPLIT: the stream-K scheme of streamk_plan.hpp / gemm_common.hpp for grids that do not fill the part (tiles <= resident workgroups, e.g. layer4_rn: 46
// tiles of 108 k-tiles on 256 CUs): the tiles' k-tile units are cut into equal contiguous runs, one per workgroup; a run that does
// not cover a tile's whole k range leaves its accumulators in a workspace slot and the last piece of a tile to arrive merges them in
// run order and applies the epilogue.  SPLIT = false is the plain grid and compiles to the code it was before.
template <int WGM, int EP, bool SPLIT, bool BUF>
__global__ __launch_bounds__(256, 4) void conv3_dma_kernel(const GemmDesc g, const GemmSplit sp) {
    constexpr int WGN = 4 / WGM;
    constexpr int BM = 32 * WGM, BN = 32 * WGN;
    constexpr int IA = BM / 32, IB = BN / 32;  // DMA instructions per wave per k-tile (8 rows x 128 B each)
    constexpr int STAGE = (BM + BN) * CBK;
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const bool prelu = g.pre_relu != 0;
    const int wm = wave / WGN, wn = wave % WGN;
    const int tiles_n = (g.N + BN - 1) / BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    // BUF: descriptors over the input tensor (exactly its bytes: a lane sent past the end reads zeros) and the packed weight
    const unsigned a_bytes = BUF ? (unsigned)((g.M > 0 ? ((g.M - 1) / (g.cOH * g.cOW) + 1) : 0) * (long long)g.cH * g.cW * g.cC * 4) : 0u;
    const auto rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.A), 0, a_bytes, 0x00020000);
    const auto rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.W), 0, 0xffffffff, 0x00020000);
    const int srow = lane >> 3, spos = lane & 7;
    const float *zero = g_zero_page + spos * 4;
    const int opix = g.cOH * g.cOW;
    const int nkt = g.K / CBK;

    // SPLIT: the workgroup's run of the split (these plans have no whole rounds and stride 1: run `bid`); plain: one whole tile
    const int run = split_run(sp, SPLIT, bid);
    long long u = split_run_begin(sp, run);
    const long long u_end = split_run_end(sp, run, u);
    bool once = true;
    for (;;) {
        int tile, kt0, kt1, lt = 0;
        float *part = nullptr;
        if (SPLIT) {
            if (u >= u_end) break;
            lt = (int)(u / nkt);
            kt0 = (int)(u - (long long)lt * nkt);
            const long long left = u_end - u;
            kt1 = kt0 + left < nkt ? kt0 + (int)left : nkt;
            tile = lt;
            if (!(kt0 == 0 && kt1 == nkt)) part = split_slot<SPLIT_SLOT>(sp, run, u);  // a piece: not the tile's whole k range
            u += kt1 - kt0;
        } else {
            if (!once) break;
            once = false;
            tile = bid;
            kt0 = 0;
            kt1 = nkt;
        }
        const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
        const long long m0 = (long long)tm * BM;
        const int n0 = tn * BN;

        // per-lane A rows: output pixel -> pointer to the (dy, dx) = (0, 0) tap of its window, validity bits per dy and dx
        const float *pa[IA];
        unsigned va[IA], vb[IB];  // BUF: byte offsets (A: of the window's centre tap)
        int okmask[IA];  // bits 0..2: row iy0 + dy inside the image; bits 3..5: column ix0 + dx inside
#pragma unroll
        for (int i = 0; i < IA; ++i) {
            const int r = (BM / 4) * wave + 8 * i + srow;
            // (tile_chunk / tile_edge_row of dma_tile.hpp, written out here and below: as calls they change the k loop of four instantiations)
            const int c = spos ^ ((r >> 1) & 7);  // logical 16-byte chunk that lives at this LDS position
            long long m = m0 + r;
            m = m < g.M ? m : g.M - 1;  // rows past the edge read a valid pixel; their results are never stored
            // (BUF: M < 2^30, so the pixel decode is 32-bit arithmetic -- a 64-bit division is ~95 VALU instructions per row)
            const long long f = BUF ? (long long)((unsigned)m / (unsigned)opix) : m / opix;
            const int p = BUF ? (int)((unsigned)m - (unsigned)f * (unsigned)opix) : (int)(m - f * opix);
            const int oy = p / g.cOW, ox = p - oy * g.cOW;
            const int iy0 = oy * g.cS - 1, ix0 = ox * g.cS - 1;
            pa[i] = g.A + ((f * g.cH + iy0) * (long long)g.cW + ix0) * g.cC + c * 4;
            va[i] = (unsigned)((((f * g.cH + iy0 + 1) * (long long)g.cW + ix0 + 1) * g.cC + c * 4) * 4);  // the window's CENTRE tap: always inside
            int mk = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (iy0 + d >= 0 && iy0 + d < g.cH) mk |= 1 << d;
                if (ix0 + d >= 0 && ix0 + d < g.cW) mk |= 8 << d;
            }
            okmask[i] = mk;
        }
        const float *pb[IB];
#pragma unroll
        for (int i = 0; i < IB; ++i) {
            const int r = (BN / 4) * wave + 8 * i + srow;
            const int c = spos ^ ((r >> 1) & 7);
            int n = n0 + r;
            n = n < g.N ? n : g.N - 1;
            pb[i] = g.W + (long long)n * g.ldw + c * 4;
            vb[i] = (unsigned)(((long long)n * g.ldw + c * 4) * 4);
        }
        // tap state of the NEXT k-tile to stage (uniform; advanced by 32 channels per call instead of dividing k by Cin every time)
        int n_c0, n_dy, n_dx;
        {
            const int k = kt0 * CBK, tap = k / g.cC;
            n_c0 = k - tap * g.cC;
            n_dy = tap / 3;
            n_dx = tap - n_dy * 3;
        }
        auto issue = [&](int kt, int st) {
            float *sA = smem + st * STAGE, *sB = sA + BM * CBK;
            const int k = kt * CBK;
            const int dy = n_dy, dx = n_dx, c0 = n_c0;
            n_c0 += CBK;
            if (n_c0 == g.cC) {
                n_c0 = 0;
                if (++n_dx == 3) {
                    n_dx = 0;
                    ++n_dy;
                }
            }
            const long long off = ((long long)dy * g.cW + dx) * g.cC + c0;
            const int need = (1 << dy) | (8 << dx);
#pragma unroll
            for (int i = 0; i < IA; ++i) {
                if constexpr (BUF) {
                    // valid tap: the centre tap's byte offset plus the tap's (signed, uniform) distance from it -- the sum is formed here, in 32
                    // bits, because the descriptor path adds voffset + soffset without wrapping; the channel advance rides in the scalar
                    // operand.  Padding tap: an offset beyond the descriptor -> the lane writes zeros.
                    const int delta = (((dy - 1) * g.cW + (dx - 1)) * g.cC) * 4;
                    const unsigned vo = (okmask[i] & need) == need ? va[i] + (unsigned)delta : 0x80000000u + a_bytes;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void *)(sA + ((BM / 4) * wave_s + 8 * i) * CBK), 16, (unsigned)vo,
                                                             (int)(c0 * 4), 0, 0);
                } else {
                    const float *src = (okmask[i] & need) == need ? pa[i] + off : zero;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                     (__attribute__((address_space(3))) void *)(sA + ((BM / 4) * wave + 8 * i) * CBK), 16, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < IB; ++i) {
                if constexpr (BUF)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (__attribute__((address_space(3))) void *)(sB + ((BN / 4) * wave_s + 8 * i) * CBK), 16, (unsigned)vb[i], (int)(k * 4), 0,
                                                             0);
                else
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(pb[i] + k),
                                                     (__attribute__((address_space(3))) void *)(sB + ((BN / 4) * wave + 8 * i) * CBK), 16, 0, 0);
            }
        };
        const float *fpa[4], *fpb[4];  // fragment read addresses in stage 0
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            fpa[q] = tile_frag_ptr(smem, wm * 32 + l31, q, lh);
            fpb[q] = tile_frag_ptr(smem + BM * CBK, wn * 32 + l31, q, lh);
        }

        EpiCols<1> cols;
        if (EP != 0) cols = gemm_epilogue_prefetch<1>(g, n0, wn * 32, l31);
        float w2v = 0.f, b2v = 0.f;  // EP >= 8 (the fused 1x1, gemm_common.hpp): the lane's column of w2, and b2
        if constexpr (EP >= 8) {
            w2v = g.w2[n0 + l31 < g.N ? n0 + l31 : g.N - 1];
            if (g.b2) b2v = g.b2[0];
        }
        f32x16 acc[1][1];
        auto epilogue = [&]() {
            if constexpr (EP >= 8) {
                static_assert(EP < 8 || (WGM == 4 && BUF && !SPLIT), "the fused 1x1 needs every column of a row in one wave, and 32-bit offsets");
                gemm_epilogue_dot<EP - 8>(g, acc[0][0], cols, w2v, b2v, m0 + wave_s * 32, n0, l31, lh);
            } else if constexpr (BUF && EP >= 1 && EP <= 3)  // addresses in scalar registers, edge rows / columns masked by the descriptor (gemm_common.hpp)
                gemm_epilogue_buf<EP - 1>(g, acc[0][0], cols, m0 + (wave_s / WGN) * 32, n0 + (wave_s % WGN) * 32, l31, lh);
            else
                gemm_epilogue_ep<1, 1, STORE_ROWS, EP>(g, acc, cols, m0, n0, wm * 32, wn * 32, l31, lh);
        };
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;

        // tile_k_loop of dma_tile.hpp, written out (called as the shared function it moves the blocks of conv3_dma_kernel<4, 0, false, true>:
        // profiles/dma_tile_refactor_notes.txt); one uniform prelu branch per k-tile
        issue(kt0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        auto ktile = [&](int kt, auto st_tag) {
            constexpr int ST = decltype(st_tag)::value;
            if (kt + 1 < kt1) issue(kt + 1, ST ^ 1);
            tile_multiply(fpa, ST * STAGE, fpb, ST * STAGE, acc[0][0], prelu);
        };
        {
            int kt = kt0;
            for (; kt + 1 < kt1; kt += 2) {
                ktile(kt, std::integral_constant<int, 0>{});
                ktile(kt + 1, std::integral_constant<int, 1>{});
            }
            if (kt < kt1) ktile(kt, std::integral_constant<int, 0>{});
        }
        if (SPLIT && part) {
            // piece hand-off (gemm_common.hpp); both LDS stages are idle here
            split_store_piece(part, wave, lane, acc[0][0]);
            const long long ub = (long long)lt * nkt;
            int g0, g1;
            const bool last = split_handoff(sp, &sp.cnt[lt], ub, nkt, reinterpret_cast<int *>(smem), tid, g0, g1);
            if (last) {
                acc[0][0] = split_merge_pieces<SPLIT_SLOT>(sp, wave, lane, g0, g1, ub);
                epilogue();
            }
        } else {
            // (its own call site on purpose, see gemm_dma.hip)
            epilogue();
        }
    }
}

template <int WGM, int EP, bool SPLIT>
void launch_variant(const GemmDesc &d, const GemmSplit &sp, bool buf, unsigned grid, hipStream_t st) {
    if (buf) EDV_LAUNCH((conv3_dma_kernel<WGM, EP, SPLIT, true>), dim3(grid), dim3(256), 0, st, d, sp);
    else EDV_LAUNCH((conv3_dma_kernel<WGM, EP, SPLIT, false>), dim3(grid), dim3(256), 0, st, d, sp);
}

// (Build note, hipcc 7.2: in the HOST pass an amdgcn builtin whose integer arguments need an implicit conversion from a captured lvalue makes
// the kernel specialization silently invalid -- "no matching function" at the launch, or an undefined __device_stub__ at load time -- while
// the device pass compiles it.  Hence the explicit (unsigned) / (int) casts on the buffer-load offsets.)
template <int WGM, int EP>
int conv_slots() {
    static DeviceSlotCache cache;
    // at most 4: 32 KB of LDS -- the API says 5, the part places 4 (scratch/ubench/lds_residency.hip)
    return resident_workgroups(cache, (const void *)conv3_dma_kernel<WGM, EP, true, true>, 256, 0, 4, nullptr, nullptr);
}

template <int WGM, int EP>
int launch_conv_ep(const GemmDesc &d, long long tiles, hipStream_t st) {
    static const bool split_on = env_int("EDV_CONV_SPLIT", 1) != 0;  // 0: plain grid always (A/B runs)
    static const bool buf_off = env_int("EDV_CONV_BUF", 1) == 0;     // 0: flat 64-bit DMA source addresses + zero page as in round 1 (A/B runs)
    // 32-bit byte offsets reach every operand (dma_tile.hpp).  OPEN: 64 rows past M is the 64 x 64 tile's figure; the 128 x 32 tile (WGM = 4) runs
    // up to 127 past M and should pass 128.  It differs only for an output within 32 KB of 4 GB (33 M pixels at Cout <= 32).
    const bool buf = !buf_off && conv_inputs_fit(d) && buffer_outputs_fit(d, 64);
    const SplitPolicy &pol = conv_dma_split_policy();
    GemmSplit sp{};
    long long grid;
    plan_plain(tiles, pol, &sp, &grid);
    if (split_on && d.ws && plan_split(tiles, conv_slots<WGM, EP>(), d.K / CBK, pol, &sp, &grid)) {
        split_bind(&sp, d.ws, pol);
        if (split_ws_floats(sp, pol) <= d.ws_floats && (uintptr_t)d.ws % 16 == 0) {
            launch_variant<WGM, EP, true>(d, sp, buf, (unsigned)grid, st);
            EDV_LAUNCH_OK();
            return 0;
        }
        grid = tiles;  // a workspace too small for this plan: the plain grid (which does not read sp)
    }
    launch_variant<WGM, EP, false>(d, sp, buf, (unsigned)grid, st);
    EDV_LAUNCH_OK();
    return 0;
}

template <int WGM>
int launch_conv(const GemmDesc &d, hipStream_t st) {
    constexpr int BM = 32 * WGM, BN = 32 * (4 / WGM);
    const long long tiles = ((d.M + BM - 1) / BM) * (long long)((d.N + BN - 1) / BN);
    EDV_CHECK(tiles > 0 && tiles < (1ll << 31), "bad grid");
    switch (epilogue_kind(d)) {
        case 1: return launch_conv_ep<WGM, 1>(d, tiles, st);
        case 3: return launch_conv_ep<WGM, 3>(d, tiles, st);
        default: return launch_conv_ep<WGM, 0>(d, tiles, st);
    }
}

// process-wide implementation switch (edv_set_conv_impl)
std::atomic<int> g_conv_impl{0};

// the operand limits of BUF = true (launch_conv_ep) for a launch without C / R1 / R2, plus the one-float-per-row output
bool dot_fits_buffer(const GemmDesc &d) {
    return conv_inputs_fit(d) && (d.M + 128) * 4 < (1ll << 32) - (1 << 20);
}

template <int EP>
int launch_conv_dot(const GemmDesc &d, hipStream_t st) {
    const long long tiles = (d.M + 127) / 128;
    EDV_CHECK(tiles > 0 && tiles < (1ll << 31), "bad grid");
    GemmSplit sp{};
    long long grid;
    plan_plain(tiles, conv_dma_split_policy(), &sp, &grid);
    EDV_LAUNCH((conv3_dma_kernel<4, EP, false, true>), dim3((unsigned)grid), dim3(256), 0, st, d, sp);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace

void set_conv_impl(int mode) { g_conv_impl.store(mode < 0 || mode > 2 ? 0 : mode, std::memory_order_relaxed); }
int conv_impl() { return g_conv_impl.load(std::memory_order_relaxed); }
bool conv_dot_enabled() {
    // EDV_CONV_DOT=0: never fuse the 1x1 into the convolution (A/B runs).  Read at every call -- a few per forward -- and not cached like the other
    // flags: tests/test_conv_halo_gpu.py switches it inside one process to compare the halo kernel alone with the parent's path bit for bit.
    return conv_impl() != 1 && env_int("EDV_CONV_DOT", 1) != 0;
}

// Which launches split: grids that do not fill the part and whose tiles are deep (Cin >= 192: 54+ k-tiles), or that leave most of it idle (8 tiles
// per resident slot).  Measured (scratch/kb_conv_split.py, plain / split us): layer4_rn 46 tiles x 108 k-tiles 91 / 31, resize_layers.3
// 276 x 108: 144 / 89, layer3_rn 172 x 54: 48 / 38, RCU at 19x19 46 x 18: 18.9 / 14.2 -- but RCU at 37x37 172 x 18: 19.3 / 24.9 and at
// 74x74 685 x 18: 39.8 / 46.4, so shallow tiles on a half-full grid stay plain.
const SplitPolicy &conv_dma_split_policy() {
    static const SplitPolicy p{.min_kt = 18, .min_tiles = 16, .max_rounds = 0, .widen = false, .counters = SPLIT_MAX_COUNTERS, .slot_floats = SPLIT_SLOT,
                               .whole_rounds = false, .deep_kt = 48, .idle_factor = 8};
    return p;
}

bool conv_dma_supported(const GemmDesc &d) {
    return d.loader == LOAD_CONV3 && d.store == STORE_ROWS && d.cC % CBK == 0 && d.K == 9 * d.cC && d.ldw % 4 == 0 && d.M > 0 && d.N > 0;
}

bool conv_dot_supported(const GemmDesc &d) {
    return conv_dma_supported(d) && d.N <= 32 && (d.act == ACT_NONE || d.act == ACT_RELU) && d.act2 != ACT_GELU && d.act2 >= ACT_NONE && d.act2 <= ACT_SIGMOID_NEG &&
           !d.gamma && !d.R1 && !d.R2 && !d.P1 && d.c_map.period == 0 && dot_fits_buffer(d);
}

// The convolution with the 1x1 to one channel in its epilogue: the plain grid of conv3_dma_kernel<4, ...> (every launch this serves fills the part).
int conv_dot(const GemmDesc &d, hipStream_t st) {
    EDV_CHECK(d.A && d.W && d.w2 && d.dot_out, "null operand");
    EDV_CHECK(conv_dot_supported(d), "fused 1x1 epilogue: Cin % 32 == 0, Cout <= 32, post-activation none / ReLU, no residual, operands below 2 GB");
    EDV_CHECK(((uintptr_t)d.A % 16 == 0) && ((uintptr_t)d.W % 16 == 0), "A/W must be 16-byte aligned");
    if (conv_halo_wanted(d)) return conv_halo(d, st);
    return d.act == ACT_RELU ? launch_conv_dot<8 + ACT_RELU>(d, st) : launch_conv_dot<8 + ACT_NONE>(d, st);
}

int conv_dma(const GemmDesc &d, hipStream_t st) {
    EDV_CHECK(d.A && d.W && d.C, "null operand");
    EDV_CHECK(conv_dma_supported(d), "LDS-DMA convolution needs Cin % 32 == 0");
    EDV_CHECK(((uintptr_t)d.A % 16 == 0) && ((uintptr_t)d.W % 16 == 0), "A/W must be 16-byte aligned");
    if (conv_halo_wanted(d)) return conv_halo(d, st);
    return d.N <= 32 ? launch_conv<4>(d, st) : launch_conv<2>(d, st);
}

}  // namespace edv
