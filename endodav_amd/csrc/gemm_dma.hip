// fp32-MFMA GEMM with LDS-DMA staging (global_load_lds, 16 bytes per lane): dense A only, K % 32 == 0.
//
// Same contract and epilogues as gemm.hip.  What changes is how the 64x64x32 tiles reach LDS: each wave issues
// four DMA instructions per k-tile (8 rows x 128 B each) that write LDS directly — no VGPR round trip, no ds_write,
// 48 instead of 100 registers per lane and 32 KB of LDS for two stages (which places 4 workgroups per CU: the LDS allocation
// granule is 1280 B, so five 32 KB blocks do not fit 160 KB -- scratch/ubench/lds_residency.hip).
// The ablation in scratch/ubench/gemm_ablate.hip priced exactly these staging instructions at ~20 % of the loop.
//
// LDS image (unpadded, swizzled 128-byte rows), the multiply of one k-tile and the two-stage pipeline -- tile k+1 in flight while tile k is
// multiplied, each wave waiting for its own DMAs before the raw s_barrier that publishes the stage -- are dma_tile.hpp's, shared with conv_dma.hip.
//
// Measured (profiles/r01_gemm_tile_sweep.txt), with the full epilogue: T=8 qkv 120 -> 111 us, fc2 162 -> 152 us,
// T=32 qkv 363 -> 340 us (114 TF/s); end to end +2..3 % on ViT-S/B/L.  On bare 8192x8192x1024 the DMA fill rate per CU
// caps it near 100 TF/s (register staging: 117), a regime the model does not reach with its K <= 4096, N <= 4096.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "dma_tile.hpp"

// Timeline hook for scratch/ubench/gemm_trace.hip; expands to nothing in the product build.
#ifndef EDV_GEMM_STAMP
#define EDV_GEMM_STAMP(slot)
#endif

namespace edv {
namespace {

constexpr int DBK = TILE_BK, DBM = 64, DBN = 64;
constexpr int DSTAGE = (DBM + DBN) * DBK;  // floats per stage (16 KB)

// Work split: the persistent grid with a stream-K tail of streamk_plan.hpp (scheme and host planner; the device side is in gemm_common.hpp).
// Here 3 workgroups per CU: the split instantiation holds ~116 VGPRs, and a grid beyond the real residency loses everything the split gains.
//
// Why it matters (profiles/r01_gemm_tile_sweep.txt, warm clocks): a CU retires tiles at a fixed MFMA-bound rate, so a grid of
// 1032 tiles on 256 CUs (N = 384 at 8 x 1370 rows) takes as long as 1280 tiles: fc2 138 us vs 112 us at 1020 tiles; with the split
// 121 us.  It pays for deep tiles (K >= 768) and for small grids; 12-k-tile tiles lose more to the static assignment than they gain.
constexpr int SLOT = SPLIT_SLOT;
constexpr int MAX_COUNTERS = SPLIT_MAX_COUNTERS;

// SPLIT = false is the plain grid (one whole tile per workgroup): the split bookkeeping and the merge compile away, which
// keeps the hot instantiation at 48 VGPRs and its code in the instruction cache (with the merge inlined the same launches ran
// 2 % slower end to end).
//
// The k loop carries NO vector-ALU instruction (round 2).  On this part the f32 MFMA and the VALU do not overlap: v_mfma_f32_32x32x2_f32 runs at
// exactly the f32 vector rate, and every VALU instruction a wave issues between its MFMAs takes its 4-8 cycles out of the matrix pipe's time, for
// all waves of the SIMD (scratch/ubench/mfma_feed.hip: 160 VALU instructions per 128 MFMAs cost 19 % whether issued as a burst or interleaved;
// LDS reads, barriers and accumulator-to-operand forwarding cost nothing).  The round-1 loop spent ~23 VALU instructions per 16 MFMAs on
// addresses: 64-bit adds for the four DMA sources, a v_readfirstlane per DMA for M0 (the wave index is "divergent" to the compiler), an add
// per fragment read for the stage toggle.  Now: the DMA goes through buffer descriptors (per-lane 32-bit byte offset computed once per tile, the
// k advance in the SCALAR offset), the wave index is made scalar once, and the loop is unrolled by two so that the LDS stage is a
// compile-time immediate of ds_read_b128.  BUF = false keeps the flat-address form for operands beyond 4 GB.
// BUF: 0 = flat 64-bit DMA source addresses, 1 = buffer descriptors, 2 = buffer descriptors and identity A rows (a_map.period == 0: the row map's
// 64-bit division is not even compiled in; most launches).  __launch_bounds__(256, 4): four workgroups per CU is what LDS allows anyway, and with the
// 128-register budget spelled out the compiler keeps the accumulators in architectural VGPRs (no v_accvgpr_write / _read, which are VALU instructions).
template <int STORE, int EP, bool SPLIT, int BUF>
__global__ __launch_bounds__(256, 4) void gemm_dma_kernel(const GemmDesc g, const GemmSplit sp) {
    __shared__ __attribute__((aligned(16))) float smem[2 * DSTAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);  // the same number, provably wave-uniform: M0 and LDS bases become scalar arithmetic
    const auto rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.A), 0, 0xffffffff, 0x00020000);
    const auto rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.W), 0, 0xffffffff, 0x00020000);
    EDV_GEMM_STAMP(0);
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (g.N + DBN - 1) / DBN;
    const int G = gridDim.x;
    const int bid = xcd_remap(blockIdx.x, G);
    const int nkt = g.K / DBK;
    const int srow = lane >> 3, spos = lane & 7;

    const int tile_l0 = sp.whole_rounds * G;
    const int run = split_run(sp, SPLIT, bid);
    long long u = split_run_begin(sp, run);
    const long long u_end = split_run_end(sp, run, u);
    int round = 0;
    for (;;) {
        int tile, kt0, kt1, lt = 0;
        float *part = nullptr;
        if (round < sp.whole_rounds) {
            tile = round * G + bid;
            kt0 = 0;
            kt1 = nkt;
            ++round;
        } else if (SPLIT && u < u_end) {
            const int t = (int)(u / nkt);
            kt0 = (int)(u - (long long)t * nkt);
            const long long left = u_end - u;
            kt1 = kt0 + left < nkt ? kt0 + (int)left : nkt;
            tile = tile_l0 + t;
            lt = t;
            if (!(kt0 == 0 && kt1 == nkt)) part = split_slot<SLOT>(sp, run, u);  // a piece: not the tile's whole k range
            u += kt1 - kt0;
        } else {
            break;
        }
        const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
        const long long m0 = (long long)tm * DBM;
        const int n0 = tn * DBN;

        // staging: wave w owns rows [16w, 16w+16) of the A tile and of the W tile; one DMA instruction = 8 rows x 128 B
        const float *ga[2], *gb[2];
        unsigned va[2], vb[2];  // BUF: byte offsets of this lane's 16 bytes in k-tile 0
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = 16 * wave + 8 * i + srow;   // row within the tile
            const int c = tile_chunk(r, spos);
            const long long m = tile_edge_row<long long>(m0 + r, g.M);
            const int n = tile_edge_row(n0 + r, g.N);
            const long long am = BUF == 2 ? m : g.a_map(m);
            ga[i] = g.A + am * g.lda + c * 4;
            gb[i] = g.W + (long long)n * g.ldw + c * 4;
            va[i] = (unsigned)((am * g.lda + c * 4) * 4);
            vb[i] = (unsigned)(((long long)n * g.ldw + c * 4) * 4);
        }
        auto issue = [&](int kt, int st) {
            float *sA = smem + st * DSTAGE, *sB = sA + DBM * DBK;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if constexpr (BUF) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void *)(sA + (16 * wave_s + 8 * i) * DBK), 16, (unsigned)va[i],
                                                             (int)(kt * (DBK * 4)), 0, 0);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (__attribute__((address_space(3))) void *)(sB + (16 * wave_s + 8 * i) * DBK), 16, (unsigned)vb[i],
                                                             (int)(kt * (DBK * 4)), 0, 0);
                } else {
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(ga[i] + kt * DBK),
                                                     (__attribute__((address_space(3))) void *)(sA + (16 * wave + 8 * i) * DBK), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gb[i] + kt * DBK),
                                                     (__attribute__((address_space(3))) void *)(sB + (16 * wave + 8 * i) * DBK), 16, 0, 0);
                }
            }
        };
        const float *pa[4], *pb[4];  // fragment read addresses in stage 0
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            pa[q] = tile_frag_ptr(smem, wm * 32 + l31, q, lh);
            pb[q] = tile_frag_ptr(smem + DBM * DBK, wn * 32 + l31, q, lh);
        }

        EpiCols<1> cols;
        if (EP != 0) cols = gemm_epilogue_prefetch<1>(g, n0, wn * 32, l31);
        f32x16 acc[1][1];
        auto epilogue = [&](long long em0, int en0) {
            if constexpr (EP == 6) {
                // GEGLU: the wave pair (wm, 0) / (wm, 1) holds values / gates of the same 32 output columns.  The gate wave leaves gelu(gate) in LDS
                // (both stages are idle here), the value wave multiplies and stores 32 columns of the half-width output through a buffer descriptor.
                float *ex = smem + (wave_s >> 1) * (16 * 64);
                if (wave_s & 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) ex[r * 64 + lane] = gelu_erf(acc[0][0][r] + cols.bias[0]);
                }
                __syncthreads();
                if (!(wave_s & 1)) {
                    const auto rc = __builtin_amdgcn_make_buffer_rsrc(g.C, 0, (int)(unsigned)(g.M * g.ldc * 4), 0x00020000);
                    const unsigned vo = (unsigned)((4 * lh * g.ldc + l31) * 4);
                    const unsigned so = (unsigned)(((em0 + (wave_s >> 1) * 32) * g.ldc + (en0 >> 1)) * 4);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = (acc[0][0][r] + cols.bias[0]) * ex[r * 64 + lane];
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, (int)vo, (int)(so + (unsigned)(((r & 3) + 8 * (r >> 2)) * g.ldc * 4)), 0);
                    }
                }
                __syncthreads();  // (a persistent instantiation would refill the stages next)
            } else if constexpr (BUF && STORE == STORE_ROWS && EP >= 1 && EP <= 3)
                gemm_epilogue_buf<EP - 1>(g, acc[0][0], cols, em0 + (wave_s >> 1) * 32, en0 + (wave_s & 1) * 32, l31, lh);
            else
                gemm_epilogue_ep<1, 1, STORE, EP>(g, acc, cols, em0, en0, wm * 32, wn * 32, l31, lh);
        };
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;

        tile_k_loop<DSTAGE>(kt0, kt1, issue, pa, pb, acc[0][0], false, [](int slot) { EDV_GEMM_STAMP(slot); });
        EDV_GEMM_STAMP(3);
        if (SPLIT && part) {
            // piece hand-off (gemm_common.hpp: sc1 stores, every wave's vmcnt(0), barrier, one agent-scope counter add; the last arriver acquires
            // and then reads every piece with sc1 loads in run order); both LDS stages are idle between the k loop and the next tile's first DMA
            split_store_piece(part, wave, lane, acc[0][0]);
            const long long ub = (long long)lt * nkt;
            int g0, g1;
            const bool last = split_handoff(sp, &sp.cnt[lt], ub, nkt, reinterpret_cast<int *>(smem), tid, g0, g1);
            if (last) {
                acc[0][0] = split_merge_pieces<SLOT>(sp, wave, lane, g0, g1, ub);
                epilogue(m0, n0);
            }
        } else {
            // (a second, separate epilogue call site on purpose: with one shared call behind a flag the split instantiation ran
            // 142 us instead of 122 us on fc2 at T=8)
            epilogue(m0, n0);
        }
        EDV_GEMM_STAMP(4);
    }
}

// operands the 32-bit buffer offsets reach (byte offset of the last element the loop may touch, rows clamped to the edge)
inline bool fits_buffer(const GemmDesc &d) {
    const long long a_rows = d.a_map(d.M - 1) + 1, lim = (1ll << 32) - (1 << 20);
    return a_rows * d.lda * 4 < lim && (long long)d.N * d.ldw * 4 < lim && buffer_outputs_fit(d, DBM);  // (a tile's rows run up to 63 past M)
}

template <int STORE, int EP>
int dma_slots() {
    static DeviceSlotCache cache;
    static const std::string label = "gemm_dma_kernel<" + std::to_string(STORE) + "," + std::to_string(EP) + ">";
    // The occupancy API answers 5 (5 x 32 KB = the whole 160 KB of LDS), the hardware places 4: the timeline of
    // scratch/ubench/gemm_trace.hip shows exactly 4 x 256 workgroups alive.  A persistent grid must match what is really
    // resident, or the surplus workgroups start only when others finish.  EDV_GEMM_SLOTS_PER_CU overrides.
    constexpr int placed = 4;
    // ... and 3 is what the split runs with: at 3 and at 4 persistent workgroups per CU the step takes the same time (interleaved A/B,
    // profiles/r02_notes.txt), and 768 runs leave a quarter fewer pieces to write and re-read than 1024 (fc2 at T = 8: 32 vs 48 MB written).
    constexpr int cap = placed > 3 ? 3 : placed;
    return resident_workgroups(cache, (const void *)gemm_dma_kernel<STORE, EP, true, 2>, 256, 0, cap, "EDV_GEMM_SLOTS_PER_CU", label.c_str());
}

template <int STORE, int EP, bool SPLIT>
void launch_variant(const GemmDesc &d, const GemmSplit &sp, bool buf, long long grid, hipStream_t st) {
    if (buf && d.a_map.period == 0) EDV_LAUNCH((gemm_dma_kernel<STORE, EP, SPLIT, 2>), dim3((unsigned)grid), dim3(256), 0, st, d, sp);
    else if (buf) EDV_LAUNCH((gemm_dma_kernel<STORE, EP, SPLIT, 1>), dim3((unsigned)grid), dim3(256), 0, st, d, sp);
    else EDV_LAUNCH((gemm_dma_kernel<STORE, EP, SPLIT, 0>), dim3((unsigned)grid), dim3(256), 0, st, d, sp);
}

template <int STORE, int EP>
int launch_dma(const GemmDesc &d, long long tiles, hipStream_t st) {
    static const bool buf_off = env_int("EDV_GEMM_BUF", 1) == 0;  // 0: flat 64-bit DMA source addresses as in round 1 (A/B runs)
    const bool buf = !buf_off && fits_buffer(d);
    const SplitPolicy &pol = gemm_dma_split_policy();
    GemmSplit sp{};
    long long grid;
    plan_plain(tiles, pol, &sp, &grid);
    const int slots = dma_slots<STORE, EP>();
    EDV_CHECK(slots > 0 && slots <= MAX_COUNTERS, "occupancy query failed");
    if (d.ws && !gemm_plain_forced() && plan_split(tiles, slots, d.K / DBK, pol, &sp, &grid)) {
        split_bind(&sp, d.ws, pol);
        EDV_CHECK(split_ws_floats(sp, pol) <= d.ws_floats && (uintptr_t)d.ws % 16 == 0, "stream-K workspace too small (gemm_workspace)");
        launch_variant<STORE, EP, true>(d, sp, buf, grid, st);
    } else {
        launch_variant<STORE, EP, false>(d, sp, buf, grid, st);
    }
    EDV_LAUNCH_OK();
    return 0;
}

// GEGLU epilogue (EP = 6): shallow tiles (K = C of a motion module), always the plain grid, buffer descriptors only (gemm_geglu_supported)
int launch_geglu(const GemmDesc &d, long long tiles, hipStream_t st) {
    GemmSplit sp{};
    long long grid;
    plan_plain(tiles, gemm_dma_split_policy(), &sp, &grid);
    if (d.a_map.period == 0) EDV_LAUNCH((gemm_dma_kernel<STORE_ROWS, 6, false, 2>), dim3((unsigned)grid), dim3(256), 0, st, d, sp);
    else EDV_LAUNCH((gemm_dma_kernel<STORE_ROWS, 6, false, 1>), dim3((unsigned)grid), dim3(256), 0, st, d, sp);
    EDV_LAUNCH_OK();
    return 0;
}

}  // namespace

// Which launches split.  Worth it only when the grid is a few rounds deep (beyond ~5 the last round is a small fraction and the persistent
// form's 1-2 % deficit outweighs it: ViT-L fc2 at T=32, 10.7 rounds, measures -2 %) and the tiles are deep: statically assigned persistent
// workgroups lose 1-10 % against the hardware's dynamic dispatch of the plain grid when a tile is only 12 k-tiles long (K = 384), and win
// 5-15 % from K = 768 up (warm A/B in profiles/r01_gemm_tile_sweep.txt).  Small grids with deep tiles gain the most: 46 tiles x 48 k-tiles
// 33.7 -> 16.1 us, the C = 384 motion module's ff.net.2 (276 tiles) 57.5 -> 40.0.
const SplitPolicy &gemm_dma_split_policy() {
    static const int max_rounds = env_int("EDV_GEMM_SPLIT_MAX_ROUNDS", 8);
    static const SplitPolicy p{.min_kt = env_int("EDV_GEMM_SPLIT_MIN_KT", 24),        // k-tiles per tile from which the split is used (A/B runs)
                               .min_tiles = env_int("EDV_GEMM_SPLIT_MIN_TILES", 16),  // smaller grids run plain (A/B runs)
                               .max_rounds = max_rounds > 0 ? max_rounds : 8,         // grids of at least this many rounds run plain (A/B runs)
                               .widen = env_int("EDV_GEMM_SPLIT_WIDEN", 1) != 0,      // 0: never move a whole round into the split set (A/B runs)
                               .counters = MAX_COUNTERS, .slot_floats = SLOT, .whole_rounds = true};
    return p;
}

size_t gemm_workspace() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return (size_t)MAX_COUNTERS + (size_t)cus * 8 * 2 * SLOT;  // arrival counters + two slots for each of at most 8 workgroups per CU
}

size_t gemm_counter_bytes() { return (size_t)MAX_COUNTERS * sizeof(int); }

bool gemm_dma_supported(const GemmDesc &d) {
    return d.loader == LOAD_DENSE && d.K % DBK == 0 && d.lda % 4 == 0 && d.ldw % 4 == 0 && d.M > 0 && d.N > 0;
}

bool gemm_geglu_supported(const GemmDesc &d) {
    return gemm_dma_supported(d) && d.store == STORE_ROWS && d.N % 64 == 0 && d.ldc >= d.N / 2 && !d.R1 && !d.R2 && !d.P1 && !d.gamma && d.bias &&
           d.c_map.period == 0 && fits_buffer(d);
}

int gemm_dma(const GemmDesc &d, hipStream_t st) {
    EDV_CHECK(d.A && d.W && d.C, "null operand");
    EDV_CHECK(gemm_dma_supported(d), "LDS-DMA GEMM needs a dense A and K % 32 == 0");
    EDV_CHECK(d.lda >= d.K && d.ldw >= d.K, "leading dimensions");
    EDV_CHECK(((uintptr_t)d.A % 16 == 0) && ((uintptr_t)d.W % 16 == 0), "A/W must be 16-byte aligned");
    if (d.store == STORE_SHUFFLE) {
        EDV_CHECK(d.ps_s > 0 && d.N == d.ps_s * d.ps_s * d.ps_C, "pixel-shuffle N");
        EDV_CHECK(d.R1 == nullptr && d.R2 == nullptr && d.P1 == nullptr, "pixel-shuffle store takes no residual");
    }
    const long long tiles = ((d.M + DBM - 1) / DBM) * (long long)((d.N + DBN - 1) / DBN);
    EDV_CHECK(tiles > 0 && tiles < (1ll << 31), "bad grid");
    if (d.store == STORE_SHUFFLE) return launch_dma<STORE_SHUFFLE, 0>(d, tiles, st);
    switch (epilogue_kind(d)) {
        case 1: return launch_dma<STORE_ROWS, 1>(d, tiles, st);
        case 2: return launch_dma<STORE_ROWS, 2>(d, tiles, st);
        case 3: return launch_dma<STORE_ROWS, 3>(d, tiles, st);
        case 5: return launch_dma<STORE_ROWS, 5>(d, tiles, st);
        case 6:
            EDV_CHECK(gemm_geglu_supported(d), "GEGLU epilogue: dense A, K % 32 == 0, N % 64 == 0, bias, no residual, outputs below 4 GB");
            return launch_geglu(d, tiles, st);
        default: return launch_dma<STORE_ROWS, 0>(d, tiles, st);
    }
}

}  // namespace edv
