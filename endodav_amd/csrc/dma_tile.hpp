// The LDS-DMA tile pipeline of gemm_dma.hip, conv_dma.hip and (W side) conv_halo.hip, stated once: the swizzled LDS row image, the multiply of one
// 32-deep k-tile, the two-stage k loop, and the host-side limits of the 32-bit buffer offsets.  The kernels keep what differs between them: where a
// lane's 16 bytes come from (the `issue` callable), the tile walk and the epilogue.
// A use is a call only where the call compiles to the kernel's instruction counts of before (profiles/dma_tile_refactor_notes.txt has the tables
// and the uses that stay written out, each with a comment at its place: conv_dma.hip's staging map and k loop, conv_halo.hip's multiply).  A kernel
// that changes one of those copies changes it here as well; a new kernel calls these.
#pragma once
#include <algorithm>
#include <type_traits>

#include "gemm_common.hpp"

namespace edv {

constexpr int TILE_BK = 32;  // floats per LDS row: one k-tile

// ---- the image ------------------------------------------------------------------------------------------------------------------------------
// Unpadded 128-byte rows (the destination of an LDS-DMA instruction is lane-linear: lane l writes row l >> 3, 16-byte position l & 7 of the 8 rows
// it covers), the logical chunk c of row r stored at position c ^ ((r >> 1) & 7).  The swizzle is applied to the per-lane SOURCE address and to the
// fragment read (rule 21 of the CDNA guide); a 16-lane ds_read_b128 group then covers 16 distinct (r & 1, chunk) pairs = all 64 banks.
// Staging side: the logical chunk that lives at position spos of tile row r.
__device__ __forceinline__ int tile_chunk(int r, int spos) { return spos ^ ((r >> 1) & 7); }
// A tile row past the operand's edge stages the last valid row instead: its results are never stored.
template <class T>
__device__ __forceinline__ T tile_edge_row(T row, T rows) {
    return row < rows ? row : rows - 1;
}
// Read side: the q-th fragment address, in stage 0, of the lane that multiplies row `row` of the tile part at `rows` -- logical chunk 2q + lh, i.e.
// k = 8q + 4 lh .. 8q + 4 lh + 3 (the permuted-k trick of gemm.hip).  The stage is an immediate offset at the read (tile_multiply).
__device__ __forceinline__ const float *tile_frag_ptr(const float *rows, int row, int q, int lh) {
    return rows + row * TILE_BK + (((2 * q + lh) ^ ((row >> 1) & 7)) << 2);
}

// ---- one k-tile -----------------------------------------------------------------------------------------------------------------------------
// All eight fragment reads (the lane's four 16-byte A and B fragments at pa[q] + off_a, pb[q] + off_b floats: the offsets are compile-time at every
// call, so they are immediates of ds_read_b128), sixteen MFMAs in the fixed (q, e) order -- the k order every kernel's bits depend on -- then
// publish / release: this wave's DMAs of the next tile have landed (vmcnt), its fragment reads of this one are done (lgkmcnt; a raw s_barrier waits
// for neither, and after it the other waves' DMAs refill this stage: tests/test_isa_barriers_cpu.py).
// prelu (wave-uniform, one branch per k-tile; a literal false compiles away): ReLU on the A fragments, one v_med3 per element -- med3(x, 0, +inf) =
// max(x, 0); fmaxf costs two instructions.
// The two scheduling fences.  First: all eight reads are in flight before the first MFMA waits for its pair (left alone the scheduler sinks each pair
// of reads to its four MFMAs and re-uses one register quad: an LDS round trip exposed four times per k-tile).  Second: the MFMAs stay above the
// waits: they touch registers only, and the scheduler otherwise sinks fifteen of them below the barrier -- the wave then waits for its DMA one MFMA
// after issuing it instead of sixteen.
__device__ __forceinline__ void tile_multiply(const float *const (&pa)[4], int off_a, const float *const (&pb)[4], int off_b, f32x16 &acc, bool prelu) {
    f32x4 fa[4], fb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        fa[q] = *reinterpret_cast<const f32x4 *>(pa[q] + off_a);
        fb[q] = *reinterpret_cast<const f32x4 *>(pb[q] + off_b);
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

// ---- the two-stage k loop -------------------------------------------------------------------------------------------------------------------
// k-tiles kt0 .. kt1 - 1 out of two stages of STAGE floats, A and B fragments both from the swizzled image (pa, pb: stage-0 addresses): tile k + 1
// is in flight while tile k is multiplied.  issue(kt, st) starts the kernel's DMAs of k-tile kt into stage st.  The loop is unrolled by two so that
// the stage is a compile-time immediate of ds_read_b128 (a run-time toggle costs an add per fragment read, and the k loop carries no VALU
// instruction).  The other stage was last read in the previous k-tile, whose barrier has passed; the barrier that ended the previous run's last
// k-tile released both.  stamp(1) / stamp(2): first DMA issued / first tile landed, the timeline hook of gemm_dma.hip; nothing otherwise.
template <int STAGE, class Issue, class Stamp>
__device__ __forceinline__ void tile_k_loop(int kt0, int kt1, Issue &&issue, const float *const (&pa)[4], const float *const (&pb)[4], f32x16 &acc, bool prelu,
                                            Stamp &&stamp) {
    issue(kt0, 0);
    stamp(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    stamp(2);
    auto ktile = [&](int kt, auto st_tag) {
        constexpr int ST = decltype(st_tag)::value;
        if (kt + 1 < kt1) issue(kt + 1, ST ^ 1);
        tile_multiply(pa, ST * STAGE, pb, ST * STAGE, acc, prelu);
    };
    int kt = kt0;
    for (; kt + 1 < kt1; kt += 2) {
        ktile(kt, std::integral_constant<int, 0>{});
        ktile(kt + 1, std::integral_constant<int, 1>{});
    }
    if (kt < kt1) ktile(kt, std::integral_constant<int, 0>{});
}

// ---- host: what the 32-bit buffer offsets reach ---------------------------------------------------------------------------------------------
// Output side.  The buffer epilogues (gemm_epilogue_buf: identity row maps, EP 1..3) address C, R1 and R2 with 32-bit byte offsets and mask ragged
// edges through the descriptor alone: a tile's rows run up to rows_past - 1 past M, and their scalar offsets ((row0 + dr) * ld + col0) * 4 are
// computed in 32 bits -- they must not wrap, or a row past the end would come back INTO range and be stored.  Lanes past column N carry 0xfffff000,
// which must lie at or beyond num_records = M * ld * 4.  Both hold iff (M + rows_past) rows of the widest operand stay below 2^32 - 4096 bytes.
inline bool buffer_outputs_fit(const GemmDesc &d, int rows_past) {
    const long long ld = std::max(std::max(d.ldc, d.R1 ? d.ldr1 : 0), d.R2 ? d.ldr2 : 0);
    return (d.M + rows_past) * ld * 4 < (1ll << 32) - 4096;
}
// Input side of the 3x3 convolutions: the per-lane offsets must reach every tap of every pixel of the frames the launch reads, with room for the
// "beyond the end" offset of padding lanes (0x80000000 + the tensor's bytes), and every row of the packed weight.
inline bool conv_inputs_fit(const GemmDesc &d) {
    const long long frames = (d.M - 1) / ((long long)d.cOH * d.cOW) + 1;
    return frames * d.cH * d.cW * d.cC * 4 < (1ll << 31) - (1 << 20) && (long long)d.N * d.ldw * 4 < (1ll << 32) - (1 << 20);
}

}  // namespace edv
