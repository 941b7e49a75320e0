// Pieces shared by the fp32-MFMA GEMMs (gemm.hip, gemm_dma.hip, conv_dma.hip; experiments/gemm_sb.hip used them too): all accumulate 32x32
// tiles whose C/D register layout is  col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)  (dtype-independent on gfx950).
#pragma once
#include "ops.hpp"

namespace edv {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == ACT_GELU) return gelu_erf(v);
    if (act == ACT_RELU) return fmaxf(v, 0.0f);
    return v;
}

// The merging workgroup's acquire (round 3).  The piece exchange stores and loads every piece word sc1 behind a drained, barrier-ordered counter add:
// the form MI355X_MICROARCH.md ("Valid forms") measures as sufficient WITHOUT an acquire -- but only at one workgroup per CU, and the split launches
// run three.  Outside that table the guide says "keep the acquire", so the ONE lane whose counter add completes a tile invalidates its CU's L1
// (buffer_inv sc1) and waits for it before the workgroup barrier that precedes the piece loads: poll -> acquire -> vmcnt(0) -> barrier -> loads, the
// guide's consumer sequence.  Only the last arriver of a split tile pays it (priced at 1.7-7 us by the guide; measured on the step in
// profiles/r03_notes.txt).  -DEDV_SPLIT_ACQUIRE=0 builds the round-2 form for A/B runs.
#ifndef EDV_SPLIT_ACQUIRE
#define EDV_SPLIT_ACQUIRE 1
#endif
__device__ __forceinline__ void split_merge_acquire() {
#if EDV_SPLIT_ACQUIRE
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}
constexpr int SPLIT_SLOT = 64 * 64;        // floats per piece: a 64x64 or 128x32 tile in accumulator order, (wave * 16 + r) * 64 + lane
constexpr int SPLIT_MAX_COUNTERS = 4096;   // >= the tiles a launch may split
// EDV_GEMM_PLAIN=1: one workgroup per tile even with a workspace (A/B runs of gemm_dma.hip and gemm_x6.hip)
inline bool gemm_plain_forced() {
    static const bool on = env_int("EDV_GEMM_PLAIN", 0) != 0;
    return on;
}

// ---- device side of the stream-K split (streamk_plan.hpp has the scheme and the host planner) ------------------------------------------------
// Used by gemm_dma.hip, conv_dma.hip and gemm_x6.hip.  Their form is what kept every kernel's instruction stream unchanged when they were factored
// out: GemmSplit travels BY VALUE (through a reference the kernel-argument loads lose their amdgpu.noclobber marking and the merge's addressing
// changes), the merge RETURNS its accumulators (filled through a reference it changes the k loops' waits or the registers of twelve
// instantiations), and the segment arithmetic stays in each kernel (moving it moved the generated code).
// Run cursor: the run a workgroup owns (run j = bid / stride; only workgroups with bid % stride == 0 and j < nsplit own one; -1: none), its first
// unit, one past its last.
__device__ __forceinline__ int split_run(const GemmSplit sp, bool split, int bid) {
    return (split && sp.units > 0 && bid % sp.stride == 0 && bid / sp.stride < sp.nsplit) ? bid / sp.stride : -1;
}
__device__ __forceinline__ long long split_run_begin(const GemmSplit sp, int run) { return run >= 0 ? (long long)run * sp.chunk : 0; }
__device__ __forceinline__ long long split_run_end(const GemmSplit sp, int run, long long u) {
    return run >= 0 ? (u + sp.chunk < sp.units ? u + sp.chunk : sp.units) : 0;
}
// The slot rule.  A run longer than a tile's k range has up to three segments: the tail of a tile, whole tiles, the head of a tile.  Only the first
// and the last can be pieces.  Slot 0 = the piece that holds the run's first unit, slot 1 = the other one.  split_slot is the producer's side (the
// segment of run `run` that starts at unit u; SLOT floats per piece), split_piece the merge's, from the tile's side: run start inside the tile -> slot 0.
template <int SLOT>
__device__ __forceinline__ float *split_slot(const GemmSplit sp, int run, long long u) {
    return sp.ws + ((long long)run * 2 + (u == (long long)run * sp.chunk ? 0 : 1)) * SLOT;
}
// run g's piece of the split tile whose first unit is ub, relative to `base` (sp.ws plus, or followed by, the lane's offset inside a piece)
template <int SLOT>
__device__ __forceinline__ const float *split_piece(const float *base, const GemmSplit sp, int g, long long ub) {
    return base + ((long long)g * 2 + ((long long)g * sp.chunk >= ub ? 0 : 1)) * SLOT;
}

// Piece hand-off.  Pieces travel between workgroups on different XCDs (separate L2s, non-coherent L1s).  An agent-scope
// release / acquire fence pair would do it, but on this part the release writes back the WHOLE L2 (buffer_wbl2) -- measured
// +140 us per launch with every other workgroup's output tiles dirty in it.  Instead:
//   producer  every piece word is stored with an agent-scope relaxed atomic store (global_store ... sc1: write-through);
//             every storing wave then executes s_waitcnt vmcnt(0) (its stores are acknowledged), the workgroup meets at a
//             barrier, and ONE lane adds 1 to the tile's agent-scope counter;
//   consumer  the workgroup whose add returns "all pieces in" broadcasts that through LDS behind a workgroup barrier and
//             reads every piece word with agent-scope relaxed atomic loads (global_load ... sc1: served by L2, never by this
//             CU's L1), in run order whatever the arrival order was.
// This is the "sc1 stores + drained counter + sc1 loads" hand-off the CDNA4 guide measures as valid (MI355X_MICROARCH.md,
// Workgroup dispatch ..., Valid forms: one lane signals for all of its workgroup's stores after every wave's vmcnt(0) and
// the barrier; every load of the handed-off bytes is an sc1 load issued after the add has returned and a barrier) -- measured
// there at ONE workgroup per CU; these launches run up to four, so the merging workgroup also executes the agent-scope acquire the
// guide prescribes outside its table (split_merge_acquire above).  It is
// an ISA-level contract of gfx950 / ROCm 7.2, NOT a guarantee of the C++ memory model: the __syncthreads() between the
// counter add and the loads is what keeps the compiler from hoisting the loads (a workgroup-scope fence), the hardware
// ordering comes from sc1.  tests/test_streamk_fuzz_gpu.py::test_piece_exchange_contract_under_uneven_load is the gate to
// re-run after a toolchain change; the fenced form to switch to is spelled out there.
//
// split_handoff: what follows a workgroup's piece stores for split tile lt (split_store_piece below for the kernels whose wave holds one 32x32
// block, gemm_dma.hip and conv_dma.hip; gemm_x6.hip keeps its own stores: a wave of it holds other accumulators).  cnt = &sp.cnt[lt], ub = lt * nkt
// = the tile's first unit.  Returns, to every thread of the workgroup, whether this was the tile's last piece to arrive -- the workgroup then
// merges runs g0 .. g1 (the runs whose unit ranges intersect [ub, ub + nkt)) with agent-scope loads in run order (split_piece) and applies the
// epilogue.  s_last: one int of LDS that is idle between the k loop and the next tile's first staging write.
__device__ __forceinline__ bool split_handoff(const GemmSplit sp, int *cnt, long long ub, int nkt, int *s_last, int tid, int &g0, int &g1) {
    g0 = (int)(ub / sp.chunk), g1 = (int)((ub + nkt - 1) / sp.chunk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int arrived = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = arrived == g1 - g0;
        if (last) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // all pieces in: zero for the next launch
        if (last) split_merge_acquire();  // this CU's L1 may hold stale lines of the piece slots
        *s_last = last;
    }
    __syncthreads();
    const bool last = *s_last != 0;
    __syncthreads();  // s_last is read before the next tile's staging may overwrite it
    return last;
}

// The piece of a wave that holds ONE 32x32 block (gemm_dma.hip, conv_dma.hip), in accumulator order: word (wave * 16 + r) * 64 + lane.
// split_store_piece is the producer's side, before split_handoff; split_merge_pieces the last arriver's, after it: it returns the sum of the pieces of
// runs g0 .. g1 in run order whatever the arrival order was, two pieces in flight, (acc + a) + b -- the order is part of the result's bits.
__device__ __forceinline__ void split_store_piece(float *part, int wave, int lane, const f32x16 &acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) __hip_atomic_store(&part[(wave * 16 + r) * 64 + lane], acc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int SLOT>
__device__ __forceinline__ f32x16 split_merge_pieces(const GemmSplit sp, int wave, int lane, int g0, int g1, long long ub) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *base = sp.ws + (wave * 16) * 64 + lane;
    int gg = g0;
    for (; gg + 1 <= g1; gg += 2) {
        const float *pa = split_piece<SLOT>(base, sp, gg, ub);
        const float *pb = split_piece<SLOT>(base, sp, gg + 1, ub);
        float ta[16], tb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ta[r] = __hip_atomic_load(pa + r * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tb[r] = __hip_atomic_load(pb + r * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = (acc[r] + ta[r]) + tb[r];
    }
    if (gg <= g1) {
        const float *pa = split_piece<SLOT>(base, sp, gg, ub);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += __hip_atomic_load(pa + r * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return acc;
}

// XCD-aware, bijective block remap: blocks b and b+8 share an XCD (and its L2); give each XCD a contiguous run of
// logical tiles so that tiles sharing an operand panel hit the same L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7, loc = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + loc;
}

// v = acc + bias[n] + P1[p1_map(m), n];  v = act(v) * gamma[n];  v += R1[r1_map(m), n] + R2[c_row, n];  store
template <int FM, int FN, int STORE>
__device__ __forceinline__ void gemm_epilogue(const GemmDesc &g, f32x16 (&acc)[FM][FN], long long m0, int n0, int wrow, int wcol, int l31, int lh) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wcol + j * 32 + l31;
        if (n >= g.N) continue;
        const float bias = g.bias ? g.bias[n] : 0.f;
        const float gam = g.gamma ? g.gamma[n] : 1.f;
        int ps_sub = 0, ps_co = 0, ps_dy = 0, ps_dx = 0;
        if (STORE == STORE_SHUFFLE) {
            ps_sub = n / g.ps_C;
            ps_co = n - ps_sub * g.ps_C;
            ps_dy = ps_sub / g.ps_s;
            ps_dx = ps_sub - ps_dy * g.ps_s;
        }
#pragma unroll
        for (int i = 0; i < FM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= g.M) continue;
                float pre = acc[i][j][r] + bias;
                if (g.P1) pre += g.P1[g.p1_map(m) * g.ldp1 + n];
                float v = apply_act(pre, g.act) * gam;
                if (STORE == STORE_ROWS) {
                    const long long crow = g.c_map(m);
                    if (g.R1) v += g.R1[g.r1_map(m) * g.ldr1 + n];
                    if (g.R2) v += g.R2[crow * g.ldr2 + n];
                    g.C[crow * g.ldc + n] = v;
                } else {
                    const int gp = g.ps_h * g.ps_w;
                    const long long f = m / gp;
                    const int p = (int)(m - f * gp);
                    const int y = p / g.ps_w, x = p - y * g.ps_w;
                    const long long orow = (f * g.ps_h * g.ps_s + (long long)y * g.ps_s + ps_dy) * (g.ps_w * g.ps_s) + x * g.ps_s + ps_dx;
                    g.C[orow * g.ps_C + ps_co] = v;
                }
            }
        }
    }
}


// The same epilogue for ONE element (used by the stream-K fix-up kernel, which sums the pieces of a split tile).
template <int STORE>
__device__ __forceinline__ void gemm_epilogue_elem(const GemmDesc &g, float accv, long long m, int n) {
    float pre = accv + (g.bias ? g.bias[n] : 0.f);
    if (g.P1) pre += g.P1[g.p1_map(m) * g.ldp1 + n];
    float v = apply_act(pre, g.act) * (g.gamma ? g.gamma[n] : 1.f);
    if (STORE == STORE_ROWS) {
        const long long crow = g.c_map(m);
        if (g.R1) v += g.R1[g.r1_map(m) * g.ldr1 + n];
        if (g.R2) v += g.R2[crow * g.ldr2 + n];
        g.C[crow * g.ldc + n] = v;
    } else {
        const int ps_sub = n / g.ps_C, ps_co = n - ps_sub * g.ps_C;
        const int ps_dy = ps_sub / g.ps_s, ps_dx = ps_sub - ps_dy * g.ps_s;
        const int gp = g.ps_h * g.ps_w;
        const long long f = m / gp;
        const int p = (int)(m - f * gp);
        const int y = p / g.ps_w, x = p - y * g.ps_w;
        const long long orow = (f * g.ps_h * g.ps_s + (long long)y * g.ps_s + ps_dy) * (g.ps_w * g.ps_s) + x * g.ps_s + ps_dx;
        g.C[orow * g.ps_C + ps_co] = v;
    }
}

// ---- compact epilogue for the common case -----------------------------------------------------------------------------
// The general epilogue above unrolls 16 rows x every optional feature (row maps with 64-bit divisions, P1, a runtime
// activation switch with an inlined erff per row): ~11 000 instructions, more than the 64 KB instruction cache two CUs
// share.  A workgroup timeline (scratch/ubench/gemm_trace.hip) showed 7.8 us of a 27 us workgroup life inside it.  Every
// encoder linear and every convolution needs only: identity row maps, no P1, a compile-time activation.
//   EP = 0: general;  EP = 1 + ACT (ACT_NONE / ACT_GELU / ACT_RELU): fast.
//   EP = 6: GEGLU (gemm_dma.hip): the tile's columns 0..31 are values, 32..63 their gates; C gets value * gelu(gate), half as wide.
//   EP = 5: row-mapped output (and residual) with one period >= 32 rows, no activation -- the patch-embed GEMM, whose rows go to
//           frame f's token slots behind the class token and take the position table as a per-frame-periodic residual.
inline int epilogue_kind(const GemmDesc &d) {
    if (d.geglu) return 6;  // (gemm_dma.hip only; gemm_geglu_supported() is the caller's gate)
    if (d.store == STORE_ROWS && !d.P1 && !d.R2 && d.act == ACT_NONE && d.c_map.period >= 32 && d.c_map.inner == 1 &&
        (!d.R1 || (d.r1_map.period == d.c_map.period && d.r1_map.inner == 1)))
        return 5;
    if (d.store != STORE_ROWS || d.P1 || d.c_map.period != 0 || (d.R1 && d.r1_map.period != 0)) return 0;
    if (d.act != ACT_NONE && d.act != ACT_GELU && d.act != ACT_RELU) return 0;
    return 1 + d.act;
}

// Per-column epilogue operands, fetched BEFORE the k loop: at the end of the loop the load would queue behind the
// other workgroups' tile traffic and its latency would be fully exposed.
#ifndef EDV_EPI_STORE_COND
#define EDV_EPI_STORE_COND  // ablation hook of scratch/ubench/gemm_trace.hip; empty in the product build
#endif
template <int FN>
struct EpiCols {
    float bias[FN], gam[FN];
};
template <int FN>
__device__ __forceinline__ EpiCols<FN> gemm_epilogue_prefetch(const GemmDesc &g, int n0, int wcol, int l31) {
    EpiCols<FN> c;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        int n = n0 + wcol + j * 32 + l31;
        n = n < g.N ? n : g.N - 1;
        c.bias[j] = g.bias ? g.bias[n] : 0.f;
        c.gam[j] = g.gamma ? g.gamma[n] : 1.f;
    }
    return c;
}

template <int FM, int FN, int ACT>
__device__ __forceinline__ void gemm_epilogue_fast(const GemmDesc &g, f32x16 (&acc)[FM][FN], const EpiCols<FN> &cols, long long m0, int n0, int wrow,
                                                   int wcol, int l31, int lh) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wcol + j * 32 + l31;
        if (n >= g.N) continue;
        const float bias = cols.bias[j], gam = cols.gam[j];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const long long mb = m0 + wrow + i * 32 + 4 * lh;  // row of register r: mb + (r&3) + 8*(r>>2)
            const int left = (int)(g.M - mb < 32 ? g.M - mb : 32);
            float res[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r] = 0.f;
            if (g.R1) {
                const float *rp = g.R1 + mb * g.ldr1 + n;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dr = (r & 3) + 8 * (r >> 2);
                    if (dr < left) res[r] = rp[(long long)dr * g.ldr1];
                }
            }
            if (g.R2) {
                const float *rp = g.R2 + mb * g.ldr2 + n;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dr = (r & 3) + 8 * (r >> 2);
                    if (dr < left) res[r] += rp[(long long)dr * g.ldr2];
                }
            }
            float *cp = g.C + mb * g.ldc + n;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2);
                float v = acc[i][j][r] + bias;
                if (ACT == ACT_GELU) v = gelu_erf(v);
                if (ACT == ACT_RELU) v = fmaxf(v, 0.0f);
                if (dr < left EDV_EPI_STORE_COND) cp[(long long)dr * g.ldc] = v * gam + res[r];
            }
        }
    }
}

// Epilogue of one wave's 32x32 block through buffer descriptors (LDS-DMA kernels, gemm_dma.hip / conv_dma.hip) (EP = 1..3: identity row maps, compile-time activation).  The general form
// (gemm_epilogue_fast) spends ~20 VALU instructions per output register on 64-bit addresses, row-bound compares and exec masks -- a few
// hundred per tile, and on this part every VALU instruction is matrix-pipe time (a K = 384 GEMM tile is only 192 MFMAs per wave).  Here the
// per-lane offset (4 lh rows + column l31) is one multiply per tile and the row advance lives in the SCALAR offset of buffer_load /
// buffer_store: the address arithmetic is SALU, the VALU work is the arithmetic the epilogue exists for (bias, activation, gamma, residual).
// Edge tiles need no second code path: the descriptors end at row M (num_records = M x ld x 4 bytes; the hardware range-checks voffset + soffset
// as one sum without wrap-around -- scratch/ubench/buf_range.hip -- so stores to rows past M are dropped and loads return 0), and a lane whose
// column is past N gets a per-lane offset near 2^32, which no scalar offset brings back into range.
// cache policy of the output stores (aux bits of buffer_store: 0 = default, 2 = nt / streaming): A/B builds only
#ifndef EDV_EPI_STORE_AUX
#define EDV_EPI_STORE_AUX 0
#endif
template <int ACT>
__device__ __forceinline__ void gemm_epilogue_buf(const GemmDesc &g, f32x16 &acc, const EpiCols<1> &cols, long long row0, int col0, int l31, int lh) {
    // row0 / col0: first row / column of the wave's block -- wave-uniform (callers derive them from readfirstlane(wave)), so they live in SGPRs
    using f32x2 = __attribute__((ext_vector_type(2))) float;
    f32x2 res[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) res[i] = f32x2{0.f, 0.f};
    if (g.R1) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.R1), 0, (int)(unsigned)(g.M * g.ldr1 * 4), 0x00020000);
        const unsigned vo = (unsigned)((4 * lh * g.ldr1 + l31) * 4);
        const unsigned so = (unsigned)((row0 * g.ldr1 + col0) * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            res[r >> 1][r & 1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, (int)(so + (unsigned)(((r & 3) + 8 * (r >> 2)) * g.ldr1 * 4)), 0));
    }
    if (g.R2) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.R2), 0, (int)(unsigned)(g.M * g.ldr2 * 4), 0x00020000);
        const unsigned vo = (unsigned)((4 * lh * g.ldr2 + l31) * 4);
        const unsigned so = (unsigned)((row0 * g.ldr2 + col0) * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            res[r >> 1][r & 1] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, (int)(so + (unsigned)(((r & 3) + 8 * (r >> 2)) * g.ldr2 * 4)), 0));
    }
    const unsigned lane_out = col0 + l31 >= g.N ? 0xfffff000u : 0u;  // past the last column: out of every descriptor's range (fits_buffer: < 2^32 - 2^20)
    const auto rc = __builtin_amdgcn_make_buffer_rsrc(g.C, 0, (int)(unsigned)(g.M * g.ldc * 4), 0x00020000);
    const unsigned vo = (unsigned)((4 * lh * g.ldc + l31) * 4) | lane_out;
    const unsigned so = (unsigned)((row0 * g.ldc + col0) * 4);
    const f32x2 bias = {cols.bias[0], cols.bias[0]}, gam = {cols.gam[0], cols.gam[0]};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f32x2 v = f32x2{acc[2 * i], acc[2 * i + 1]} + bias;
        if (ACT == ACT_GELU) v = f32x2{gelu_erf(v[0]), gelu_erf(v[1])};
        if (ACT == ACT_RELU) v = f32x2{fmaxf(v[0], 0.0f), fmaxf(v[1], 0.0f)};
        v = v * gam + res[i];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int r = 2 * i + e;
            const float ve = e ? v[1] : v[0];  // (a bit_cast applied directly to the vector element v[e] compiles to element 0 for both e)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ve), rc, (int)vo, (int)(so + (unsigned)(((r & 3) + 8 * (r >> 2)) * g.ldc * 4)), EDV_EPI_STORE_AUX);
        }
    }
}

// Fused 1x1 to one channel (GemmDesc::w2; EP = 8 + ACT in conv_dma.hip) for a wave that holds ALL columns of its 32 rows (one column tile, N <= 32):
//   y[row] = act2(sum_n w2[n] * act(acc[row][n] + bias[n]) + b2),  one float per row instead of the N-wide tile.
// A lane holds column l31 of 16 rows, so the sum over n is a sum over the 32 lanes of a wave half, taken in registers: v_permlane16_swap
// (gfx950) exchanges the odd 16-lane rows of one register with the even rows of its neighbour, so one swap + one add folds lanes l and l ^ 16 of TWO
// registers into one (even rows: register 2i, odd rows: register 2i + 1); four DPP adds (quad swaps, half-row mirror, row mirror) finish
// each of the eight.  No LDS, no barrier: 8 swaps + 40 adds for 16 rows.  Every lane of a 16-lane row then holds the row's sum; lane i < 8 of it
// keeps register i and stores that row's value.  w2v, b2v: the lane's w2[n] (any value for n >= N: those lanes add 0) and b2, fetched before the k loop.
// gemm_dot_reduce returns the lane's value: for lane i = l31 & 15 < 8 the finished y of accumulator register r = 2 i + (l31 >> 4), i.e. of row
// (r & 3) + 8 (r >> 2) + 4 lh of the wave's block; lanes 8..15 of a 16-lane row hold nothing to store.  Shared by conv_dma.hip and conv_halo.hip.
template <int ACT>
__device__ __forceinline__ float gemm_dot_reduce(const GemmDesc &g, const f32x16 &acc, const EpiCols<1> &cols, float w2v, float b2v, bool col_in, int l31) {
    float t[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = acc[r] + cols.bias[0];
        if (ACT == ACT_RELU) v = fmaxf(v, 0.0f);
        t[r] = col_in ? w2v * v : 0.f;
    }
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(t[2 * i]), __float_as_uint(t[2 * i + 1]), false, false);
        float v = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
        v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]: lane ^ 1
        v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]: lane ^ 2
        v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x141, 0xf, 0xf, true));  // row_half_mirror: the other quad of 8
        v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x140, 0xf, 0xf, true));  // row_mirror: the other half of 16
        s[i] = v;
    }
    const int i = l31 & 15;
    float v = s[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) v = i == k ? s[k] : v;
    v += b2v;
    if (g.act2 == ACT_RELU) v = fmaxf(v, 0.f);
    else if (g.act2 == ACT_SIGMOID) v = 1.f / (1.f + expf(-v));
    else if (g.act2 == ACT_SIGMOID_NEG) v = 1.f / (1.f + expf(v));
    return v;
}

// ... and its store for a wave whose 32 rows are consecutive rows of M from row0 (conv3_dma_kernel)
template <int ACT>
__device__ __forceinline__ void gemm_epilogue_dot(const GemmDesc &g, f32x16 &acc, const EpiCols<1> &cols, float w2v, float b2v, long long row0, int col0, int l31,
                                                  int lh) {
    const float v = gemm_dot_reduce<ACT>(g, acc, cols, w2v, b2v, col0 + l31 < g.N, l31);
    const int i = l31 & 15, r = 2 * i + (l31 >> 4);
    const unsigned row = (unsigned)((r & 3) + 8 * (r >> 2) + 4 * lh);
    // descriptor ends at row M: rows past it (an edge tile) are dropped, as in gemm_epilogue_buf
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(g.dot_out, 0, (int)(unsigned)(g.M * 4), 0x00020000);
    const unsigned vo = i < 8 ? row * 4u : 0xfffff000u;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, (int)vo, (int)(unsigned)(row0 * 4), EDV_EPI_STORE_AUX);
}

// EP = 5 (see epilogue_kind): rows m = mb + dr of a 32-row block cross at most one period boundary, so one division per block suffices
template <int FM, int FN>
__device__ __forceinline__ void gemm_epilogue_mapped(const GemmDesc &g, f32x16 (&acc)[FM][FN], const EpiCols<FN> &cols, long long m0, int n0, int wrow,
                                                     int wcol, int l31, int lh) {
    const int P = g.c_map.period;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wcol + j * 32 + l31;
        if (n >= g.N) continue;
        const float bias = cols.bias[j], gam = cols.gam[j];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const long long mb = m0 + wrow + i * 32 + 4 * lh;
            const int left = (int)(g.M - mb < 32 ? g.M - mb : 32);
            const long long f0 = mb / P;
            const int in0 = (int)(mb - f0 * P);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2);
                if (dr >= left) continue;
                const int t = in0 + dr;
                const int wrap = t >= P ? 1 : 0;
                const long long f = f0 + wrap;
                const int pin = t - wrap * P;
                float v = (acc[i][j][r] + bias) * gam;
                if (g.R1) v += g.R1[(f * g.r1_map.stride + g.r1_map.offset + pin) * g.ldr1 + n];
                g.C[(f * g.c_map.stride + g.c_map.offset + pin) * g.ldc + n] = v;
            }
        }
    }
}

template <int FM, int FN, int STORE, int EP>
__device__ __forceinline__ void gemm_epilogue_ep(const GemmDesc &g, f32x16 (&acc)[FM][FN], const EpiCols<FN> &cols, long long m0, int n0, int wrow,
                                                 int wcol, int l31, int lh) {
    if constexpr (EP == 0)
        gemm_epilogue<FM, FN, STORE>(g, acc, m0, n0, wrow, wcol, l31, lh);
    else if constexpr (EP == 5)
        gemm_epilogue_mapped<FM, FN>(g, acc, cols, m0, n0, wrow, wcol, l31, lh);
    else
        gemm_epilogue_fast<FM, FN, EP - 1>(g, acc, cols, m0, n0, wrow, wcol, l31, lh);
}

}  // namespace edv
