// Host planner of the persistent grids with a stream-K tail (gemm_dma.hip, gemm_x6.hip, conv_dma.hip, attn_spatial.hip, attn_spatial_bwd.hip).
// Pure integer arithmetic and nothing from HIP: a plain host compiler builds it, and tests/test_split_plan_cpu.py runs it for every slot count
// (edv_split_plan), not only the ones one MI355X reports.
//
// The scheme.  G = grid persistent workgroups, all co-resident (`slots` = CUs x resident workgroups per CU is the most a launch may use).  Every
// workgroup first computes `whole_rounds` whole output tiles (tile = round * G + id).  The remaining tiles are `units` = split tiles x k-tiles
// k-tile units; they are cut into `nsplit` contiguous runs of `chunk` units, run j going to the workgroup with id j * stride (spread over the
// CUs).  A run that does not cover a tile's whole k range leaves its raw accumulators in workspace slot (j * 2 + segment) and bumps the tile's
// arrival counter; the LAST run to arrive sums all pieces of that tile in run order (so the result does not depend on the arrival order) and
// applies the epilogue: no fix-up launch, no spinning (gemm_common.hpp: split_handoff).  The counters live at the head of the workspace, must be
// zero before the first launch, and are left zero by every launch.  Without a workspace the launch is the plain grid: G = tiles, one whole tile each.
// What the planner and the kernels' walk must agree on -- the runs cover [0, units) exactly once, a run leaves at most two pieces in distinct
// slots, a tile's counter sees exactly g1 - g0 + 1 arrivals, the workspace holds counters + nsplit * 2 slots -- is what the CPU test asserts.
#pragma once
#include <cstddef>

namespace edv {

// Work split of one launch (host-made, passed to the kernel by value: the member layout is part of every kernel's signature).
struct GemmSplit {
    int whole_rounds, chunk, nsplit, stride;
    long long units;
    float *ws;   // piece slots (after the counters)
    int *cnt;    // one arrival counter per split tile
    int group_m = 1;  // gemm_x6.hip: row blocks per tile group of its tile order
    // gemm_x6.hip, the remainder walk (plan_remainder below).  front != 0: the workgroups with raw block index < nsplit own run blockIdx.x and
    // nothing else, every later one computes one whole tile (front_whole_tile), and the split tiles start at tile index first_split.
    int front = 0, first_split = 0;
};

// Which launches of a kernel family take the split (each family's measured thresholds stand beside its policy object).
struct SplitPolicy {
    int min_kt;         // k-tiles per tile from which the split is used
    int min_tiles;      // grids of at most this many tiles run plain
    int max_rounds;     // whole rounds: grids of at least this many rounds run plain
    bool widen;         // whole rounds: a leftover too small for an even share takes one whole round into the split set
    int counters;       // arrival counters at the head of the workspace = the most tiles a launch may split
    int slot_floats;    // floats per piece
    bool whole_rounds;  // true: rounds of whole tiles, then the leftover round split (the GEMMs).  false: only grids that do not fill the part,
                        // every tile split, one run per workgroup (the convolution)
    int deep_kt = 0, idle_factor = 0;  // no whole rounds: tiles shallower than deep_kt split only when tiles * idle_factor <= slots
};

// The plain grid: one whole tile per workgroup, nothing split.
inline void plan_plain(long long tiles, const SplitPolicy &p, GemmSplit *sp, long long *grid) {
    sp->whole_rounds = p.whole_rounds ? 1 : 0;
    sp->chunk = 1;
    sp->nsplit = 0;
    sp->stride = 1;
    sp->units = 0;
    sp->front = 0;
    sp->first_split = 0;
    *grid = tiles;
}

// Fills sp (all but its pointers and group_m) and the grid for `tiles` tiles of `nkt` k-tiles on `slots` resident workgroups.
// false: this launch does not split; sp and grid are untouched (the caller's plan_plain stands).
inline bool plan_split(long long tiles, int slots, int nkt, const SplitPolicy &p, GemmSplit *sp, long long *grid) {
    if (slots <= 0 || tiles <= p.min_tiles || nkt < p.min_kt) return false;
    const long long left = p.whole_rounds ? tiles % slots : tiles;
    if (p.whole_rounds ? !(left > 0 && tiles < (long long)p.max_rounds * slots)
                       : !(tiles <= slots && tiles <= p.counters && (nkt >= p.deep_kt || tiles * p.idle_factor <= slots)))
        return false;
    sp->whole_rounds = p.whole_rounds ? (int)(tiles / slots) : 0;
    long long split_tiles = left;
    // run length: an even share of the units over ALL workgroups.  When the leftover is too small for that (an even share would
    // be under 1/4 of a tile's k range, i.e. a handful of workgroups would carry the whole tail and the merge would chain up to
    // ~5 L2-bypassing loads at the very end of the launch), one whole round joins the split set instead: every workgroup then
    // runs whole_rounds - 1 whole tiles plus 1 + left/slots tiles' worth of k-tiles, and every split tile has 2-3 pieces.
    const long long chunk_min = (nkt + 3) / 4;
    if (p.widen && sp->whole_rounds > 0 && (left * nkt + slots - 1) / slots < chunk_min && left + slots <= p.counters) {
        --sp->whole_rounds;
        split_tiles += slots;
    }
    sp->units = split_tiles * nkt;
    long long chunk = (sp->units + slots - 1) / slots;
    chunk = chunk > chunk_min ? chunk : chunk_min;
    sp->chunk = (int)chunk;
    sp->nsplit = (int)((sp->units + chunk - 1) / chunk);
    *grid = sp->whole_rounds ? slots : (sp->nsplit > 0 ? sp->nsplit : 1);
    sp->stride = (int)(*grid / sp->nsplit) > 0 ? (int)(*grid / sp->nsplit) : 1;
    return true;
}

// ---- the remainder plan (gemm_x6.hip) ----------------------------------------------------------------------------------------------------------
// For a plain grid that ends a handful of tiles past a whole number of rounds of CUs -- M = 8 x 1370 rows are 86 row tiles, so the ViT-S linears are
// 256 + 2, 768 + 6 and 1024 + 8 tiles on 256 CUs -- where plan_split declines (shallow tiles) or would cut every tile.  Those L = tiles mod CUs tiles cost a
// round of their own (a CU that carries one more tile than the others sets the launch's time).  Here only they are split: the LAST L tile indices
// are cut along k into `nsplit` runs of `chunk` k-tiles, the other tiles stay whole, and the grid is nsplit + whole tiles workgroups.  The first
// nsplit RAW block indices own run blockIdx.x and nothing else, so the hardware starts the pieces first and deals them round-robin over the XCDs;
// their hand-off and merge (the same split_slot / split_handoff / split_piece path) finish under the first round of whole tiles instead of forming
// a tail.  Every later workgroup computes one whole tile, dispatched dynamically like the plain grid's.
struct RemainderPolicy {
    int left_div;     // by policy only L <= CUs / left_div leftover tiles are worth it (more: the pieces themselves fill a good part of a round),
                      // and only grids that are resident at once (grid <= CUs x workgroups per CU): those cleared the spread of their repetitions
    int run_div;      // run length = k-tiles / run_div ...
    int min_run;      // ... but at least this many k-tiles (a piece costs a prologue, 64 KB of stores and a counter add); shallower tiles run plain
    int runs_per_cu;  // runs (two piece slots each) that gemm_workspace() holds per CU at this family's slot size
    int counters;
};

// Fills sp (all but its pointers and group_m) and the grid.  `everywhere`: wherever the walk is supported (any L > 0), not only where the policy
// expects a gain.  false: the plan does not apply; sp and grid are untouched.
inline bool plan_remainder(long long tiles, int nkt, int cus, int wgs_per_cu, bool everywhere, const RemainderPolicy &p, GemmSplit *sp, long long *grid) {
    if (cus <= 0 || wgs_per_cu <= 0 || tiles < cus || nkt < p.min_run) return false;
    const long long left = tiles % cus;
    if (left == 0 || left > p.counters || (!everywhere && left * p.left_div > cus)) return false;
    const long long units = left * nkt;
    // every run is resident in the first wave of the dispatch and has its two slots in the workspace
    const long long cap = (long long)cus * (wgs_per_cu < p.runs_per_cu ? wgs_per_cu : p.runs_per_cu);
    long long chunk = nkt / p.run_div > p.min_run ? nkt / p.run_div : p.min_run;
    if ((units + cap - 1) / cap > chunk) chunk = (units + cap - 1) / cap;
    const long long nsplit = (units + chunk - 1) / chunk;
    if (!everywhere && nsplit + (tiles - left) > (long long)cus * wgs_per_cu) return false;
    sp->whole_rounds = 1;
    sp->chunk = (int)chunk;
    sp->nsplit = (int)nsplit;
    sp->stride = 1;
    sp->units = units;
    sp->front = 1;
    sp->first_split = (int)(tiles - left);
    *grid = sp->nsplit + (tiles - left);
    return true;
}

// The whole tile of raw block index b >= nsplit in a remainder grid of G workgroups.  Blocks b and b + 8 share an XCD; as in xcd_remap each XCD gets
// a contiguous run of tile indices, counted over the whole-tile blocks only: a bijection from [nsplit, G) onto [0, G - nsplit).
#ifdef __HIPCC__
__host__ __device__
#endif
inline int front_whole_tile(int b, int G, int nsplit) {
    const int x = b & 7;
    const int before = ((G >> 3) * x + (x < (G & 7) ? x : (G & 7))) - ((nsplit >> 3) * x + (x < (nsplit & 7) ? x : (nsplit & 7)));  // whole blocks of XCDs < x
    return before + (b >> 3) - ((nsplit + 7 - x) >> 3);
}

// floats of workspace a split launch needs: the counters, then two slots per run
inline size_t split_ws_floats(const GemmSplit &sp, const SplitPolicy &p) { return (size_t)p.counters + (size_t)sp.nsplit * 2 * p.slot_floats; }

inline void split_bind(GemmSplit *sp, float *ws, const SplitPolicy &p) {
    sp->cnt = reinterpret_cast<int *>(ws);
    sp->ws = ws + p.counters;
}

// The task-level form of the two spatial-attention files: `ntasks` tasks of `ntiles` key tiles; whole rounds of tasks, then the leftover tasks'
// tiles cut into one run per workgroup (stride 1), whose pieces a combine launch merges.  A caller's workspace is pieces() x rows x columns floats.
struct TaskSplit {
    int grid, whole_rounds, chunk, leftover, nsplit;
    long long units;
    size_t pieces() const { return (size_t)nsplit * 2; }
};
inline TaskSplit plan_tasks(long long ntasks, int ntiles, int slots, bool plain) {
    TaskSplit p;
    if (plain || slots <= 0) {  // one workgroup per task
        p.grid = (int)ntasks; p.whole_rounds = 1; p.leftover = 0; p.units = 0; p.chunk = 1; p.nsplit = 0;
        return p;
    }
    p.whole_rounds = (int)(ntasks / slots);
    p.leftover = (int)(ntasks - (long long)p.whole_rounds * slots);
    p.units = (long long)p.leftover * ntiles;
    p.chunk = p.units ? (int)((p.units + slots - 1) / slots) : 1;
    p.nsplit = (int)((p.units + p.chunk - 1) / p.chunk);
    p.grid = p.whole_rounds ? slots : p.nsplit;
    return p;
}

}  // namespace edv
