"""The host planner of the persistent stream-K grids (csrc/streamk_plan.hpp through edv_split_plan), on the CPU, for slot counts no single
MI355X reports (partitioned and mixed nodes give other CU counts):

1. it plans exactly what the five planners it replaced planned (transcribed below from their last per-file versions), field for field;
2. every split plan satisfies what the kernels' walk relies on: the runs cover [0, units) exactly once, a run leaves at most two pieces in
   distinct slots, the producer's and the merge's slot rules agree, a tile's counter sees exactly g1 - g0 + 1 arrivals, and the counters and
   piece slots fit the workspace.

The EDV_* planner knobs must be unset (the policies read them once per process)."""
import ctypes as C
import os

import numpy as np
import pytest

SLOTS = (1, 2, 3, 7, 8, 32, 64, 96, 128, 256, 304, 512, 768, 1024)
NKT = (12, 18, 24, 27, 48, 54, 64, 96, 108, 128, 256)
TILES = tuple(range(1, 200)) + tuple(range(200, 9001, 37))
GEMM_DMA, GEMM_X6, CONV, ATTN = 0, 1, 2, 3
COUNTERS = 4096                                            # SPLIT_MAX_COUNTERS
SLOT_FLOATS = {GEMM_DMA: 64 * 64, GEMM_X6: 128 * 128, CONV: 64 * 64}
PER_CU_CAP = {GEMM_DMA: 3, GEMM_X6: 2, CONV: 4}            # resident workgroups per CU each kind's slot query allows at most
KNOBS = ("EDV_GEMM_SPLIT_MIN_KT", "EDV_GEMM_SPLIT_MIN_TILES", "EDV_GEMM_SPLIT_MAX_ROUNDS", "EDV_GEMM_SPLIT_WIDEN", "EDV_X6_SPLIT_MIN_KT")


# ---- the planners this one replaced, as they stood in gemm_dma.hip / gemm_x6.hip / conv_dma.hip / attn_spatial.hip / attn_spatial_bwd.hip --------
# (split, grid, whole_rounds, chunk, nsplit, stride | leftover, units, workspace floats | pieces)
def old_gemm(tiles, slots, nkt, min_kt, slot_floats):
    """launch_dma (min_kt 24, min_tiles 16, max_rounds 8, widen on) and launch_x6 (min_kt 48, the literals 16 and 8): the same arithmetic."""
    left = tiles % slots
    if not (left > 0 and tiles > 16 and tiles < 8 * slots and nkt >= min_kt):
        return (0, tiles, 1, 1, 0, 1, 0, 0)
    whole_rounds = tiles // slots
    split_tiles = left
    chunk_min = (nkt + 3) // 4
    if whole_rounds > 0 and (left * nkt + slots - 1) // slots < chunk_min and left + slots <= COUNTERS:
        whole_rounds -= 1
        split_tiles += slots
    units = split_tiles * nkt
    chunk = max((units + slots - 1) // slots, chunk_min)
    nsplit = (units + chunk - 1) // chunk
    grid = slots if whole_rounds else (nsplit if nsplit > 0 else 1)
    stride = grid // nsplit if grid // nsplit > 0 else 1
    return (1, grid, whole_rounds, chunk, nsplit, stride, units, COUNTERS + nsplit * 2 * slot_floats)


def old_conv(tiles, slots, nkt):
    """launch_conv_ep: no whole rounds, stride 1."""
    if not (slots > 0 and tiles > 16 and tiles <= slots and tiles <= COUNTERS and nkt >= 18 and (nkt >= 48 or tiles * 8 <= slots)):
        return (0, tiles, 0, 1, 0, 1, 0, 0)
    units = tiles * nkt
    chunk = max((units + slots - 1) // slots, (nkt + 3) // 4)
    nsplit = (units + chunk - 1) // chunk
    return (1, nsplit, 0, chunk, nsplit, 1, units, COUNTERS + nsplit * 2 * 64 * 64)


def old_attn_fwd(ntasks, slots, ntiles):
    """make_plan after its kernel choice (slots > 0 checked before); ws_floats = split_wgs * 2 * rows * columns."""
    whole_rounds = ntasks // slots
    leftover = ntasks - whole_rounds * slots
    units = leftover * ntiles
    chunk = (units + slots - 1) // slots if units else 1
    split_wgs = (units + chunk - 1) // chunk
    grid = slots if whole_rounds else split_wgs
    return (int(split_wgs > 0), grid, whole_rounds, chunk, split_wgs, leftover, units, split_wgs * 2)


def old_attn_bwd(ntasks, slots, ntiles):
    """make_bwd_plan: the same, and plain for slots <= 0."""
    if slots <= 0:
        return (0, ntasks, 1, 1, 0, 0, 0, 0)
    return old_attn_fwd(ntasks, slots, ntiles)


@pytest.fixture(scope="module")
def plan(lib):
    assert not [k for k in KNOBS if k in os.environ], "the planner knobs must be unset for this test"
    out = (C.c_int64 * 8)()

    def call(kind, n, slots, nkt):
        assert lib.edv_split_plan(kind, n, slots, nkt, out) == 0
        return tuple(out)

    return call


@pytest.fixture(scope="module")
def sweep(plan):
    """{kind: [(tiles, slots, nkt, plan)]} over the whole sweep, computed once."""
    return {kind: [(t, s, k, plan(kind, t, s, k)) for s in SLOTS for k in NKT for t in TILES] for kind in (GEMM_DMA, GEMM_X6, CONV, ATTN)}


def test_plans_equal_the_per_file_planners(sweep, plan):
    for t, s, k, got in sweep[GEMM_DMA]:
        assert got == old_gemm(t, s, k, 24, 64 * 64), ("gemm_dma", t, s, k)
    for t, s, k, got in sweep[GEMM_X6]:
        assert got == old_gemm(t, s, k, 48, 128 * 128), ("gemm_x6", t, s, k)
    for t, s, k, got in sweep[CONV]:
        assert got == old_conv(t, s, k), ("conv", t, s, k)
    for t, s, k, got in sweep[ATTN]:
        assert got == old_attn_fwd(t, s, k) == old_attn_bwd(t, s, k), ("attention", t, s, k)
    for t in (1, 5, 700):
        assert plan(ATTN, t, 0, 11) == old_attn_bwd(t, 0, 11)
        assert plan(CONV, t, 0, 108) == old_conv(t, 0, 108)
    assert sum(p[0] for kind in (GEMM_DMA, GEMM_X6, CONV) for *_, p in sweep[kind]) > 40000  # the sweep does reach the split


def walk(kind, nkt, grid, chunk, nsplit, stride, units):
    """The kernels' walk of one split plan.  Run j belongs to the workgroup with bid % stride == 0 and bid / stride < nsplit; it is cut into
    segments [kt0, kt1) of successive tiles; a segment that is not a tile's whole k range is a piece and goes to slot 0 iff it holds the run's
    first unit; the merge of a tile takes run g's piece from slot 0 iff g * chunk >= tile * nkt."""
    bid = np.arange(grid, dtype=np.int64)
    assert int(((bid % stride == 0) & (bid // stride < nsplit)).sum()) == nsplit, "owners inside the grid"
    run = np.arange(nsplit, dtype=np.int64)
    start = run * chunk
    end = np.minimum(start + chunk, units)
    assert (start < end).all(), "an empty run"
    t0, t1 = start // nkt, (end - 1) // nkt
    nseg = t1 - t0 + 1
    r = np.repeat(run, nseg)                                   # one row per (run, tile) segment, in unit order
    tile = t0[r] + (np.arange(len(r)) - np.repeat(np.cumsum(nseg) - nseg, nseg))
    lo, hi = np.maximum(start[r], tile * nkt), np.minimum(end[r], (tile + 1) * nkt)
    assert lo[0] == 0 and hi[-1] == units and (lo[1:] == hi[:-1]).all() and (lo < hi).all(), "the k ranges are not covered exactly once"
    piece = ~((lo == tile * nkt) & (hi == (tile + 1) * nkt))
    slot = np.where(lo == start[r], 0, 1)
    pr, pt, ps = r[piece], tile[piece], slot[piece]
    assert len(np.unique(pr * 2 + ps)) == len(pr), "a run uses a slot twice"
    assert (ps == np.where(pr * chunk >= pt * nkt, 0, 1)).all(), "the producer's and the merge's slot rules differ"
    ntiles = units // nkt
    assert ntiles * nkt == units
    arrivals = np.bincount(pt, minlength=ntiles)
    tl = np.arange(ntiles, dtype=np.int64)
    g0, g1 = tl * nkt // chunk, (tl * nkt + nkt - 1) // chunk
    assert (g1 < nsplit).all()
    assert (arrivals[arrivals > 0] == (g1 - g0 + 1)[arrivals > 0]).all(), "a tile's counter does not see g1 - g0 + 1 arrivals"
    assert ((arrivals > 0) | (g0 == g1)).all(), "a tile without pieces must lie in one run"
    if kind == ATTN:
        assert nseg.max() <= 2, "the attention kernels number a run's segments 0, 1: a third would take the next run's slot"
    return len(pr)


def test_walk_invariants(sweep):
    seen, pieces = set(), 0
    for kind in (GEMM_DMA, GEMM_X6, CONV, ATTN):
        for t, s, k, (split, grid, whole_rounds, chunk, nsplit, stride, units, ws) in sweep[kind]:
            if not split:
                continue
            if kind == ATTN:
                stride = 1  # (the field holds the leftover tasks; every workgroup below nsplit owns a run)
                assert units == (t - whole_rounds * s) * k and grid == (s if whole_rounds else nsplit) and ws == nsplit * 2
            else:
                assert units // k <= COUNTERS, "more split tiles than arrival counters"
                assert units == (t - whole_rounds * grid) * k, "whole rounds and split tiles do not add up to the grid's tiles"
                assert ws == COUNTERS + nsplit * 2 * SLOT_FLOATS[kind]
                # gemm_workspace() = counters + CUs * 8 * 2 * 4096 floats, with slots = CUs * per_cu at the kind's cap
                assert (ws - COUNTERS) * PER_CU_CAP[kind] <= s * 8 * 2 * 4096, "the plan does not fit gemm_workspace()"
            assert nsplit <= grid <= s
            key = (kind == ATTN, k, grid, chunk, nsplit, stride, units)
            if key not in seen:
                seen.add(key)
                pieces += walk(kind, k, grid, chunk, nsplit, stride, units)
    assert pieces > 0
