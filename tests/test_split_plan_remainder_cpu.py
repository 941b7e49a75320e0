"""The remainder plan of the bf16 x 6 GEMM (csrc/streamk_plan.hpp: plan_remainder, through edv_split_plan kinds 4 and 5), on the CPU: a grid a
few tiles past a whole number of rounds of CUs splits only those tiles along k and starts their pieces first.  The invariants are those of
test_split_plan_cpu.py::walk, restated for this walk (the run owners are the raw block indices below nsplit, which is that walk at stride 1):

1. whole tiles + split tiles = tiles, and the whole-tile blocks map onto the whole tiles one to one;
2. the runs cover [0, units) exactly once, a run leaves at most two pieces in distinct slots, the producer's and the merge's slot rules agree,
   a tile's counter sees exactly its number of pieces;
3. the counters and slots fit gemm_workspace().

The EDV_X6_* planner knobs must be unset (the policies read them once per process)."""
import ctypes as C
import os

import numpy as np
import pytest

from .test_split_plan_cpu import COUNTERS, GEMM_X6, walk

REMAINDER, WHOLE_TILE = 4, 5
CUS = (1, 2, 7, 8, 32, 256, 304)
WGS = (1, 2, 3)
NKT = (3, 4, 5, 7, 8, 12, 23, 24, 25, 47, 48, 96)
SLOT_FLOATS = 128 * 128
KNOBS = ("EDV_X6_SPLIT_MIN_KT",)


def tiles_of(cus):
    """Every count from one round to past four rounds for the small parts; for the large ones every count near a whole number of rounds and a
    stride through the rest."""
    if cus <= 32:
        return tuple(range(1, 4 * cus + 3))
    near = [r * cus + d for r in (1, 2, 3, 4, 7) for d in range(-2, 24)]
    return tuple(sorted(set(near) | set(range(1, 5 * cus, 37))))


@pytest.fixture(scope="module")
def plan(lib):
    assert not [k for k in KNOBS if k in os.environ], "the planner knobs must be unset for this test"
    out = (C.c_int64 * 8)()

    def call(tiles, cus, wgs, nkt, mode):
        out[0], out[1] = wgs, mode
        assert lib.edv_split_plan(REMAINDER, tiles, cus, nkt, out) == 0
        return tuple(out)

    return call


@pytest.fixture(scope="module")
def sweep(plan):
    return [(t, c, w, k, mode, plan(t, c, w, k, mode)) for mode in (1, 2) for c in CUS for w in WGS for k in NKT for t in tiles_of(c)]


def test_where_the_plan_applies(sweep, plan):
    taken = {1: 0, 2: 0}
    for t, c, w, k, mode, (rem, *rest) in sweep:
        left = t % c
        if mode == 2:  # wherever the walk is supported
            assert rem == (t >= c and left > 0), (t, c, w, k)
        else:          # by policy: a few tiles past a round, and the whole grid resident at once
            units, cap = left * k, c * min(w, 2)
            chunk = max(3, k // 6, -(-units // cap))
            assert rem == (t >= c and 0 < left and left * 16 <= c and (t - left) + -(-units // chunk) <= c * w), (t, c, w, k)
        if not rem:
            assert rest == [0] * 7
        taken[mode] += rem
    assert taken[1] > 200 and taken[2] > 10000  # the sweep does reach the plan
    # the headline launches (ViT-S, 518^2, T = 8: 86 row tiles) on 256 CUs x 2: proj takes it, and fc2 (96 k-tiles), whose stream-K plan would cut all
    # 258 tiles; qkv and fc1 are more than one wave of resident workgroups and stay plain
    assert [plan(t, 256, 2, k, 1)[0] for t, k in ((258, 24), (774, 24), (1032, 24), (258, 96))] == [1, 0, 0, 1]
    # ViT-B (T = 16: 172 row tiles, 48 and 192 k-tiles) and ViT-L (64 and 256 k-tiles) keep the plans they had
    for n_tiles, kts in (((6, 18, 24), (48, 192)), ((8, 24, 32), (64, 256))):
        assert not any(plan(172 * n, 256, 2, k, 1)[0] for n in n_tiles for k in kts)


def test_walk_invariants(sweep, lib):
    out = (C.c_int64 * 8)()
    seen, grids, pieces = set(), set(), 0
    for t, c, w, k, mode, (rem, grid, first_split, chunk, nsplit, split_tiles, units, ws) in sweep:
        if not rem:
            continue
        assert split_tiles == t % c and first_split + split_tiles == t, "whole tiles and split tiles do not add up"
        assert units == split_tiles * k and grid == nsplit + first_split
        assert chunk >= 3 and nsplit == -(-units // chunk)
        assert split_tiles <= COUNTERS, "more split tiles than arrival counters"
        assert nsplit <= c * w, "a run that is not resident in the first wave of the dispatch"
        assert ws == COUNTERS + nsplit * 2 * SLOT_FLOATS
        assert ws - COUNTERS <= c * 8 * 2 * 4096, "the plan does not fit gemm_workspace() = counters + CUs * 8 * 2 * 4096 floats"
        key = (k, chunk, nsplit, units)
        if key not in seen:  # the run owners are the first nsplit raw block indices: walk's rule at stride 1
            seen.add(key)
            pieces += walk(GEMM_X6, k, grid, chunk, nsplit, 1, units)
        if (grid, nsplit) not in grids and grid <= 2000:
            grids.add((grid, nsplit))
            got = []
            for b in range(nsplit, grid):
                assert lib.edv_split_plan(WHOLE_TILE, b, grid, nsplit, out) == 0
                got.append(out[0])
            got = np.array(got)
            assert (np.sort(got) == np.arange(first_split)).all(), "the whole-tile blocks do not map onto the whole tiles one to one"
            xcd = np.arange(nsplit, grid) & 7  # blocks b and b + 8 share an XCD: each XCD gets one contiguous, ascending run of tiles
            for x in range(8):
                mine = got[xcd == x]
                assert len(mine) == 0 or (np.diff(mine) == 1).all()
    assert pieces > 0 and len(grids) > 100
