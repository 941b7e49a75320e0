"""Inputs shared by tests/test_track_robust_cpu.py and tests/test_track_robust_gpu.py: the single-frame scene of tests/track_cases.py with a block
of the live frame (rows 8..21, columns 30..49: 12.5 % of the pixels) spoilt in two ways, and the options of the robust tracker used on them."""
import functools

import numpy as np

from tests import track_cases as tc

HUBER, MIN_COS, HUBER_COLOUR = 0.005, 0.985, 8.0     # a third of a voxel; some 10 degrees; eight levels of 255
ROWS, COLS = slice(8, 22), slice(30, 50)
SHIFT = 0.04                                        # the block comes nearer by this: inside ``max_dist`` = 0.1, so every pair passes the distance test
TILT = 0.006                                        # depth per pixel along x of the plane that replaces the block

# every combination of the two geometric options, named
OPTIONS = {"plain": {}, "huber": dict(huber=HUBER), "normals": dict(min_cos=MIN_COS), "both": dict(huber=HUBER, min_cos=MIN_COS)}


@functools.lru_cache(maxsize=None)
def scene(kind="untouched"):
    """(live depth float32 [1, H, W], true pose): ``tc.single()`` as it is, or with the block changed.
    "shift": the block's depth minus 0.04.  "tilt": the block replaced by the plane z = z[15, 40] + 0.006 * (x + 0.5 - 40)."""
    live, truth = tc.single()
    live = live.copy()
    if kind == "shift":
        live[0, ROWS, COLS] -= np.float32(SHIFT)
    elif kind == "tilt":
        x = np.arange(COLS.start, COLS.stop)
        live[0, ROWS, COLS] = (live[0, 15, 40] + TILT * (x + 0.5 - 40)).astype(np.float32)[None, :]
    elif kind != "untouched":
        raise ValueError(kind)
    live.setflags(write=False)
    return live, truth


def ubits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
