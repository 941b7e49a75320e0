"""Inputs shared by tests/test_track_scale_cpu.py and tests/test_track_scale_gpu.py: the scene of tests/track_cases.py with its live depth in
another unit than the volume's, one frame or a clip whose unit drifts, and where the 29 sums of the 6-column system lie among the 37."""
import functools

import numpy as np

from tests import track_cases as tc

SCALES = (1.0, 1.02, 1.05, 0.9)   # the live depth is the scene's divided by s: the tracker has to find sigma = s
DRIFT = 1.02                      # frame i of the clip is divided by DRIFT**i

# The 37 sums: J_j*J_k for 0 <= j <= k <= 6 row-major (28), J_j*e (7), e*e, 1.  The 6-column sums hold the same products for j <= k <= 5 in the
# same order (21), J_j*e for j <= 5 (6), e*e, 1: position i of the 29 is position SHARED[i] of the 37.
SHARED = [t for t, (j, k) in enumerate((j, k) for j in range(7) for k in range(j, 7)) if k <= 5] + [28, 29, 30, 31, 32, 33] + [35, 36]
NEW = [6, 12, 17, 21, 24, 26, 27, 34]   # J_0*J_6 .. J_6*J_6 and J_6*e: what the seventh column adds
assert SHARED == [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 15, 16, 18, 19, 20, 22, 23, 25, 28, 29, 30, 31, 32, 33, 35, 36]
assert sorted(SHARED + NEW) == list(range(37))


@functools.lru_cache(maxsize=None)
def single(s):
    """(live depth [1, H, W] of ``tc.single()`` divided by s, true pose); the guess is the identity and the scale to find is s."""
    live, truth = tc.single()
    scaled = (live / s).astype(np.float32)
    scaled.setflags(write=False)
    return scaled, truth


@functools.lru_cache(maxsize=None)
def clip(drift=DRIFT):
    """(depth [5, H, W], true poses [5, 4, 4], true scales [5]) of ``tc.clip()`` with frame i divided by drift**i."""
    depth, truth = tc.clip()
    scales = np.array([drift ** i for i in range(5)])
    drifting = np.stack([(depth[i] / scales[i]).astype(np.float32) for i in range(5)])
    drifting.setflags(write=False)
    return drifting, truth, scales


def same_tracked(got, want):
    """Two ``Tracked`` with scales, bit for bit."""
    assert got.poses.shape == want.poses.shape and np.array_equal(tc.bits(got.poses), tc.bits(want.poses))
    assert got.pairs.dtype == np.int64 and np.array_equal(got.pairs, want.pairs)
    assert np.array_equal(tc.bits(got.rms), tc.bits(want.rms))
    assert got.lost.dtype == np.bool_ and np.array_equal(got.lost, want.lost)
    assert got.scales is not None and want.scales is not None and got.scales.dtype == np.float64 and got.scales.shape == want.scales.shape
    assert np.array_equal(tc.bits(got.scales), tc.bits(want.scales))
