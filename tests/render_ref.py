"""Yardstick of the device rendering (tests/test_render_cpu.py pins it, tests/test_render_gpu.py uses it): a numpy restatement of the
reference's colouring lines -- utils/eval_utils.py:284-295 ``save_video``, evaluate_depth_video.py:32-36 ``render_depth`` and the robust
range of test_simple.py:156-167 -- with every scalar an explicit ``np.float32``, so that it does not depend on numpy's promotion rules.

  den = (hi - lo) + eps;  t = (x - lo) / den;  clip: t = np.clip(t, 0, 1);  idx = (t * 255).astype(uint8);  out = table[idx]

Where the reference would divide 0 by 0 (a constant frame under "frame") the index is 0.  "quantile" takes the order statistics
``np.sort(frame.ravel())[floor(q * (m - 1))]``: ``np.percentile(frame, 100 q, method="lower")``."""
import math

import numpy as np

F32 = np.float32


def ranges_ref(x, norm, lo=None, hi=None, q=(0.0, 0.95)):
    """x float32 [n, h, w] -> (lo, hi) per frame, float32 [n, 2]."""
    x = np.asarray(x, F32)
    n = x.shape[0]
    flat = x.reshape(n, -1)
    if norm == "video":
        return np.tile(np.array([x.min(), x.max()], F32), (n, 1))
    if norm == "frame":
        return np.stack([flat.min(axis=1), flat.max(axis=1)], axis=1).astype(F32)
    if norm == "fixed":
        return np.tile(np.array([lo, hi], F32), (n, 1))
    assert norm == "quantile"
    m = flat.shape[1]
    r_lo, r_hi = int(math.floor(float(q[0]) * (m - 1))), int(math.floor(float(q[1]) * (m - 1)))
    s = np.sort(flat, axis=1)
    return np.stack([s[:, r_lo], s[:, r_hi]], axis=1).astype(F32)


def index_ref(frame, lo, hi, eps, clip):
    """One frame -> uint8 indices, the arithmetic of the module docstring in float32."""
    frame = np.asarray(frame, F32)
    lo, hi, eps = F32(lo), F32(hi), F32(eps)
    den = F32(F32(hi - lo) + eps)
    if den == 0:
        return np.zeros(frame.shape, np.uint8)
    t = (frame - lo) / den
    assert t.dtype == F32
    if clip:
        t = np.clip(t, F32(0), F32(1))
    s = t * F32(255.0)
    assert s.dtype == F32 and s.min() >= 0 and s.max() < 256  # inside uint8: the cast below is a plain truncation
    return s.astype(np.uint8)


EPS = {"video": F32(1e-6), "frame": F32(0), "fixed": F32(0), "quantile": F32(0)}
CLIP = {"video": False, "frame": False, "fixed": True, "quantile": True}


def colorize_ref(x, norm, table, lo=None, hi=None, q=(0.0, 0.95), frames=None):
    """x float32 [n, h, w], table uint8 [256, 3] -> uint8 [n, h, w, 3]; with ``frames`` uint8 [n, h, w, 3]: [n, h, 2w, 3], frame | colour."""
    x = np.asarray(x, F32)
    table = np.asarray(table)
    assert table.dtype == np.uint8 and table.shape == (256, 3)
    rng = ranges_ref(x, norm, lo, hi, q)
    out = np.stack([table[index_ref(f, r[0], r[1], EPS[norm], CLIP[norm])] for f, r in zip(x, rng)])
    return out if frames is None else np.concatenate([np.asarray(frames), out], axis=2)
