"""Yardstick of the device metrics (tests/test_metrics_args_cpu.py pins it, tests/test_metrics_gpu.py uses it): ``metrics_ref64``, an fp64
restatement of ``evaluate.compute_errors`` / ``tae`` / ``tas`` that works from the float32 ``pred`` and ``gt``.

Every sum and every term that enters a sum is fp64.  What is a DECISION rather than a sum stays as the host makes it: the delta < 1.25^k tests
on the float32 ratio, and the splat image, which is float32 on the host (``_splat`` writes z into a float32 array).  The splat's target
coordinates come from fp64 arithmetic in a fixed left-to-right order, one fused multiply-add per term (``project64``): the chain the kernel
uses, restated here with an exact software FMA (``fma64``), not taken from BLAS."""
import numpy as np

MIN_DEPTH = np.float32(1e-3)
EPS = 1e-6


def errors_ref64(gt, pred, valid):
    """-> [count, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3] in fp64; NaN where there is no valid pixel."""
    g32, p32 = gt[valid], pred[valid]
    n = g32.size
    if n == 0:
        return np.array([0.0] + [np.nan] * 7)
    ratio = np.maximum(g32 / p32, p32 / g32)  # float32, as the host decides it
    acc = [np.count_nonzero(ratio < np.float32(1.25 ** k)) / n for k in (1, 2, 3)]
    g, p = g32.astype(np.float64), p32.astype(np.float64)
    d = g - p
    return np.array([n, (np.abs(d) / g).sum() / n, (d * d / g).sum() / n, np.sqrt((d * d).sum() / n), np.sqrt(((np.log(g) - np.log(p)) ** 2).sum() / n)] + acc)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    c = 134217729.0  # 2^27 + 1: Veltkamp's split
    ah = c * a
    ah = ah - (ah - a)
    al = a - ah
    bh = c * b
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64(a, b, c):
    """RN(a * b + c) on float64 arrays, exactly (Boldo & Melquiond: error-free product and sums, the small parts added with rounding to odd)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    z, e = _two_sum(tl, vl)
    fix = ((z.view(np.int64) & 1) == 0) & (e != 0)
    z = np.where(fix, np.nextafter(z, np.where(e > 0, np.inf, -np.inf)), z)
    return vh + z


def _dot4(m, j, X, Y, Z):
    """Row j of m times (X, Y, Z, 1), left to right, one fused multiply-add per term: the kernel's chain."""
    return fma64(1.0, m[j, 3], fma64(Z, m[j, 2], fma64(Y, m[j, 1], X * m[j, 0])))


def project64(depth, mask, i2w_src, i2w_dst):
    """Masked pixels of the source, lifted and projected into the target: -> (row-major source indices, x / z, y / z, z), fp64, every dot product
    a left-to-right chain of fused multiply-adds.  Points with z <= 1e-6 are kept (their coordinates are x / 1e-6, as on the host) so the caller sees them."""
    h, w = depth.shape
    idx = np.flatnonzero(mask.ravel())
    d = depth.ravel()[idx].astype(np.float64)
    X, Y = ((idx % w) + 0.5) * d, ((idx // w) + 0.5) * d
    wx, wy, wz = (_dot4(i2w_src, j, X, Y, d) for j in range(3))
    inv = np.linalg.inv(i2w_dst)
    qx, qy, z = (_dot4(inv, j, wx, wy, wz) for j in range(3))
    zc = np.maximum(z, EPS)
    return idx, qx / zc, qy / zc, z


def splat64(depth, mask, i2w_src, mask_dst, i2w_dst):
    """``evaluate._splat(evaluate._lift(...))`` with ``project64``'s coordinates: float32 image, later points overwrite earlier ones."""
    h, w = mask_dst.shape
    idx, u, v, z = project64(depth, mask, i2w_src, i2w_dst)
    u, v = np.rint(u), np.rint(v)
    ok = (z > EPS) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    out = np.zeros((h, w), dtype=np.float32)
    out[v[ok].astype(np.int64), u[ok].astype(np.int64)] = z[ok]
    return out * mask_dst


def pair_ref64(depth_a, mask_a, i2w_a, depth_b, mask_b, i2w_b):
    """-> (tae, tas) of one pair in fp64 (tae not x 100); NaN where a direction has no overlap."""
    e = []
    for (ds, ms, ws, dt, mt, wt) in ((depth_a, mask_a, i2w_a, depth_b, mask_b, i2w_b), (depth_b, mask_b, i2w_b, depth_a, mask_a, i2w_a)):
        warp = splat64(ds, ms, ws, mt, wt)
        m = (warp > np.float32(EPS)) & mt
        t32, w32 = dt[m], warp[m]
        if t32.size == 0:
            e.append((np.nan, np.nan))
            continue
        t, wv = t32.astype(np.float64), w32.astype(np.float64)
        e.append(((np.abs(t - wv) / t).sum() / t.size, np.count_nonzero(np.maximum(t32 / w32, w32 / t32) < np.float32(1.25)) / t.size))
    return 0.5 * (e[0][0] + e[1][0]), 0.5 * (e[0][1] + e[1][1])


def metrics_ref64(pred, gt, i2ws, eval_max_depth=150.0):
    """pred, gt: float32 [n, h, w]; i2ws: [n, 4, 4] fp64 (inv(K @ pose)).  -> (errors [n, 8], temporal [n - 1, 2])."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    valid = (gt > MIN_DEPTH) & (gt < np.float32(eval_max_depth))
    errors = np.stack([errors_ref64(g, p, v) for g, p, v in zip(gt, pred, valid)])
    temporal = [pair_ref64(pred[i], valid[i], i2ws[i], pred[i + 1], valid[i + 1], i2ws[i + 1]) for i in range(len(pred) - 1)]
    return errors, np.array(temporal, dtype=np.float64).reshape(len(pred) - 1, 2)
