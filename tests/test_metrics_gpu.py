"""evaluate_video(metrics="device") on MI355X: the kernels of csrc/metrics.hip alone through ctypes, then the public calls with the micro model.

Yardstick of the numeric gates: ``tests/metrics_ref.metrics_ref64`` (fp64 sums and terms from the float32 ``pred`` and ``gt``; pinned on the CPU by
tests/test_metrics_args_cpu.py).  u = 2^-24 is one float32 rounding.

  exact   medians, ``pred`` for "scale" / no alignment, valid counts, a1..a3, the splat images and TAS: equal to the host's, bit for bit
  GATE    abs_rel, sq_rel, rmse, TAE and the scale_shift scalars: 4 u relative to the fp64 value.  A term passes at most three float32 roundings
          (difference, square or quotient, quotient) before it enters an fp64 sum of non-negative terms, so the sum is within 3 u; the fp64
          sums, divide and square root add ~1e-16.  A mean absolute deviation passes one rounding per term and one of the mean: 2 u.
  rmse_log  the larger of (i) the host path's own distance from the yardstick on the same inputs and (ii) the bound that follows from HIP's
          documented logf error of 1 ulp: each term L = fl(logf(g) - logf(p)) is off by at most d = 2 u (|log g| + |log p|) + u |L|, its square
          by 2 |L| d + d^2 + u L^2, and the root of the mean moves by sqrt(m) - sqrt(m - D) with D the mean of those (computed from the data).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, synth
from endodav_amd import evaluate as ev
from tests.golden.make_golden import metrics_inputs
from tests.metrics_ref import errors_ref64, metrics_ref64, project64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GATE = 4 * U
CAP = 150.0


# ---- ctypes helpers -------------------------------------------------------------------------------------------------------------------------
def _st(cuda):
    return C.c_void_p(_lib.stream_ptr(cuda))


def _ws(n, h, w, cuda):
    return torch.empty(int(_lib.load().edv_metrics_workspace(n, h, w)), dtype=torch.uint8, device=cuda)


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def dev_median(x, gate, lo, hi, cuda, alias=False):
    """-> (median as np.float32, count); ``alias``: the gate IS x (one device buffer)."""
    lib = _lib.load()
    with torch.cuda.device(cuda):
        xd = _up(x, cuda)
        gd = xd if alias else _up(gate, cuda)
        out = torch.full((2,), -1.0, dtype=torch.float64, device=cuda)
        ws = _ws(0, 0, 0, cuda)
        _lib.check(lib.edv_masked_median(xd.data_ptr(), gd.data_ptr(), xd.numel(), lo, hi, out.data_ptr(), ws.data_ptr(), ws.numel(), _st(cuda)), "edv_masked_median")
        o = out.cpu().numpy()
    return np.float32(o[0]), int(o[1])


def dev_pred(disp, gt, align, cuda, factor=1.0, cap=CAP, min_depth=0.1, max_depth=150.0):
    """-> (pred [n, h, w] float32, scalars [8] fp64)"""
    lib = _lib.load()
    n, h, w = disp.shape
    with torch.cuda.device(cuda):
        dd, gd = _up(disp, cuda), _up(gt, cuda)
        pred = torch.full_like(dd, float("nan"))
        scal = torch.full((8,), -1.0, dtype=torch.float64, device=cuda)
        ws = _ws(n, h, w, cuda)
        _lib.check(lib.edv_metrics_pred(dd.data_ptr(), gd.data_ptr(), pred.data_ptr(), n, h, w, min_depth, max_depth, ev.ALIGN_MODES.get(align, 0), factor, cap,
                                        scal.data_ptr(), ws.data_ptr(), ws.numel(), _st(cuda)), "edv_metrics_pred")
        return pred.cpu().numpy(), scal.cpu().numpy()


def dev_errors(pred, gt, cuda, cap=CAP):
    lib = _lib.load()
    n, h, w = pred.shape
    with torch.cuda.device(cuda):
        pd, gd = _up(pred, cuda), _up(gt, cuda)
        out = torch.full((n, 8), -1.0, dtype=torch.float64, device=cuda)
        ws = _ws(n, h, w, cuda)
        _lib.check(lib.edv_metrics_errors(pd.data_ptr(), gd.data_ptr(), n, h, w, cap, out.data_ptr(), ws.data_ptr(), ws.numel(), _st(cuda)), "edv_metrics_errors")
        return out.cpu().numpy()


def _mats(i2ws):
    return np.stack([np.stack([m, np.linalg.inv(m)]) for m in i2ws]).astype(np.float64)


def dev_temporal(pred, gt, i2ws, cuda, cap=CAP):
    """-> (out [n - 1, 2] = (tae, tas), warp [n - 1, 2, h, w])"""
    lib = _lib.load()
    n, h, w = pred.shape
    with torch.cuda.device(cuda):
        pd, gd, md = _up(pred, cuda), _up(gt, cuda), _up(_mats(i2ws), cuda)
        out = torch.full((n - 1, 2), -1.0, dtype=torch.float64, device=cuda)
        warp = torch.full((n - 1, 2, h, w), float("nan"), dtype=torch.float32, device=cuda)
        ws = _ws(n, h, w, cuda)
        _lib.check(lib.edv_metrics_temporal(pd.data_ptr(), gd.data_ptr(), n, h, w, cap, md.data_ptr(), out.data_ptr(), warp.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _st(cuda)), "edv_metrics_temporal")
        return out.cpu().numpy(), warp.cpu().numpy()


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _odd_clip():
    """2 x 37 x 53: 3922 pixels, no multiple of 4 (one pixel per access), with rows below and above the range."""
    gt = synth.uniform("metrics:odd:gt", (2, 37, 53), 5.0, 120.0)
    gt[0, :2] = 0.0
    gt[1, -4:] = 170.0
    pred = (gt * synth.uniform("metrics:odd:noise", (2, 37, 53), 0.8, 1.3) + 1.0).astype(np.float32)
    disp = synth.uniform("metrics:odd:disp", (2, 37, 53), 0.0, 1.0)
    return dict(gt=gt, pred=pred, disp=disp)


def _wide_clip():
    """2 x 130 x 257 = 33410 pixels a frame: the per-frame reduction spans all of its blocks."""
    gt = synth.uniform("metrics:wide:gt", (2, 130, 257), 5.0, 120.0)
    gt[0, :5] = 0.0
    pred = (gt * synth.uniform("metrics:wide:noise", (2, 130, 257), 0.8, 1.3) + 1.0).astype(np.float32)
    return dict(gt=gt, pred=pred)


CLIPS = {"kat": metrics_inputs, "odd": _odd_clip, "wide": _wide_clip}


# ---- 1. the median --------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 4, 1000, 1001, 70001, 70002)


def _values(kind, m):
    if kind == "uniform":
        return synth.uniform(f"median:{m}", (m,), 5.0, 120.0)
    if kind == "equal":
        return np.full(m, 42.5, np.float32)
    rng = np.random.default_rng(m)
    if kind == "two":  # the middle pair straddles the two values when m is even: the mean of both
        v = np.where(np.arange(m) < m // 2, np.float32(1.0), np.float32(3.0)).astype(np.float32)
        return rng.permutation(v)
    pool = np.array([-1e30, -3.5, -1e-40, 0.0, 1e-40, 3e-39, 2.5, 1e30], dtype=np.float32)  # negative, zero, subnormal, huge
    v = pool[rng.integers(0, len(pool), size=m)]
    return np.where(rng.random(m) < 0.5, v, rng.standard_normal(m).astype(np.float32) * np.float32(1e-3)).astype(np.float32)


@pytest.mark.parametrize("kind", ["uniform", "equal", "two", "mixed"])
def test_median_is_np_median_bit_for_bit(cuda, kind):
    """Every count with the selected elements scattered among unselected ones (gate 0, 200 or NaN), at a total that is a multiple of 4
    (16-byte accesses) and at one that is not.  70001 / 70002 selected of ~93000 span many workgroups."""
    for m in COUNTS:
        vals = _values(kind, m)
        for pad_to4 in (True, False):
            total = m + m // 3 + 5
            total += (-total) % 4 if pad_to4 else (1 if total % 4 == 0 else 0)
            rng = np.random.default_rng(total)
            where = np.sort(rng.permutation(total)[:m])
            x = rng.standard_normal(total).astype(np.float32) * np.float32(50.0)  # what the gate rejects must not matter
            gate = rng.choice(np.array([0.0, 200.0, np.nan, 1e-3, 150.0], dtype=np.float32), size=total)
            x[where], gate[where] = vals, np.float32(7.0)
            sel = (gate > np.float32(1e-3)) & (gate < np.float32(150.0))
            assert sel.sum() == m
            want = np.median(x[sel])
            assert want.dtype == np.float32
            got, cnt = dev_median(x, gate, 1e-3, 150.0, cuda)
            assert cnt == m and _bits(got) == _bits(want), f"{kind} m={m} total={total}: device {got!r} numpy {want!r}"


def test_median_of_nothing_and_of_the_gate_itself(cuda):
    x = synth.uniform("median:none", (1001,), 5.0, 120.0)
    got, cnt = dev_median(x, np.zeros(1001, np.float32), 1e-3, 150.0, cuda)
    assert cnt == 0 and np.isnan(got)
    for total in (70003, 70004):  # x aliases gate: the median of the ground truth over its own valid range
        g = synth.uniform(f"median:alias:{total}", (total,), -10.0, 200.0)
        sel = (g > np.float32(1e-3)) & (g < np.float32(150.0))
        got, cnt = dev_median(g, None, 1e-3, 150.0, cuda, alias=True)
        assert cnt == sel.sum() and _bits(got) == _bits(np.median(g[sel]))


# ---- 2. the prediction ----------------------------------------------------------------------------------------------------------------------
def _host_pred(disp, gt, align, factor=1.0, cap=CAP):
    _, pred = ev.disp_to_depth(disp, 0.1, 150.0)
    extra = None
    if align == "scale":
        pred, extra = ev.median_scaling(gt, pred)
    elif align == "scale_shift":
        pred, *extra = ev.align_shift_and_scale(gt, pred)
    return np.clip(pred * factor, 1e-3, cap), extra


@pytest.mark.parametrize("clip", ["kat", "odd"])
def test_pred_scale_and_none_are_the_hosts_bits(cuda, clip):
    x = CLIPS[clip]()
    for align, factor, cap in (("scale", 1.0, CAP), ("none", 1.0, CAP), ("none", 17.0, 60.0), ("scale", 0.9, 40.0)):
        want, ratio = _host_pred(x["disp"], x["gt"], align, factor, cap)
        assert want.dtype == np.float32 and (cap == CAP or 0.02 < (want == np.float32(cap)).mean() < 0.98)  # the low caps clip a part
        got, scal = dev_pred(x["disp"], x["gt"], align, cuda, factor, cap)
        assert np.array_equal(_bits(got), _bits(want)), f"{clip} {align}: {np.count_nonzero(_bits(got) != _bits(want))} elements differ"
        if align == "scale":
            assert _bits(np.float32(scal[0])) == _bits(ratio) and scal[5] == ((x["gt"] > 1e-3) & (x["gt"] < 150)).sum()


def _align64(disp, gt):
    """The fp64 evaluation of align_shift_and_scale on the float32 depth: -> (depth fp32, [t_gt, s_gt, t_pred, s_pred] fp64)."""
    _, depth = ev.disp_to_depth(disp, 0.1, 150.0)
    valid = (gt > np.float32(1e-3)) & (gt < np.float32(150.0))
    g, p = gt[valid].astype(np.float64), depth[valid].astype(np.float64)
    t_gt, t_pred = float(np.median(gt[valid])), float(np.median(depth[valid]))
    return depth, np.array([t_gt, np.abs(g - t_gt).mean(), t_pred, np.abs(p - t_pred).mean()])


def check_scale_shift(disp, gt, got, scal, what):
    """Scalars: the medians are exact; a mean absolute deviation is 2 u from fp64 (gate 4 u).  pred = fl(fl(fl(fl(p - t_p) * q) + t_g) * factor)
    with q = fl(s_g / s_p) passes NINE roundings against the fp64 value r = (p - t_p) (s_g / s_p) + t_g: two in each of s_g, s_p, one in q, one in
    the difference and one in the product, all relative to A = |(p - t_p) q| (7 u A); the sum and the factor are relative to |r| (2 u |r|).
    The clip does not expand a difference."""
    depth, a64 = _align64(disp, gt)
    rel = np.abs(scal[1:5] - a64) / np.abs(a64)
    print(f"\n[{what}] scale_shift scalars vs fp64: {rel / U} u (t_gt, s_gt, t_pred, s_pred)")
    assert rel[0] == 0 and rel[2] == 0 and (rel <= GATE).all()
    t_gt, s_gt, t_pred, s_pred = a64
    A = (depth.astype(np.float64) - t_pred) * (s_gt / s_pred)
    r = A + t_gt
    ref = np.clip(r, float(np.float32(1e-3)), CAP)
    bound = U * (7 * np.abs(A) + 2 * np.abs(r)) * (1 + 2.0 ** -20)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"[{what}] scale_shift pred vs fp64: worst {np.max(err / bound):.3f} of the bound, {np.max(err / np.abs(ref)) / U:.2f} u relative")
    assert (err <= bound).all()


@pytest.mark.parametrize("clip", ["kat", "odd"])
def test_pred_scale_shift_within_the_rounding_bound(cuda, clip):
    x = CLIPS[clip]()
    got, scal = dev_pred(x["disp"], x["gt"], "scale_shift", cuda)
    check_scale_shift(x["disp"], x["gt"], got, scal, clip)
    host, _ = _host_pred(x["disp"], x["gt"], "scale_shift")
    print(f"[{clip}] device vs host pred: {np.max(np.abs(got - host) / np.abs(host)) / U:.2f} u")


# ---- 3. the errors --------------------------------------------------------------------------------------------------------------------------
def rmse_log_bound(gt, pred, valid):
    g, p = gt[valid].astype(np.float64), pred[valid].astype(np.float64)
    L = np.log(g) - np.log(p)
    d = 2 * U * (np.abs(np.log(g)) + np.abs(np.log(p))) + U * np.abs(L)
    m, D = (L * L).mean(), (2 * np.abs(L) * d + d * d + U * L * L).mean()
    return np.sqrt(m) - np.sqrt(max(m - D, 0.0))


def check_errors(dev, pred, gt, what, cap=CAP):
    """dev [n, 8] against the yardstick, frame by frame; prints the device's and the host path's distance for every metric."""
    valid = (gt > np.float32(1e-3)) & (gt < np.float32(cap))
    for i in range(len(gt)):
        ref = errors_ref64(gt[i], pred[i], valid[i])
        if ref[0] == 0:
            assert dev[i, 0] == 0 and np.isnan(dev[i, 1:]).all()
            continue
        host = np.array(ev.compute_errors(gt[i], pred[i], valid[i]), dtype=np.float64)
        d_dev, d_host = np.abs(dev[i, 1:] - ref[1:]) / ref[1:], np.abs(host - ref[1:]) / ref[1:]
        bound = rmse_log_bound(gt[i], pred[i], valid[i]) / ref[4]
        print(f"\n[{what} frame {i}] distance from fp64 in u, device | host: " + ", ".join(f"{n} {a / U:.3f} | {b / U:.3f}" for n, a, b in zip(ev.METRIC_NAMES, d_dev, d_host)))
        print(f"[{what} frame {i}] rmse_log gate: host's own distance {d_host[3] / U:.3f} u, bound from logf's 1 ulp {bound / U:.3f} u; device {d_dev[3] / U:.3f} u")
        assert dev[i, 0] == ref[0] and np.array_equal(dev[i, 5:], ref[5:]) and np.array_equal(dev[i, 5:], host[4:])
        assert (d_dev[:3] <= GATE).all(), d_dev[:3] / U
        assert d_dev[3] <= max(d_host[3], bound)


@pytest.mark.parametrize("clip", ["kat", "odd", "wide"])
def test_errors_match_fp64_restatement(cuda, clip):
    x = CLIPS[clip]()
    pred = np.clip(x["pred"], 1e-3, CAP)
    check_errors(dev_errors(pred, x["gt"], cuda), pred, x["gt"], clip)


def test_frame_without_a_valid_pixel_is_nan_and_skipped(cuda):
    x = _odd_clip()
    gt = np.concatenate([x["gt"], np.zeros_like(x["gt"][:1])])
    pred = np.concatenate([x["pred"], x["pred"][:1]])
    dev = dev_errors(pred, gt, cuda)
    assert dev[2, 0] == 0 and np.isnan(dev[2, 1:]).all() and np.isfinite(dev[:2]).all()
    item = {"depths": gt, "poses": np.stack([np.eye(4)] * 3), "Ks": np.stack([np.eye(4)] * 3)}
    disp = np.concatenate([x["disp"], x["disp"][:1]])
    rec = ev.clip_metrics_device(_up(disp, cuda), item, 0.1, 150.0, "scale", 1.0, CAP)
    want = ev.clip_metrics_host(disp, item, 0.1, 150.0, "scale", 1.0, CAP)
    assert len(rec["errors"]) == len(want["errors"]) == 2 and len(rec["temporal"]) == len(want["temporal"]) == 2
    assert rec["ratio"] == want["ratio"]
    assert np.isnan(rec["temporal"][1]).all() and np.isnan(want["temporal"][1]).all()


# ---- 4. the temporal metrics ----------------------------------------------------------------------------------------------------------------
def _K(h, w, f):
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = w / 2.0, h / 2.0
    return K


def _pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    P = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    P[0, 0], P[0, 2], P[2, 0], P[2, 2] = c, s, -s, c
    P[:3, 3] = tx, ty, tz
    return P


def temporal_case(name):
    """-> (depths [2, h, w] float32, gt [2, h, w] float32 that carries the masks, i2w [2, 4, 4])"""
    if name == "kat":  # 40 x 56, the first three rows masked
        x = metrics_inputs()
        depth = np.stack([x["depth_a"], x["depth_b"]])
        gt = np.full_like(depth, 10.0)
        gt[:, :3] = 0.0
        return depth, gt, np.stack([np.linalg.inv(x["K"] @ x["pose_a"]), np.linalg.inv(x["K"] @ x["pose_b"])])
    h, w = 37, 53
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = 30.0 + 6.0 * np.sin(xx / 7.0) + 4.0 * np.cos(yy / 5.0)
    depth = np.stack([smooth + synth.uniform(f"temporal:{name}:a", (h, w), -0.5, 0.5), smooth * 1.02 + synth.uniform(f"temporal:{name}:b", (h, w), -0.5, 0.5)]).astype(np.float32)
    gt = np.full_like(depth, 10.0)
    gt[0, -2:] = 0.0
    gt[1, :, :3] = 200.0
    K = _K(h, w, 45.0)
    pose_b = {"forward": _pose(0.31, -0.17, -11.0),       # the second camera 11 units further in: b -> a shrinks by a third and collides
              "behind": _pose(2.0, 0.7, -27.0, yaw=0.12),  # depths 20..41 against 27: part of frame a lies behind camera b, part leaves the image
              "apart": _pose(4000.0, 1.7, -2.3, yaw=0.01)}[name]  # no overlap at all
    return depth, gt, np.stack([np.linalg.inv(K @ np.eye(4)), np.linalg.inv(K @ pose_b)])


def temporal_preconditions(depth, gt, i2w):
    """Conditions on the INPUTS, from the fixed-order fp64 projection: the smallest distance of a projected coordinate from a half-integer among
    the points in front of the camera, and per direction (points in front and inside the image, distinct targets, points behind, points outside)."""
    valid = (gt > np.float32(1e-3)) & (gt < np.float32(CAP))
    h, w = depth.shape[1:]
    tie, stats = np.inf, []
    for s, t in ((0, 1), (1, 0)):
        _, u, v, z = project64(depth[s], valid[s], i2w[s], i2w[t])
        front = z > 1e-6
        for c in (u[front], v[front]):
            if c.size:
                tie = min(tie, np.abs(c - np.floor(c) - 0.5).min())
        ru, rv = np.rint(u), np.rint(v)
        inside = front & (ru >= 0) & (ru < w) & (rv >= 0) & (rv < h)
        stats.append((int(inside.sum()), len(set(zip(rv[inside].tolist(), ru[inside].tolist()))), int((~front).sum()), int((front & ~inside).sum())))
    return tie, stats


@pytest.mark.parametrize("name", ["kat", "forward", "behind", "apart"])
def test_temporal_splat_tas_and_tae(cuda, name):
    depth, gt, i2w = temporal_case(name)
    valid = (gt > np.float32(1e-3)) & (gt < np.float32(CAP))
    tie, stats = temporal_preconditions(depth, gt, i2w)
    landed, distinct = sum(s[0] for s in stats), sum(s[1] for s in stats)
    print(f"\n[{name}] nearest rounding tie {tie:.2e} px; per direction (landed, distinct targets, behind, outside): {stats}")
    assert tie > 1e-9  # BLAS and the fixed-order fp64 then agree on every target
    if name == "kat":
        assert [s[:2] for s in stats] == [(1920, 1885), (2072, 1952)]
    elif name == "forward":
        assert landed - distinct >= 0.25 * landed
    elif name == "behind":
        assert stats[0][2] > 100 and stats[0][3] > 100 and stats[0][0] > 20  # behind, outside, and some that land
    else:
        assert landed == 0
    out, warp = dev_temporal(depth, gt, i2w, cuda)
    a, b = (depth[0], valid[0], i2w[0]), (depth[1], valid[1], i2w[1])
    want_ab, want_ba = ev._splat(ev._lift(*a), valid[1], i2w[1]), ev._splat(ev._lift(*b), valid[0], i2w[0])
    assert np.array_equal(_bits(warp[0, 0]), _bits(want_ab)) and np.array_equal(_bits(warp[0, 1]), _bits(want_ba))
    if name == "apart":
        assert np.isnan(out).all()
        return
    _, ref = metrics_ref64(depth, gt, i2w)
    host_tae, host_tas = ev.tae(*a, *b), ev.tas(*a, *b)
    d_dev, d_host = abs(out[0, 0] - ref[0, 0]) / ref[0, 0], abs(float(host_tae) - ref[0, 0]) / ref[0, 0]
    print(f"[{name}] tae {out[0, 0]:.9f}: distance from fp64 in u, device {d_dev / U:.3f} | host {d_host / U:.3f}; tas {out[0, 1]:.9f}")
    assert out[0, 1] == host_tas == ref[0, 1]
    assert d_dev <= GATE


def test_temporal_chunks_of_pairs(cuda):
    """11 frames = 10 pairs = three chunks (4, 4, 2) that reuse one set of key images: every pair equals the same pair run alone."""
    da, ga, ia = temporal_case("forward")
    dk, gk, ik = temporal_case("behind")
    order = [0, 1, 0, 1, 1, 0, 0, 1, 0, 0, 1]
    depth = np.stack([(da if k % 2 == 0 else dk)[o] for k, o in enumerate(order)])
    gt = np.stack([(ga if k % 3 else gk)[o] for k, o in enumerate(order)])
    i2w = np.stack([(ia if k % 2 else ik)[o] for k, o in enumerate(order)])
    out, warp = dev_temporal(depth, gt, i2w, cuda)
    for k in range(10):
        one, w1 = dev_temporal(depth[k:k + 2], gt[k:k + 2], i2w[k:k + 2], cuda)
        assert np.array_equal(out[k], one[0], equal_nan=True) and np.array_equal(_bits(warp[k]), _bits(w1[0])), k


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_repeats_its_bits(cuda):
    x, wide = metrics_inputs(), _wide_clip()
    depth, gt, i2w = temporal_case("forward")
    g = synth.uniform("median:repeat", (70002,), -10.0, 200.0)
    runs = []
    for _ in range(2):
        pred, scal = dev_pred(x["disp"], x["gt"], "scale_shift", cuda)
        out, warp = dev_temporal(depth, gt, i2w, cuda)
        runs.append([np.float64(dev_median(g, None, 1e-3, 150.0, cuda, alias=True)[0]), pred, scal, dev_errors(wide["pred"], wide["gt"], cuda), out, warp])
    for a, b in zip(*runs):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


class _EndToEnd:
    def __init__(self, cuda):
        m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
        synth.fill_module_(m)
        self.model = m.to(cuda)
        self.ds = ev.SyntheticVideos(n_clips=2, n_frames=40, height=NET_H, width=NET_W)  # two windows a clip
        self.items = [self.ds[c] for c in range(2)]
        self.disp_dev = [self.model.infer_video_depth(i["colors"], device="cuda:0", stitch="device", output="device") for i in self.items]


@pytest.fixture(scope="module")
def e2e(cuda):
    return _EndToEnd(cuda)


def _i2ws(item):
    return np.stack([np.linalg.inv(K @ pose) for K, pose in zip(item["Ks"], item["poses"])])


def test_device_output_is_the_host_output(cuda, e2e):
    for item, dev in zip(e2e.items, e2e.disp_dev):
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32 and dev.shape == (40, NET_H, NET_W)
        host = e2e.model.infer_video_depth(item["colors"], device="cuda:0", stitch="device", output="host")
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(dev.cpu().numpy()), _bits(host))


class _Tilted:
    """The same clips seen by a camera that also drifts in y and z and turns a little.  SyntheticVideos' own camera moves along x alone, so
    every point projects to y + 0.5 up to rounding noise -- an exact rounding tie; here no coordinate is near one, and any order of the dot
    products gives the same targets."""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, c):
        item = dict(self.ds[c])
        poses = item["poses"].copy()
        for k in range(len(poses)):
            poses[k] = _pose(0.05 * k, 0.031 * k, -0.043 * k, yaw=0.0007 * k)
        item["poses"] = poses
        return item


def _evaluate_both(e2e, ds, align):
    kw = dict(depth_align=align, device="cuda:0")
    host = ev.evaluate_video(e2e.model, ds, metrics="host", stitch="device", **kw)
    dev = ev.evaluate_video(e2e.model, ds, metrics="device", **kw)
    for key in ("errors", "temporal", "ratios", "aligns", "inference_times"):
        assert dev[key].shape == host[key].shape, key
    return host, dev


def _pair_ties(pred, item):
    """Smallest distance from a rounding tie over the pairs of a clip (temporal_preconditions)."""
    i2ws = _i2ws(item)
    return min(temporal_preconditions(pred[k:k + 2], item["depths"][k:k + 2], i2ws[k:k + 2])[0] for k in range(len(pred) - 1))


def test_evaluate_video_on_the_device_scale(cuda, e2e):
    host, dev = _evaluate_both(e2e, e2e.ds, "scale")
    assert dev["errors"].shape == (80, 7) and dev["temporal"].shape == (78, 2)
    assert np.array_equal(dev["errors"][:, 4:], host["errors"][:, 4:])
    assert np.array_equal(dev["ratios"], host["ratios"])
    # the other columns against the yardstick on the host's prediction, which is the device's bit for bit (items 3 and 4)
    for c, (item, disp) in enumerate(zip(e2e.items, e2e.disp_dev)):
        pred, _ = _host_pred(disp.cpu().numpy(), item["depths"], "scale")
        rows = np.concatenate([np.zeros((40, 1)), dev["errors"][40 * c:40 * c + 40]], axis=1)
        rows[:, 0] = ((item["depths"] > 1e-3) & (item["depths"] < CAP)).sum(axis=(1, 2))
        check_errors(rows, pred, item["depths"], f"clip {c}")
        _, ref = metrics_ref64(pred, item["depths"], _i2ws(item))
        got = dev["temporal"][39 * c:39 * c + 39]
        rel = np.abs(got[:, 0] - ref[:, 0] * 100.0) / (ref[:, 0] * 100.0)
        print(f"\n[clip {c}] tae vs fp64: worst {rel.max() / U:.3f} u; host {np.max(np.abs(host['temporal'][39 * c:39 * c + 39, 0] - ref[:, 0] * 100.0) / (ref[:, 0] * 100.0)) / U:.3f} u")
        assert (rel <= GATE + 2.0 ** -52).all()  # x 100 in fp64: one more rounding of 2^-53
        assert np.array_equal(got[:, 1], ref[:, 1])  # TAS against the fixed-order projection of the yardstick


def test_evaluate_video_tas_equals_the_hosts(cuda, e2e):
    """On SyntheticVideos(n_clips=2, n_frames=40) the device's TAS equals the host's, although the dataset's camera moves along x alone and
    every point therefore projects to y + 0.5 up to rounding noise: all of them sit ON a rounding tie (distance 0.0 px, printed below), the case
    the kernel tests exclude by their precondition.  The tie falls with the noise of the dot products, so the kernel forms them as the host's
    dgemm does: the first product rounded, then one fused multiply-add per term, left to right (dot4 in csrc/metrics.hip; measured on two x86
    hosts, ``pts @ M.T`` equals that chain entry for entry and an unfused chain in 3 of 4).  With unfused products the device differed from the
    host in 78 of 78 pairs here, by up to 1.34e-2."""
    host, dev = _evaluate_both(e2e, e2e.ds, "scale")
    for c, (item, disp) in enumerate(zip(e2e.items, e2e.disp_dev)):
        pred, _ = _host_pred(disp.cpu().numpy(), item["depths"], "scale")
        print(f"\n[clip {c}] nearest rounding tie {_pair_ties(pred, item):.2e} px")
    diff = np.abs(dev["temporal"][:, 1] - host["temporal"][:, 1])
    print(f"TAS device vs host: {np.count_nonzero(diff)} of {diff.size} pairs differ, by at most {diff.max():.2e}")
    assert np.array_equal(dev["temporal"][:, 1], host["temporal"][:, 1])


def test_evaluate_video_tas_equals_the_hosts_off_the_ties(cuda, e2e):
    ds = _Tilted(e2e.ds)
    for c in range(2):
        pred, _ = _host_pred(e2e.disp_dev[c].cpu().numpy(), ds[c]["depths"], "scale")
        tie = _pair_ties(pred, ds[c])
        print(f"\n[tilted clip {c}] nearest rounding tie {tie:.2e} px")
        assert tie > 1e-9
    host, dev = _evaluate_both(e2e, ds, "scale")
    assert np.array_equal(dev["temporal"][:, 1], host["temporal"][:, 1]) and np.array_equal(dev["errors"][:, 4:], host["errors"][:, 4:])
    rel = np.abs(dev["temporal"][:, 0] - host["temporal"][:, 0]) / host["temporal"][:, 0]
    print(f"[tilted] tae device vs host: worst {rel.max() / U:.2f} u")


def test_evaluate_video_on_the_device_scale_shift(cuda, e2e):
    """The host's deviations are float32 sums, so its prediction is not the device's: the device's own prediction is held to item 2's bound, and
    its metrics to the yardstick evaluated on that prediction."""
    host, dev = _evaluate_both(e2e, e2e.ds, "scale_shift")
    assert dev["aligns"].shape == (2, 4) and dev["ratios"].shape == (0,)
    for c, (item, disp) in enumerate(zip(e2e.items, e2e.disp_dev)):
        d = disp.cpu().numpy()
        pred, scal = dev_pred(d, item["depths"], "scale_shift", cuda)
        check_scale_shift(d, item["depths"], pred, scal, f"clip {c}")
        assert np.array_equal(dev["aligns"][c], scal[1:5])
        rec = ev.clip_metrics_device(disp, item, 0.1, 150.0, "scale_shift", 1.0, CAP)
        assert np.array_equal(np.array(rec["errors"]), dev["errors"][40 * c:40 * c + 40]) and np.array_equal(np.array(rec["temporal"]), dev["temporal"][39 * c:39 * c + 39])
        rows = np.concatenate([np.zeros((40, 1)), dev["errors"][40 * c:40 * c + 40]], axis=1)
        rows[:, 0] = ((item["depths"] > 1e-3) & (item["depths"] < CAP)).sum(axis=(1, 2))
        check_errors(rows, pred, item["depths"], f"clip {c} scale_shift")
        _, ref = metrics_ref64(pred, item["depths"], _i2ws(item))
        got = dev["temporal"][39 * c:39 * c + 39]
        assert np.array_equal(got[:, 1], ref[:, 1])
        assert (np.abs(got[:, 0] - ref[:, 0] * 100.0) / (ref[:, 0] * 100.0) <= GATE + 2.0 ** -52).all()
