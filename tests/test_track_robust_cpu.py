"""CPU: robust camera tracking (``fusion.Track(min_cos=..., huber=..., huber_colour=...)``) on the numpy mirror and at the C boundary (the refusals
of ``edv_frame_normals`` and ``edv_icp_robust_sums`` launch nothing, so they need no GPU).  The GPU tests hold the kernels to this mirror bit for
bit (tests/test_track_robust_gpu.py); what the rule computes and what the tracker gains from it is checked here alone."""
import ctypes as C
import math

import numpy as np
import pytest

from endodav_amd import _lib, fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Track
from tests import track_cases as tc
from tests import track_colour_cases as cc
from tests import track_robust_cases as rc
from tests.test_track_colour_cpu import _colour_at, _y

T6, T7 = 29, 37


# ---- 1. the live normals on known answers -------------------------------------------------------------------------------------------------------
def test_a_fronto_parallel_plane():
    depth = np.full((2, tc.H, tc.W), 0.6, np.float32)
    for step in (1, 3):
        got = fusion.frame_normals_host(depth, tc.spec(step=step))
        oh, ow = -(-tc.H // step), -(-tc.W // step)
        assert got.shape == (2, oh, ow, 3) and got.dtype == np.float32
        inner = got[:, 1:-1, 1:-1]
        assert (inner[..., 0] == 0.0).all() and (inner[..., 1] == 0.0).all() and (inner[..., 2] == -1.0).all()    # towards the camera, exactly
        border = np.ones((oh, ow), bool)
        border[1:-1, 1:-1] = False
        assert np.array_equal(rc.ubits(got[:, border]), np.zeros((2, int(border.sum()), 3), np.uint32))         # +0, every one


def test_a_plane_tilted_about_y():
    """The plane Z = z0 + s X seen through K = (f, f, cx, cy): z(u) = z0 / (1 - s (u - cx) / f), and its normal towards the camera is
    (s, 0, -1) / sqrt(1 + s^2) everywhere.  Central differences of points on a plane give it exactly; what is left is the rounding of z to
    float32, half an ulp of at most 1.2e-7 (z < 1.2) at either end of a baseline 2 z / f >= 0.2 (f = 6, z >= 0.6): 3.2e-7 of angle along x and
    as much along y, and 3e-8 for the float32 result: below the 1e-6 asked."""
    f, s, z0 = 6.0, 0.1, 0.6
    K = np.array([[f, 0.0, 28.0], [0.0, f, 20.0], [0.0, 0.0, 1.0]])
    u = np.arange(tc.W) + 0.5
    z = np.broadcast_to(z0 / (1.0 - s * (u - 28.0) / f), (1, tc.H, tc.W)).astype(np.float32)
    assert 0.3 < z.min() and z.max() < 1.2
    got = fusion.frame_normals_host(z, Cloud(K=K, source="depth", far=10.0))
    want = np.array([s, 0.0, -1.0]) / math.sqrt(1.0 + s * s)
    worst = np.abs(got[0, 1:-1, 1:-1].astype(np.float64) - want).max()
    print(f"\nthe worst component is {worst:.3e} from the analytic normal")
    assert worst <= 1.0e-6
    assert not got[0, 0].any() and not got[0, :, 0].any() and not got[0, -1].any() and not got[0, :, -1].any()


def test_a_hole_zeroes_itself_and_its_four_neighbours():
    live, _ = tc.single()
    whole = fusion.frame_normals_host(live, tc.spec())
    length = np.linalg.norm(whole[0].astype(np.float64), axis=-1)
    assert ((length == 0.0) | (np.abs(length - 1.0) <= 1.0e-7)).all() and (length[5:-5, 5:-5] > 0.0).all()     # unit or none, and none missing in the middle
    for bad in (0.0, np.nan, np.inf, -1.0, 20.0):                         # 20 is beyond ``far``
        holed = live.copy()
        holed[0, 12, 33] = bad
        got = fusion.frame_normals_host(holed, tc.spec())
        gone = ~got[0].any(axis=-1) & whole[0].any(axis=-1)
        want = np.zeros((tc.H, tc.W), bool)
        want[12, 33] = want[12, 32] = want[12, 34] = want[11, 33] = want[13, 33] = True
        assert np.array_equal(gone, want), bad
        assert np.array_equal(rc.ubits(got[0][~want]), rc.ubits(whole[0][~want]))                              # and nothing else moved


def _normals_one_by_one(depth, spec):
    """The rule applied to one pixel at a time in Python floats (float32 for the depth rule), independent of the vectorised mirror."""
    n, h, w = depth.shape
    step = int(spec.step)
    oh, ow = -(-h // step), -(-w // step)
    lo, span, gain, near, far = spec.scalars()
    mask, cams = spec.frame_mask(n, h, w), spec.cams(n)
    out = np.zeros((n, oh, ow, 3), np.float32)

    def vertex(f, oy, ox):
        sy, sx = min(oy * step + step // 2, h - 1), min(ox * step + step // 2, w - 1)
        x = depth[f, sy, sx]
        with np.errstate(all="ignore"):
            z = x * gain if spec.source == "depth" else (np.float32(1.0) / (lo + span * x)) * gain
        kept = bool(z > near and z < far) and (mask is None or bool((mask[f] if mask.ndim == 3 else mask)[sy, sx]))
        kinv = cams[f if cams.shape[0] > 1 else 0]
        u, v = (ox + 0.5) * step, (oy + 0.5) * step
        return kept, [float(((kinv[3 * i] * u + kinv[3 * i + 1] * v) + kinv[3 * i + 2]) * float(z)) for i in range(3)]

    for f in range(n):
        for oy in range(1, oh - 1):
            for ox in range(1, ow - 1):
                here, left, right, up, down = (vertex(f, oy + dy, ox + dx) for dy, dx in ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0)))
                if not (here[0] and left[0] and right[0] and up[0] and down[0]):
                    continue
                a, b = [right[1][i] - left[1][i] for i in range(3)], [down[1][i] - up[1][i] for i in range(3)]
                c = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
                length = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
                if length > 0.0:
                    out[f, oy, ox] = [np.float32(c[i] / length) for i in range(3)]
    return out


@pytest.mark.parametrize("source", ["depth", "disparity"])
def test_the_normals_one_pixel_at_a_time(source):
    """Step 3 on the ragged 17 x 23 and step 1 on 7 x 9, two frames with a K each, a mask, and NaN, Inf and 0 among the depths: the vectorised
    mirror equals the rule taken one pixel at a time, as bit patterns."""
    for (h, w), step, seed in (((17, 23), 3, 11), ((7, 9), 1, 12), ((17, 23), 1, 13)):
        depth, mask = tc.live((2, h, w), source, "shared", seed=seed)
        depth[1, h // 2, w // 2], depth[0, 1, 1], depth[1, 2, 5] = np.nan, np.inf, 0.0
        base = tc.live_spec((2, h, w), np.eye(4), step, source, mask)
        K = np.stack([base.K[0], base.K[0] * np.array([[1.1, 1.0, 0.95], [1.0, 0.9, 1.05], [1.0, 1.0, 1.0]])])
        for spec in (base, Cloud(K=K, step=step, source=source, far=10.0, mask=np.stack([mask, mask[::-1, ::-1]]), gain=1.02)):
            got, want = fusion.frame_normals_host(depth, spec), _normals_one_by_one(depth, spec)
            assert np.array_equal(rc.ubits(got), rc.ubits(want)), (h, w, step)
            assert got.any(axis=-1).sum() >= (1 if step == 3 else 4), (h, w, step, int(got.any(axis=-1).sum()))
            assert np.isfinite(got).all()


def test_frames_too_small_for_a_neighbourhood():
    K = np.array([[5.0, 0.0, 1.5], [0.0, 5.0, 1.5], [0.0, 0.0, 1.0]])
    spec = Cloud(K=K, source="depth", far=10.0)
    assert not fusion.frame_normals_host(np.full((1, 1, 9), 0.5, np.float32), spec).any()
    assert not fusion.frame_normals_host(np.full((1, 2, 2), 0.5, np.float32), spec).any()
    got = fusion.frame_normals_host(np.full((1, 3, 3), 0.5, np.float32), spec)
    assert got.shape == (1, 3, 3, 3) and np.array_equal(got[0, 1, 1], [0.0, 0.0, -1.0]) and got.any(axis=-1).sum() == 1
    with pytest.raises(ValueError):
        fusion.frame_normals_host(np.zeros((1, 3, 3), np.float64), spec)
    with pytest.raises(ValueError):
        fusion.frame_normals_host(np.zeros((0, 3, 3), np.float32), spec)


# ---- 2. the sums ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("step,gain", [(1, 1.0), (3, 1.02)])
def test_with_every_option_off_the_sums_are_the_plain_ones(step, gain, scale):
    live, frames, _ = cc.single()
    cast, views = cc.model()
    for guess in (np.eye(4), tc.pose(tc.CLIP_ROTATION, tc.CLIP_TRANSLATION)):
        at = tc.spec(pose=guess, step=step, gain=gain)
        plain = fusion.icp_sums_host(live, at, cast, views, 0.1, scale=scale)
        for kw in ({}, dict(huber=math.inf), dict(huber=np.inf, min_cos=None)):
            got = fusion.icp_robust_sums_host(live, at, cast, views, 0.1, scale=scale, **kw)
            assert got.shape == (T7 if scale else T6,) and np.array_equal(tc.bits(got), tc.bits(plain))
        both = fusion.icp_colour_sums_host(live, frames, at, cast, views, 0.1, scale=scale)
        for kw in ({}, dict(huber=math.inf, huber_colour=math.inf)):
            got = fusion.icp_robust_sums_host(live, at, cast, views, 0.1, scale=scale, frames=frames, **kw)
            assert got.shape == (2, T7 if scale else T6) and np.array_equal(tc.bits(got), tc.bits(both))
        assert plain[-1] > 100 and both[1, -1] > 100


def test_a_pair_inside_the_threshold_keeps_its_bits_and_one_outside_loses_weight():
    """A threshold above every residual changes nothing; one below some changes the system's sums and neither e e nor the count."""
    live, _ = rc.scene("shift")
    cast, views = tc.model()
    plain = fusion.icp_sums_host(live, tc.spec(), cast, views, 0.1)
    wide = fusion.icp_robust_sums_host(live, tc.spec(), cast, views, 0.1, huber=0.2)               # max_dist is 0.1: |e| <= 0.1 for every pair
    assert np.array_equal(tc.bits(wide), tc.bits(plain))
    tight = fusion.icp_robust_sums_host(live, tc.spec(), cast, views, 0.1, huber=rc.HUBER)
    assert np.array_equal(tc.bits(tight[-2:]), tc.bits(plain[-2:])) and (tight[:-2] != plain[:-2]).all()
    diagonal = [0, 6, 11, 15, 18, 20]
    assert (tight[diagonal] < plain[diagonal]).all() and (tight[diagonal] > 0.0).all()             # weights in (0, 1]: every square shrinks
    fewer = fusion.icp_robust_sums_host(live, tc.spec(), cast, views, 0.1, min_cos=rc.MIN_COS)
    assert 100 < fewer[-1] < plain[-1]
    assert fusion.icp_robust_sums_host(live, tc.spec(), cast, views, 0.1, min_cos=-1.0)[-1] < plain[-1]   # the border of the frame has no live normal


def _sums_one_by_one(depth, frames, spec, cast, views, max_dist2, cols, min_cos, huber, huber_colour):
    """(geometric rows, colour rows) of per-pixel terms under the robust rule, one pixel at a time in Python floats; the live normals are
    ``_normals_one_by_one``'s."""
    cam = spec.cams(1)[0]
    mc = np.concatenate([views.cams()[0], fusion.cameras(Cloud(K=views.K, pose=views.pose), 1)[0]])
    lo, span, gain, near, far = spec.scalars()
    h, w = depth.shape[1:]
    mh, mw = views.size
    normals = _normals_one_by_one(depth, spec)[0]
    R = cam[9:18].reshape(3, 3)

    def rows(J, e, threshold):
        weight = 1.0 if abs(e) <= threshold else threshold / abs(e)
        Jw = [weight * j for j in J]
        return [Jw[j] * J[k] for j in range(cols) for k in range(j, cols)] + [Jw[j] * e for j in range(cols)] + [e * e, 1.0]

    geometric, colour = [], []
    for oy in range(h):
        for ox in range(w):
            z = depth[0, oy, ox] * gain
            if not (z > near and z < far):
                continue
            u, v, z = ox + 0.5, oy + 0.5, float(z)
            l = [(cam[3 * i] * u + cam[3 * i + 1] * v) + cam[3 * i + 2] for i in range(3)]
            rho = [float(((R[i, 0] * l[0] + R[i, 1] * l[1]) + R[i, 2] * l[2]) * z) for i in range(3)]
            P = [float(cam[18 + i] + rho[i]) for i in range(3)]
            q = [((mc[21 + 4 * i] * P[0] + mc[22 + 4 * i] * P[1]) + mc[23 + 4 * i] * P[2]) + mc[24 + 4 * i] for i in range(3)]
            if not q[2] > 0.0:
                continue
            um, vm = ((mc[33] * q[0] + mc[34] * q[1]) + mc[35] * q[2]) / q[2], ((mc[36] * q[0] + mc[37] * q[1]) + mc[38] * q[2]) / q[2]
            if not (0.0 <= um < mw and 0.0 <= vm < mh):
                continue
            px, py = int(um), int(vm)
            dm, N = float(cast.depth[0, py, px]), [float(c) for c in cast.normals[0, py, px]]
            if not dm > 0.0 or not (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2] > 0.0:
                continue
            lm = [(mc[3 * i] * (px + 0.5) + mc[3 * i + 1] * (py + 0.5)) + mc[3 * i + 2] for i in range(3)]
            D = [float((mc[18 + i] + ((mc[9 + 3 * i] * lm[0] + mc[10 + 3 * i] * lm[1]) + mc[11 + 3 * i] * lm[2]) * dm) - P[i]) for i in range(3)]
            if not (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2] <= max_dist2:
                continue
            if min_cos is not None:
                nl = [float(c) for c in normals[oy, ox]]
                if not (nl[0] * nl[0] + nl[1] * nl[1]) + nl[2] * nl[2] > 0.0:
                    continue
                nw = [float((R[i, 0] * nl[0] + R[i, 1] * nl[1]) + R[i, 2] * nl[2]) for i in range(3)]
                if not (N[0] * nw[0] + N[1] * nw[1]) + N[2] * nw[2] >= min_cos:
                    continue
            e = (N[0] * D[0] + N[1] * D[1]) + N[2] * D[2]
            J = [rho[1] * N[2] - rho[2] * N[1], rho[2] * N[0] - rho[0] * N[2], rho[0] * N[1] - rho[1] * N[0], N[0], N[1], N[2]]
            if cols == 7:
                J.append((rho[0] * N[0] + rho[1] * N[1]) + rho[2] * N[2])
            geometric.append(rows(J, e, huber))
            found = _colour_at(P, mc, cast, mh, mw)
            if found[0] != "pair":
                continue
            g, r = found[2], _y(frames[0, oy, ox]) - found[1]
            Jc = [rho[1] * g[2] - rho[2] * g[1], rho[2] * g[0] - rho[0] * g[2], rho[0] * g[1] - rho[1] * g[0], g[0], g[1], g[2]]
            if cols == 7:
                Jc.append((rho[0] * g[0] + rho[1] * g[1]) + rho[2] * g[2])
            colour.append(rows(Jc, r, huber_colour))
    return geometric, colour


@pytest.mark.parametrize("scale", [False, True])
def test_the_sums_one_pixel_at_a_time(scale):
    """The 7 x 9 case (one partial tile) with finite thresholds and the normal test, step 1, source "depth", a guess a little aside: every sum
    lies within 1e-12 of ``math.fsum`` of the terms of the pixels taken one by one, relative to the sum of their magnitudes, and both pair counts
    are exact.  The thresholds are chosen so that both weights and the normal test bite."""
    shape = (1, 7, 9)
    depth, _, frames = cc.live(shape, "depth", "none", seed=3)
    cast, views = cc.model()
    spec = tc.live_spec(shape, tc.pose((0.01, -0.01, 0.0), (0.004, -0.003, 0.002)))
    options = dict(min_cos=0.9, huber=0.002, huber_colour=2.0)
    got = fusion.icp_robust_sums_host(depth, spec, cast, views, 0.1, scale=scale, frames=frames, **options)
    off = fusion.icp_robust_sums_host(depth, spec, cast, views, 0.1, scale=scale, frames=frames)
    blocks = _sums_one_by_one(depth, frames, spec, cast, views, 0.01, 7 if scale else 6, **options)
    assert got.shape == (2, T7 if scale else T6)
    worst = 0.0
    for block, rows in zip(got, blocks):
        assert block[-1] == len(rows) >= 8
        for t, terms in enumerate(zip(*rows)):
            exact, size = math.fsum(terms), math.fsum(abs(x) for x in terms)
            worst = max(worst, abs(block[t] - exact) / size)
            assert abs(block[t] - exact) <= 1.0e-12 * size, (t, block[t], exact)
    print(f"\n[scale {scale}] {len(blocks[0])} pairs of {int(off[0, -1])}, {len(blocks[1])} with colour; the worst sum is {worst:.2e} of its terms' magnitudes from the exact one")
    assert got[0, -1] < off[0, -1]                                        # the normal test dropped some
    assert (np.abs(got[:, :-2]) < np.abs(off[:, :-2])).any(axis=1).all()  # and the weights bit in both blocks


def test_the_python_layer_refuses_bad_arguments():
    live, frames, _ = cc.single()
    cast, views = cc.model()
    bare, _ = tc.model()
    for kw in (dict(min_cos=1.5), dict(min_cos=-1.01), dict(min_cos=float("nan")), dict(min_cos="0.9"), dict(min_cos=True), dict(huber=0.0), dict(huber=-1.0),
               dict(huber=float("nan")), dict(huber="1"), dict(huber=True), dict(frames=frames, huber_colour=0.0), dict(frames=frames, huber_colour=float("nan")),
               dict(huber_colour=4.0), dict(scale=1)):
        with pytest.raises(ValueError):
            fusion.icp_robust_sums_host(live, tc.spec(), cast, views, 0.1, **kw)
    with pytest.raises(ValueError):
        fusion.icp_robust_sums_host(live, tc.spec(), bare, views, 0.1, frames=frames)              # a model without colours
    assert fusion.icp_robust_sums_host(live, tc.spec(), cast, views, 0.1, min_cos=-1, huber=1, frames=frames, huber_colour=np.float32(3.0)).shape == (2, T6)


# ---- 3. what it is for ----------------------------------------------------------------------------------------------------------------------------
def _run(kind, **kw):
    live, truth = rc.scene(kind)
    T, pairs, rms, lost = tc.fused().track(live, tc.spec(), tc.track(**kw))
    end = tc.errors(T, truth)
    print(f"[{kind}] {kw or 'plain'}: rotation {end[0]:.3e} rad, translation {end[1]:.3e}; {pairs} pairs, rms {rms:.3e}, lost {lost}")
    assert not lost
    return end


@pytest.mark.parametrize("kind,option", [("shift", dict(huber=rc.HUBER)), ("tilt", dict(min_cos=rc.MIN_COS))], ids=["shift", "tilt"])
def test_the_spoilt_block_is_seen_through(kind, option):
    """A block of 12.5 % of the live frame is wrong and every pair in it passes the distance test.  Measured on the mirror (6 iterations from the
    identity; rotation in rad / translation):
        shift (the block 0.04 nearer)      plain 2.373e-2 / 1.401e-2    huber = 0.005    5.53e-3 / 3.79e-3   (0.23 and 0.27 of the plain errors)
        tilt (the block a plane, 0.006/px) plain 8.50e-3 / 3.06e-3      min_cos = 0.985  1.32e-3 / 6.8e-4    (0.16 and 0.22)
    Asked: half the plain tracker's errors, a margin of about two over those ratios.  The plain tracker is the behaviour before the options and
    is run here on the same input."""
    print()
    plain, robust = _run(kind), _run(kind, **option)
    assert robust[0] <= 0.5 * plain[0] and robust[1] <= 0.5 * plain[1]


def test_on_the_untouched_frame_the_options_cost_nothing():
    """Measured: plain 9.4e-4 / 4.5e-4; huber 9.3e-4 / 4.5e-4; min_cos 3.4e-4 / 1.8e-4; both 3.4e-4 / 1.8e-4.  Asked: at most 1.5 times the plain errors."""
    print()
    plain = _run("untouched")
    for option in (dict(huber=rc.HUBER), dict(min_cos=rc.MIN_COS), rc.OPTIONS["both"]):
        got = _run("untouched", **option)
        assert got[0] <= 1.5 * plain[0] and got[1] <= 1.5 * plain[1]


def test_with_the_scale_and_with_colour():
    """The options combine with ``scale`` and ``colour``: the untouched frame keeps the tolerances of the existing tests and its scale factor
    stays within 0.5 % of 1; with the scale free the tilted block is still seen through (half the plain errors of the same track).  The shifted
    block is not asked with the scale: a nearer patch and a smaller scale explain the same residuals, and both trackers trade one for the other."""
    print()
    depth, frames, truth = cc.single()
    for scale in (False, True):
        T, pairs, rms, lost, *factor = cc.fused().track(depth, tc.spec(), tc.track(colour=cc.WEIGHT, scale=scale, huber_colour=rc.HUBER_COLOUR, **rc.OPTIONS["both"]), frames=frames)
        end, start = tc.errors(T, truth), tc.errors(np.eye(4), truth)
        print(f"[scale {scale}] rotation {end[0]:.3e} rad, translation {end[1]:.3e}; {pairs} pairs, rms {rms:.3e} {factor}")
        assert not lost and end[0] <= 0.1 * start[0] and end[1] <= 0.1 * start[1] and all(abs(f - 1.0) <= 0.005 for f in factor)
    live, truth = rc.scene("tilt")                                       # measured: plain 1.24e-2 / 2.30e-2, factor 0.968; robust 2.3e-4 / 8.4e-4, factor 0.9988
    plain = tc.errors(tc.fused().track(live, tc.spec(), tc.track(scale=True))[0], truth)
    T, _, _, lost, factor = tc.fused().track(live, tc.spec(), tc.track(scale=True, **rc.OPTIONS["both"]))
    end = tc.errors(T, truth)
    print(f"[tilt, scale] plain {plain[0]:.3e} / {plain[1]:.3e}; robust {end[0]:.3e} / {end[1]:.3e}, factor {factor:.5f}")
    assert not lost and end[0] <= 0.5 * plain[0] and end[1] <= 0.5 * plain[1] and abs(factor - 1.0) <= 0.005


def test_a_clip_is_tracked_with_the_options():
    depth, truth = tc.clip()
    got = fusion.TsdfHost(tc.volume(), coloured=False).track_clip(depth, tc.spec(), tc.track(**rc.OPTIONS["both"]))
    moved = tc.errors(np.eye(4), truth[4])
    assert not got.lost.any() and got.scales is None
    for i in range(5):
        end = tc.errors(got.poses[i], truth[i])
        assert end[0] <= 0.1 * moved[0] and end[1] <= 0.1 * moved[1], i


# ---- 4. arguments and defaults --------------------------------------------------------------------------------------------------------------------
def test_track_takes_the_options_and_validates_them():
    plain = Track(near=0.2, far=1.2)
    assert plain.min_cos is None and plain.huber is None and plain.huber_colour is None and plain.robust() == {}
    t = Track(near=0.2, far=1.2, min_cos=1, huber=np.float32(0.5), colour=0.001, huber_colour=4)
    assert (t.min_cos, t.huber, t.huber_colour) == (1.0, 0.5, 4.0) and all(isinstance(v, float) for v in (t.min_cos, t.huber, t.huber_colour))
    assert t.robust() == dict(min_cos=1.0, huber=0.5, huber_colour=4.0)
    assert Track(near=0.2, far=1.2, min_cos=-1.0).robust() == dict(min_cos=-1.0) and Track(near=0.2, far=1.2, min_cos=0).min_cos == 0.0
    for bad in (1.0001, -1.5, float("nan"), float("inf"), True, "0.9", (0.9,)):
        with pytest.raises(ValueError):
            Track(near=0.2, far=1.2, min_cos=bad)
    for bad in (0.0, -0.001, float("nan"), float("inf"), True, False, "0.005", (0.005,)):
        with pytest.raises(ValueError):
            Track(near=0.2, far=1.2, huber=bad)
        with pytest.raises(ValueError):
            Track(near=0.2, far=1.2, colour=0.001, huber_colour=bad)
    with pytest.raises(ValueError):
        Track(near=0.2, far=1.2, huber_colour=4.0)                        # weighs a residual that is not there
    with pytest.raises(ValueError):
        Track(near=0.2, far=1.2, huber=0.005, huber_colour=4.0)


def test_without_the_options_nothing_changes():
    """A ``Track`` with none of them runs the plain sums: the track equals the one put together from ``icp_sums_host``, ``icp_solve`` and
    ``apply_twist``, bit for bit."""
    live, _ = tc.single()
    track = tc.track(min_cos=None, huber=None, huber_colour=None)
    T = np.eye(4)
    views = track.views(tc.K, T, (tc.H, tc.W))
    model = tc.fused().raycast(views, min_weight=track.min_weight, normals=True)
    for _ in range(track.iterations):
        sums = fusion.icp_sums_host(live, tc.spec(pose=T), model, views, track.max_dist)
        T = fusion.apply_twist(T, fusion.icp_solve(sums, track.min_pairs))
    U, _, Vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = U @ Vt
    got = tc.fused().track(live, tc.spec(), track)
    assert np.array_equal(tc.bits(got[0]), tc.bits(T)) and got[1:] == (int(sums[-1]), math.sqrt(sums[-2] / sums[-1]), False)


# ---- 5. the C boundary ----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    lib = _lib.load()
    assert lib.edv_abi_version() == 15 == _lib.ABI_VERSION
    for name in ("edv_frame_normals", "edv_icp_robust_workspace", "edv_icp_robust_sums"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["edv_icp_robust_sums"][1]) == len(_lib.SIGNATURES["edv_icp_colour_sums"][1]) + 4
    assert len(_lib.SIGNATURES["edv_frame_normals"][1]) == 7
    with open(_lib.__file__.replace("endodav_amd/_lib.py", "include/endodav_hip.h")) as fh:
        header = fh.read()
    assert "size_t edv_icp_robust_workspace(int32_t h, int32_t w, int32_t step, int32_t cols, int32_t colour);" in header
    assert "int edv_icp_robust_sums(" in header and "int edv_frame_normals(" in header


def test_workspace_size():
    lib = _lib.load()
    for h, w, step in ((1, 1, 1), (16, 16, 1), (17, 23, 3), (40, 56, 1), (518, 518, 1), (5, 7, 100), (46340, 46340, 1)):
        oh, ow = -(-h // step), -(-w // step)
        for cols, terms in ((6, T6), (7, T7)):
            for colour in (0, 1):
                assert lib.edv_icp_robust_workspace(h, w, step, cols, colour) == (1 + colour) * terms * 8 * -(-(oh * ow) // 256), (h, w, step, cols, colour)
        assert lib.edv_icp_robust_workspace(h, w, step, 6, 0) == lib.edv_icp_workspace(h, w, step)
        assert lib.edv_icp_robust_workspace(h, w, step, 7, 0) == lib.edv_icp_scaled_workspace(h, w, step)
        assert lib.edv_icp_robust_workspace(h, w, step, 7, 1) == lib.edv_icp_colour_workspace(h, w, step, 7)
    for h, w, step, cols, colour in ((0, 5, 1, 6, 0), (5, 0, 1, 7, 1), (5, 5, 0, 6, 0), (46341, 46341, 1, 6, 0), (5, 5, 1, 5, 0), (5, 5, 1, 8, 1), (5, 5, 1, 0, 0), (5, 5, 1, 6, 2),
                                     (5, 5, 1, 7, -1)):
        assert lib.edv_icp_robust_workspace(h, w, step, cols, colour) == 0, (h, w, step, cols, colour)


FAKE = 0x10000


def _sel(**kw):
    fields = dict(x_dev=FAKE, n=3, h=40, w=56, step=1, mode=0, lo=0.0, span=1.0, gain=1.0, near_z=0.001, far_z=10.0, mask_dev=None, mask_stride=0)
    fields.update(kw)
    return C.byref(_lib.CloudSelection(*fields.values()))


BAD_SELECTIONS = [dict(step=0), dict(step=-2), dict(x_dev=None), dict(n=0), dict(n=65536), dict(h=0), dict(w=-1), dict(h=2 ** 16, w=2 ** 15), dict(mode=2),
                  dict(mask_dev=FAKE, mask_stride=7), dict(x_dev=FAKE + 2)]


def test_the_sums_refuse_and_launch_nothing():
    """Every call below is refused before anything is launched (there is no GPU here) and before either camera array is read.  The pointers are
    made-up addresses with the alignment a real one has; none is dereferenced.  The list is that of ``edv_icp_colour_sums`` in
    tests/test_track_colour_cpu.py with the options; without the frames or the colours there is no colour block, and the workspace may be half."""
    lib = _lib.load()
    live, model_cam = (C.c_double * 21)(), (C.c_double * 39)()
    need = lib.edv_icp_robust_workspace(40, 56, 1, 7, 1)
    ok = dict(sel=_sel(), frame=0, frames=FAKE, live=live, model=model_cam, depth=FAKE, normals=FAKE, colors=FAKE + 1, mh=40, mw=56, max_dist2=0.01, cols=7, live_normals=FAKE,
              min_cos=0.9, huber=0.005, huber_colour=math.inf, sums=FAKE, ws=FAKE, ws_bytes=need)
    nan, inf = float("nan"), math.inf
    bad = [dict(sel=None), dict(live=None), dict(model=None), dict(depth=None), dict(normals=None), dict(sums=None), dict(ws=None),
           dict(cols=5), dict(cols=8), dict(cols=0), dict(cols=-7), dict(cols=29),
           dict(frame=-1), dict(frame=3), dict(frame=2 ** 40),
           dict(mh=0), dict(mw=0), dict(mh=-3), dict(mh=2 ** 16, mw=2 ** 15),
           dict(max_dist2=-1.0), dict(max_dist2=nan), dict(max_dist2=inf), dict(max_dist2=-inf),
           dict(min_cos=1.0000001), dict(min_cos=-1.5), dict(min_cos=nan), dict(min_cos=inf), dict(min_cos=-inf), dict(min_cos=nan, live_normals=None),
           dict(huber=0.0), dict(huber=-0.005), dict(huber=nan), dict(huber=-inf), dict(huber_colour=0.0), dict(huber_colour=-1.0), dict(huber_colour=nan),
           dict(huber_colour=nan, frames=None), dict(live_normals=FAKE + 2), dict(live_normals=FAKE + 1),
           dict(ws_bytes=need - 1), dict(ws_bytes=lib.edv_icp_robust_workspace(40, 56, 1, 6, 1)), dict(ws_bytes=lib.edv_icp_robust_workspace(40, 56, 1, 7, 0)), dict(ws_bytes=0),
           dict(frames=None, ws_bytes=need // 2 - 1), dict(colors=None, ws_bytes=need // 2 - 1), dict(frames=None, colors=None, ws_bytes=0),
           dict(ws=FAKE + 4), dict(sums=FAKE + 4), dict(depth=FAKE + 2), dict(normals=FAKE + 1)]
    bad += [dict(sel=_sel(**kw)) for kw in BAD_SELECTIONS]
    for kw in bad:
        assert lib.edv_icp_robust_sums(*{**ok, **kw}.values(), None) != 0, kw
        assert lib.edv_last_error(), kw


def test_the_normals_refuse_and_launch_nothing():
    lib = _lib.load()
    ok = dict(sel=_sel(), cams=FAKE, stride=21, first=0, count=3, normals=FAKE)
    bad = [dict(sel=None), dict(cams=None), dict(normals=None), dict(cams=FAKE + 4), dict(normals=FAKE + 2), dict(stride=1), dict(stride=9), dict(stride=-21), dict(stride=42),
           dict(first=-1), dict(first=3, count=1), dict(first=0, count=0), dict(first=0, count=-1), dict(first=0, count=4), dict(first=2, count=2), dict(first=2 ** 40, count=1),
           dict(first=1, count=2 ** 62), dict(first=0, count=2 ** 63 - 1)]
    bad += [dict(sel=_sel(**kw)) for kw in BAD_SELECTIONS]
    for kw in bad:
        assert lib.edv_frame_normals(*{**ok, **kw}.values(), None) != 0, kw
        assert lib.edv_last_error(), kw
