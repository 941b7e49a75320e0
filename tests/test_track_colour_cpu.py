"""CPU: camera tracking by colour too (``fusion.Track(colour=...)``), on the numpy mirror and at the C boundary (the refusals of
``edv_icp_colour_sums`` launch nothing, so they need no GPU).  The GPU tests hold the kernel to this mirror bit for bit
(tests/test_track_colour_gpu.py); what the term computes and what the tracker converges to is checked here alone."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from endodav_amd import _lib, fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Raycast, Track, Tracked, TsdfHost
from tests import track_cases as tc
from tests import track_colour_cases as cc

T6, T7 = 29, 37


# ---- 1. arguments and defaults ------------------------------------------------------------------------------------------------------------------
def test_track_takes_the_weight_and_validates_it():
    assert Track(near=0.2, far=1.2).colour is None
    t = Track(near=0.2, far=1.2, colour=1)
    assert t.colour == 1.0 and isinstance(t.colour, float)
    assert Track(near=0.2, far=1.2, colour=np.float32(0.5), scale=True).colour == 0.5
    for bad in (0.0, -0.001, float("nan"), float("inf"), True, False, "0.001", (0.001,)):
        with pytest.raises(ValueError):
            Track(near=0.2, far=1.2, colour=bad)


def _track_as_before(host, depth, spec, track):
    """``track`` as it was before the option, from the public pieces: the sums, the solve, the twist."""
    T = fusion._pose4(spec.pose[0])
    views = track.views(spec.K[0], T, depth.shape[1:])
    model = host.raycast(views, min_weight=track.min_weight, normals=True)
    for _ in range(track.iterations):
        sums = fusion.icp_sums_host(depth, dataclasses.replace(spec, pose=T), model, views, track.max_dist)
        T = fusion.apply_twist(T, fusion.icp_solve(sums, track.min_pairs))
    U, _, Vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = U @ Vt
    return T, int(sums[-1]), math.sqrt(sums[-2] / sums[-1]), False


def test_without_the_weight_nothing_changes():
    live, _ = tc.single()
    want = _track_as_before(tc.fused(), live, tc.spec(), tc.track())
    frames = cc.single()[1]
    for host, kw in ((tc.fused(), {}), (tc.fused(), dict(frames=frames)), (tc.fused(), dict(frames=None))):
        got = host.track(live, tc.spec(), tc.track(colour=None), **kw)                # an uncoloured volume: the frames are not looked at
        assert len(got) == 4 and np.array_equal(tc.bits(got[0]), tc.bits(want[0])) and got[1:] == want[1:]
    assert len(tc.fused().track(live, tc.spec(), tc.track(scale=True))) == 5
    # the clip: frame by frame what the steps gave before, on an uncoloured and on a coloured volume
    depth, _ = tc.clip()
    plain = TsdfHost(tc.volume(), coloured=False).track_clip(depth, tc.spec(), tc.track())
    steps = TsdfHost(tc.volume(), coloured=False)
    steps.integrate(depth[:1], tc.spec())
    T = np.eye(4)
    for i in range(1, 5):
        T, pairs, rms, _ = _track_as_before(steps, depth[i:i + 1], tc.spec(pose=T), tc.track())
        assert np.array_equal(tc.bits(plain.poses[i]), tc.bits(T)) and plain.pairs[i] == pairs and plain.rms[i] == rms
        steps.integrate(depth[i:i + 1], tc.spec(pose=T))
    assert plain.scales is None and not plain.lost.any()
    coloured = TsdfHost(tc.volume()).track_clip(depth, tc.spec(), tc.track(), cc.clip()[1])
    cc.same_tracked(coloured, plain)                                                   # colours in the volume do not reach the tracker


def test_the_python_layer_refuses_bad_arguments():
    live, frames, _ = cc.single()
    track = tc.track(colour=cc.WEIGHT)
    with pytest.raises(ValueError):
        tc.fused().track(live, tc.spec(), track, frames=frames)                        # an uncoloured volume
    with pytest.raises(ValueError):
        cc.fused().track(live, tc.spec(), track)                                       # no frames
    with pytest.raises(ValueError):
        cc.fused().track(live, tc.spec(), track, frames=frames[:, :-1])
    with pytest.raises(ValueError):
        cc.fused().track(live, tc.spec(), track, frames=frames.astype(np.float32))
    with pytest.raises(ValueError):
        TsdfHost(tc.volume(), coloured=False).track_clip(tc.clip()[0], tc.spec(), track)
    cast, views = cc.model()
    bare, _ = tc.model()
    with pytest.raises(ValueError):
        fusion.icp_colour_sums_host(live, frames, tc.spec(), bare, views, 0.1)         # a model without colours
    with pytest.raises(ValueError):
        fusion.icp_colour_sums_host(live, None, tc.spec(), cast, views, 0.1)
    with pytest.raises(ValueError):
        fusion.icp_colour_sums_host(live, frames, tc.spec(), Raycast(cast.depth, cast.normals, cast.colors[..., :2]), views, 0.1)
    with pytest.raises(ValueError):
        fusion.icp_colour_sums_host(live, frames, tc.spec(), cast, views, 0.1, scale=1)
    got = fusion.icp_colour_sums_host(live, frames, tc.spec(), cast, views, 0.1)
    assert got.shape == (2, T6) and got.dtype == np.float64
    assert fusion.icp_colour_sums_host(live, frames, tc.spec(), cast, views, 0.1, scale=True).shape == (2, T7)


# ---- 2. the geometric block is icp_sums' ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("gain", [1.0, 1.02])
@pytest.mark.parametrize("step", [1, 3])
def test_the_geometric_block_has_the_same_bits(step, gain, scale):
    live, frames, _ = cc.single()
    cast, views = cc.model()
    spec = tc.spec(step=step, gain=gain)
    both = fusion.icp_colour_sums_host(live, frames, spec, cast, views, 0.1, scale=scale)
    alone = fusion.icp_sums_host(live, spec, cast, views, 0.1, scale=scale)
    assert both.shape == (2, T7 if scale else T6) and np.array_equal(tc.bits(both[0]), tc.bits(alone))
    assert alone[-1] > 100 and 0.8 * alone[-1] < both[1, -1] <= alone[-1] and (both[1] != 0.0).all()


# ---- 3. the colour terms, one pixel at a time -----------------------------------------------------------------------------------------------------
def _y(rgb):
    return (0.299 * float(rgb[0]) + 0.587 * float(rgb[1])) + 0.114 * float(rgb[2])


def _colour_at(P, mc, cast, mh, mw):
    """The colour rule at the world point P in Python floats: ("pair", Im, g [3], (x0, y0), (Iu, Iv, cross), (um, vm), q_2), or the reason
    there is none: "behind", "outside", "left", "right", "above", "below", "narrow", "miss"."""
    q = [((mc[21 + 4 * i] * P[0] + mc[22 + 4 * i] * P[1]) + mc[23 + 4 * i] * P[2]) + mc[24 + 4 * i] for i in range(3)]
    if not q[2] > 0.0:
        return ("behind",)
    K = mc[33:39]
    um, vm = ((K[0] * q[0] + K[1] * q[1]) + K[2] * q[2]) / q[2], ((K[3] * q[0] + K[4] * q[1]) + K[5] * q[2]) / q[2]
    if not (0.0 <= um < mw and 0.0 <= vm < mh):
        return ("outside",)
    gu, gv = um - 0.5, vm - 0.5
    if mw < 2 or mh < 2:
        return ("narrow",)
    for bad, why in ((gu < 0.0, "left"), (gu > mw - 1, "right"), (gv < 0.0, "above"), (gv > mh - 1, "below")):
        if bad:
            return (why,)
    x0, y0 = min(int(gu), mw - 2), min(int(gv), mh - 2)
    fx, fy = gu - x0, gv - y0
    if not all(cast.depth[0, y0 + j, x0 + i] > 0 for i in (0, 1) for j in (0, 1)):
        return ("miss",)
    I00, I10, I01, I11 = (_y(cast.colors[0, y0 + j, x0 + i]) for j in (0, 1) for i in (0, 1))
    top, bot = I00 + fx * (I10 - I00), I01 + fx * (I11 - I01)
    Im = top + fy * (bot - top)
    Iu = (I10 - I00) + fy * ((I11 - I01) - (I10 - I00))
    Iv = (I01 - I00) + fx * ((I11 - I10) - (I01 - I00))
    a, b = K[0] * q[0] + K[1] * q[1], K[3] * q[0] + K[4] * q[1]
    gq = [(Iu * K[0] + Iv * K[3]) / q[2], (Iu * K[1] + Iv * K[4]) / q[2], -((Iu * a + Iv * b) / (q[2] * q[2]))]
    g = [float((mc[21 + j] * gq[0] + mc[25 + j] * gq[1]) + mc[29 + j] * gq[2]) for j in range(3)]
    return "pair", float(Im), g, (x0, y0), (float(Iu), float(Iv), float((I11 - I01) - (I10 - I00))), (float(um), float(vm)), float(q[2])


def _pixels_one_by_one(depth, frames, spec, cast, views, max_dist2, frame=0):
    """{output pixel index: (rho, P, what ``_colour_at`` says, Yl)} of the frame's geometric pairs: the rule applied to one pixel at a time in Python
    floats, independent of the vectorised mirror.  The depth rule is the source "depth" one."""
    cam = spec.cams(1)[0]
    mc = np.concatenate([views.cams()[0], fusion.cameras(Cloud(K=views.K, pose=views.pose), 1)[0]])
    lo, span, gain, near, far = spec.scalars()
    step = int(spec.step)
    h, w = depth.shape[1:]
    mh, mw = views.size
    ow = -(-w // step)
    mask = spec.frame_mask(depth.shape[0], h, w)
    out = {}
    for oy in range(-(-h // step)):
        for ox in range(ow):
            sy, sx = min(oy * step + step // 2, h - 1), min(ox * step + step // 2, w - 1)
            if mask is not None and not (mask[frame] if mask.ndim == 3 else mask)[sy, sx]:
                continue
            z = depth[frame, sy, sx] * gain
            if not (z > near and z < far):
                continue
            u, v, z = (ox + 0.5) * step, (oy + 0.5) * step, float(z)
            l = [(cam[3 * i] * u + cam[3 * i + 1] * v) + cam[3 * i + 2] for i in range(3)]
            rho = [float(((cam[9 + 3 * i] * l[0] + cam[10 + 3 * i] * l[1]) + cam[11 + 3 * i] * l[2]) * z) for i in range(3)]
            P = [float(cam[18 + i] + rho[i]) for i in range(3)]
            found = _colour_at(P, mc, cast, mh, mw)
            if found[0] in ("behind", "outside"):
                continue
            q = [((mc[21 + 4 * i] * P[0] + mc[22 + 4 * i] * P[1]) + mc[23 + 4 * i] * P[2]) + mc[24 + 4 * i] for i in range(3)]
            px = int(((mc[33] * q[0] + mc[34] * q[1]) + mc[35] * q[2]) / q[2])
            py = int(((mc[36] * q[0] + mc[37] * q[1]) + mc[38] * q[2]) / q[2])
            dm, N = float(cast.depth[0, py, px]), [float(c) for c in cast.normals[0, py, px]]
            if not dm > 0.0 or not (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2] > 0.0:
                continue
            lm = [(mc[3 * i] * (px + 0.5) + mc[3 * i + 1] * (py + 0.5)) + mc[3 * i + 2] for i in range(3)]
            D = [float((mc[18 + i] + ((mc[9 + 3 * i] * lm[0] + mc[10 + 3 * i] * lm[1]) + mc[11 + 3 * i] * lm[2]) * dm) - P[i]) for i in range(3)]
            if not (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2] <= max_dist2:
                continue
            out[oy * ow + ox] = (rho, P, found, _y(frames[frame, sy, sx]))
    return out, mc


def _colour_columns(pixels, cols):
    """The T lists of per-pixel colour terms, in the block's layout."""
    rows = []
    for rho, _, found, yl in pixels.values():
        if found[0] != "pair":
            continue
        g, r = found[2], yl - found[1]
        J = [rho[1] * g[2] - rho[2] * g[1], rho[2] * g[0] - rho[0] * g[2], rho[0] * g[1] - rho[1] * g[0], g[0], g[1], g[2]]
        if cols == 7:
            J.append((rho[0] * g[0] + rho[1] * g[1]) + rho[2] * g[2])
        rows.append([J[j] * J[k] for j in range(cols) for k in range(j, cols)] + [J[j] * r for j in range(cols)] + [r * r, 1.0])
    return [list(c) for c in zip(*rows)]


MODELS = {"same": {}, "other": dict(size=tc.OTHER_SIZE, intrinsics=tc.OTHER_K), "skew": dict(intrinsics=cc.SKEW_K)}


@pytest.mark.parametrize("which,step,gain,scale", [("same", 1, 1.0, False), ("same", 3, 1.02, True), ("other", 1, 1.0, True), ("skew", 1, 1.0, False), ("skew", 3, 1.0, True)])
def test_the_colour_block_one_pixel_at_a_time(which, step, gain, scale):
    """Each colour sum lies within n * 2^-53 * sum|terms| of ``math.fsum`` of the terms of the pixels taken one by one, n the number of output
    pixels: the bound of any order of fp64 additions of terms that are themselves the same single products.  Both pair counts are exact.  The
    model is the live camera's, one of another size and K (``OTHER_SIZE``, ``OTHER_K``), or one whose K has skew."""
    live, frames, _ = cc.single()
    cast, views = cc.model(**MODELS[which])
    spec = tc.spec(step=step, gain=gain)
    sums = fusion.icp_colour_sums_host(live, frames, spec, cast, views, 0.1, scale=scale)
    pixels, _ = _pixels_one_by_one(live, frames, spec, cast, views, 0.1 * 0.1)
    n = (-(-tc.H // step)) * (-(-tc.W // step))
    columns = _colour_columns(pixels, 7 if scale else 6)
    assert sums[0, -1] == len(pixels) and sums[1, -1] == len(columns[-1]) and 0.4 * n < len(columns[-1]) <= len(pixels) < n
    assert len(columns) == sums.shape[1]
    worst = 0.0
    for t, terms in enumerate(columns):
        exact, bound = math.fsum(terms), n * 2.0 ** -53 * math.fsum(abs(x) for x in terms)
        worst = max(worst, abs(sums[1, t] - exact) / bound)
        assert abs(sums[1, t] - exact) <= bound, (t, sums[1, t], exact, bound)
    print(f"\n[{which} step {step} gain {gain} scale {scale}] {len(pixels)} pairs, {len(columns[-1])} with colour; the worst sum is at {worst:.3f} of its bound")


# ---- 4. the gradient ------------------------------------------------------------------------------------------------------------------------------
def test_the_gradient_is_the_derivative_of_the_sample():
    """g . d against the central difference (Im(P + d) - Im(P - d)) / 2 of the same rule, for pairs whose three samples share a cell.
    Inside a cell the sample is exactly B(u0 + a, v0 + b) = Im + Iu*a + Iv*b + c*a*b with c = (I11 - I01) - (I10 - I00), its one second-order term,
    and the projection moves along a line: u(P + t d) = u0 + u' t / (1 + eps t), eps = (W[2] . d) / q_2, and v likewise.  With a+, b+ the pixel
    offsets of P + d and a-, b- those of P - d (formed by this test from the projection), the difference is
        Iu (a+ - a-)/2 + Iv (b+ - b-)/2 + c (a+ b+ - a- b-)/2,   (a+ - a-)/2 = u' / (1 - eps^2),
    so it leaves g . d = Iu u' + Iv v' by at most (|Iu u'| + |Iv v'|) eps^2 / (1 - eps^2) + |c| |a+ b+ - a- b-| / 2, plus rounding: each Im
    takes about ten operations on values below 255 (255 * 2^-53 = 2.8e-14 each) and sits on a u or v of magnitude below 60 with as many
    roundings, times a slope below 30 levels a pixel: 1e-11 covers both samples."""
    live, frames, _ = cc.single()
    cast, views = cc.model()
    mh, mw = views.size
    guess = tc.pose(tc.CLIP_ROTATION, tc.CLIP_TRANSLATION)                             # from the identity every point falls on a cell's corner
    pixels, mc = _pixels_one_by_one(live, frames, tc.spec(pose=guess), cast, views, 0.1 * 0.1)
    rng = np.random.default_rng(3)
    checked, worst, largest = 0, 0.0, 0.0
    for p in sorted(pixels)[::37]:
        _, P, found, _ = pixels[p]
        if found[0] != "pair":
            continue
        _, _, g, cell, (Iu, Iv, cross), (um, vm), q2 = found
        d = rng.standard_normal(3)
        d = 5.0e-4 * d / np.linalg.norm(d)                                              # half a millimetre: some 0.05 pixel
        plus, minus = (_colour_at([P[i] + s * d[i] for i in range(3)], mc, cast, mh, mw) for s in (1.0, -1.0))
        if plus[0] != "pair" or minus[0] != "pair" or plus[3] != cell or minus[3] != cell:
            continue
        ap, bp, am, bm = plus[5][0] - um, plus[5][1] - vm, minus[5][0] - um, minus[5][1] - vm
        eps = float(mc[29:32] @ d) / q2
        du, dv = 0.5 * (ap - am) * (1.0 - eps * eps), 0.5 * (bp - bm) * (1.0 - eps * eps)
        bound = (abs(Iu * du) + abs(Iv * dv)) * eps * eps / (1.0 - eps * eps) + 0.5 * abs(cross) * abs(ap * bp - am * bm) + 1.0e-11
        central, linear = 0.5 * (plus[1] - minus[1]), float(np.dot(g, d))
        assert abs(central - linear) <= bound, (p, central, linear, bound)
        checked, worst, largest = checked + 1, max(worst, abs(central - linear) / bound), max(largest, abs(linear))
    print(f"\n{checked} pairs; the worst is at {worst:.3f} of its bound; the largest change is {largest:.3f} levels")
    assert checked >= 20 and largest > 0.05                                             # the changes are ten orders above the bound's floor


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------------------
def _counts(depth, frames, spec, cast, views, frame=0):
    """(the mirror's two pair counts, the same from the pixels one by one, the reasons of the pairs that are geometric only)."""
    sums = fusion.icp_colour_sums_host(depth, frames, spec, cast, views, 0.1, frame)
    pixels, _ = _pixels_one_by_one(depth, frames, spec, cast, views, 0.1 * 0.1, frame)
    why = [f[0] for _, _, f, _ in pixels.values()]
    return (int(sums[0, -1]), int(sums[1, -1])), (len(why), why.count("pair")), set(why) - {"pair"}


def test_pairs_past_the_outermost_centres_are_geometric_only():
    """From the identity every point falls on a pixel's centre; a guess 3 mm aside (0.3 pixel at K = 60 px and z = 0.6) pushes the outermost
    column and row past the last centre, gu > mw - 1 or gu < 0: those pairs have a model pixel, and no cell."""
    live, frames, _ = cc.single()
    cast, views = cc.model(size=(30, 40), intrinsics=(60.0, 0.0, 20.0, 0.0, 60.0, 15.0, 0.0, 0.0, 1.0))    # the middle of the view: hits up to its border
    assert (cast.depth > 0).all()
    inside, _, _ = _counts(live, frames, tc.spec(), cast, views)
    for sign, reasons in ((1.0, {"right", "below"}), (-1.0, {"left", "above"})):
        guess = tc.pose((0.0, 0.0, 0.0), (sign * 0.003, sign * 0.003, 0.0))
        got, want, why = _counts(live, frames, tc.spec(pose=guess), cast, views)
        assert got == want and got[0] > got[1] > 1000 and reasons <= why, (sign, got, why)
        assert inside[1] - got[1] >= 20                                                # a column and a row of them


def test_a_miss_among_the_four_drops_the_colour_pair():
    live, frames, _ = cc.single()
    cast, views = cc.model()
    before, _, _ = _counts(live, frames, tc.spec(), cast, views)
    depth = cast.depth.copy()
    depth[0, 20, 30] = 0.0
    holed = Raycast(depth, cast.normals, cast.colors)
    got, want, why = _counts(live, frames, tc.spec(), holed, views)
    assert got == want and "miss" in why
    assert before[0] - got[0] < before[1] - got[1]                                      # one model pixel loses its own pairs; four cells lose their colour


def test_a_view_one_pixel_wide_has_no_colour_pairs():
    live, frames, _ = cc.single()
    for size, K in (((tc.H, 1), (60.0, 0.0, 0.5, 0.0, 60.0, 20.0, 0.0, 0.0, 1.0)), ((1, tc.W), (60.0, 0.0, 28.0, 0.0, 60.0, 0.5, 0.0, 0.0, 1.0))):
        cast, views = cc.model(size=size, intrinsics=K)
        got, want, why = _counts(live, frames, tc.spec(), cast, views)
        assert got == want and got[0] >= 10 and got[1] == 0 and why == {"narrow"}, (size, got, why)


def test_a_guess_that_looks_away_sums_to_zero():
    live, frames, _ = cc.single()
    cast, views = cc.model()
    for scale, count in ((False, T6), (True, T7)):
        zeros = fusion.icp_colour_sums_host(live, frames, tc.spec(pose=tc.AWAY), cast, views, 0.1, scale=scale)
        assert np.array_equal(tc.bits(zeros), tc.bits(np.zeros((2, count))))            # +0, every one
    T, pairs, rms, lost = cc.fused().track(live, tc.spec(pose=tc.AWAY), tc.track(colour=cc.WEIGHT), frames=frames)
    assert lost and pairs == 0 and np.array_equal(T, tc.AWAY)


def test_live_pixels_that_are_not_kept_have_neither_pair():
    live, frames, _ = cc.single()
    cast, views = cc.model()
    before, _, _ = _counts(live, frames, tc.spec(), cast, views)
    holed = live.copy()
    holed[0, 10:14, 20:30] = np.nan
    holed[0, 25:28, 5:45] = 0.0
    holed[0, 0, 0], holed[0, 39, 55] = np.inf, -1.0
    got, want, _ = _counts(holed, frames, tc.spec(), cast, views)
    assert got == want and got[0] <= before[0] - 150 and got[1] <= before[1] - 150
    sums = fusion.icp_colour_sums_host(holed, frames, tc.spec(), cast, views, 0.1)
    assert np.isfinite(sums).all()


def test_a_masked_clip():
    depth, mask, frames = cc.live((2, 17, 23), kind="shared", seed=5)
    cast, views = cc.model()
    spec = tc.live_spec((2, 17, 23), np.eye(4), 1, "depth", mask)
    open_spec = tc.live_spec((2, 17, 23), np.eye(4), 1, "depth", None)
    for frame in (0, 1):
        got, want, _ = _counts(depth, frames, spec, cast, views, frame)
        unmasked, _, _ = _counts(depth, frames, open_spec, cast, views, frame)
        assert got == want and 50 < got[1] <= got[0] < unmasked[0]
    per_frame = np.stack([mask, ~mask])
    got, want, _ = _counts(depth, frames, tc.live_spec((2, 17, 23), np.eye(4), 1, "depth", per_frame), cast, views, 1)
    assert got == want and 0 < got[0] < unmasked[0]


# ---- 6. what it is for ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotation,translation,rot_bound,tr_bound", [((0.0, 0.0, 0.0), cc.SLIDE, 3.5e-3, 2.0e-3), (cc.ROLL, cc.ROLL_SLIDE, 1.2e-3, 6.0e-4)],
                         ids=["slide", "roll"])
def test_colour_sees_the_sliding_on_a_plane(rotation, translation, rot_bound, tr_bound):
    """A textured plane at z = 0.6, fused at the identity and seen from a camera moved inside the plane.  Every normal is (0, 0, -1) and every
    residual 0 at the guess: the rows of J that belong to x, y and the roll are zero, numpy's solve returns 0 for them or refuses, and the
    estimate keeps the whole in-plane motion; at least 0.8 of it is asked.  With colour, measured on the mirror (6 iterations, weight 0.001):
        slide (0.02, -0.015, 0): rotation 1.16e-3 rad, translation 6.5e-4 of 2.5e-2
        roll 0.03 about z with 0.03 along x: rotation 4.0e-4 rad of 3.0e-2, translation 1.9e-4 of 3.0e-2
    The bounds are three times those, and in any case below a quarter of the motion: the live frame is a ray-cast of voxel-averaged colours, so
    the figures depend on the scene."""
    depth, frames, truth = cc.single("plane", rotation, translation)
    start = tc.errors(np.eye(4), truth)
    T, _, _, lost = cc.fused("plane").track(depth, tc.spec(), tc.track(), frames=frames)
    blind = tc.errors(T, truth)
    print(f"\ngeometry alone: rotation {start[0]:.3e} -> {blind[0]:.3e} rad, translation {start[1]:.3e} -> {blind[1]:.3e}, lost {lost}")
    assert blind[1] >= 0.8 * start[1]
    T, pairs, rms, lost = cc.fused("plane").track(depth, tc.spec(), tc.track(colour=cc.WEIGHT), frames=frames)
    end = tc.errors(T, truth)
    print(f"with colour: rotation {end[0]:.3e} rad, translation {end[1]:.3e}; {pairs} pairs, rms {rms:.3e}")
    assert not lost and pairs > 1000
    assert end[1] <= tr_bound <= 0.25 * start[1] and end[0] <= rot_bound
    if start[0] > 0.0:
        assert rot_bound <= 0.25 * start[0]


def test_on_the_curved_surface_colour_keeps_the_tolerances():
    """``tc.single()``'s motion on the curved surface, where geometry alone already converges: measured rotation 6.7e-4 of 3.9e-2 rad and
    translation 4.0e-4 of 2.7e-2; asked, as in tests/test_track_cpu.py, a tenth of the start error."""
    depth, frames, truth = cc.single()
    start = tc.errors(np.eye(4), truth)
    for scale in (False, True):
        T, pairs, rms, lost, *factor = cc.fused().track(depth, tc.spec(), tc.track(colour=cc.WEIGHT, scale=scale), frames=frames)
        end = tc.errors(T, truth)
        print(f"\n[scale {scale}] rotation {start[0]:.3e} -> {end[0]:.3e} rad, translation {start[1]:.3e} -> {end[1]:.3e}; {pairs} pairs, rms {rms:.3e} {factor}")
        assert not lost and end[0] <= 0.1 * start[0] and end[1] <= 0.1 * start[1]
        assert len(factor) == int(scale) and all(abs(f - 1.0) <= 0.005 for f in factor)
        assert isinstance(pairs, int) and isinstance(rms, float) and isinstance(lost, bool) and 64 <= pairs <= tc.H * tc.W
        assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)


def test_the_weight_enters_squared_and_the_counts_stay_geometric():
    live, frames, _ = cc.single()
    cast, views = cc.model()
    both = fusion.icp_colour_sums_host(live, frames, tc.spec(), cast, views, 0.1)
    mixed = fusion._with_colour(both.reshape(-1), 0.5)
    assert mixed.shape == (T6,) and np.array_equal(mixed[:-2], both[0, :-2] + 0.25 * both[1, :-2]) and np.array_equal(mixed[-2:], both[0, -2:])
    none = both.copy()
    none[1] = 0.0
    assert np.array_equal(tc.bits(fusion._with_colour(none.reshape(-1), 0.5)), tc.bits(both[0]))   # no colour pairs: nothing is added


# ---- 7. a clip ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
def test_five_frames_are_tracked_with_colour(scale):
    """Measured on the mirror: the worst frame ends 0.023 (rotation) and 0.018 (translation) of frame 4's motion from its truth with and without
    the scale, the scales within 8e-4 of 1; asked, as in the existing clip tests, a tenth."""
    depth, frames, truth = cc.clip()
    host = TsdfHost(tc.volume())
    got = host.track_clip(depth, tc.spec(), tc.track(colour=cc.WEIGHT, scale=scale), frames)
    assert isinstance(got, Tracked) and not got.lost.any() and np.array_equal(got.poses[0], np.eye(4))
    moved = tc.errors(np.eye(4), truth[4])
    for i in range(5):
        end = tc.errors(got.poses[i], truth[i])
        print(f"\nframe {i}: rotation {end[0] / moved[0]:.4f}, translation {end[1] / moved[1]:.4f} of frame 4's motion; {got.pairs[i]} pairs")
        assert end[0] <= 0.1 * moved[0] and end[1] <= 0.1 * moved[1]
    assert (got.scales is not None) == scale and host.weight.max() == 5.0
    if scale:
        assert got.scales[0] == 1.0 and (np.abs(got.scales - 1.0) <= 0.005).all()


# ---- 8. the C boundary ----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    lib = _lib.load()
    assert lib.edv_abi_version() == 15 == _lib.ABI_VERSION
    for name in ("edv_icp_colour_workspace", "edv_icp_colour_sums"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["edv_icp_colour_sums"][1]) == len(_lib.SIGNATURES["edv_icp_sums"][1]) + 3
    with open(_lib.__file__.replace("endodav_amd/_lib.py", "include/endodav_hip.h")) as fh:
        header = fh.read()
    assert "size_t edv_icp_colour_workspace(int32_t h, int32_t w, int32_t step, int32_t cols);" in header and "int edv_icp_colour_sums(" in header


def test_workspace_size():
    lib = _lib.load()
    for h, w, step in ((1, 1, 1), (16, 16, 1), (17, 23, 3), (40, 56, 1), (518, 518, 1), (5, 7, 100), (46340, 46340, 1)):
        oh, ow = -(-h // step), -(-w // step)
        for cols, terms in ((6, T6), (7, T7)):
            assert lib.edv_icp_colour_workspace(h, w, step, cols) == 2 * terms * 8 * -(-(oh * ow) // 256), (h, w, step, cols)
        assert lib.edv_icp_colour_workspace(h, w, step, 6) == 2 * lib.edv_icp_workspace(h, w, step)
    for h, w, step, cols in ((0, 5, 1, 6), (5, 0, 1, 7), (5, 5, 0, 6), (46341, 46341, 1, 6), (5, 5, 1, 5), (5, 5, 1, 8), (5, 5, 1, 0), (5, 5, 1, -6)):
        assert lib.edv_icp_colour_workspace(h, w, step, cols) == 0, (h, w, step, cols)


def test_refusals_launch_nothing():
    """Every call below is refused before anything is launched (there is no GPU here) and before either camera array is read.  The pointers are
    made-up addresses with the alignment a real one has; none is dereferenced.  The list is that of ``edv_icp_sums`` in tests/test_track_cpu.py
    with the frames, the model's colours and the column count."""
    lib = _lib.load()
    FAKE = 0x10000
    live, model_cam = (C.c_double * 21)(), (C.c_double * 39)()

    def sel(**kw):
        fields = dict(x_dev=FAKE, n=3, h=40, w=56, step=1, mode=0, lo=0.0, span=1.0, gain=1.0, near_z=0.001, far_z=10.0, mask_dev=None, mask_stride=0)
        fields.update(kw)
        return C.byref(_lib.CloudSelection(*fields.values()))

    need = lib.edv_icp_colour_workspace(40, 56, 1, 7)
    ok = dict(sel=sel(), frame=0, frames=FAKE, live=live, model=model_cam, depth=FAKE, normals=FAKE, colors=FAKE + 1, mh=40, mw=56, max_dist2=0.01, cols=7, sums=FAKE,
              ws=FAKE, ws_bytes=need)
    bad = [dict(sel=None), dict(frames=None), dict(live=None), dict(model=None), dict(depth=None), dict(normals=None), dict(colors=None), dict(sums=None), dict(ws=None),
           dict(cols=5), dict(cols=8), dict(cols=0), dict(cols=-7), dict(cols=29),
           dict(frame=-1), dict(frame=3), dict(frame=2 ** 40),
           dict(sel=sel(step=0)), dict(sel=sel(step=-2)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)), dict(sel=sel(n=65536)), dict(sel=sel(h=0)), dict(sel=sel(w=-1)),
           dict(sel=sel(h=2 ** 16, w=2 ** 15)), dict(sel=sel(mode=2)), dict(sel=sel(mask_dev=FAKE, mask_stride=7)), dict(sel=sel(x_dev=FAKE + 2)),
           dict(mh=0), dict(mw=0), dict(mh=-3), dict(mh=2 ** 16, mw=2 ** 15),
           dict(max_dist2=-1.0), dict(max_dist2=float("nan")), dict(max_dist2=float("inf")), dict(max_dist2=-float("inf")),
           dict(ws_bytes=need - 1), dict(ws_bytes=lib.edv_icp_colour_workspace(40, 56, 1, 6)), dict(ws_bytes=lib.edv_icp_scaled_workspace(40, 56, 1)), dict(ws_bytes=0),
           dict(ws=FAKE + 4), dict(sums=FAKE + 4), dict(depth=FAKE + 2), dict(normals=FAKE + 1)]
    for kw in bad:
        assert lib.edv_icp_colour_sums(*{**ok, **kw}.values(), None) != 0, kw
        assert lib.edv_last_error(), kw
