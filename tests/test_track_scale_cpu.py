"""CPU: camera tracking with the frame's depth scale as a seventh unknown (``fusion.Track(scale=True)``), on the numpy mirror and at the C boundary
(the refusals of ``edv_icp_scaled_sums`` launch nothing, so they need no GPU).  The GPU tests hold the kernel to this mirror bit for bit
(tests/test_track_scale_gpu.py); what the tracker converges to is checked here alone."""
import ctypes as C
import math

import numpy as np
import pytest

from endodav_amd import _lib, fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Track, Tracked, TsdfHost
from tests import track_cases as tc
from tests import track_scale_cases as sc


# ---- 1. arguments -------------------------------------------------------------------------------------------------------------------------------
def test_track_takes_the_option_and_validates_it():
    t = Track(near=0.2, far=1.2)
    assert t.scale is False and t.max_scale_step == 0.25
    t = Track(near=0.2, far=1.2, scale=True, max_scale_step=0.5)
    assert t.scale is True and t.max_scale_step == 0.5 and isinstance(t.max_scale_step, float)
    for kw in (dict(scale=1), dict(scale=0), dict(scale="yes"), dict(scale=None), dict(scale=1.0),
               dict(max_scale_step=0.0), dict(max_scale_step=-0.25), dict(max_scale_step=float("nan")), dict(max_scale_step=float("inf")), dict(max_scale_step=None),
               dict(max_scale_step=True)):
        with pytest.raises(ValueError):
            Track(**{**dict(near=0.2, far=1.2), **kw})
    live, _ = tc.single()
    cast, views = tc.model()
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError):
            fusion.icp_sums_host(live, tc.spec(), cast, views, 0.1, scale=bad)
    with pytest.raises(ValueError):
        fusion.icp_solve(np.zeros(30), 1)


def test_the_defaults_change_nothing():
    live, _ = tc.single()
    got = tc.fused().track(live, tc.spec(), tc.track())
    assert len(got) == 4
    host = TsdfHost(tc.volume(), coloured=False)
    tracked = host.track_clip(tc.clip()[0][:2], tc.spec(), tc.track())
    assert tracked.scales is None
    assert Tracked(np.zeros((1, 4, 4)), np.zeros(1, np.int64), np.zeros(1), np.zeros(1, bool)).scales is None     # as it was constructed before
    with_scale = tc.fused().track(live, tc.spec(), tc.track(scale=True))
    assert len(with_scale) == 5 and isinstance(with_scale[4], float)


# ---- 2. the columns shared with the 6-column sums -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 1.02])
@pytest.mark.parametrize("step", [1, 3])
def test_the_shared_sums_have_the_same_bits(step, gain):
    live, _ = tc.single()
    cast, views = tc.model()
    spec = tc.spec(step=step, gain=gain)
    seven = fusion.icp_sums_host(live, spec, cast, views, 0.1, scale=True)
    six = fusion.icp_sums_host(live, spec, cast, views, 0.1, scale=False)
    assert seven.shape == (37,) and seven.dtype == np.float64 and six.shape == (29,)
    assert len(sc.SHARED) == 29 and np.array_equal(tc.bits(seven[sc.SHARED]), tc.bits(six))
    assert six[28] > 100 and all(seven[j] != 0.0 for j in sc.NEW)
    assert np.array_equal(tc.bits(fusion.icp_sums_host(live, spec, cast, views, 0.1)), tc.bits(six))            # the default is the 29


# ---- 3. the seventh column, one pixel at a time -------------------------------------------------------------------------------------------------
def _pixels_one_by_one(depth, spec, cast, views, max_dist2):
    """{output pixel index: (e, [J_0..J_6], (px, py))} of frame 0's pairs: the rule applied to one pixel at a time in Python floats, independent
    of the vectorised mirror."""
    cam = spec.cams(1)[0]
    mc = np.concatenate([views.cams()[0], fusion.cameras(Cloud(K=views.K, pose=views.pose), 1)[0]])
    lo, span, gain, near, far = spec.scalars()
    step = int(spec.step)
    h, w = depth.shape[1:]
    mh, mw = views.size
    ow = -(-w // step)
    out = {}
    for oy in range(-(-h // step)):
        for ox in range(ow):
            z = depth[0, min(oy * step + step // 2, h - 1), min(ox * step + step // 2, w - 1)] * gain
            if not (z > near and z < far):
                continue
            u, v, z = (ox + 0.5) * step, (oy + 0.5) * step, float(z)
            l = [(cam[3 * i] * u + cam[3 * i + 1] * v) + cam[3 * i + 2] for i in range(3)]
            rho = [float(((cam[9 + 3 * i] * l[0] + cam[10 + 3 * i] * l[1]) + cam[11 + 3 * i] * l[2]) * z) for i in range(3)]
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
            e = (N[0] * D[0] + N[1] * D[1]) + N[2] * D[2]
            J = [rho[1] * N[2] - rho[2] * N[1], rho[2] * N[0] - rho[0] * N[2], rho[0] * N[1] - rho[1] * N[0], N[0], N[1], N[2],
                 (rho[0] * N[0] + rho[1] * N[1]) + rho[2] * N[2]]
            out[oy * ow + ox] = (e, J, (px, py))
    return out


@pytest.mark.parametrize("step,gain", [(1, 1.0), (3, 1.02)])
def test_the_seventh_column_one_pixel_at_a_time(step, gain):
    """Each of the eight sums the seventh column adds lies within n * 2^-53 * sum|terms| of ``math.fsum`` of the terms of the pixels taken one by
    one, n the number of output pixels: the bound of any order of fp64 additions of terms that are themselves the same single products."""
    live, _ = tc.single()
    cast, views = tc.model()
    spec = tc.spec(step=step, gain=gain)
    sums = fusion.icp_sums_host(live, spec, cast, views, 0.1, scale=True)
    pixels = _pixels_one_by_one(live, spec, cast, views, 0.1 * 0.1)
    n = (-(-tc.H // step)) * (-(-tc.W // step))
    assert sums[36] == len(pixels) and 0.5 * n < len(pixels) < n
    columns = {sc.NEW[j]: [J[j] * J[6] for _, J, _ in pixels.values()] for j in range(7)}
    columns[34] = [J[6] * e for e, J, _ in pixels.values()]
    assert sorted(columns) == sc.NEW
    for t, terms in columns.items():
        exact, bound = math.fsum(terms), n * 2.0 ** -53 * math.fsum(abs(x) for x in terms)
        print(f"\n[step {step} gain {gain}] sums[{t}] = {sums[t]!r}, fsum {exact!r}, off by {abs(sums[t] - exact):.3e} of {bound:.3e}")
        assert abs(sums[t] - exact) <= bound, (t, sums[t], exact, bound)
    assert sums[27] > 0.0                                                                # J_6 * J_6


# ---- 4. the derivative --------------------------------------------------------------------------------------------------------------------------
def test_the_column_is_the_derivative_of_the_residual():
    """e(gain * (1 + delta)) - e(gain) = -delta * J_6 per pixel, for the pixels that are paired with the same model pixel under both gains (the
    model's vertex and normal are then the same, and e depends on the scale through P = t + r * z alone, linearly: no second-order term).  With
    gain = 1 and delta = 2^-10 both gains are float32 numbers and z(gain) = x exactly, so the one rounding that separates the two sides is that of
    z(gain * (1 + delta)) = float32(x * (1 + delta)), at most 2^-24 relative: |J_6| * (1 + delta) * 2^-24, under the |J_6| * 2^-23 asked here.  The
    fp64 roundings of e itself, some 1e-16 each on values below 1, are orders below what is left."""
    live, _ = tc.single()
    cast, views = tc.model()
    delta = 2.0 ** -10
    assert float(np.float32(1.0 + delta)) == 1.0 + delta
    before = _pixels_one_by_one(live, tc.spec(gain=1.0), cast, views, 0.1 * 0.1)
    after = _pixels_one_by_one(live, tc.spec(gain=1.0 + delta), cast, views, 0.1 * 0.1)
    stay = [p for p in before if p in after and before[p][2] == after[p][2]]
    assert len(stay) > 0.9 * len(before) > 1000
    worst = 0.0
    for p in stay:
        (e0, J, _), (e1, _, _) = before[p], after[p]
        off, bound = abs((e1 - e0) + delta * J[6]), abs(J[6]) * 2.0 ** -23
        worst = max(worst, off / bound)
        assert off <= bound, (p, e0, e1, J[6], off, bound)
    print(f"\n{len(stay)} of {len(before)} pairs stay; the worst pixel is at {worst:.3f} of its bound")
    assert min(abs(before[p][1][6]) for p in stay) > 1e-3                                # the room |J_6| * 2^-24 leaves is above 5e-11 everywhere on this scene


# ---- 5. one frame -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sc.SCALES)
def test_single_frame_finds_pose_and_scale(s):
    """Measured on the mirror, as a fraction of the start error: rotation 0.017 and translation 0.037 for every s, sigma / s - 1 = 1.5e-3.  Without
    the option at s = 1.02: 0.31 and 0.52."""
    live, truth = sc.single(s)
    start = tc.errors(np.eye(4), truth)
    T, pairs, rms, lost, factor = tc.fused().track(live, tc.spec(), tc.track(scale=True))
    end = tc.errors(T, truth)
    print(f"\n[s = {s}] rotation {end[0] / start[0]:.4f}, translation {end[1] / start[1]:.4f} of the start error; sigma {factor:.6f}, off by {abs(factor / s - 1.0):.3e}; {pairs} pairs, rms {rms:.3e}")
    assert not lost and T.shape == (4, 4) and T.dtype == np.float64
    assert end[0] <= 0.1 * start[0] and end[1] <= 0.1 * start[1]
    assert isinstance(factor, float) and abs(factor / s - 1.0) <= 0.005
    assert isinstance(pairs, int) and isinstance(rms, float) and isinstance(lost, bool) and 64 <= pairs <= tc.H * tc.W
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)
    if s == 1.02:                                                                        # why the option exists
        T6, _, _, lost6 = tc.fused().track(live, tc.spec(), tc.track())
        end6 = tc.errors(T6, truth)
        print(f"\n[s = {s}, six columns] rotation {end6[0] / start[0]:.4f}, translation {end6[1] / start[1]:.4f} of the start error")
        assert not lost6 and end6[0] > 0.1 * start[0] and end6[1] > 0.1 * start[1]


# ---- 6. a clip whose scale drifts ---------------------------------------------------------------------------------------------------------------
def test_a_drifting_clip_is_tracked_and_fused():
    """Frame i is divided by 1.02**i.  Measured on the mirror: the worst frame ends 0.049 (rotation) and 0.037 (translation) of frame 4's motion
    from its truth, the scales within 2.7e-3 of 1.02**i."""
    depth, truth, scales = sc.clip()
    host = TsdfHost(tc.volume(), coloured=False)
    got = host.track_clip(depth, tc.spec(), tc.track(scale=True))
    assert isinstance(got, Tracked) and got.scales.shape == (5,) and got.scales.dtype == np.float64
    assert not got.lost.any() and got.scales[0] == 1.0 and np.array_equal(got.poses[0], np.eye(4))
    moved = tc.errors(np.eye(4), truth[4])
    for i in range(5):
        end = tc.errors(got.poses[i], truth[i])
        print(f"\nframe {i}: rotation {end[0] / moved[0]:.4f}, translation {end[1] / moved[1]:.4f} of frame 4's motion; sigma {got.scales[i]:.6f}, off by {abs(got.scales[i] / scales[i] - 1.0):.3e}")
        assert end[0] <= 0.1 * moved[0] and end[1] <= 0.1 * moved[1]
        if i:
            assert abs(got.scales[i] / 1.02 ** i - 1.0) <= 0.005
    assert host.weight.max() == 5.0


# ---- 7. lost frames -----------------------------------------------------------------------------------------------------------------------------
def test_lost_frames_keep_pose_and_scale():
    depth, _, _ = sc.clip()
    holed = depth.copy()
    holed[2] = 0.0                                                                       # sees nothing
    host = TsdfHost(tc.volume(), coloured=False)
    got = host.track_clip(holed, tc.spec(), tc.track(scale=True))
    assert list(got.lost) == [False, False, True, False, False]
    assert np.array_equal(got.poses[2], got.poses[1]) and got.scales[2] == got.scales[1] and got.pairs[2] == 0
    assert abs(got.scales[4] / 1.02 ** 4 - 1.0) <= 0.005 and host.weight.max() == 4.0   # frame 3 is found from frame 1's pose and scale
    # a frame in quite another unit: lost, and the volume stays what frames 0 and 1 made it
    far_off = depth[:3].copy()
    far_off[2] = (depth[2] / 1.5).astype(np.float32)
    two = TsdfHost(tc.volume(), coloured=False)
    want = two.track_clip(depth[:2], tc.spec(), tc.track(scale=True, max_scale_step=0.25))
    three = TsdfHost(tc.volume(), coloured=False)
    got = three.track_clip(far_off, tc.spec(), tc.track(scale=True, max_scale_step=0.25))
    assert list(got.lost) == [False, False, True] and np.array_equal(got.poses[2], want.poses[1]) and got.scales[2] == want.scales[1]
    assert np.array_equal(three.weight, two.weight) and np.array_equal(three.tsdf, two.tsdf)
    # the step of the scale is what loses a frame that is otherwise found: s = 1.05 with a hundredth allowed
    live, _ = sc.single(1.05)
    T, pairs, rms, lost, factor = tc.fused().track(live, tc.spec(), tc.track(scale=True, max_scale_step=0.01))
    assert lost and pairs >= 64 and rms > 0.0 and factor == 1.0 and np.array_equal(T, np.eye(4))
    T, _, _, lost, factor = tc.fused().track(live, tc.spec(), tc.track(scale=True, max_scale_step=0.1))    # the first step overshoots to 1.075
    assert not lost and abs(factor / 1.05 - 1.0) <= 0.005
    # the lost cases of the six columns are lost here too, with the guess and factor 1
    empty = TsdfHost(tc.volume(), coloured=False)
    for tsdf, spec, track in ((empty, tc.spec(), tc.track(scale=True)), (tc.fused(), tc.spec(pose=tc.AWAY), tc.track(scale=True)),
                              (tc.fused(), tc.spec(), tc.track(scale=True, min_pairs=tc.H * tc.W))):
        T, pairs, rms, lost, factor = tsdf.track(tc.single()[0], spec, track)
        assert lost and factor == 1.0 and np.array_equal(T, fusion._pose4(spec.pose[0]))
    zeros = fusion.icp_sums_host(tc.single()[0], tc.spec(pose=tc.AWAY), *tc.model(), 0.1, scale=True)
    assert np.array_equal(tc.bits(zeros), tc.bits(np.zeros(37))) and fusion.icp_solve(zeros, 1) is None


def test_solve_takes_both_layouts():
    rng = np.random.default_rng(1)
    J, e = rng.standard_normal((100, 7)), rng.standard_normal(100)
    A, b = J.T @ J, J.T @ e
    sums = np.concatenate([A[np.triu_indices(7)], b, [e @ e, 100.0]])
    assert sums.shape == (37,)
    x = fusion.icp_solve(sums, 64)
    assert x.shape == (7,) and np.allclose(x, np.linalg.solve(A, b), rtol=1e-12, atol=0.0)
    six = fusion.icp_solve(sums[sc.SHARED], 64)
    assert six.shape == (6,) and np.allclose(six, np.linalg.solve(A[:6, :6], b[:6]), rtol=1e-12, atol=0.0)
    assert fusion.icp_solve(sums, 101) is None


# ---- 8. the C boundary --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    lib = _lib.load()
    assert lib.edv_abi_version() == 15 == _lib.ABI_VERSION
    for name in ("edv_icp_scaled_workspace", "edv_icp_scaled_sums"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["edv_icp_scaled_sums"] == _lib.SIGNATURES["edv_icp_sums"]
    assert _lib.SIGNATURES["edv_icp_scaled_workspace"] == _lib.SIGNATURES["edv_icp_workspace"]
    assert fusion.ICP_SCALED_TERMS == 37 and fusion.ICP_TERMS == 29


def test_workspace_size():
    lib = _lib.load()
    for h, w, step in ((1, 1, 1), (16, 16, 1), (17, 33, 1), (17, 33, 3), (40, 56, 1), (518, 518, 1), (518, 518, 4), (5, 7, 100), (46340, 46340, 1)):
        oh, ow = -(-h // step), -(-w // step)
        assert lib.edv_icp_scaled_workspace(h, w, step) == 37 * 8 * -(-(oh * ow) // 256), (h, w, step)
    for h, w, step in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, 0), (5, 5, -1), (2 ** 16, 2 ** 15, 1), (46341, 46341, 1)):
        assert lib.edv_icp_scaled_workspace(h, w, step) == 0, (h, w, step)


def test_refusals_launch_nothing():
    """Every call below is refused before anything is launched (there is no GPU here) and before either camera array is read.  The pointers are
    made-up addresses with the alignment a real one has; none is dereferenced.  The list is that of ``edv_icp_sums`` in tests/test_track_cpu.py."""
    lib = _lib.load()
    FAKE = 0x10000
    live, model_cam = (C.c_double * 21)(), (C.c_double * 39)()

    def sel(**kw):
        fields = dict(x_dev=FAKE, n=3, h=40, w=56, step=1, mode=0, lo=0.0, span=1.0, gain=1.0, near_z=0.001, far_z=10.0, mask_dev=None, mask_stride=0)
        fields.update(kw)
        return C.byref(_lib.CloudSelection(*fields.values()))

    need = lib.edv_icp_scaled_workspace(40, 56, 1)
    assert need > lib.edv_icp_workspace(40, 56, 1)
    ok = dict(sel=sel(), frame=0, live=live, model=model_cam, depth=FAKE, normals=FAKE, mh=40, mw=56, max_dist2=0.01, sums=FAKE, ws=FAKE, ws_bytes=need)
    bad = [dict(sel=None), dict(live=None), dict(model=None), dict(depth=None), dict(normals=None), dict(sums=None), dict(ws=None),
           dict(frame=-1), dict(frame=3), dict(frame=2 ** 40),
           dict(sel=sel(step=0)), dict(sel=sel(step=-2)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)), dict(sel=sel(n=65536)), dict(sel=sel(h=0)), dict(sel=sel(w=-1)),
           dict(sel=sel(h=2 ** 16, w=2 ** 15)), dict(sel=sel(mode=2)), dict(sel=sel(mask_dev=FAKE, mask_stride=7)), dict(sel=sel(x_dev=FAKE + 2)),
           dict(mh=0), dict(mw=0), dict(mh=-3), dict(mh=2 ** 16, mw=2 ** 15),
           dict(max_dist2=-1.0), dict(max_dist2=float("nan")), dict(max_dist2=float("inf")), dict(max_dist2=-float("inf")),
           dict(ws_bytes=need - 1), dict(ws_bytes=lib.edv_icp_workspace(40, 56, 1)), dict(ws_bytes=0), dict(ws=FAKE + 4), dict(sums=FAKE + 4), dict(depth=FAKE + 2),
           dict(normals=FAKE + 1)]
    for kw in bad:
        assert lib.edv_icp_scaled_sums(*{**ok, **kw}.values(), None) != 0, kw
        assert lib.edv_last_error(), kw
