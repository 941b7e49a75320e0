"""CPU: camera tracking against the fused surface, on the numpy mirror (``fusion.TsdfHost.track`` / ``track_clip``, ``fusion.icp_sums_host``) and at
the C boundary (the refusals of ``edv_icp_sums`` launch nothing, so they need no GPU).  The GPU tests hold the kernel to this mirror bit for bit
(tests/test_track_gpu.py); what the tracker converges to is checked here alone."""
import ctypes as C
import math

import numpy as np
import pytest

import endodav_amd
from endodav_amd import _lib, fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Raycast, Track, Tracked, TsdfHost, Views
from tests import track_cases as tc


# ---- 1. convergence -----------------------------------------------------------------------------------------------------------------------------
def test_single_frame_converges():
    """The guess is the identity, the truth 3.9e-2 rad and 2.7e-2 away.  Measured on the mirror: 1.3e-2 rad and 1.0e-2 after one step, 6.9e-4 and
    3.9e-4 after two, 9.4e-4 rad and 4.5e-4 from the third on (41 and 59 times closer than the guess), with 1951 pairs of 2240 pixels and an
    rms of 5.2e-4.  What remains is set by nearest-pixel association and the voxel size, not by the solver; the condition asks for a tenth."""
    live, truth = tc.single()
    start = tc.errors(np.eye(4), truth)
    assert 3.8e-2 < start[0] < 4.0e-2 and 2.6e-2 < start[1] < 2.8e-2
    T, pairs, rms, lost = tc.fused().track(live, tc.spec(), tc.track())
    end = tc.errors(T, truth)
    print(f"\nrotation {start[0]:.3e} -> {end[0]:.3e} rad, translation {start[1]:.3e} -> {end[1]:.3e}; {pairs} pairs, rms {rms:.3e}")
    assert not lost and T.shape == (4, 4) and T.dtype == np.float64
    assert end[0] <= 0.1 * start[0] and end[1] <= 0.1 * start[1]
    assert 64 <= pairs <= tc.H * tc.W and 0.0 < rms < 0.1
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)     # the rotation comes back orthonormal
    assert isinstance(pairs, int) and isinstance(rms, float) and isinstance(lost, bool)


def test_five_frames_are_tracked_and_fused():
    """Frame i is i times a motion of 2.1e-2 rad and 1.6e-2.  Measured on the mirror: frame 1 ends 1.1e-3 rad and 6.1e-5 from its truth, frame 2
    1.0e-3 and 5.2e-4, frame 3 2.1e-3 and 7.2e-4, frame 4 3.0e-3 and 1.2e-3 (of 8.3e-2 and 6.2e-2); 2009, 1954, 1891 and 1825 pairs."""
    depth, truth = tc.clip()
    host = TsdfHost(tc.volume(), coloured=False)
    got = host.track_clip(depth, tc.spec(), tc.track())
    assert isinstance(got, Tracked) and got.poses.shape == (5, 4, 4) and got.poses.dtype == np.float64
    assert got.pairs.dtype == np.int64 and got.rms.dtype == np.float64 and got.lost.dtype == np.bool_
    assert np.array_equal(got.poses[0], np.eye(4)) and got.pairs[0] == 0 and got.rms[0] == 0.0
    assert not got.lost.any()
    for i in range(1, 5):
        moved, end = tc.errors(np.eye(4), truth[i]), tc.errors(got.poses[i], truth[i])
        print(f"\nframe {i}: rotation {moved[0]:.3e} -> {end[0]:.3e} rad, translation {moved[1]:.3e} -> {end[1]:.3e}; {got.pairs[i]} pairs, rms {got.rms[i]:.3e}")
        assert end[0] <= 0.1 * moved[0] and end[1] <= 0.1 * moved[1]
    once = TsdfHost(tc.volume(), coloured=False)                    # every frame was integrated: the weights say so
    once.integrate(depth[:1], tc.spec())
    assert host.weight.max() == 5.0 and host.weight.sum() > 3.0 * once.weight.sum()


# ---- 2. the sums --------------------------------------------------------------------------------------------------------------------------------
def _pairs_one_by_one(depth, spec, cast, views, max_dist2):
    """The number of pairs of frame 0, the rule applied to one pixel at a time in Python floats: independent of the vectorised mirror."""
    cam = spec.cams(1)[0]
    mc = np.concatenate([views.cams()[0], fusion.cameras(Cloud(K=views.K, pose=views.pose), 1)[0]])
    lo, span, gain, near, far = spec.scalars()
    step = int(spec.step)
    h, w = depth.shape[1:]
    mh, mw = views.size
    count = 0
    for oy in range(-(-h // step)):
        for ox in range(-(-w // step)):
            z = depth[0, min(oy * step + step // 2, h - 1), min(ox * step + step // 2, w - 1)] * gain
            if not (z > near and z < far):
                continue
            u, v, z = (ox + 0.5) * step, (oy + 0.5) * step, float(z)
            l = [(cam[3 * i] * u + cam[3 * i + 1] * v) + cam[3 * i + 2] for i in range(3)]
            P = [cam[18 + i] + ((cam[9 + 3 * i] * l[0] + cam[10 + 3 * i] * l[1]) + cam[11 + 3 * i] * l[2]) * z for i in range(3)]
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
            D = [(mc[18 + i] + ((mc[9 + 3 * i] * lm[0] + mc[10 + 3 * i] * lm[1]) + mc[11 + 3 * i] * lm[2]) * dm) - P[i] for i in range(3)]
            count += (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2] <= max_dist2
    return count


@pytest.mark.parametrize("step", [1, 3])
def test_the_ordered_sum_drops_nothing(step):
    """Against ``math.fsum`` of the same per-pixel terms each of the 28 real sums lies within n * 2^-53 * sum|terms|, n the pixel count: the bound
    of any order of fp64 additions.  The count is exact."""
    live, _ = tc.single()
    cast, views = tc.model()
    spec = tc.spec(step=step)
    sums = fusion.icp_sums_host(live, spec, cast, views, 0.1)
    assert sums.shape == (29,) and sums.dtype == np.float64
    ctx = fusion._IcpHost(live, spec, cast, views, 0.1, 0)
    terms = ctx.terms(fusion._estimate(ctx, spec, 0))
    n = terms.shape[0]
    assert n == (-(-tc.H // step)) * (-(-tc.W // step)) and terms.shape[1] == 29
    for j in range(28):
        exact, bound = math.fsum(terms[:, j]), n * 2.0 ** -53 * math.fsum(np.abs(terms[:, j]))
        assert abs(sums[j] - exact) <= bound, (j, sums[j], exact, bound)
    pairs = _pairs_one_by_one(live, spec, cast, views, 0.1 * 0.1)
    assert sums[28] == pairs and 0.5 * n < pairs < n
    assert sums[27] > 0.0 and all(sums[j] > 0.0 for j in (0, 6, 11, 15, 18, 20))     # the diagonal of J J^T


def test_the_order_is_the_tiles_waves_and_butterfly():
    """On terms whose sum depends on the order, the mirror's total is the one include/endodav_hip.h states, spelt out lane by lane."""
    rng = np.random.default_rng(3)
    terms = rng.standard_normal((600, 29)) * 10.0 ** rng.integers(-8, 8, (600, 29))
    padded = np.zeros((768, 29))
    padded[:600] = terms
    tiles = []
    for b in range(3):
        waves = []
        for wv in range(4):
            x = [padded[256 * b + 64 * wv + lane] for lane in range(64)]
            for s in (32, 16, 8, 4, 2, 1):
                x = [x[lane] + x[lane ^ s] for lane in range(64)]
            assert all(np.array_equal(x[0], other) for other in x)
            waves.append(x[0])
        tiles.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    want = (tiles[0] + tiles[1]) + tiles[2]
    assert np.array_equal(tc.bits(fusion._ordered_sum(terms)), tc.bits(want))
    assert not np.array_equal(tc.bits(want), tc.bits(terms.sum(axis=0)))                # the order matters for these terms


# ---- 3. lost ------------------------------------------------------------------------------------------------------------------------------------
def test_lost_cases():
    live, truth = tc.single()
    cast, views = tc.model()
    zeros = tc.bits(np.zeros(29))
    missed = Raycast(np.zeros_like(cast.depth), np.zeros_like(cast.normals), None)
    sums = fusion.icp_sums_host(live, tc.spec(), missed, views, 0.1)
    assert np.array_equal(tc.bits(sums), zeros) and fusion.icp_solve(sums, 64) is None and fusion.icp_solve(sums, 1) is None
    sums = fusion.icp_sums_host(live, tc.spec(pose=tc.AWAY), cast, views, 0.1)           # every q_2 <= 0
    assert np.array_equal(tc.bits(sums), zeros) and fusion.icp_solve(sums, 64) is None
    empty = TsdfHost(tc.volume(), coloured=False)                                        # nothing fused: the ray-cast misses everywhere
    for host, spec, track in ((empty, tc.spec(), tc.track()), (tc.fused(), tc.spec(pose=tc.AWAY), tc.track())):
        T, pairs, rms, lost = host.track(live, spec, track)
        assert lost and pairs == 0 and math.isnan(rms) and np.array_equal(T, fusion._pose4(spec.pose[0]))
    T, pairs, rms, lost = tc.fused().track(live, tc.spec(), tc.track(min_pairs=tc.H * tc.W))
    assert lost and 64 < pairs < tc.H * tc.W and rms > 0.0 and np.array_equal(T, np.eye(4))
    sums = fusion.icp_sums_host(live, tc.spec(), cast, views, 0.1)
    assert fusion.icp_solve(sums, int(sums[28])) is not None and fusion.icp_solve(sums, int(sums[28]) + 1) is None
    flat = sums.copy()                                                                   # a singular system, and one whose solution is not finite
    flat[:21] = 0.0
    assert fusion.icp_solve(flat, 1) is None
    flat[21] = np.nan
    assert fusion.icp_solve(flat, 1) is None
    depth, _ = tc.clip()                                                                 # a lost frame keeps the previous pose and is not integrated
    host = TsdfHost(tc.volume(), coloured=False)
    got = host.track_clip(depth[:3], tc.spec(), tc.track(min_pairs=tc.H * tc.W))
    assert list(got.lost) == [False, True, True] and np.array_equal(got.poses, np.stack([np.eye(4)] * 3)) and (got.pairs[1:] > 64).all()
    assert np.array_equal(host.weight, tc.fused().weight) and np.array_equal(host.tsdf, tc.fused().tsdf)


def test_apply_twist_and_solve():
    T = tc.pose((0.3, -0.2, 0.5), (1.0, 2.0, 3.0))
    assert np.array_equal(fusion.apply_twist(T, np.zeros(6)), T)                         # theta = 0 is the identity
    moved = fusion.apply_twist(T, [0.0, 0.0, 0.0, 0.5, -0.5, 0.25])
    assert np.array_equal(moved[:3, :3], T[:3, :3]) and np.array_equal(moved[:3, 3], [1.5, 1.5, 3.25])
    quarter = fusion.apply_twist(np.eye(4), [0.0, 0.0, math.pi / 2.0, 0.0, 0.0, 0.0])    # Rodrigues: a quarter turn about z takes x to y
    assert np.allclose(quarter[:3, :3] @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], atol=1e-15)
    turned = fusion.apply_twist(T, [0.1, 0.2, -0.3, 0.0, 0.0, 0.0])                      # about the camera centre: t stays
    assert np.array_equal(turned[:3, 3], T[:3, 3]) and np.allclose(turned[:3, :3] @ turned[:3, :3].T, np.eye(3), atol=1e-15)
    rng = np.random.default_rng(0)                                                       # the 29 sums hold the upper triangle row-major, then J e
    J, e = rng.standard_normal((100, 6)), rng.standard_normal(100)
    A, b = J.T @ J, J.T @ e
    sums = np.concatenate([A[np.triu_indices(6)], b, [e @ e, 100.0]])
    assert np.allclose(fusion.icp_solve(sums, 64), np.linalg.solve(A, b), rtol=1e-12, atol=0.0)


# ---- 4. validation ------------------------------------------------------------------------------------------------------------------------------
def test_track_validates_its_fields():
    t = Track(near=0.2, far=1.2)
    assert (t.step, t.iterations, t.max_dist, t.min_pairs, t.min_weight) == (None, 6, None, 64, 1.0)
    with pytest.raises(TypeError):
        Track(0.2, 1.2)                                                                  # keyword only
    with pytest.raises(TypeError):
        Track(near=0.2)
    bad = [dict(near=-0.1), dict(near=1.2), dict(near=float("nan")), dict(far=float("inf")), dict(near="0"), dict(step=0.0), dict(step=float("inf")), dict(step=True),
           dict(iterations=0), dict(iterations=2.0), dict(iterations=True), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")),
           dict(min_pairs=0), dict(min_pairs=6.5), dict(min_weight=-1.0), dict(min_weight=float("nan")), dict(min_weight=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError):
            Track(**{**dict(near=0.2, far=1.2), **kw})
    with pytest.raises(ValueError, match="samples"):
        tc.fused().track(tc.single()[0], tc.spec(), Track(near=0.0, far=100.0, step=1e-4))


def test_the_python_layer_refuses_bad_arguments():
    live, _ = tc.single()
    cast, views = tc.model()
    host, ok = tc.fused(), dict(depth=live, spec=tc.spec(), model=cast, views=views, max_dist=0.1)
    two = Views(tc.K, np.stack([np.eye(4)] * 2), size=(tc.H, tc.W), near=0.2, far=1.2)
    bad = [dict(depth=live.astype(np.float64)), dict(depth=live[0]), dict(spec=None), dict(frame=1), dict(frame=-1), dict(frame=0.0), dict(views=two), dict(views=None),
           dict(model=Raycast(cast.depth, None, None)), dict(model=Raycast(cast.depth[:, :-1], cast.normals, None)), dict(model=cast.depth),
           dict(model=Raycast(cast.depth, cast.normals.astype(np.float64), None)), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=None),
           dict(spec=tc.spec(mask=np.ones((3, 3), bool))), dict(spec=Cloud(K=np.stack([tc.K] * 2), source="depth"))]
    for kw in bad:
        with pytest.raises(ValueError):
            fusion.icp_sums_host(**{**ok, **kw})
    for kw in (dict(track=None), dict(track=dict(tc.TRACK)), dict(frame=1), dict(depth=live[0])):
        with pytest.raises(ValueError):
            host.track(**{**dict(depth=live, spec=tc.spec(), track=tc.track()), **kw})
    fresh = TsdfHost(tc.volume(), coloured=False)
    poses = np.stack([np.eye(4)] * 5)
    for kw in (dict(spec=tc.spec(pose=poses)), dict(spec=tc.spec(step=2)), dict(track=None), dict(frames=np.zeros((5, tc.H, tc.W, 3), np.uint8))):
        with pytest.raises(ValueError):
            fresh.track_clip(**{**dict(depth=tc.clip()[0], spec=tc.spec(), track=tc.track()), **kw})
    assert fresh.weight.max() == 0.0                                                     # refused before anything was integrated


def test_video_surface_refuses_before_inference():
    """On the CPU nothing can be inferred: every refusal below comes before the network is touched."""
    model = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(42, 56), lora_type="none", disable_conv_head=True).eval()
    frames = np.zeros((3, 42, 56, 3), np.uint8)
    several = Cloud(K=tc.K, pose=np.stack([np.eye(4)] * 3))
    with pytest.raises(ValueError, match="one pose"):
        model.video_surface(frames, several, tc.volume(), device="cpu", track=tc.track())
    with pytest.raises(ValueError, match="Track"):
        model.video_surface(frames, Cloud(K=tc.K), tc.volume(), device="cpu", track=dict(tc.TRACK))
    with pytest.raises(ValueError, match="samples"):
        model.video_surface(frames, Cloud(K=tc.K), tc.volume(), device="cpu", track=Track(near=0.0, far=100.0, step=1e-4))


# ---- 5. the C boundary --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    lib = _lib.load()
    assert lib.edv_abi_version() == 15 == _lib.ABI_VERSION
    for name in ("edv_icp_tile_pixels", "edv_icp_workspace", "edv_icp_sums"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.edv_icp_tile_pixels() == 256 == fusion.ICP_TILE
    assert _lib.SIGNATURES["edv_icp_sums"][1][2:4] == [C.POINTER(C.c_double)] * 2       # the cameras are host arrays


def test_workspace_size():
    lib = _lib.load()
    for h, w, step in ((1, 1, 1), (16, 16, 1), (17, 33, 1), (17, 33, 3), (40, 56, 1), (518, 518, 1), (518, 518, 4), (5, 7, 100), (46340, 46340, 1)):
        oh, ow = -(-h // step), -(-w // step)
        assert lib.edv_icp_workspace(h, w, step) == 29 * 8 * -(-(oh * ow) // 256), (h, w, step)
    for h, w, step in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, 0), (5, 5, -1), (2 ** 16, 2 ** 15, 1), (46341, 46341, 1)):
        assert lib.edv_icp_workspace(h, w, step) == 0, (h, w, step)


def test_refusals_launch_nothing():
    """Every call below is refused before anything is launched (there is no GPU here) and before either camera array is read.  The pointers are
    made-up addresses with the alignment a real one has; none is dereferenced."""
    lib = _lib.load()
    FAKE = 0x10000
    live, model_cam = (C.c_double * 21)(), (C.c_double * 39)()

    def sel(**kw):
        fields = dict(x_dev=FAKE, n=3, h=40, w=56, step=1, mode=0, lo=0.0, span=1.0, gain=1.0, near_z=0.001, far_z=10.0, mask_dev=None, mask_stride=0)
        fields.update(kw)
        return C.byref(_lib.CloudSelection(*fields.values()))

    need = lib.edv_icp_workspace(40, 56, 1)
    ok = dict(sel=sel(), frame=0, live=live, model=model_cam, depth=FAKE, normals=FAKE, mh=40, mw=56, max_dist2=0.01, sums=FAKE, ws=FAKE, ws_bytes=need)
    bad = [dict(sel=None), dict(live=None), dict(model=None), dict(depth=None), dict(normals=None), dict(sums=None), dict(ws=None),
           dict(frame=-1), dict(frame=3), dict(frame=2 ** 40),
           dict(sel=sel(step=0)), dict(sel=sel(step=-2)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)), dict(sel=sel(n=65536)), dict(sel=sel(h=0)), dict(sel=sel(w=-1)),
           dict(sel=sel(h=2 ** 16, w=2 ** 15)), dict(sel=sel(mode=2)), dict(sel=sel(mask_dev=FAKE, mask_stride=7)), dict(sel=sel(x_dev=FAKE + 2)),
           dict(mh=0), dict(mw=0), dict(mh=-3), dict(mh=2 ** 16, mw=2 ** 15),
           dict(max_dist2=-1.0), dict(max_dist2=float("nan")), dict(max_dist2=float("inf")), dict(max_dist2=-float("inf")),
           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=FAKE + 4), dict(sums=FAKE + 4), dict(depth=FAKE + 2), dict(normals=FAKE + 1)]
    for kw in bad:
        assert lib.edv_icp_sums(*{**ok, **kw}.values(), None) != 0, kw
        assert lib.edv_last_error(), kw
