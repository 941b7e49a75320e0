"""Surface fusion without a GPU: ``fusion.TsdfHost``, the numpy mirror the kernels are held to, against a slow scalar reference written here,
against exact geometry, and at its edges; then every refusal of ``Volume``, ``integrate`` and ``surface``."""
import numpy as np
import pytest

from endodav_amd import fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import TsdfHost, Volume
from tests import cloud_cases as cases
from tests import fusion_cases as fc

F32, F64 = np.float32, np.float64


# ---- a. the slow reference --------------------------------------------------------------------------------------------------------------------
def _slow_integrate(vol, state, depth, spec, frames):
    """include/endodav_hip.h, edv_tsdf_integrate, one scalar at a time."""
    tsdf, weight, color = state
    nx, ny, nz = vol.dims
    n, h, w = depth.shape
    cams = fusion.cameras(spec, n)
    lo, span, gain, near, far = spec.scalars()
    origin, voxel, trunc, cap = [F64(o) for o in vol.origin], F64(vol.voxel), F64(vol.trunc), F32(vol.max_weight)
    mask = spec.frame_mask(n, h, w)
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                c = [origin[k] + (F64(i) + F64(0.5)) * voxel for k, i in enumerate((ix, iy, iz))]
                for f in range(n):
                    cam = cams[f if cams.shape[0] > 1 else 0]
                    W, K = cam[:12].reshape(3, 4), cam[12:].reshape(2, 3)
                    q = [((W[i, 0] * c[0] + W[i, 1] * c[1]) + W[i, 2] * c[2]) + W[i, 3] for i in range(3)]
                    if not q[2] > 0:
                        continue
                    u = ((K[0, 0] * q[0] + K[0, 1] * q[1]) + K[0, 2] * q[2]) / q[2]
                    v = ((K[1, 0] * q[0] + K[1, 1] * q[1]) + K[1, 2] * q[2]) / q[2]
                    if not (u >= 0 and u < w and v >= 0 and v < h):
                        continue
                    px, py = int(u), int(v)
                    x = F32(depth[f, py, px])
                    if spec.source == "depth":
                        z = x * gain
                    else:
                        scaled = lo + span * x
                        z = F32(1.0) / scaled
                        z = z * gain
                    m = 1 if mask is None else int((mask[f] if mask.ndim == 3 else mask)[py, px])
                    if not (m != 0 and z > near and z < far):
                        continue
                    sdf = F64(z) - q[2]
                    if sdf < -trunc:
                        continue
                    r = sdf / trunc
                    d = F32(r if r < 1.0 else F64(1.0))
                    wt = weight[iz, iy, ix]
                    wn = wt + F32(1.0)
                    tsdf[iz, iy, ix] = (tsdf[iz, iy, ix] * wt + d) / wn
                    if color is not None:
                        for ch in range(3):
                            color[iz, iy, ix, ch] = (color[iz, iy, ix, ch] * wt + F32(frames[f, py, px, ch])) / wn
                    weight[iz, iy, ix] = wn if wn < cap else cap


def _slow_surface(vol, state, min_weight):
    tsdf, weight, color = state
    nx, ny, nz = vol.dims
    origin, voxel, mw = [F64(o) for o in vol.origin], F64(vol.voxel), F32(min_weight)
    points, colors = [], []
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                i = (ix, iy, iz)
                for k in range(3):
                    j = [ix, iy, iz]
                    j[k] += 1
                    if j[k] >= vol.dims[k]:
                        continue
                    ta, tb = tsdf[iz, iy, ix], tsdf[j[2], j[1], j[0]]
                    if not (weight[iz, iy, ix] >= mw and weight[j[2], j[1], j[0]] >= mw and (ta < 0) != (tb < 0)):
                        continue
                    t = ta / (ta - tb)
                    points.append([F32(origin[a] + ((F64(i[a]) + F64(0.5)) + F64(t) if a == k else F64(i[a]) + F64(0.5)) * voxel) for a in range(3)])
                    if color is not None:
                        ca, cb = color[iz, iy, ix], color[j[2], j[1], j[0]]
                        c = [ca[ch] + t * (cb[ch] - ca[ch]) for ch in range(3)]
                        colors.append([np.uint8(min(F32(255), max(F32(0), np.floor(v + F32(0.5))))) for v in c])
    return np.array(points, F32).reshape(-1, 3), (np.array(colors, np.uint8).reshape(-1, 3) if color is not None else None)


@pytest.mark.parametrize("source,per_frame,kind", [("depth", True, "per-frame"), ("disparity", False, "shared")])
def test_the_mirror_equals_a_slow_scalar_reference(source, per_frame, kind):
    vol, spec, depth, frames = fc.case((4, 3, 5), (2, 6, 8), source, per_frame, kind, seed=3)
    host = TsdfHost(vol, coloured=True)
    host.integrate(depth, spec, frames)
    slow = TsdfHost(vol, coloured=True).arrays()
    with np.errstate(all="ignore"):
        _slow_integrate(vol, slow, depth, spec, frames)
    touched = int((slow[1] > 0).sum())
    assert 0 < touched < vol.voxels and (slow[1] > 1).any()
    fc.same_state(host.arrays(), slow)
    got = host.surface(min_weight=1.0)
    with np.errstate(all="ignore"):
        points, colors = _slow_surface(vol, slow, 1.0)
    assert len(got) == points.shape[0] > 0
    assert np.array_equal(fc.bits(got.points), fc.bits(points)) and np.array_equal(got.colors, colors)
    assert np.array_equal(got.offsets, [0, points.shape[0]])


# ---- b. exact plane -----------------------------------------------------------------------------------------------------------------------------
Z0 = 1.0 + 1.0 / 64.0
PLANE_K = np.array([[8.0, 0.0, 4.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]])


def _plane_volume():
    """x, y in [-1/4, 1/4], z in [1/2, 3/2], voxels of 1/16: dyadic throughout, and wholly inside the frustum of an 8 x 8 image with focal
    length 8 (|x| < z / 2) placed at the origin."""
    return Volume(origin=(-0.25, -0.25, 0.5), voxel=1.0 / 16.0, dims=(8, 8, 16))


def _plane_crossings(cloud):
    """z-axis crossings only, one per (x, y) column in voxel order; returns their z."""
    assert len(cloud) == 64 and cloud.colors is None
    centres = -0.25 + (np.arange(8) + 0.5) / 16.0
    assert np.array_equal(cloud.points[:, 0], np.tile(centres, 8).astype(F32)) and np.array_equal(cloud.points[:, 1], np.repeat(centres, 8).astype(F32))
    return cloud.points[:, 2].astype(F64)


def test_a_plane_seen_head_on_is_recovered_exactly():
    vol = _plane_volume()
    depth = np.full((1, 8, 8), Z0, F32)
    host = TsdfHost(vol, coloured=False)
    host.integrate(depth, Cloud(K=PLANE_K, source="depth"))
    tsdf, weight, _ = host.arrays()
    assert (weight[:8] == 1).all()                       # the whole volume is inside the frustum, and nothing in front of the plane is skipped
    assert (weight[-3:] == 0).all()                      # more than trunc = 1/4 behind it
    # five fp32 roundings on the path (d of either voxel, their difference, the quotient, the point): about 5 * 2^-24 against a bound of 1e-5
    z = _plane_crossings(host.surface())
    assert np.abs(z - Z0).max() <= 1e-5 * Z0
    # a second view from a pose translated along x: the plane is where it was, and still no crossing along x or y although only part of the
    # volume is seen twice
    pose = np.eye(4)
    pose[0, 3] = 0.125
    host.integrate(depth, Cloud(K=PLANE_K, source="depth", pose=pose))
    _, weight2, _ = host.arrays()
    assert (weight2 == 2).any() and (weight2[:8] == 1).any()
    z2 = _plane_crossings(host.surface())
    assert np.abs(z2 - Z0).max() <= 1e-5 * Z0 and np.abs(z2 - z).max() <= 1e-5 * Z0


# ---- c. weights, split calls, skipped voxels -----------------------------------------------------------------------------------------------------
def test_the_weight_stops_at_max_weight():
    vol, spec, depth, frames = fc.case((5, 3, 2), (1, 6, 8), max_weight=2.0)
    clip, rgb = np.repeat(depth, 3, axis=0), np.repeat(frames, 3, axis=0)
    host = TsdfHost(vol)
    host.integrate(clip, spec, rgb)
    _, weight, _ = host.arrays()
    assert set(np.unique(weight)) == {0.0, 2.0}
    uncapped = TsdfHost(Volume(vol.origin, vol.voxel, vol.dims))
    uncapped.integrate(clip, spec, rgb)
    assert set(np.unique(uncapped.arrays()[1])) == {0.0, 3.0}


@pytest.mark.parametrize("per_frame", [False, True])
def test_one_call_equals_consecutive_calls_with_the_halves(per_frame):
    shape = (4, 6, 8)
    vol, spec, depth, frames = fc.case((9, 5, 4), shape, "depth", per_frame, "per-frame", seed=7)
    whole = TsdfHost(vol)
    whole.integrate(depth, spec, frames)
    assert (whole.arrays()[1] > 1).any()
    halves = TsdfHost(vol)
    for part in (slice(0, 2), slice(2, 4)):
        sub = Cloud(K=spec.K[part] if per_frame else spec.K, pose=spec.pose[part] if per_frame else spec.pose, source="depth", far=fc.FAR, mask=spec.mask[part])
        halves.integrate(depth[part], sub, frames[part])
    fc.same_state(halves.arrays(), whole.arrays())
    fc.same_cloud(halves.surface(), whole.surface())


def _fresh(host):
    tsdf, weight, color = host.arrays()
    return (tsdf == 1).all() and (weight == 0).all() and (color == 0).all()


def test_skipped_voxels_stay_fresh():
    K = PLANE_K
    depth, rgb = np.full((1, 8, 8), 1.0, F32), cases.colours((1, 8, 8))
    inside = _plane_volume()
    seen = TsdfHost(inside)
    seen.integrate(depth, Cloud(K=K, source="depth"), rgb)
    assert (seen.arrays()[1] == 1).sum() > 0                                            # the control: this view does update the volume
    behind = TsdfHost(Volume(origin=(-0.25, -0.25, -1.5), voxel=1.0 / 16.0, dims=(8, 8, 16)))      # z in [-3/2, -1/2]
    behind.integrate(depth, Cloud(K=K, source="depth"), rgb)
    assert _fresh(behind)
    aside = TsdfHost(Volume(origin=(2.0, -0.25, 0.5), voxel=1.0 / 16.0, dims=(8, 8, 16)))           # x >= 2 > z / 2
    aside.integrate(depth, Cloud(K=K, source="depth"), rgb)
    assert _fresh(aside)
    masked = TsdfHost(inside)
    masked.integrate(depth, Cloud(K=K, source="depth", mask=np.zeros((8, 8), bool)), rgb)
    assert _fresh(masked)
    for bad in (np.nan, np.inf, -np.inf, 0.0):
        broken = TsdfHost(inside)
        with np.errstate(all="ignore"):
            broken.integrate(np.full((1, 8, 8), bad, F32), Cloud(K=K, source="depth", far=np.inf), rgb)
        assert _fresh(broken)
    far_behind = TsdfHost(inside)                                                       # the surface at 1/8: every voxel is more than 1/4 behind it
    far_behind.integrate(np.full((1, 8, 8), 0.125, F32), Cloud(K=K, source="depth"), rgb)
    assert _fresh(far_behind)
    # partly: voxels more than trunc behind the plane at 1 keep their bits, the others do not
    tsdf, weight, color = seen.arrays()
    cz = 0.5 + (np.arange(16) + 0.5) / 16.0
    assert np.array_equal(weight[:, 0, 0] == 0, 1.0 - cz < -0.25) and (tsdf[weight == 0] == 1).all() and (color[weight == 0] == 0).all()


# ---- d. extraction order and colour -------------------------------------------------------------------------------------------------------------------
def test_extraction_order_and_colour_rounding():
    vol = Volume(origin=(0.0, 0.0, 0.0), voxel=1.0, dims=(2, 2, 2))
    host = TsdfHost(vol)
    host.weight[:] = 1
    host.tsdf[:] = 0.5
    host.tsdf[0, 0, 0] = -0.5                    # voxel 0 crosses towards x, y and z, in that order
    host.tsdf[1, 1, 0] = -0.25                   # voxel 6 = (0, 1, 1) crosses towards x; voxels 2 and 4 cross into it along z and y
    host.color[0, 0, 0] = (10.0, 20.0, 254.6)
    host.color[0, 0, 1] = (11.0, 300.0, 255.9)   # the +x neighbour of voxel 0
    got = host.surface()
    want = np.array([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0],     # voxel 0: x, y, z at t = 1/2
                     [0.5, 1.5, 0.5 + 2.0 / 3.0],                           # voxel 2 = (0, 1, 0) along z: t = 0.5 / 0.75
                     [0.5, 0.5 + 2.0 / 3.0, 1.5],                           # voxel 4 = (0, 0, 1) along y
                     [0.5 + 1.0 / 3.0, 1.5, 1.5]], F64)                     # voxel 6 along x: t = -0.25 / -0.75
    assert np.array_equal(got.offsets, [0, 6]) and np.abs(got.points - want).max() < 1e-6
    assert np.array_equal(got.points[:3], want[:3].astype(F32))
    # t = 1/2: 10.5 -> floor(11.0) = 11; (20 + 300) / 2 = 160; 255.25 -> floor(255.75) = 255; a colour above 255 is clamped
    assert list(got.colors[0]) == [11, 160, 255]
    host.color[0, 0, 0] = (-3.0, 600.0, 0.49)
    host.color[0, 0, 1] = (-3.0, 600.0, 0.49)
    assert list(host.surface().colors[0]) == [0, 255, 0]
    # zero and minus zero are outside: no crossing against a positive neighbour, one against a negative neighbour
    for zero in (0.0, -0.0):
        flat = TsdfHost(Volume(origin=(0.0, 0.0, 0.0), voxel=1.0, dims=(3, 1, 1)), coloured=False)
        flat.weight[:] = 1
        flat.tsdf[0, 0] = (0.5, zero, -0.5)
        got = flat.surface()
        assert len(got) == 1 and got.colors is None and np.array_equal(got.points, np.array([[1.5, 0.5, 0.5]], F32))     # t = 0 / (0 + 0.5)
    # a pair counts only when both weights reach min_weight
    host.weight[0, 0, 1] = 0.5
    assert len(host.surface(min_weight=1.0)) == 5 and len(host.surface(min_weight=0.5)) == 6 and len(host.surface(min_weight=2.0)) == 0


# ---- e. validation --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(origin=(0, 0)), dict(origin=(0, 0, np.nan)), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=np.inf), dict(voxel="1"),
                                dict(dims=(4, 4)), dict(dims=(4, 0, 4)), dict(dims=(4, 4, 2.0)), dict(dims=(2048, 1024, 1024)), dict(dims=4),
                                dict(trunc=0.0), dict(trunc=np.nan), dict(max_weight=0.0), dict(max_weight=np.inf), dict(max_weight=1e-50)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_volume_refuses(kw):
    good = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, dims=(4, 4, 4))
    Volume(**good)
    with pytest.raises(ValueError):
        Volume(**{**good, **kw})


def test_volume_defaults_and_bounding():
    vol = Volume(origin=[1, 2, 3], voxel=0.25, dims=np.array([4, 5, 6]))
    assert vol.trunc == 1.0 and vol.max_weight == 64.0 and vol.dims == (4, 5, 6) and vol.voxels == 120 and vol.origin == (1.0, 2.0, 3.0)
    assert Volume(origin=(0, 0, 0), voxel=0.25, dims=(1, 1, 1), trunc=0.1).trunc == 0.1
    assert Volume(origin=(0, 0, 0), voxel=1.0, dims=(2047, 1024, 1024)).voxels < 2 ** 31
    points = np.random.default_rng(0).uniform(-3.0, 5.0, (200, 3))
    for voxel, margin in ((0.1, None), (0.37, 0.0), (1.0, 2.5)):
        vol = Volume.bounding(points, voxel, margin=margin)
        lo, hi = np.asarray(vol.origin), np.asarray(vol.origin) + np.asarray(vol.dims) * vol.voxel
        pad = 4 * voxel if margin is None else margin
        assert (lo <= points.min(axis=0) - pad).all() and (hi >= points.max(axis=0) + pad).all() and (hi - points.max(axis=0) - pad < 2 * voxel).all()
    assert Volume.bounding(np.zeros((1, 3)), 0.5, margin=0.0).dims == (1, 1, 1)
    for bad in (np.zeros((0, 3)), np.zeros((4, 2)), np.full((2, 3), np.nan)):
        with pytest.raises(ValueError):
            Volume.bounding(bad, 0.5)
    with pytest.raises(ValueError):
        Volume.bounding(points, 0.0)
    with pytest.raises(ValueError):
        Volume.bounding(points, 0.5, margin=-1.0)


def test_integrate_and_surface_refuse():
    vol, spec, depth, frames = fc.case((5, 3, 2), (3, 6, 8))
    host = TsdfHost(vol)
    K, before = spec.K[0], host.arrays()
    bad_K = K.copy()
    bad_K[2] = (0.0, 1e-3, 1.0)
    for args, match in [((depth, Cloud(K=K, step=2, source="depth"), frames), "step"),
                        ((depth, Cloud(K=bad_K, source="depth"), frames), "last row"),
                        ((depth[:0], spec, frames[:0]), "frames per call"),
                        ((depth, spec, None), "coloured"),
                        ((depth, None, frames), "spec"),
                        ((depth.astype(F64), spec, frames), "float32"),
                        ((depth, spec, frames[:2]), "frames"),
                        ((depth, Cloud(K=np.stack([K, K]), source="depth"), frames), "matrices"),
                        ((depth, Cloud(K=K, source="depth", mask=np.ones((5, 5), bool)), frames), "mask")]:
        with pytest.raises(ValueError, match=match):
            host.integrate(*args)
    with pytest.raises(ValueError, match="coloured"):
        TsdfHost(vol, coloured=False).integrate(depth, spec, frames)
    with pytest.raises(ValueError, match="frames per call"):      # refused from the shape alone, before any element is read
        host.integrate(np.broadcast_to(F32(1.0), (65536, 6, 8)), spec, np.broadcast_to(np.uint8(0), (65536, 6, 8, 3)))
    fc.same_state(host.arrays(), before)
    for kw in (dict(min_weight=np.nan), dict(min_weight=-1.0), dict(min_weight=np.inf), dict(min_weight="1"), dict(output="disk")):
        with pytest.raises(ValueError):
            host.surface(**kw)
    with pytest.raises(ValueError, match="Volume"):
        TsdfHost((4, 4, 4))
    with pytest.raises(ValueError, match="GPU"):
        fusion.Tsdf(vol, device="cpu")
