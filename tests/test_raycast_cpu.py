"""Views of the fused surface without a GPU: ``fusion.TsdfHost.raycast`` against a scalar reference written here straight from the rule of the
``fusion`` module docstring (one ray at a time, Python floats for float64 and ``np.float32`` scalars for float32), then against geometry it does not
know (a plane, a sphere), the edges of the rule, and the refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import endodav_amd
from endodav_amd import _lib, fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Raycast, TsdfHost, Views, Volume
from tests import fusion_cases as fc
from tests import mesh_cases as mc
from tests import raycast_cases as rc

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the scalar reference ------------------------------------------------------------------------------------------------------------------------------
def reference(host, views, min_weight=1.0, normals=True):
    """(Raycast, brackets): the rule, one ray at a time.  ``brackets[(f, y, x)]`` lists the voxels (ix, iy, iz) the two samples around a hit read."""
    vol = host.volume
    n = vol.dims
    step, steps = views.march(vol.voxel)
    cams, inv, near = views.cams(), 1.0 / vol.voxel, views.near
    h, w = views.size
    mw = F32(min_weight)
    depth = np.zeros((views.count, h, w), F32)
    unit = np.zeros((views.count, h, w, 3), F32) if normals else None
    colors = np.zeros((views.count, h, w, 3), np.uint8) if host.color is not None else None
    brackets = {}

    def cell(g):
        c = [min(max(int(g[i]), 0), n[i] - 2) for i in range(3)]
        return c, [F32(g[i] - float(c[i])) for i in range(3)]

    def corners(c):
        return [(c[0] + dx, c[1] + dy, c[2] + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]

    def interpolate(q, f):                                        # q: the eight values, x fastest, as np.float32
        a00, a10 = q[0] + f[0] * (q[1] - q[0]), q[2] + f[0] * (q[3] - q[2])
        a01, a11 = q[4] + f[0] * (q[5] - q[4]), q[6] + f[0] * (q[7] - q[6])
        b0, b1 = a00 + f[1] * (a10 - a00), a01 + f[1] * (a11 - a01)
        return b0 + f[2] * (b1 - b0)

    def gradient(ix, iy, iz, k):
        i = [ix, iy, iz]
        hi, lo = list(i), list(i)
        hi[k], lo[k] = min(i[k] + 1, n[k] - 1), max(i[k] - 1, 0)
        return host.tsdf[hi[2], hi[1], hi[0]] - host.tsdf[lo[2], lo[1], lo[0]]

    if min(n) < 2:
        return Raycast(depth, unit, colors), brackets
    for f in range(views.count):
        kinv, rot, pos = cams[f, :9].reshape(3, 3), cams[f, 9:18].reshape(3, 3), cams[f, 18:]
        for y in range(h):
            for x in range(w):
                u, v = x + 0.5, y + 0.5
                l = [float((kinv[i, 0] * u + kinv[i, 1] * v) + kinv[i, 2]) for i in range(3)]
                r = [float((rot[i, 0] * l[0] + rot[i, 1] * l[1]) + rot[i, 2] * l[2]) for i in range(3)]
                o = [float((pos[i] - vol.origin[i]) * inv - 0.5) for i in range(3)]
                d = [r[i] * inv for i in range(3)]
                prev = None                                       # (s, k, the voxels read) of the previous sample, when it was valid and outside
                for k in range(steps):
                    z = near + float(k) * step
                    g = [o[i] + d[i] * z for i in range(3)]
                    if not all(0.0 <= g[i] <= n[i] - 1 for i in range(3)):
                        prev = None
                        continue
                    c, fr = cell(g)
                    read = corners(c)
                    if not all(host.weight[iz, iy, ix] >= mw for ix, iy, iz in read):
                        prev = None
                        continue
                    s = interpolate([host.tsdf[iz, iy, ix] for ix, iy, iz in read], fr)
                    if not s < 0:
                        prev = (s, k, read)
                        continue
                    if prev is None:
                        break                                     # entered the surface from unobserved space, or started inside
                    t = prev[0] / (prev[0] - s)
                    assert t.dtype == F32 and prev[1] == k - 1
                    zs = (near + float(k - 1) * step) + float(t) * step
                    depth[f, y, x] = F32(zs)
                    brackets[(f, y, x)] = prev[2] + read
                    c, fr = cell([o[i] + d[i] * zs for i in range(3)])
                    read = corners(c)
                    if normals:
                        nv = [interpolate([gradient(ix, iy, iz, j) for ix, iy, iz in read], fr) for j in range(3)]
                        length = np.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
                        assert length.dtype == F32
                        unit[f, y, x] = [nv[j] / length for j in range(3)] if length > 0 else [0.0, 0.0, 0.0]
                    if colors is not None:
                        for ch in range(3):
                            col = interpolate([host.color[iz, iy, ix, ch] for ix, iy, iz in read], fr)
                            colors[f, y, x, ch] = np.uint8(min(F32(255.0), max(F32(0.0), np.floor(col + F32(0.5)))))
                    break
    return Raycast(depth, unit, colors), brackets


def _noise_views():
    """Two cameras 0.6 in front of the (6, 7, 9) noise volume of mesh_cases, the second turned by 0.3 rad about y around the volume's centre."""
    centre = np.array([-1.0 + 0.09, 0.25 + 0.105, 3.0 + 0.135])
    poses = []
    for angle in (0.0, 0.3):
        T = np.eye(4)
        c, s = np.cos(angle), np.sin(angle)
        T[:3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
        T[:3, 3] = centre - 0.6 * T[:3, 2]
        poses.append(T)
    return Views(np.array([[28.0, 0.0, 5.6], [0.0, 28.0, 4.4], [0.0, 0.0, 1.0]]), np.stack(poses), size=(9, 11), near=0.3, far=0.9, step=0.01)


# ---- 1. the mirror equals the scalar reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["noise", "integrated"])
def test_the_mirror_equals_the_scalar_reference(scene):
    if scene == "noise":
        host, views = mc.noise((6, 7, 9), seed=6), _noise_views()
    else:
        host, (vol, spec, depth, frames) = mc.integrated((67, 9, 5), (3, 37, 53))
        views = rc.scene_views(spec, (9, 11), step=vol.voxel / 4.0)
    assert views.count == 2 and views.size == (9, 11)
    for mw in (1.0, 2.0):
        with np.errstate(all="ignore"):
            want, _ = reference(host, views, mw)
            got = host.raycast(views, min_weight=mw)
        rc.same_raycast(got, want)
        rc.miss_is_zero(got)
        print(f"\n[{scene}] min_weight {mw}: {rc.hits(got)} hits of {got.depth.size}")
        assert 0 < rc.hits(got) < got.depth.size
        assert got.colors is not None and got.colors[got.depth > 0].any()


# ---- 2. a plane -------------------------------------------------------------------------------------------------------------------------------------
def _plane():
    host = TsdfHost(Volume(origin=(-0.5, -0.5, 0.5), voxel=1.0 / 16.0, dims=(16, 16, 16)), coloured=False)
    host.integrate(np.full((1, 8, 8), rc.Z0, F32), Cloud(K=rc.PLANE_K, source="depth"))
    return host


def test_a_plane_is_recovered():
    """1e-5 is the bound tests/test_fusion_cpu.py uses for this plane, for the same handful of fp32 roundings."""
    host = _plane()
    for step in (1.0 / 16.0, 1.0 / 32.0):
        got = host.raycast(Views(rc.PLANE_K, size=(8, 8), near=0.5, far=1.5, step=step))
        err, nerr = np.abs(got.depth.astype(np.float64) - rc.Z0).max(), np.abs(got.normals - np.array([0.0, 0.0, -1.0], F32)).max()
        print(f"\n[plane] step {step}: {rc.hits(got)} hits, depth error {err / rc.Z0:.2e}, normal error {nerr:.2e}")
        assert rc.hits(got) == 64 and got.colors is None
        assert err <= 1e-5 * rc.Z0 and nerr <= 1e-5
    views = Views(rc.OBLIQUE_K, rc.oblique_pose(), size=(10, 12), near=0.3, far=1.5)
    got = host.raycast(views)
    z = rc.world_points(views, got.depth)[..., 2]
    err, nerr = np.abs(z - rc.Z0).max(), np.abs(got.normals - np.array([0.0, 0.0, -1.0], F32)).max()
    print(f"[plane] oblique: {rc.hits(got)} hits, z error {err / rc.Z0:.2e}, normal error {nerr:.2e}")
    assert rc.hits(got) == 120
    assert err <= 1e-5 * rc.Z0 and nerr <= 1e-5


# ---- 3. a sphere ------------------------------------------------------------------------------------------------------------------------------------
def test_a_sphere():
    """Trilinear interpolation of an exact distance field is off by about h^2 / (8 R) per axis, 0.09 voxel in all; a half-voxel offset in g would
    give 0.5, and a flipped or axis-swapped normal a negative or small dot product."""
    views = rc.sphere_views()
    whole = mc.sphere().raycast(views)
    hit = whole.depth > 0
    assert 0 < hit.sum() < 256
    radial = rc.world_points(views, whole.depth)[hit] - np.array(mc.SPHERE_C)
    dist = np.linalg.norm(radial, axis=1)
    cos = (whole.normals[hit].astype(np.float64) * radial).sum(axis=1) / dist
    print(f"\n[sphere] {hit.sum()} hits, radius error {np.abs(dist - mc.SPHERE_R).max():.3f} voxel, normal . radial >= {cos.min():.5f}")
    assert np.abs(dist - mc.SPHERE_R).max() <= 0.25
    assert cos.min() >= 0.99
    holed = mc.sphere(holes=0.03, seed=1)
    got = holed.raycast(views)
    want, brackets = reference(holed, views)
    rc.same_raycast(got, want)
    assert 0 < rc.hits(got) < hit.sum() and len(brackets) == rc.hits(got)
    assert (holed.weight == 0).any()
    assert all(holed.weight[iz, iy, ix] >= 1 for read in brackets.values() for ix, iy, iz in read)


# ---- 4. edges of the rule ---------------------------------------------------------------------------------------------------------------------------
def _all_miss(result, shape):
    assert result.depth.shape == shape and result.depth.dtype == F32 and rc.hits(result) == 0
    rc.miss_is_zero(result)


@pytest.mark.parametrize("dims", mc.NO_CELL, ids=str)
def test_a_volume_without_a_cell_gives_no_hit(dims):
    host = mc.noise(dims, seed=1, unobserved=0.0)
    T = np.eye(4)
    T[:3, 3] = (-1.0, 0.25, 2.5)
    got = host.raycast(Views(np.array([[10.0, 0.0, 3.0], [0.0, 10.0, 2.0], [0.0, 0.0, 1.0]]), T, size=(4, 6), near=0.1, far=1.0))
    _all_miss(got, (1, 4, 6))
    assert got.normals.shape == (1, 4, 6, 3) and got.colors.shape == (1, 4, 6, 3)


def test_looking_away_and_starting_inside():
    host = _plane()
    back = np.diag([-1.0, 1.0, -1.0, 1.0])                       # turned by pi about y: the volume lies behind the camera
    _all_miss(host.raycast(Views(rc.PLANE_K, back, size=(8, 8), near=0.5, far=1.5)), (1, 8, 8))
    ball = mc.sphere()
    T = np.eye(4)
    T[:3, 3] = mc.SPHERE_C                                      # at the centre: the first valid sample is negative, and the way out is no hit
    inside = ball.raycast(Views(np.array([[20.0, 0.0, 8.0], [0.0, 20.0, 8.0], [0.0, 0.0, 1.0]]), T, size=(16, 16), near=0.0, far=12.0, step=0.5))
    _all_miss(inside, (1, 16, 16))


def test_unobserved_voxels_in_front_of_the_surface():
    """The plane crosses between the voxel layers 7 and 8 (g_z = 7.75).  With layer 7 unobserved the samples of 6 <= g_z < 8 are not valid, so the
    first valid sample behind them is negative with nothing remembered: a miss.  min_weight 0 consults no weight, and the stored distances of the
    layer are still there: the hits of the untouched volume."""
    host = _plane()
    views = Views(rc.PLANE_K, size=(8, 8), near=0.5, far=1.5, step=1.0 / 32.0)
    before = host.raycast(views)
    host.weight[7] = 0.0
    _all_miss(host.raycast(views), (1, 8, 8))
    rc.same_raycast(host.raycast(views, min_weight=0.0), before)
    assert rc.hits(before) == 64
    host.weight[7], host.weight[5] = 1.0, 0.0                     # a gap well in front of the surface: valid outside samples follow it, so the hit stays
    rc.same_raycast(host.raycast(views), before)


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_a_sample_of_exactly_zero_is_outside(zero):
    """Layers of constant distance along z, unit voxels, one ray along +z whose samples fall on the voxel centres: the first sample reads exactly 0
    (or -0) and the second -0.5.  Zero counts as outside, so this is a hit at the first sample; were it inside, the ray would have started inside."""
    layers = np.array([zero, -0.5, -1.0, -1.0, -1.0])
    host = mc.filled((3, 3, 5), np.repeat(layers, 9))
    T = np.eye(4)
    T[:3, 3] = (1.5, 1.5, -0.5)                                  # g_z = k at z_k = 1 + k
    views = Views(np.array([[100.0, 0.0, 0.5], [0.0, 100.0, 0.5], [0.0, 0.0, 1.0]]), T, size=(1, 1), near=1.0, far=5.0, step=1.0)
    got = host.raycast(views)
    want, _ = reference(host, views)
    rc.same_raycast(got, want)
    assert got.depth[0, 0, 0] == F32(1.0) and got.colors is None
    host.tsdf[0] = 0.5                                           # the same ray from free space: t = 0.5, half a voxel further
    assert host.raycast(views).depth[0, 0, 0] == F32(1.5)
    host.tsdf[0] = zero
    host.tsdf[1:] = np.array([0.5, zero, -0.5, -1.0], F32)[:, None, None]      # zero in the middle: remembered as outside, hit at t = 0 behind it
    got = host.raycast(views)
    assert got.depth[0, 0, 0] == F32(3.0) and np.array_equal(got.normals[0, 0, 0], np.array([0.0, 0.0, -1.0], F32))


def test_outputs_that_are_left_out_and_views_in_one_call():
    host, (vol, spec, depth, frames) = mc.integrated((67, 9, 5), (3, 37, 53))
    views = rc.scene_views(spec, (5, 7), step=vol.voxel / 4.0)
    both = host.raycast(views)
    assert 0 < rc.hits(both) < both.depth.size
    rc.miss_is_zero(both)
    lengths = np.linalg.norm(both.normals[both.depth > 0].astype(np.float64), axis=1)
    assert np.abs(lengths - 1.0).max() <= 4 * 2.0 ** -24
    plain = host.raycast(views, normals=False)
    assert plain.normals is None and np.array_equal(fc.bits(plain.depth), fc.bits(both.depth)) and np.array_equal(plain.colors, both.colors)
    bare = TsdfHost(vol, coloured=False)
    bare.tsdf[:], bare.weight[:] = host.tsdf, host.weight
    got = bare.raycast(views)
    assert got.colors is None and np.array_equal(fc.bits(got.depth), fc.bits(both.depth)) and np.array_equal(fc.bits(got.normals), fc.bits(both.normals))
    for f in range(views.count):
        one = host.raycast(Views(views.K, views.pose[f], size=views.size, near=views.near, far=views.far, step=views.step))
        rc.same_raycast(one, Raycast(both.depth[f:f + 1], both.normals[f:f + 1], both.colors[f:f + 1]))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_views_refuse():
    K, ok = rc.PLANE_K, dict(size=(4, 5), near=0.5, far=1.5)
    assert Views(K, **ok).count == 1 and Views(np.stack([K, K]), **ok).count == 2 and Views(K, np.stack([np.eye(4)] * 3), **ok).count == 3
    assert Views(K, **ok).march(0.25) == (0.25, 5) and Views(K, step=0.1, **ok).march(0.25)[0] == 0.1
    assert fusion.MAX_STEPS == 65536 and Views(K, size=(1, 1), near=0.0, far=65535.0, step=1.0).march(7.0) == (1.0, 65536)
    singular = np.array([[8.0, 0.0, 4.0], [16.0, 0.0, 8.0], [0.0, 0.0, 1.0]])
    bad = [dict(K=np.eye(4)), dict(K=np.zeros((0, 3, 3))), dict(K=K[:2]), dict(K=singular), dict(K=np.full((3, 3), np.nan)), dict(K=np.where(K > 0, np.inf, K)),
           dict(pose=np.eye(3)), dict(pose=np.full((4, 4), np.nan)), dict(pose=np.stack([np.eye(4)] * 2), K=np.stack([K] * 3)),
           dict(size=(4,)), dict(size=(0, 5)), dict(size=(4, -1)), dict(size=(4.0, 5)), dict(size=5), dict(size=(2 ** 16, 2 ** 15)),
           dict(near=1.5), dict(near=2.0), dict(near=-0.1), dict(near=math.nan), dict(far=math.inf), dict(far=math.nan), dict(near="0"),
           dict(step=0.0), dict(step=-1.0), dict(step=math.nan), dict(step=math.inf), dict(step=1e-6), dict(step=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            Views(**{**dict(K=K), **ok, **kw})
    with pytest.raises(TypeError):
        Views(K)                                                  # size, near and far have no default
    with pytest.raises(ValueError, match="samples"):
        Views(K, **ok).march(1e-6)


def test_raycast_refuses():
    host = _plane()
    views = Views(rc.PLANE_K, size=(4, 5), near=0.5, far=1.5)
    for kw in (dict(min_weight=math.nan), dict(min_weight=-1.0), dict(min_weight=math.inf), dict(normals="yes"), dict(output="disk"), dict(output="device")):
        with pytest.raises(ValueError):
            host.raycast(views, **kw)
    for not_views in (None, Cloud(K=rc.PLANE_K), (4, 5)):
        with pytest.raises(ValueError, match="Views"):
            host.raycast(not_views)
    tiny = TsdfHost(Volume(origin=(0.0, 0.0, 0.0), voxel=1e-6, dims=(2, 2, 2)), coloured=False)
    with pytest.raises(ValueError, match="samples"):
        tiny.raycast(views)                                       # step=None takes the voxel: a million samples


def test_video_surface_refuses_before_it_infers():
    model = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(42, 56), lora_type="none", disable_conv_head=True)
    frames = np.zeros((2, 42, 56, 3), np.uint8)
    spec, vol = Cloud(K=rc.PLANE_K), Volume(origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(4, 4, 4))
    views = Views(rc.PLANE_K, size=(4, 5), near=0.5, far=1.5)
    model.infer_video_depth = None                               # every refusal comes before the video is inferred
    with pytest.raises(ValueError, match="views"):
        model.video_surface(frames, spec, vol, surface="views")
    for surface in ("points", "mesh"):
        with pytest.raises(ValueError, match="views"):
            model.video_surface(frames, spec, vol, surface=surface, views=views)
    with pytest.raises(ValueError, match="views"):
        model.video_surface(frames, spec, vol, views=views)
    with pytest.raises(ValueError, match="Views"):
        model.video_surface(frames, spec, vol, surface="views", views=spec)
    with pytest.raises(ValueError, match="samples"):
        model.video_surface(frames, spec, Volume(origin=(0.0, 0.0, 0.0), voxel=1e-6, dims=(4, 4, 4)), surface="views", views=views)
    with pytest.raises(ValueError, match="surface"):
        model.video_surface(frames, spec, vol, surface="cubes")


# ---- 6. ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "endodav_hip.h")).read()
    assert "int edv_tsdf_raycast(const edv_tsdf_volume *vol, const double *cams_dev" in header
    assert hasattr(C.CDLL(_lib.LIB_PATH), "edv_tsdf_raycast")
    restype, args = _lib.SIGNATURES["edv_tsdf_raycast"]
    assert restype is C.c_int and len(args) == 13
    assert _lib.load().edv_abi_version() == 15
