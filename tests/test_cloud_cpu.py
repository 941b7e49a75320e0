"""Point clouds, the parts that need no GPU: the ``Cloud`` spec, ``lift_host`` (the yardstick of tests/test_cloud_gpu.py) against an
independent float64 formulation of the reference's expressions, its order, grid and offsets, the ``.ply`` files, the ABI, and the C entry
points' refusal of bad arguments."""
import ctypes as C
import os

import numpy as np
import pytest

from endodav_amd import _lib, cloud
from endodav_amd.cloud import Cloud, PointCloud
from tests import cloud_cases as cases

ENTRY_POINTS = ("edv_cloud_tile_pixels", "edv_cloud_workspace", "edv_cloud_count", "edv_cloud_scatter")
K0 = cases.intrinsics(10, 12)


# ---- 1. the spec ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(K=np.eye(4)), dict(K=np.ones((2, 2, 3, 3))), dict(K=np.zeros((3, 3))), dict(K=K0, pose=np.eye(3)), dict(K=K0, pose=np.ones((2, 3, 3))),
    dict(K=K0, step=0), dict(K=K0, step=-2), dict(K=K0, step=1.5), dict(K=K0, source="inverse"), dict(K=K0, near=1.0, far=1.0), dict(K=K0, near=2.0, far=1.0),
    dict(K=K0, near=float("nan")), dict(K=K0, min_depth=0.0), dict(K=K0, min_depth=5.0, max_depth=1.0), dict(K=K0, mask=np.ones((2, 2, 2, 2), bool)),
    dict(K=K0, mask=np.ones((4, 4), np.float32)),
], ids=lambda kw: ",".join(sorted(kw)))
def test_cloud_rejects_bad_specs(kw):
    with pytest.raises(ValueError):
        Cloud(**kw)


def test_cloud_cameras():
    spec = Cloud(K=K0)
    cams = spec.cams(5)
    assert cams.shape == (1, 21) and cams.dtype == np.float64
    assert np.array_equal(cams[0, :9].reshape(3, 3), np.linalg.inv(K0.astype(np.float64)))
    assert np.array_equal(cams[0, 9:18].reshape(3, 3), np.eye(3)) and np.array_equal(cams[0, 18:], np.zeros(3))   # the default pose is the identity
    T = cases.poses(4)
    per = Cloud(K=K0, pose=T[:, :3]).cams(4)
    assert per.shape == (4, 21)
    assert np.array_equal(per[2, 9:18].reshape(3, 3), T[2, :3, :3]) and np.array_equal(per[2, 18:], T[2, :3, 3])
    assert np.array_equal(Cloud(K=K0, pose=T).cams(4), per)   # [4, 4] and [3, 4] are the same pose
    with pytest.raises(ValueError, match="pose"):
        Cloud(K=K0, pose=T).cams(5)
    lo, span, gain, near, far = Cloud(K=K0).scalars()
    assert lo == np.float32(1 / 150.0) and span == np.float32(1 / 0.1 - 1 / 150.0) and (gain, near, far) == (np.float32(1.0), np.float32(1e-3), np.float32(150.0))
    with pytest.raises(ValueError, match="spec"):
        cloud.lift_host(np.zeros((1, 2, 2), np.float32), None)
    with pytest.raises(ValueError, match="float32"):
        cloud.lift_host(np.zeros((1, 2, 2)), spec)
    with pytest.raises(ValueError, match="frames"):
        cloud.lift_host(np.zeros((1, 2, 2), np.float32), spec, np.zeros((1, 2, 3, 3), np.uint8))
    with pytest.raises(ValueError, match="mask"):
        cloud.lift_host(np.zeros((1, 2, 2), np.float32), Cloud(K=K0, mask=np.ones((3, 3), bool)))


# ---- 2. the yardstick against the reference's expressions --------------------------------------------------------------------------------------
def _ulps_apart(a, b):
    """Distance in float32 steps between two finite arrays, through the order-preserving integer image of the bits."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _matmul_cloud(depth, spec, frames):
    """The loaders' get_point_cloud in matrix form: homogeneous pixel positions through inv(K), the rotation and the translation, in float64,
    cast once.  Written from the formula, with the sampling of this project (one pixel for depth, mask and colour)."""
    n, h, w = depth.shape
    s = spec.step
    ys, xs = np.arange(0, h, s), np.arange(0, w, s)                      # rgb[::s, ::s] has this many rows and columns
    py, px = np.minimum(ys + s // 2, h - 1), np.minimum(xs + s // 2, w - 1)
    gx, gy = np.meshgrid((np.arange(len(xs)) + 0.5) * s, (np.arange(len(ys)) + 0.5) * s)
    homo = np.stack([gx, gy, np.ones_like(gx)], axis=-1)                 # [oh, ow, 3]
    pts, cols, counts = [], [], []
    for f in range(n):
        K = spec.K[f if spec.K.shape[0] > 1 else 0]
        T = spec.pose[f if spec.pose.shape[0] > 1 else 0]
        x = depth[f][np.ix_(py, px)]
        if spec.source == "disparity":
            lo, span = np.float32(1 / spec.max_depth), np.float32(1 / spec.min_depth - 1 / spec.max_depth)
            z = np.float32(1) / (lo + span * x)
        else:
            z = x
        z = z * np.float32(spec.gain)
        keep = (z > np.float32(spec.near)) & (z < np.float32(spec.far))
        if spec.mask is not None:
            m = spec.mask if spec.mask.ndim == 2 else spec.mask[f]
            keep &= m[np.ix_(py, px)] != 0
        dirs = np.einsum("ij,bj->bi", T[:, :3], np.einsum("ij,bj->bi", np.linalg.inv(K), homo[keep]))
        pts.append((T[:, 3] + dirs * z[keep].astype(np.float64)[:, None]).astype(np.float32))
        cols.append(frames[f][np.ix_(py, px)][keep])
        counts.append(int(keep.sum()))
    return np.concatenate(pts), np.concatenate(cols), np.array(counts)


@pytest.mark.parametrize("source", cloud.SOURCES)
@pytest.mark.parametrize("step", [1, 2, 3, 8])
@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per-frame"])
def test_lift_host_agrees_with_the_matrix_form_to_one_ulp(source, step, per_frame):
    """Both are float64 evaluations of the same three-term sums and differ by a few float64 roundings, so their float32 roundings differ by at
    most one unit in the last place unless terms cancel; the poses of cloud_cases keep |t| below the clouds' extent so that they do not."""
    shape = (3, 21, 26)
    depth, frames = cases.clip(shape, source), cases.colours(shape)
    mask = np.random.default_rng(1).random(shape) < 0.8
    spec = cases.spec_for(shape, source, step, per_frame, mask=mask, gain=1.25)
    got = cloud.lift_host(depth, spec, frames)
    pts, cols, counts = _matmul_cloud(depth, spec, frames)
    assert 0 < len(got) < shape[0] * (-(-21 // step)) * (-(-26 // step))
    assert got.points.dtype == np.float32 and got.points.shape == pts.shape and np.isfinite(got.points).all()
    assert _ulps_apart(got.points, pts).max() <= 1
    assert np.array_equal(got.colors, cols)
    assert np.array_equal(np.diff(got.offsets), counts) and got.offsets[0] == 0 and got.offsets.dtype == np.int64


# ---- 3. - 6. order, grid, offsets, dropped values ---------------------------------------------------------------------------------------------
def test_order_grid_and_offsets():
    """Identity camera with unit focal length and depth 1 everywhere: the points are the grid positions themselves, in the order of rgb[mask]."""
    n, h, w, step = 2, 7, 10, 3                                            # h % step = 1, w % step = 1
    depth = np.ones((n, h, w), np.float32)
    frames = cases.colours((n, h, w))
    mask = np.random.default_rng(3).random((n, h, w)) < 0.6
    spec = Cloud(K=np.eye(3), step=step, source="depth", mask=mask)
    got = cloud.lift_host(depth, spec, frames)
    oh, ow = 3, 4
    assert (oh, ow) == (-(-h // step), -(-w // step)) == frames[0, ::step, ::step].shape[:2]
    sy, sx = [1, 4, 6], [1, 4, 7, 9]                                         # min(o * 3 + 1, size - 1): the last row and column are clamped
    sub_rgb, keep = frames[:, sy][:, :, sx], mask[:, sy][:, :, sx]
    assert np.array_equal(got.offsets, np.concatenate([[0], np.cumsum(keep.reshape(n, -1).sum(axis=1))]))
    assert len(got) == keep.sum() == got.points.shape[0]
    gx, gy = np.meshgrid((np.arange(ow) + 0.5) * step, (np.arange(oh) + 0.5) * step)
    for f in range(n):
        p, c = got.frame(f)
        assert np.array_equal(c, sub_rgb[f].reshape(-1, 3)[keep[f].ravel()])
        assert np.array_equal(p, np.stack([gx, gy, np.ones_like(gx)], axis=-1).reshape(-1, 3)[keep[f].ravel()].astype(np.float32))
    assert isinstance(got, PointCloud) and cloud.lift_host(depth, spec).colors is None
    full = cloud.lift_host(depth, Cloud(K=np.eye(3), step=1, source="depth"), frames)     # step 1, no mask: every pixel, row-major
    assert np.array_equal(full.colors, frames.reshape(-1, 3)) and np.array_equal(full.offsets, [0, h * w, 2 * h * w])


def test_nan_inf_and_out_of_range_depths_are_dropped():
    depth = np.array([[[np.nan, np.inf, -np.inf, 0.5, 1.0, 2.0, 3.0, -1.0, 0.0, 1.5]]], np.float32)
    got = cloud.lift_host(depth, Cloud(K=np.eye(3), source="depth", near=0.5, far=3.0))
    assert np.array_equal(got.points[:, 2], np.array([1.0, 2.0, 1.5], np.float32))      # z <= near and z >= far are dropped, the bounds included
    got = cloud.lift_host(depth, Cloud(K=np.eye(3), source="depth", near=0.0, far=float("inf")))
    assert np.array_equal(got.points[:, 2], np.array([0.5, 1.0, 2.0, 3.0, 1.5], np.float32)) and np.isfinite(got.points).all()   # +Inf fails z < +Inf
    disp = np.array([[[np.nan, np.inf, -np.inf, 0.0, 1.0]]], np.float32)                   # 1 / scaled: NaN, +0, -0, about 150, about 0.1
    got = cloud.lift_host(disp, Cloud(K=np.eye(3), near=0.0, far=float("inf")))
    assert np.isfinite(got.points).all() and len(got) == 2 and np.allclose(got.points[:, 2], [150.0, 0.1], rtol=1e-5)
    empty = cloud.lift_host(np.zeros((0, 4, 5), np.float32), Cloud(K=np.eye(3)))
    assert len(empty) == 0 and empty.points.shape == (0, 3) and np.array_equal(empty.offsets, [0])


# ---- 7. .ply -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coloured", [True, False])
def test_ply_round_trip(tmp_path, coloured):
    shape = (2, 9, 11)
    got = cloud.lift_host(cases.clip(shape, "depth"), cases.spec_for(shape), cases.colours(shape) if coloured else None)
    path = os.path.join(tmp_path, "a.ply")
    cloud.write_ply(path, got)
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(got)}"]
    assert lines[3:] == ["property float x", "property float y", "property float z"] + (["property uchar red", "property uchar green", "property uchar blue"] if coloured else [])
    assert len(body) == len(got) * (15 if coloured else 12)
    back = cloud.read_ply(path)
    assert np.array_equal(back.points.view(np.uint32), got.points.view(np.uint32)) and np.array_equal(back.offsets, [0, len(got)])
    assert np.array_equal(back.colors, got.colors) if coloured else back.colors is None
    again = os.path.join(tmp_path, "b.ply")
    cloud.write_ply(again, back)
    assert open(again, "rb").read() == data                                  # byte-exact round trip
    cloud.write_ply(again, got, frame=1)
    one = cloud.read_ply(again)
    assert np.array_equal(one.points, got.frame(1)[0]) and len(one) == got.offsets[2] - got.offsets[1]
    with open(again, "wb") as fh:
        fh.write(b"not a ply")
    with pytest.raises(ValueError):
        cloud.read_ply(again)


# ---- 8. the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_types_the_entry_points(lib):
    assert _lib.ABI_VERSION == 15 and lib.edv_abi_version() == 15
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "endodav_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f"{name}(" in header, name
    assert "typedef struct edv_cloud_selection" in header and "#define EDV_ABI_VERSION 15" in header
    P = cloud.TILE_PIXELS
    assert P == lib.edv_cloud_tile_pixels() and P >= 256 and P % 64 == 0
    assert lib.edv_cloud_workspace(1, 1, 1, 1) == 8 and lib.edv_cloud_workspace(3, 1, P + 1, 1) == 3 * 2 * 8 and lib.edv_cloud_workspace(2, 64, P // 32, 1) == 2 * 2 * 8
    assert lib.edv_cloud_workspace(1, 1, P + 1, 2) == 8
    assert lib.edv_cloud_workspace(32, 1024, 1280, 1) * 100 < 32 * 1024 * 1280 * 4       # well under 1 % of the depth


# ---- 9. bad arguments: refused before anything touches a device -------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu(lib):
    n, h, w = 2, 6, 8
    P = 0x10000                                                               # never dereferenced: every call below is refused on the host
    B = lib.edv_cloud_workspace(n, h, w, 1)

    def sel(**kw):
        f = dict(x_dev=P, n=n, h=h, w=w, step=1, mode=1, lo=0.1, span=1.0, gain=1.0, near_z=0.0, far_z=1.0, mask_dev=None, mask_stride=0)
        f.update(kw)
        return _lib.CloudSelection(**f)

    bad_sel = [dict(x_dev=None), dict(n=0), dict(n=-1), dict(n=65536), dict(h=0), dict(w=-1), dict(step=0), dict(step=-3), dict(h=1 << 16, w=1 << 15),
               dict(mode=2), dict(mode=-1), dict(mask_dev=P, mask_stride=1), dict(mask_dev=P, mask_stride=h), dict(mask_stride=-1)]
    for kw in bad_sel:
        s = sel(**kw)
        assert lib.edv_cloud_count(C.byref(s), P, P, 1 << 40, None) != 0, kw
        assert lib.edv_last_error(), kw
        assert lib.edv_cloud_scatter(C.byref(s), P, 0, None, P, P, 1 << 40, P, None, 4, None) != 0, kw
        assert lib.edv_last_error(), kw
    assert lib.edv_cloud_workspace(0, h, w, 1) == 0 and lib.edv_cloud_workspace(n, h, w, 0) == 0 and lib.edv_cloud_workspace(65536, h, w, 1) == 0
    ok = sel()
    bad_count = [(None, P, P, B, None), (C.byref(ok), None, P, B, None), (C.byref(ok), P, None, B, None),      # null pointers
                 (C.byref(ok), P, P, B - 1, None), (C.byref(ok), P, P, 0, None), (C.byref(ok), P, P + 4, B, None)]  # workspace short or misaligned
    for args in bad_count:
        assert lib.edv_cloud_count(*args) != 0, args
        assert lib.edv_last_error()
    S = C.byref(ok)
    bad_scatter = [(None, P, 0, None, P, P, B, P, None, 4, None), (S, None, 0, None, P, P, B, P, None, 4, None), (S, P, 0, None, None, P, B, P, None, 4, None),
                   (S, P, 0, None, P, None, B, P, None, 4, None), (S, P, 0, None, P, P, B, None, None, 4, None),           # null pointers
                   (S, P, 1, None, P, P, B, P, None, 4, None), (S, P, 20, None, P, P, B, P, None, 4, None), (S, P, -21, None, P, P, B, P, None, 4, None),  # cam_stride
                   (S, P, 0, None, P, P, B - 1, P, None, 4, None), (S, P, 0, None, P, P + 4, B, P, None, 4, None),       # workspace
                   (S, P, 0, None, P, P, B, P, None, -1, None)]                                                          # capacity
    for args in bad_scatter:
        assert lib.edv_cloud_scatter(*args) != 0, args
        assert lib.edv_last_error()
