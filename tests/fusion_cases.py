"""Inputs shared by tests/test_fusion_cpu.py and tests/test_fusion_gpu.py: the seeded clips, cameras and specs of tests/cloud_cases.py and volumes
placed in front of their first camera, small enough to integrate on the host."""
import numpy as np

from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Volume
from tests import cloud_cases as cases

VOLUMES = [(5, 3, 2), (64, 4, 4), (67, 9, 5), (130, 7, 3)]   # below, at and across a wave in x; (67, 9, 5) and (130, 7, 3) span several tiles
CLIPS = [(1, 6, 8), (3, 37, 53)]


def masks(shape, kind, seed=5):
    if kind == "none":
        return None
    return np.random.default_rng(seed).random(shape[1:] if kind == "shared" else shape) < 0.7


def volume_for(dims, spec, reach=2.0, ahead=0.6, **kw):
    """A box whose longest side is ``reach``, centred ``ahead`` in front of the spec's first camera along its optical axis.  The cameras see
    about +-27 degrees and the clips hold depths about ``ahead``, so part of the box lies behind the camera, part outside the image, and the
    surface the camera sees passes through the rest."""
    T = spec.pose[0]
    centre = T[:, 3] + ahead * T[:, 2]
    voxel = reach / max(dims)
    origin = centre - 0.5 * voxel * np.asarray(dims, np.float64)
    return Volume(origin=origin, voxel=voxel, dims=dims, **kw)


def nearby_poses(n, seed=0, scale=1.0):
    """T_world_camera [n, 4, 4]: the one pose of cloud_cases.poses turned by up to 0.1 rad about a random axis and moved by up to 0.1 * scale per frame,
    so that the frames of a clip see the same voxels (independent random poses would look past each other)."""
    rng = np.random.default_rng(500 + seed)
    T = np.repeat(cases.poses(None, seed)[None], n, axis=0)
    for i in range(1, n):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        angle = rng.uniform(-0.1, 0.1)
        A = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        T[i, :3, :3] = T[0, :3, :3] @ (np.eye(3) + np.sin(angle) * A + (1.0 - np.cos(angle)) * (A @ A))
        T[i, :3, 3] = T[0, :3, 3] + scale * rng.uniform(-0.1, 0.1, 3)
    return T


FAR = 0.7   # drops the farthest sixth of the clips below


def clip(shape, source, seed=0):
    """float32 [n, h, w] whose depths are spread over 0.45 .. 0.75, as depth or as the disparity that ``disp_to_depth`` with the Cloud's default
    min_depth and max_depth turns into them: a rough surface about where volume_for centres its box, so every clip has voxels in front of it, inside
    the truncation band behind it, and beyond."""
    z = 0.45 + 0.3 * np.random.default_rng(300 + seed + 7 * shape[2]).random(shape)
    return (z if source == "depth" else (1.0 / z - 1.0 / 150.0) / (1.0 / 0.1 - 1.0 / 150.0)).astype(np.float32)


def spec_for(shape, source="depth", per_frame=False, kind="none", seed=0, **kw):
    """The Cloud of a clip: step 1, one camera or a camera per frame (nearby_poses), no mask, a shared one or one per frame."""
    n, h, w = shape
    kw.setdefault("far", FAR)
    return Cloud(K=cases.intrinsics(h, w, n if per_frame else None, seed), pose=nearby_poses(n, seed) if per_frame else cases.poses(None, seed), step=1,
                 source=source, mask=masks(shape, kind, seed=5 + seed), **kw)


def case(dims, shape, source="depth", per_frame=False, kind="none", seed=0, **kw):
    """(volume, spec, depth, frames) of one seeded scene."""
    spec = spec_for(shape, source, per_frame, kind, seed)
    kw.setdefault("reach", min(2.0, 0.12 * max(dims)))     # voxels no larger than 0.12: a box of few voxels still meets the surface, part of it outside the image
    return volume_for(dims, spec, **kw), spec, clip(shape, source, seed=seed), cases.colours(shape, seed=seed)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_state(got, want):
    """(tsdf, weight, color) triples equal bit for bit."""
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            assert g.shape == w.shape and g.dtype == np.float32 and np.array_equal(bits(g), bits(w))


def same_cloud(got, want):
    """Points, colours and offsets of two host PointClouds equal bit for bit."""
    assert isinstance(got.offsets, np.ndarray) and got.offsets.dtype == np.int64 and np.array_equal(got.offsets, want.offsets)
    assert got.points.shape == want.points.shape and got.points.dtype == np.float32 and np.array_equal(bits(got.points), bits(want.points))
    if want.colors is None:
        assert got.colors is None
    else:
        assert got.colors.shape == want.colors.shape and got.colors.dtype == np.uint8 and np.array_equal(got.colors, want.colors)
