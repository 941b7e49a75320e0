"""Inputs and checks shared by tests/test_raycast_cpu.py and tests/test_raycast_gpu.py: the views that look at the scenes of tests/fusion_cases.py,
the plane and the sphere of the yardstick tests, and bit equality of two ``fusion.Raycast``."""
import numpy as np

from endodav_amd.fusion import Raycast, Views
from tests import cloud_cases as cases
from tests import fusion_cases as fc

# the kernel's workgroup is a 16 x 16 pixel tile and a wave an 8 x 8 block of it: one pixel; inside one block; across tile edges in both directions
# with ragged last tiles; and more than a wave wide, ragged, with a single ragged row of tiles
SIZES = [(1, 1), (5, 7), (17, 33), (3, 70)]

NEAR, FAR = 0.05, 1.5       # the boxes of fusion_cases reach from 0.4 behind their first camera to 1.6 in front of it, the surface lies at 0.45 .. 0.7


def scene_views(spec, size, seed=0, **kw):
    """The cameras of a fusion_cases spec, with intrinsics made for ``size``, plus one more turned and moved a little (fc.nearby_poses)."""
    h, w = size
    extra = fc.nearby_poses(2, seed=seed)[1:, :3, :]
    kw.setdefault("near", NEAR)
    kw.setdefault("far", FAR)
    return Views(cases.intrinsics(h, w, None, seed), np.concatenate([spec.pose, extra]), size=size, **kw)


Z0 = 1.0 + 1.0 / 64.0
PLANE_K = np.array([[8.0, 0.0, 4.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]])


def oblique_pose():
    """T_world_camera of the plane's oblique view: turned 0.2 rad about y and moved to (-0.2, 0.03, 0.1)."""
    T = np.eye(4)
    c, s = np.cos(0.2), np.sin(0.2)
    T[:3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
    T[:3, 3] = (-0.2, 0.03, 0.1)
    return T


OBLIQUE_K = np.array([[24.0, 0.0, 6.0], [0.0, 24.0, 5.0], [0.0, 0.0, 1.0]])


def sphere_views(**kw):
    """16 x 16 pixels from (7.1, 6.8, -6.0) along +z at the sphere of mesh_cases: the silhouette lies inside the image."""
    T = np.eye(4)
    T[:3, 3] = (7.1, 6.8, -6.0)
    kw.setdefault("step", 1.0)
    return Views(np.array([[20.0, 0.0, 8.0], [0.0, 20.0, 8.0], [0.0, 0.0, 1.0]]), T, size=(16, 16), near=1.0, far=20.0, **kw)


def world_points(views, depth):
    """float64 [m, h, w, 3]: t + r * depth, the cloud's lift of every pixel."""
    cams = views.cams()
    h, w = views.size
    u, v = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    out = np.empty((views.count, h, w, 3))
    for f, cam in enumerate(cams):
        kinv, rot, t = cam[:9].reshape(3, 3), cam[9:18].reshape(3, 3), cam[18:]
        rays = np.stack([u, v, np.ones_like(u)], axis=-1) @ kinv.T @ rot.T
        out[f] = t + rays * np.asarray(depth[f], np.float64)[..., None]
    return out


def same_raycast(got, want):
    """Two host results equal bit for bit, with the dtypes and shapes of fusion.Raycast."""
    assert isinstance(got, Raycast)
    m, h, w = want.depth.shape
    for name, dtype, shape in (("depth", np.float32, (m, h, w)), ("normals", np.float32, (m, h, w, 3)), ("colors", np.uint8, (m, h, w, 3))):
        g, x = getattr(got, name), getattr(want, name)
        if x is None:
            assert g is None, name
            continue
        assert isinstance(g, np.ndarray) and g.dtype == dtype and g.shape == x.shape == shape, (name, g.dtype, g.shape, x.shape)
        assert np.array_equal(fc.bits(g) if dtype == np.float32 else g, fc.bits(x) if dtype == np.float32 else x), name


def hits(result):
    return int((np.asarray(result.depth) > 0).sum())


def miss_is_zero(result):
    """Where the depth is 0, as +0, the normal and the colour are exactly 0 too."""
    miss = result.depth == 0
    assert (fc.bits(result.depth)[miss] == 0).all()
    if result.normals is not None:
        assert (fc.bits(result.normals)[miss] == 0).all()
    if result.colors is not None:
        assert (result.colors[miss] == 0).all()

