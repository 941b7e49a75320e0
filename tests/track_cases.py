"""Inputs shared by tests/test_track_cpu.py and tests/test_track_gpu.py: one smooth surface fused at the identity, seen again from nearby poses
through the mirror's own ray-cast, and small seeded live frames against a model view for the sums alone."""
import functools
import math

import numpy as np

from endodav_amd import fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Track, TsdfHost, Views, Volume

H, W = 40, 56
K = np.array([[60.0, 0.0, 28.0], [0.0, 60.0, 20.0], [0.0, 0.0, 1.0]])
VOLUME = dict(origin=(-0.5, -0.4, 0.3), voxel=1.0 / 64.0, dims=(64, 52, 40))
TRACK = dict(near=0.2, far=1.2, step=1.0 / 128.0, max_dist=0.1)
ROTATION, TRANSLATION = (0.02, -0.03, 0.015), (0.02, -0.015, 0.01)            # the single frame's true pose
CLIP_ROTATION, CLIP_TRANSLATION = (0.012, -0.015, 0.008), (0.012, -0.008, 0.006)   # per frame of the five-frame clip


def track(**kw):
    return Track(**{**TRACK, **kw})


def volume():
    return Volume(**VOLUME)


def spec(pose=None, **kw):
    kw.setdefault("source", "depth")
    kw.setdefault("far", 10.0)
    return Cloud(K=K, pose=pose, **kw)


def pose(rotation, translation, scale=1.0):
    """T_world_camera [4, 4] of a rotation vector and a translation, both times ``scale``."""
    return fusion.apply_twist(np.eye(4), scale * np.concatenate([np.asarray(rotation, np.float64), np.asarray(translation, np.float64)]))


def errors(T, truth):
    """(the angle between the two rotations, the distance between the two translations)."""
    c = 0.5 * (np.trace(T[:3, :3].T @ truth[:3, :3]) - 1.0)
    return math.acos(min(1.0, max(-1.0, c))), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def surface():
    """float32 [1, H, W]: z = 0.6 + 0.05 sin(x/7) + 0.04 cos(y/5) + 0.03 sin((x+y)/9) at pixel centres."""
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    return (0.6 + 0.05 * np.sin(x / 7.0) + 0.04 * np.cos(y / 5.0) + 0.03 * np.sin((x + y) / 9.0)).astype(np.float32)[None]


@functools.lru_cache(maxsize=None)
def fused():
    """The mirror's volume after frame 0 at the identity.  Shared: callers only read it (``TsdfHost.arrays`` copies)."""
    host = TsdfHost(volume(), coloured=False)
    host.integrate(surface(), spec())
    for a in (host.tsdf, host.weight):
        a.setflags(write=False)
    return host


def seen_from(T, host=None):
    """The live frame of the camera at T: the mirror's ray-cast of the fused volume, float32 [1, H, W]; misses are 0 and fall to ``near``."""
    host = fused() if host is None else host
    return host.raycast(Views(K, T, size=(H, W), near=TRACK["near"], far=TRACK["far"], step=TRACK["step"]), normals=False).depth


@functools.lru_cache(maxsize=None)
def single():
    """(live depth [1, H, W], true pose) of the single-frame scene; the guess is the identity."""
    truth = pose(ROTATION, TRANSLATION)
    live = seen_from(truth)
    live.setflags(write=False)
    return live, truth


@functools.lru_cache(maxsize=None)
def clip():
    """(depth [5, H, W], true poses [5, 4, 4]) of the five-frame scene: frame 0 the fused surface itself, the others seen from their poses."""
    truth = np.stack([pose(CLIP_ROTATION, CLIP_TRANSLATION, float(i)) for i in range(5)])
    depth = np.concatenate([surface()] + [seen_from(truth[i]) for i in range(1, 5)])
    depth.setflags(write=False)
    return depth, truth


@functools.lru_cache(maxsize=None)
def model(size=(H, W), intrinsics=None):
    """(Raycast, Views): the fused volume seen from the identity, at the live frame's size and K or at others."""
    views = Views(K if intrinsics is None else np.asarray(intrinsics, np.float64).reshape(3, 3), None, size=size, near=TRACK["near"], far=TRACK["far"], step=TRACK["step"])
    cast = fused().raycast(views)
    for a in (cast.depth, cast.normals):
        a.setflags(write=False)
    return cast, views


OTHER_SIZE, OTHER_K = (33, 47), (52.0, 0.0, 23.1, 0.0, 49.0, 16.7, 0.0, 0.0, 1.0)   # a model view that is not the live camera's
AWAY = np.array([[-1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])   # turned by pi about y: every q_2 <= 0


def live(shape, source="depth", kind="none", seed=0):
    """(depth float32 [n, h, w], mask or None): the surface seen from the perturbed pose, resampled to h x w by nearest pixel, with seeded holes
    (zeros, which the depth rule drops) and a frame-dependent offset, as depth or as the disparity the Cloud's defaults turn into it."""
    n, h, w = shape
    rng = np.random.default_rng(900 + seed)
    base = single()[0][0]
    ys, xs = ((2 * np.arange(h) + 1) * H) // (2 * h), ((2 * np.arange(w) + 1) * W) // (2 * w)
    z = np.stack([base[ys][:, xs].astype(np.float64) + 0.002 * f for f in range(n)])
    z = np.where(rng.random(shape) < 0.05, 0.0, z)
    with np.errstate(divide="ignore"):
        x = z if source == "depth" else np.where(z > 0, (1.0 / z - 1.0 / 150.0) / (1.0 / 0.1 - 1.0 / 150.0), 1.0e9)
    mask = None if kind == "none" else rng.random((h, w)) < 0.8
    return x.astype(np.float32), mask


def live_spec(shape, T, step=1, source="depth", mask=None):
    """The Cloud of a ``live`` clip: the scene's K scaled to h x w, the pose T for every frame."""
    n, h, w = shape
    Ks = np.array([[K[0, 0] * w / W, 0.0, K[0, 2] * w / W], [0.0, K[1, 1] * h / H, K[1, 2] * h / H], [0.0, 0.0, 1.0]])
    return Cloud(K=Ks, pose=T, step=step, source=source, far=10.0, mask=mask)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
