"""Inputs shared by tests/test_track_colour_cpu.py and tests/test_track_colour_gpu.py: the scenes of tests/track_cases.py in colour.  The curved
surface and a fronto-parallel plane are fused at the identity with a smooth seeded texture as frame 0's RGB, and seen again, depth and colour,
from nearby poses through the mirror's own ray-cast."""
import functools

import numpy as np

from endodav_amd.fusion import TsdfHost, Views
from tests import track_cases as tc

H, W = tc.H, tc.W
WEIGHT = 0.001                                   # Track(colour=...): one intensity unit (of 255) against a millimetre of the scene's unit
PLANE_Z = 0.6
SLIDE = (0.02, -0.015, 0.0)                      # a translation inside the plane: 2 and 1.5 pixels at K = 60 px and z = 0.6
ROLL, ROLL_SLIDE = (0.0, 0.0, 0.03), (0.03, 0.0, 0.0)   # a roll about the optical axis with a translation along x


def texture(seed=7):
    """uint8 [1, H, W, 3]: per channel 128 + 45 sin(2 pi x / a + .) + 40 sin(2 pi y / b + .) + 25 sin(2 pi (x + y) / c + .) at pixel centres, the
    wavelengths a, b, c seeded in 9 .. 17 pixels and the phases anywhere: smooth against a pixel, and nothing repeats inside the frame's reach."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    out = np.empty((1, H, W, 3), np.uint8)
    for c in range(3):
        a, b, d = rng.uniform(9.0, 17.0, 3)
        pa, pb, pd = rng.uniform(0.0, 2.0 * np.pi, 3)
        v = 128.0 + 45.0 * np.sin(2.0 * np.pi * x / a + pa) + 40.0 * np.sin(2.0 * np.pi * y / b + pb) + 25.0 * np.sin(2.0 * np.pi * (x + y) / d + pd)
        out[0, :, :, c] = np.floor(v + 0.5).astype(np.uint8)
    out.setflags(write=False)
    return out


def shape_of(kind):
    """float32 [1, H, W]: frame 0's depth, the curved surface of track_cases or the plane z = 0.6."""
    return tc.surface() if kind == "curved" else np.full((1, H, W), PLANE_Z, np.float32)


@functools.lru_cache(maxsize=None)
def fused(kind="curved"):
    """The mirror's coloured volume after frame 0 at the identity.  Shared: callers only read it."""
    host = TsdfHost(tc.volume(), coloured=True)
    host.integrate(shape_of(kind), tc.spec(), texture())
    for a in (host.tsdf, host.weight, host.color):
        a.setflags(write=False)
    return host


def views(T=None, size=(H, W), intrinsics=None):
    K = tc.K if intrinsics is None else np.asarray(intrinsics, np.float64).reshape(3, 3)
    return Views(K, T, size=size, near=tc.TRACK["near"], far=tc.TRACK["far"], step=tc.TRACK["step"])


def seen_from(T, kind="curved"):
    """(depth float32 [1, H, W], colours uint8 [1, H, W, 3]) of the camera at T: the mirror's ray-cast; misses are depth 0 and fall to ``near``."""
    cast = fused(kind).raycast(views(T), normals=False)
    return cast.depth, cast.colors


@functools.lru_cache(maxsize=None)
def single(kind="curved", rotation=tc.ROTATION, translation=tc.TRANSLATION):
    """(live depth [1, H, W], live frames [1, H, W, 3], true pose); the guess is the identity."""
    truth = tc.pose(rotation, translation)
    depth, frames = seen_from(truth, kind)
    depth.setflags(write=False), frames.setflags(write=False)
    return depth, frames, truth


@functools.lru_cache(maxsize=None)
def clip():
    """(depth [5, H, W], frames [5, H, W, 3], true poses) of track_cases' five-frame scene in colour: frame 0 the surface and the texture."""
    truth = tc.clip()[1]
    seen = [seen_from(truth[i]) for i in range(1, 5)]
    depth = np.concatenate([tc.surface()] + [d for d, _ in seen])
    frames = np.concatenate([texture()] + [c for _, c in seen])
    depth.setflags(write=False), frames.setflags(write=False)
    return depth, frames, truth


@functools.lru_cache(maxsize=None)
def model(kind="curved", size=(H, W), intrinsics=None):
    """(Raycast with colours, Views): the fused volume seen from the identity, at the live frame's size and K or at others."""
    v = views(None, size, intrinsics)
    cast = fused(kind).raycast(v)
    for a in (cast.depth, cast.normals, cast.colors):
        a.setflags(write=False)
    return cast, v


SKEW_K = (60.0, 1.5, 28.0, 0.0, 58.0, 20.0, 0.0, 0.0, 1.0)    # K01 != 0


def live(shape, source="depth", kind="none", seed=0):
    """(depth, mask or None, frames uint8 [n, h, w, 3]): ``tc.live`` and the single scene's colours resampled the same way, each frame a few
    levels brighter than the one before."""
    n, h, w = shape
    depth, mask = tc.live(shape, source, kind, seed)
    base = single()[1][0].astype(np.int64)
    ys, xs = ((2 * np.arange(h) + 1) * H) // (2 * h), ((2 * np.arange(w) + 1) * W) // (2 * w)
    frames = np.stack([np.clip(base[ys][:, xs] + 3 * f, 0, 255) for f in range(n)]).astype(np.uint8)
    return depth, mask, frames


def same_tracked(got, want):
    """Two ``Tracked``, bit for bit, scales included where there are any."""
    assert got.poses.shape == want.poses.shape and np.array_equal(tc.bits(got.poses), tc.bits(want.poses))
    assert got.pairs.dtype == np.int64 and np.array_equal(got.pairs, want.pairs)
    assert np.array_equal(tc.bits(got.rms), tc.bits(want.rms))
    assert got.lost.dtype == np.bool_ and np.array_equal(got.lost, want.lost)
    assert (got.scales is None) == (want.scales is None)
    if want.scales is not None:
        assert np.array_equal(tc.bits(got.scales), tc.bits(want.scales))
