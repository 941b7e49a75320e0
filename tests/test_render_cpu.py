"""Rendering on the device, the parts that need no GPU: ``Render``'s validation, the committed colour tables, the yardstick of
tests/test_render_gpu.py against the reference's literal expressions, and the ``render=`` arguments with stub backends and runners."""
import os
import re

import numpy as np
import pytest

from endodav_amd import _lib, colormaps, video
from endodav_amd.render import Render
from tests.render_ref import colorize_ref, index_ref, ranges_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("edv_render_workspace", "edv_render_range", "edv_render_colorize")
FH, FW = 4, 6


# ---- 1. Render -------------------------------------------------------------------------------------------------------------------------------
def test_render_validates_at_construction():
    r = Render("quantile")
    assert r.cmap == "inferno" and r.q == (0.0, 0.95) and r.order == "rgb" and r.clip == 1 and r.eps == 0
    assert Render().norm == "video" and Render().eps == np.float32(1e-6) and Render().clip == 0
    assert Render("fixed", lo=0.5, hi=2.0).clip == 1 and Render("frame").clip == 0
    with pytest.raises(Exception):
        r.norm = "frame"                                          # frozen
    for bad in (dict(norm="clip"), dict(norm="frame", cmap="jet"), dict(norm="frame", order="gbr"),
                dict(norm="fixed"), dict(norm="fixed", lo=1.0), dict(norm="fixed", lo=1.0, hi=1.0), dict(norm="fixed", lo=2.0, hi=1.0),
                dict(norm="fixed", lo=0.0, hi=float("inf")), dict(norm="fixed", lo=1.0, hi=1.0 + 1e-12),  # equal as float32
                dict(norm="quantile", q=(0.9, 0.1)), dict(norm="quantile", q=(-0.1, 0.5)), dict(norm="quantile", q=(0.0, 1.5)), dict(norm="quantile", q=0.95),
                dict(norm="frame", cmap=np.zeros((256, 4), np.uint8)), dict(norm="frame", cmap=np.zeros((255, 3), np.uint8)),
                dict(norm="frame", cmap=np.zeros((256, 3), np.float32)), dict(norm="frame", cmap=[[0, 0, 0]] * 256)):
        with pytest.raises(ValueError):
            Render(**bad)
    own = np.arange(768, dtype=np.uint8).reshape(256, 3)
    assert np.array_equal(Render("frame", cmap=own).table(), own)
    bgr = Render("frame", cmap=own, order="bgr").table()
    assert bgr.flags.c_contiguous and np.array_equal(bgr, own[:, ::-1])
    assert np.array_equal(Render("frame", cmap="magma", order="bgr").table(), colormaps.TABLES["magma"][:, ::-1])
    assert Render("quantile", q=(0.0, 0.95)).ranks(5, 7) == (0, 32) and Render("quantile", q=(0.5, 1.0)).ranks(1, 1) == (0, 0)
    assert Render("quantile", q=(1.0, 1.0)).ranks(6, 8) == (47, 47)


def test_committed_tables_are_matplotlibs():
    assert colormaps.NAMES == ("inferno", "magma", "viridis")
    for name in colormaps.NAMES:
        t = colormaps.TABLES[name]
        assert t.dtype == np.uint8 and t.shape == (256, 3) and not t.flags.writeable
    assert colormaps.TABLES["inferno"][[0, 128, 255]].tolist() == [[0, 0, 3], [187, 55, 84], [252, 254, 164]]
    matplotlib = pytest.importorskip("matplotlib")
    for name in colormaps.NAMES:
        assert np.array_equal(colormaps.TABLES[name], (np.array(matplotlib.colormaps[name].colors) * 255).astype(np.uint8)), name


# ---- 2. the yardstick against the reference's own lines ---------------------------------------------------------------------------------------
def _clip(n=3, h=9, w=11, seed=0):
    rng = np.random.default_rng(seed)
    return (0.05 + rng.random((n, h, w), dtype=np.float32) * np.float32(3.0)).astype(np.float32)


def test_render_ref_equals_the_literal_reference_expressions():
    depths = _clip()
    table = colormaps.TABLES["inferno"]
    colormap = table.astype(np.float64) / 255.0 + 1e-9            # stands in for cm.get_cmap("inferno").colors: (colormap * 255) truncates back to the table
    assert np.array_equal((colormap * 255).astype(np.uint8), table)
    rgbs = np.random.default_rng(1).integers(0, 256, size=depths.shape + (3,), dtype=np.uint8)
    # utils/eval_utils.py:288-294 (save_video), literally
    d_min, d_max = depths.min(), depths.max()
    want = []
    for i in range(depths.shape[0]):
        depth = depths[i]
        depth_norm = ((depth - d_min) / (d_max - d_min + 1e-6) * 255).astype(np.uint8)
        depth_vis = (colormap[depth_norm] * 255).astype(np.uint8)
        rgb = rgbs[i].astype(np.uint8)
        want.append(np.concatenate([rgb, depth_vis], axis=1))
    assert np.array_equal(colorize_ref(depths, "video", table, frames=rgbs), np.stack(want))
    # evaluate_depth_video.py:33-34 (render_depth), literally; its table is cv2's and is not compared
    for disp in depths:
        lit = ((disp - disp.min()) / (disp.max() - disp.min()) * 255.0).astype(np.uint8)
        assert np.array_equal(index_ref(disp, disp.min(), disp.max(), 0, False), lit)
        assert lit.min() == 0 and lit.max() == 255
    # test_simple.py:158: the exact lower order statistic against np.percentile; the interpolated percentile lies between it and its neighbour
    rng = ranges_ref(depths, "quantile", q=(0.0, 0.95))
    for f, (lo, hi) in zip(depths, rng):
        s = np.sort(f.ravel())
        k = int(np.floor(0.95 * (s.size - 1)))
        assert lo == f.min() and hi == np.percentile(f, 95, method="lower") == s[k]
        assert s[k] <= np.percentile(f, 95) <= s[k + 1]
    # a constant frame: index 0 where the reference divides 0 by 0; "fixed" clips
    flat = np.full((1, 3, 4), 1.5, np.float32)
    for norm in ("video", "frame", "quantile"):
        assert np.array_equal(colorize_ref(flat, norm, table), np.broadcast_to(table[0], (1, 3, 4, 3)))
    x = np.array([[[-1.0, 0.0, 0.5, 1.0, 2.0, 7.0]]], np.float32)
    assert index_ref(x[0], 0.0, 2.0, 0, True).tolist() == [[0, 0, 63, 127, 255, 255]]
    assert np.array_equal(ranges_ref(x, "fixed", lo=0.0, hi=2.0), [[0.0, 2.0]])


# ---- 3. arguments ------------------------------------------------------------------------------------------------------------------------------
class StubBackend:
    """The protocol of tests/test_stream_cpu.py with coloured frames: a "frame" of the result carries its own index in every byte."""

    def __init__(self):
        self.done, self.blocks, self.windows = 0, [], 0

    def begin_push(self):
        pass

    def upload(self, first, frames):
        pass

    def window(self, k, source, upto):
        self.windows += 1
        self.blocks.append((self.done, upto))
        self.done = upto

    def collect(self, wait):
        got = [i for a, b in self.blocks for i in range(a, b)]
        self.blocks = []
        return np.broadcast_to(np.asarray(got, dtype=np.uint8).reshape(-1, 1, 1, 1), (len(got), FH, FW, 3)).copy()

    def release(self):
        pass


def test_stream_refuses_the_video_norm_and_other_objects():
    with pytest.raises(ValueError, match="video"):
        video.DepthStream(None, (FH, FW), render=Render("video"), backend=StubBackend())
    with pytest.raises(ValueError, match="render"):
        video.DepthStream(None, (FH, FW), render="inferno", backend=StubBackend())
    assert video.DepthStream(None, (FH, FW), backend=StubBackend()).render is None


@pytest.mark.parametrize("norm", ["frame", "fixed", "quantile"])
def test_stream_counts_coloured_frames(norm):
    r = Render(norm, lo=0.0, hi=1.0) if norm == "fixed" else Render(norm)
    stream = video.DepthStream(None, (FH, FW), render=r, backend=StubBackend())
    assert stream.render is r
    got = [stream.push(np.zeros((FH, FW, 3), np.uint8))]
    assert got[0].shape == (0, FH, FW, 3) and got[0].dtype == np.uint8 and (stream.pushed, stream.emitted) == (1, 0)
    got.append(stream.push(np.zeros((60, FH, FW, 3), np.uint8)))
    assert got[1].shape == (46, FH, FW, 3) and (stream.pushed, stream.emitted, stream.windows) == (61, 46, 2)
    got.append(stream.close())
    assert got[2].shape == (15, FH, FW, 3) and stream.pushed == stream.emitted == 61
    again = stream.close()
    assert again.shape == (0, FH, FW, 3) and again.dtype == np.uint8
    assert np.array_equal(np.concatenate(got)[:, 0, 0, 0], np.arange(61))


class _Runner:
    def __init__(self, frames):
        self.frames, self.calls = frames, []

    def run(self, sources):
        self.calls.append("run")
        return [np.zeros((32,) + self.frames.shape[1:3], np.float32) for _ in sources]

    def run_stitched(self, sources, n, output="host", render=None):
        self.calls.append((output, render))
        return np.zeros((n,) + self.frames.shape[1:3] + ((3,) if render is not None else ()), np.uint8 if render is not None else np.float32)


class _OldRunner(_Runner):  # a runner from before the keyword
    def run_stitched(self, sources, n, output="host"):
        return super().run_stitched(sources, n, output)


def test_render_argument_of_infer_video_depth():
    frames = np.zeros((50, 6, 8, 3), np.uint8)
    runner, r = _Runner(frames), Render("frame")
    with pytest.raises(ValueError, match="stitch"):
        video.infer_video_depth(None, frames, runner=runner, render=r)                                   # stitch defaults to "host"
    with pytest.raises(ValueError, match="stitch"):
        video.infer_video_depth(None, frames, runner=runner, stitch="host", render=r)
    with pytest.raises(ValueError, match="shard_windows"):
        video.infer_video_depth(None, frames, runner=runner, stitch="device", shard_windows=True, rank=0, world=1, render=r)
    with pytest.raises(ValueError, match="render"):
        video.infer_video_depth(None, frames, runner=runner, stitch="device", render="inferno")
    assert runner.calls == []
    out = video.infer_video_depth(None, frames, runner=runner, stitch="device", render=r)
    assert out.shape == (50, 6, 8, 3) and out.dtype == np.uint8 and runner.calls == [("host", r)]
    video.infer_video_depth(None, frames, runner=runner, stitch="device", output="device", render=r)
    assert runner.calls[-1] == ("device", r)
    old = _OldRunner(frames)  # the keyword reaches the runner only when it is given
    assert video.infer_video_depth(None, frames, runner=old, stitch="device").shape == (50, 6, 8)
    assert video.infer_video_depth(None, frames, runner=old, stitch="device", output="device").shape == (50, 6, 8)
    assert old.calls == [("host", None), ("device", None)]


# ---- 4. the C interface --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_types_the_entry_points():
    header = open(os.path.join(ROOT, "include", "endodav_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^(size_t|int) " + name + r"\(", header, re.M), name
        assert name in _lib.SIGNATURES, name
    assert "NaN is unsupported" in header
    assert _lib.ABI_VERSION == 15
