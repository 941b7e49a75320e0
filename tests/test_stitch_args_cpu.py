"""The ``stitch=`` argument of infer_video_depth and its way through the evaluation harness, with stub runners (no GPU, no model)."""
import numpy as np
import pytest

from endodav_amd import evaluate as ev
from endodav_amd import video


class _Runner:
    """HipWindowRunner stand-in: window k's 32 maps are a deterministic function of its 32 input frames."""

    def __init__(self, frames):
        self.frames = frames
        self.stitched = 0

    def run(self, sources):
        return [(0.1 + 0.8 * self.frames[idx].astype(np.float32).mean(axis=3) / 255.0).astype(np.float32) for idx in sources]

    def run_stitched(self, sources, n):
        self.stitched += 1
        return np.full((n,) + self.frames.shape[1:3], 7.0, np.float32)


def _frames(n=50, h=6, w=8):
    return np.random.default_rng(5).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def test_unknown_stitch_value_is_refused():
    frames = _frames()
    with pytest.raises(ValueError, match="stitch"):
        video.infer_video_depth(None, frames, runner=_Runner(frames), stitch="nope")


def test_device_stitch_does_not_combine_with_sharded_windows():
    frames = _frames()
    with pytest.raises(ValueError, match="shard_windows"):
        video.infer_video_depth(None, frames, runner=_Runner(frames), stitch="device", shard_windows=True, rank=0, world=1)


def test_default_is_the_host_stitch():
    frames = _frames()
    runner = _Runner(frames)
    want = video.stitch_windows(runner.run(video.window_sources(len(frames))), len(frames))
    assert np.array_equal(video.infer_video_depth(None, frames, runner=runner), want)
    assert np.array_equal(video.infer_video_depth(None, frames, runner=runner, stitch="host"), want)
    assert runner.stitched == 0
    out = video.infer_video_depth(None, frames, runner=runner, stitch="device")
    assert runner.stitched == 1 and out.shape == (50, 6, 8) and (out == 7.0).all()


def test_evaluate_video_passes_stitch_only_when_given():
    class Plain:  # takes no stitch argument, like the stand-ins of the other CPU tests
        def infer_video_depth(self, colors):
            return (0.1 + 0.8 * colors.astype(np.float32).mean(axis=3) / 255.0).astype(np.float32)

    class Knows(Plain):
        seen = []

        def infer_video_depth(self, colors, stitch="host"):
            self.seen.append(stitch)
            return super().infer_video_depth(colors)

    ds = ev.SyntheticVideos(n_clips=2, n_frames=4, height=12, width=16)
    base = ev.evaluate_video(Plain(), ds, depth_align="scale_shift", device=None, rank=0, world=1)
    got = ev.evaluate_video(Knows(), ds, depth_align="scale_shift", device=None, rank=0, world=1, stitch="device")
    assert Knows.seen == ["device", "device"]
    assert np.array_equal(got["errors"], base["errors"])
    with pytest.raises(TypeError):
        ev.evaluate_video(Plain(), ds, depth_align="scale_shift", device=None, rank=0, world=1, stitch="device")
