"""Evaluation on the device, the parts that need no GPU: the fp64 yardstick of tests/test_metrics_gpu.py against the host metrics and the
reference's known answers, the ABI, and the ``metrics=`` / ``output=`` arguments with stub runners and depthers."""
import numpy as np
import pytest

from endodav_amd import _lib
from endodav_amd import evaluate as ev
from endodav_amd import video
from tests import helpers as H
from tests.golden.make_golden import metrics_inputs
from tests.metrics_ref import errors_ref64, metrics_ref64, pair_ref64

NEW_ENTRY_POINTS = ("edv_metrics_workspace", "edv_masked_median", "edv_metrics_pred", "edv_metrics_errors", "edv_metrics_temporal")


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------------------
def test_ref64_agrees_with_the_host_metrics_and_the_known_answers():
    g, x = H.load_golden("metrics_kat"), metrics_inputs()
    valid = (x["gt"] > 1e-3) & (x["gt"] < 150)
    ref = errors_ref64(x["gt"], x["pred"], valid)
    assert ref[0] == valid.sum()
    assert np.allclose(ref[1:], ev.compute_errors(x["gt"], x["pred"], valid), rtol=1e-6)
    assert np.allclose(ref[1:], g["compute_errors"], rtol=1e-6)
    mask = np.ones_like(x["depth_a"], dtype=bool)
    mask[:3] = False
    i2w_a, i2w_b = np.linalg.inv(x["K"] @ x["pose_a"]), np.linalg.inv(x["K"] @ x["pose_b"])
    tae, tas = pair_ref64(x["depth_a"], mask, i2w_a, x["depth_b"], mask, i2w_b)
    assert np.isclose(tae, ev.tae(x["depth_a"], mask, i2w_a, x["depth_b"], mask, i2w_b), rtol=1e-6) and np.isclose(tae, g["tae"], rtol=1e-6)
    assert np.isclose(tas, ev.tas(x["depth_a"], mask, i2w_a, x["depth_b"], mask, i2w_b), rtol=1e-6) and np.isclose(tas, g["tas"], rtol=1e-6)
    # the clip form: per-frame rows and per-pair rows, an all-invalid frame is a NaN row
    gt = x["gt"].copy()
    gt[2] = 0.0
    errors, temporal = metrics_ref64(x["pred"], gt, np.stack([i2w_a, i2w_b, i2w_a]))
    assert errors.shape == (3, 8) and temporal.shape == (2, 2)
    assert errors[2, 0] == 0 and np.isnan(errors[2, 1:]).all() and np.isnan(temporal[1]).all()
    for i in range(2):
        v = (gt[i] > 1e-3) & (gt[i] < 150)
        assert np.allclose(errors[i, 1:], ev.compute_errors(gt[i], x["pred"][i], v), rtol=1e-6)
    v0, v1 = [(gt[i] > 1e-3) & (gt[i] < 150) for i in range(2)]
    assert np.isclose(temporal[0, 0], ev.tae(x["pred"][0], v0, i2w_a, x["pred"][1], v1, i2w_b), rtol=1e-6)
    assert np.isclose(temporal[0, 1], ev.tas(x["pred"][0], v0, i2w_a, x["pred"][1], v1, i2w_b), rtol=1e-6)


# ---- 2. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_14_types_the_metrics_entry_points():
    assert _lib.ABI_VERSION == 15
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.edv_abi_version() == 15
    head = lib.edv_metrics_workspace(0, 0, 0)
    assert head > 0
    # the key images of one chunk of pairs are all that depends on the shape, and nothing depends on the length of the clip
    assert lib.edv_metrics_workspace(5, 40, 56) == lib.edv_metrics_workspace(5000, 40, 56) > head
    assert lib.edv_metrics_workspace(2, 1024, 1280) - head <= 8 * 8 * 1024 * 1280


# ---- 3. arguments -------------------------------------------------------------------------------------------------------------------------
class _Runner:
    def __init__(self, frames):
        self.frames = frames
        self.outputs = []

    def run(self, sources):
        return [(0.1 + 0.8 * self.frames[idx].astype(np.float32).mean(axis=3) / 255.0).astype(np.float32) for idx in sources]

    def run_stitched(self, sources, n, output="host"):
        self.outputs.append(output)
        return np.full((n,) + self.frames.shape[1:3], 7.0, np.float32)


class _OldRunner(_Runner):  # a runner from before the keyword
    def run_stitched(self, sources, n):
        return super().run_stitched(sources, n)


def _frames(n=50, h=6, w=8):
    return np.random.default_rng(5).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def test_output_argument_of_infer_video_depth():
    frames = _frames()
    runner = _Runner(frames)
    with pytest.raises(ValueError, match="output"):
        video.infer_video_depth(None, frames, runner=runner, stitch="device", output="nope")
    with pytest.raises(ValueError, match="output"):
        video.infer_video_depth(None, frames, runner=runner, output="device")  # stitch defaults to "host"
    with pytest.raises(ValueError, match="output"):
        video.infer_video_depth(None, frames, runner=runner, stitch="host", output="device")
    with pytest.raises(ValueError, match="shard_windows"):
        video.infer_video_depth(None, frames, runner=runner, stitch="device", output="device", shard_windows=True, rank=0, world=1)
    assert runner.outputs == []
    out = video.infer_video_depth(None, frames, runner=runner, stitch="device", output="device")
    assert runner.outputs == ["device"] and out.shape == (50, 6, 8)
    old = _OldRunner(frames)  # the keyword reaches the runner only when it is "device"
    assert video.infer_video_depth(None, frames, runner=old, stitch="device").shape == (50, 6, 8)
    assert video.infer_video_depth(None, frames, runner=old, stitch="device", output="host").shape == (50, 6, 8)


class _Plain:  # knows neither keyword, like the stand-ins of the other CPU tests
    def infer_video_depth(self, colors):
        return (0.1 + 0.8 * colors.astype(np.float32).mean(axis=3) / 255.0).astype(np.float32)


class _Knows(_Plain):
    def __init__(self):
        self.seen = []

    def infer_video_depth(self, colors, stitch="host", output="host"):
        self.seen.append((stitch, output))
        return super().infer_video_depth(colors)


@pytest.mark.parametrize("align", ["scale", "scale_shift", "none"])
def test_evaluate_video_metrics_argument(monkeypatch, align):
    ds = ev.SyntheticVideos(n_clips=2, n_frames=4, height=12, width=16)
    kw = dict(depth_align=align, device=None, rank=0, world=1)
    base = ev.evaluate_video(_Plain(), ds, **kw)
    assert base["errors"].shape == (8, 7) and base["temporal"].shape == (6, 2)
    same = ev.evaluate_video(_Plain(), ds, metrics="host", **kw)  # a depther without the keywords works whenever metrics is not "device"
    with pytest.raises(ValueError, match="metrics"):
        ev.evaluate_video(_Plain(), ds, metrics="nope", **kw)
    with pytest.raises(ValueError, match="stitch"):
        ev.evaluate_video(_Knows(), ds, metrics="device", stitch="host", **kw)
    with pytest.raises(TypeError):
        ev.evaluate_video(_Plain(), ds, metrics="device", **kw)

    calls = []

    def on_host(disp_dev, item, *args):
        calls.append(item["filename"])
        return ev.clip_metrics_host(disp_dev, item, *args)

    monkeypatch.setattr(ev, "clip_metrics_device", on_host)
    depther = _Knows()
    got = ev.evaluate_video(depther, ds, metrics="device", **kw)
    assert depther.seen == [("device", "device")] * 2 and calls == ["synthetic/clip0/0", "synthetic/clip1/0"]
    for res in (same, got):
        for key in ("errors", "temporal", "ratios", "aligns"):
            assert np.array_equal(res[key], base[key]), key
    assert len(got["inference_times"]) == 2
