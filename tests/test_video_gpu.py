"""infer_video_depth on MI355X: windowing, key-frame reuse and stitching against the reference golden,
then one real end-to-end run (frames -> HIP forward -> stitched depth)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, synth, video
from endodav_amd.endodav import DashLinear
from endodav_amd.pipeline import ClipsInFlight
from tests import helpers as H
from tests.golden.make_golden import VIDEO_CASE, fake_window_disp, long_video_frames

pytestmark = pytest.mark.gpu


def _model(h, w, cuda, lora_type="none"):
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(h, w), lora_type=lora_type,
                            disable_conv_head=True).eval()
    synth.fill_module_(m)
    return m.to(cuda)


def test_windowing_keyframes_and_stitching_match_reference(cuda):
    g = H.load_golden("video_stitch")
    n, h, w = VIDEO_CASE["n_frames"], VIDEO_CASE["h"], VIDEO_CASE["w"]
    model = _model(h, w, cuda)
    frames = (synth.uniform("video:frames", (n, h, w, 3), 0.0, 1.0) * 255).astype(np.uint8)
    seen = []

    def recorder(x, lane=0):  # same stand-in forward the reference ran when the golden was made (lane: which engine context, pipeline.ClipsInFlight)
        assert x.is_cuda and x.shape == (1, 32, 3, h, w)
        seen.append(x[0].mean(dim=(1, 2, 3)).double().cpu().numpy())
        return {("disp", 0): torch.from_numpy(fake_window_disp(len(seen) - 1, h, w)).to(x.device)}

    model.forward = recorder
    out = model.infer_video_depth(frames, device="cuda:0")
    assert out.shape == (n, h, w) and out.dtype == np.float32
    assert np.abs(np.stack(seen) - g["window_input_means"]).max() < 1e-6  # padding + key-frame substitution
    assert np.abs(out - g["out"]).max() <= 2e-6 * np.abs(g["out"]).max()  # resize-to-native (identity) + stitching


def test_real_video_run_with_native_resolution_resize(cuda):
    """Frames larger than image_shape: bicubic pre-resize (unpinned), forward, bilinear back, stitch."""
    h, w = 42, 56
    model = _model(h, w, cuda)
    frames = (synth.synth_clip(1, 25, 60, 80, seed=4, kind="tissue")[0].transpose(0, 2, 3, 1) * 255).astype(np.uint8)
    out = model.infer_video_depth(frames, device="cuda:0")
    assert out.shape == (25, 60, 80) and np.isfinite(out).all() and (out >= 0).all() and out.max() > 0
    # 25 frames = two windows (the second one exercises the pipelined upload / download).  Stitching rewrites only the last INTERP_LEN = 8
    # slots of window 0, so frames 0..23 must equal the direct forward on the HIP-resized clip of window 0, brought back to the frame size
    # with torch's own bilinear (align_corners=True, endodav.py:203-204) -- the streams, the uint8 upload and the stitching add nothing
    from endodav_amd import video

    runner = video.HipWindowRunner(model, np.ascontiguousarray(frames), torch.device("cuda:0"))
    sources = video.window_sources(25)
    assert len(sources) == 2
    x = runner.resized_clip(sources[0])
    assert x.shape == (1, 32, 3, h, w)
    with torch.no_grad():
        disp = model(x)[("disp", 0)]  # [32, 1, h, w]
        direct = torch.nn.functional.interpolate(disp, size=(60, 80), mode="bilinear", align_corners=True)[:24, 0].cpu().numpy()
    assert np.abs(out[:24] - direct).max() <= 2e-6 * np.abs(direct).max()
    out2 = model.infer_video_depth(frames, device="cuda:0")
    assert np.array_equal(out, out2)  # and the pipelined run is reproducible bit for bit


def test_evaluate_video_end_to_end(cuda):
    """evaluate_depth_video.py's loop on synthetic clips through the real HIP model: plumbing + report format."""
    from endodav_amd import evaluate as ev

    model = _model(42, 56, cuda)
    ds = ev.SyntheticVideos(n_clips=2, n_frames=5, height=42, width=56)
    res = ev.evaluate_video(model, ds, depth_align="scale_shift", device="cuda:0")
    assert res["errors"].shape == (10, 7) and res["temporal"].shape == (8, 2) and np.isfinite(res["errors"]).all()
    assert len(res["inference_times"]) == 2 and res["aligns"].shape == (2, 4)
    txt = ev.format_results(res)
    assert txt.startswith("    abs_rel") and "average inference time" in txt


# ---- the real runner on long videos ----------------------------------------------------------------------------------------------------
# Expectation: every window on its own through lane 0 (model(x), the caller's stream), with the runner's own conversion / pre-resize
# (resized_clip) and the same edv_bilinear back to the frame size, then stitch_windows.  Lanes are bit-identical to lane 0
# (test_pipeline_gpu.py) and every other op is the same call, so the pipelined run must reproduce it bit for bit: no tolerance.
NET_H, NET_W = 42, 56


def _window_maps(model, runner, sources, cuda):
    lib = _lib.load()
    maps = []
    with torch.cuda.device(cuda), torch.no_grad():
        for src in sources:
            disp = model(runner.resized_clip(src))[("disp", 0)]  # [32, 1, ih, iw]
            full = torch.empty((video.INFER_LEN, runner.fh, runner.fw), device=cuda, dtype=torch.float32)
            _lib.check(lib.edv_bilinear(disp.data_ptr(), full.data_ptr(), video.INFER_LEN, disp.shape[-2], disp.shape[-1], 1, runner.fh, runner.fw,
                                        C.c_void_p(_lib.stream_ptr(cuda))), "edv_bilinear")
            maps.append(full.cpu().numpy())
    return maps


class _LongVideo:
    """One model, 120 frames (6 windows) and the per-window expectation, computed once per frame size and only read afterwards."""

    def __init__(self, cuda, fh, fw):
        self.model = _model(NET_H, NET_W, cuda)
        self.frames = long_video_frames(120, fh, fw)
        self.runner = video.HipWindowRunner(self.model, self.frames, cuda)
        assert (self.runner.th, self.runner.tw) == (NET_H, NET_W)
        self.sources = video.window_sources(120)
        assert len(self.sources) == 6
        self.maps = _window_maps(self.model, self.runner, self.sources, cuda)
        for a in self.maps:
            a.setflags(write=False)
        for i in range(6):  # every window differs from every other one: a result in the wrong place cannot pass
            for j in range(i):
                assert not np.array_equal(self.maps[i], self.maps[j])
        self.want = video.stitch_windows(self.maps, 120)
        self.want.setflags(write=False)


@pytest.fixture(scope="module")
def long_videos(cuda):
    cache = {}

    def get(fh, fw):
        if (fh, fw) not in cache:
            cache[(fh, fw)] = _LongVideo(cuda, fh, fw)
        return cache[(fh, fw)]

    return get


def _force_depth(monkeypatch, depth):
    monkeypatch.setattr(ClipsInFlight, "auto_depth", staticmethod(lambda model, frames: depth))


@pytest.mark.parametrize("fh,fw", [(NET_H, NET_W), (60, 80)], ids=["native", "resized"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_long_video_equals_window_by_window_at_every_depth(cuda, long_videos, monkeypatch, depth, fh, fw):
    """6 windows on depth + 1 = 2, 3, 4 buffer slots: every slot is reused, so the wait before a device buffer is overwritten, the wait
    before a pinned buffer is rewritten and the in-loop drain in window order all run.  Twice: the second call reuses the cached lanes."""
    lv = long_videos(fh, fw)
    _force_depth(monkeypatch, depth)
    out = lv.model.infer_video_depth(lv.frames, device="cuda:0")
    assert out.shape == (120, fh, fw) and out.dtype == np.float32
    flight = lv.model._video_flight
    assert flight.depth == depth and len(flight.lanes) == depth
    assert np.array_equal(out, lv.want)
    again = lv.model.infer_video_depth(lv.frames, device="cuda:0")
    assert lv.model._video_flight is flight  # the cached lanes, mid round-robin (6 windows on 1..3 lanes)
    assert np.array_equal(again, lv.want)


@pytest.mark.parametrize("n", [1, 22, 23])
def test_short_videos_equal_window_by_window(cuda, long_videos, n):
    """One window of one frame and 31 padding copies, one exactly full step, and the first length with a second window."""
    lv = long_videos(NET_H, NET_W)
    frames = np.ascontiguousarray(lv.frames[:n])
    runner = video.HipWindowRunner(lv.model, frames, cuda)
    sources = video.window_sources(n)
    assert len(sources) == (1 if n <= 22 else 2)
    want = video.stitch_windows(_window_maps(lv.model, runner, sources, cuda), n)
    out = lv.model.infer_video_depth(frames, device="cuda:0")
    assert out.shape == (n, NET_H, NET_W) and out.dtype == np.float32
    assert np.array_equal(out, want)


@pytest.mark.parametrize("depth", [1, 3])
def test_runner_returns_a_subset_of_windows_in_the_order_given(cuda, long_videos, monkeypatch, depth):
    """What shard_windows=True hands one rank: some windows of the video.  run() must return exactly their maps, in that order."""
    lv = long_videos(60, 80)
    _force_depth(monkeypatch, depth)
    picks = (0, 2, 3, 5)
    got = lv.runner.run([lv.sources[k] for k in picks])
    assert len(got) == len(picks)
    for k, g in zip(picks, got):
        assert g.shape == (video.INFER_LEN, 60, 80) and np.array_equal(g, lv.maps[k]), f"window {k}"
    assert lv.runner.run([]) == []


# ---- lora_type="dash": one call counter per model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [DashLinear.WARMUP - 1, 0], ids=["straddles_activation", "inside_warmup"])
def test_dash_video_counts_one_call_per_window(cuda, start):
    """The reference's infer_video_depth calls forward once per window, and DashLinear counts those calls: a 3-window video that starts at
    call count 99 runs calls 100 (plain LoRA), 101 (selects the SVD directions, folds the extra term) and 102.  The result must equal a
    twin model run window by window through model(x) from the same count, and the count must have advanced by exactly 3."""
    n = 50
    frames = long_video_frames(n, NET_H, NET_W)
    sources = video.window_sources(n)
    assert len(sources) == 3
    model, twin = _model(NET_H, NET_W, cuda, "dash"), _model(NET_H, NET_W, cuda, "dash")
    model._dash_calls = twin._dash_calls = start
    want = video.stitch_windows(_window_maps(twin, video.HipWindowRunner(twin, frames, cuda), sources, cuda), n)
    assert twin._dash_calls == start + 3
    out = model.infer_video_depth(frames, device="cuda:0")
    assert model._dash_calls == start + 3 and all(m.FLAG == start + 3 for m in model._dash_layers())
    assert model._config().dash_active == int(start + 3 > DashLinear.WARMUP)
    assert out.shape == (n, NET_H, NET_W) and np.array_equal(out, want)


# ---- run() orders itself after the caller's stream -------------------------------------------------------------------------------------
@pytest.mark.parametrize("caller", ["default_stream", "side_stream"])
def test_video_run_waits_for_weights_written_on_the_callers_stream(cuda, caller):
    """Validation straight after a training step: the weights are written in place on the caller's stream (behind other work queued there), and
    infer_video_depth is called at once, with no synchronisation.  The first forward on every lane re-folds the LoRA factors and re-packs the
    biases on the lane's stream, so the lanes must wait for the caller's stream; the result must equal that of the same call on a twin whose
    edit was synchronised first.  The work queued ahead of the edit is timed with events in this very run and must last at least twice one whole
    infer_video_depth of this video (measured just before), so a lane that does not wait certainly folds first.  Stale values at worst:
    nothing is freed or reallocated while the work is in flight."""
    n = 50  # 3 windows: one per lane at depth 3
    frames = long_video_frames(n, NET_H, NET_W)
    model, twin = _model(NET_H, NET_W, cuda, "dvlora"), _model(NET_H, NET_W, cuda, "dvlora")
    stream = torch.cuda.current_stream(cuda) if caller == "default_stream" else torch.cuda.Stream(device=cuda)

    def edit(m):
        with torch.no_grad():
            m.pretrained.blocks[0].mlp.fc1.lora_B.mul_(1.5)
            m.head.scratch.output_conv2[2].bias.add_(0.01)

    ev = lambda: torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()  # the models' weights are in place before another stream reads them
    with torch.cuda.stream(stream):
        base = model.infer_video_depth(frames, device="cuda:0")  # builds the lanes: from here on a weight change is a re-fold on the lane
        assert np.array_equal(twin.infer_video_depth(frames, device="cuda:0"), base)  # twins agree bit for bit before the edit
        t0, t1 = ev(), ev()
        t0.record(stream)
        model.infer_video_depth(frames, device="cuda:0")
        t1.record(stream)
        t1.synchronize()
        run_ms = t0.elapsed_time(t1)
        # the delay: a chain of fp32 matrix products, sized from one timed batch of them to four times the run
        a = torch.rand(4096, 4096, device=cuda)
        b = torch.empty_like(a)
        torch.mm(a, a, out=b)
        c0, c1 = ev(), ev()
        c0.record(stream)
        for _ in range(8):
            torch.mm(a, a, out=b)
        c1.record(stream)
        c1.synchronize()
        count = max(8, math.ceil(4.0 * run_ms / (c0.elapsed_time(c1) / 8)))
        d0, d1 = ev(), ev()
        d0.record(stream)
        for _ in range(count):
            torch.mm(a, a, out=b)
        d1.record(stream)
        edit(model)                                                # queued behind the delay
        got = model.infer_video_depth(frames, device="cuda:0")     # at once
        torch.cuda.synchronize()
        delay_ms = d0.elapsed_time(d1)
        print(f"\n[stream order, {caller}] one infer_video_depth {run_ms:.2f} ms; delay ahead of the edit {delay_ms:.2f} ms ({count} products)")
        assert delay_ms >= 2.0 * run_ms
        edit(twin)
        torch.cuda.synchronize()
        want = twin.infer_video_depth(frames, device="cuda:0")
    assert not np.array_equal(want, base)  # the edit shows in the result
    assert np.array_equal(got, want)
