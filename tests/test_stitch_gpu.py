"""infer_video_depth(stitch="device") on MI355X: edv_stitch_fit / edv_stitch_apply alone, then through the public call and the real runner.

Yardstick of every numeric gate: ``stitch_ref64``, an fp64 restatement of ``video.stitch_windows`` on the same window maps -- sums, solve,
affine, clamp and fade in fp64, (s, t) rounded to fp32 before they are applied, as the kernel does.

  gate A  device vs restatement: max|dev - ref64| <= 5e-7 max|ref64|.  An output element passes at most 8 fp32 roundings (s, t, the
          product, the sum, two fade weights, two fade products / their sum), each 2^-24 of a value no larger than the scale: 4.8e-7.
  gate B  device vs a reference golden: max|dev - golden| <= max|golden - ref64| + 5e-7 max|golden| (the triangle inequality; the
          golden's own distance from fp64 is computed here).
  gate C  device no worse than the host path: max|dev - ref64| <= max|host - ref64| on the same maps.
"""
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
from tests.golden.make_golden import VIDEO_CASE, VIDEO_LONG_CASE, fake_window_disp, long_video_frames

pytestmark = pytest.mark.gpu

GATE_A = 5e-7
LEN, OVERLAP, INTERP = video.INFER_LEN, video.OVERLAP, video.INTERP_LEN
STEP = LEN - OVERLAP


def stitch_ref64(maps, n_keep):
    """-> (out [n_keep, H, W] fp64, [(s, t)] of windows 1.., margin [n_keep, H, W]).  ``margin`` is the smallest |value before the clamp| among
    the clamped values an output element was made of (inf for window 0, which is not clamped): where it is tiny, fp32 and fp64 may
    land on different sides of zero."""
    step = 1.0 / (INTERP - 1)
    fade = [0.0] + [i * step for i in range(1, INTERP - 1)] + [1.0]
    out, margin, fits = [], [], []
    for wi, cur in enumerate(maps):
        cur = np.asarray(cur, dtype=np.float64)
        if wi == 0:
            out.extend(cur)
            margin.extend(np.full_like(cur, np.inf))
            continue
        pre = np.stack(out[-INTERP:])
        post = cur[OVERLAP - INTERP:OVERLAP]
        a00, a01, a11, b0, b1 = (post * post).sum(), post.sum(), float(post.size), (post * pre).sum(), pre.sum()
        det = a00 * a11 - a01 * a01
        s, t = (1.0, 0.0) if det == 0 else ((a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det)
        s, t = float(np.float32(s)), float(np.float32(t))
        fits.append((s, t))
        raw = cur * s + t
        al = np.maximum(raw, 0.0)
        for i in range(INTERP):
            j = len(out) - INTERP + i
            out[j] = pre[i] * (1 - fade[i]) + al[OVERLAP - INTERP + i] * fade[i]
            margin[j] = np.minimum(margin[j], np.abs(raw[OVERLAP - INTERP + i]))
        out.extend(al[OVERLAP:])
        margin.extend(np.abs(raw[OVERLAP:]))
    return np.stack(out[:n_keep]), fits, np.stack(margin[:n_keep])


def _stream(cuda):
    return C.c_void_p(_lib.stream_ptr(cuda))


def _upsampled(disp, fh, fw, cuda):
    """edv_bilinear of [32, ih, iw] device maps -> numpy [32, fh, fw]: what the stitch kernels must reproduce bit for bit on the fly."""
    lib = _lib.load()
    full = torch.empty((LEN, fh, fw), device=cuda, dtype=torch.float32)
    _lib.check(lib.edv_bilinear(disp.data_ptr(), full.data_ptr(), LEN, disp.shape[-2], disp.shape[-1], 1, fh, fw, _stream(cuda)), "edv_bilinear")
    return full.cpu().numpy()


def device_stitch(maps, fh, fw, cuda):
    """fit + apply through ctypes for every window in order, the output kept whole on the device.  ``maps``: numpy [32, ih, iw] per window.
    -> (out [32 + 22 (K - 1), fh, fw], fitted (s, t) [K, 2] (row 0 unused), the frame-size maps edv_bilinear makes of the same windows)."""
    lib = _lib.load()
    K = len(maps)
    with torch.cuda.device(cuda):
        out = torch.full((LEN + STEP * (K - 1), fh, fw), float("nan"), device=cuda, dtype=torch.float32)
        st = torch.zeros((K, 2), device=cuda, dtype=torch.float32)
        ws = torch.empty(int(lib.edv_stitch_workspace()), device=cuda, dtype=torch.uint8)
        full = []
        for k, m in enumerate(maps):
            d = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(cuda)
            ih, iw = d.shape[-2:]
            full.append(_upsampled(d, fh, fw, cuda))
            if k == 0:
                _lib.check(lib.edv_stitch_apply(d.data_ptr(), ih, iw, None, None, out.data_ptr(), fh, fw, _stream(cuda)), "edv_stitch_apply")
                continue
            end = LEN + STEP * (k - 1)
            tail, new = out[end - INTERP:end], out[end:end + STEP]
            _lib.check(lib.edv_stitch_fit(d.data_ptr(), ih, iw, tail.data_ptr(), fh, fw, st[k].data_ptr(), ws.data_ptr(), ws.numel(), _stream(cuda)),
                       "edv_stitch_fit")
            _lib.check(lib.edv_stitch_apply(d.data_ptr(), ih, iw, st[k].data_ptr(), tail.data_ptr(), new.data_ptr(), fh, fw, _stream(cuda)),
                       "edv_stitch_apply")
        torch.cuda.synchronize()
        return out.cpu().numpy(), st.cpu().numpy(), full


def _gate_a(dev, ref, what):
    err, scale = np.abs(dev.astype(np.float64) - ref).max(), np.abs(ref).max()
    print(f"\n[{what}] device vs fp64 restatement: {err / scale:.2e} of the scale {scale:.3f}")
    assert err <= GATE_A * scale, f"{what}: {err / scale:.3e} of the scale"
    return err


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ih,iw,fh,fw", [(28, 42, 28, 42), (28, 42, 37, 53), (42, 56, 60, 80)], ids=["identity", "odd_scalar_path", "upsampled"])
def test_kernels_match_fp64_restatement(cuda, ih, iw, fh, fw):
    """6 windows of fake_window_disp.  28 x 42: the upsample is the identity and 1176 pixels a frame take the 16-byte path with groups that
    wrap from one row (42 wide) into the next; 37 x 53 = 1961 pixels: one pixel per access; 60 x 80: 16-byte path behind a real upsample."""
    K = 6
    n = LEN + STEP * (K - 1)
    maps = [fake_window_disp(k, ih, iw)[:, 0] for k in range(K)]
    dev, st, full = device_stitch(maps, fh, fw, cuda)
    assert dev.shape == (n, fh, fw) and np.isfinite(dev).all()
    assert np.array_equal(dev[:LEN - INTERP], full[0][:LEN - INTERP])  # window 0 is the plain upsample, bit for bit edv_bilinear's
    ref, fits, _ = stitch_ref64(full, n)
    err_dev = _gate_a(dev, ref, f"kernels {ih}x{iw}->{fh}x{fw}")
    host = video.stitch_windows(full, n)
    err_host = np.abs(host.astype(np.float64) - ref).max()
    print(f"[kernels {ih}x{iw}->{fh}x{fw}] host path vs fp64 restatement: {err_host / np.abs(ref).max():.2e}")
    assert err_dev <= err_host  # gate C
    # (s, t): one fp32 rounding of nearly the same fp64 number, 2^-23.  fake_window_disp draws its base field per frame, so the fit has no
    # slope: s is 5e-3 for window 1 and falls to 1e-12 by window 5, far below the 1e-7 of fp32 noise the tail carries -- its own relative
    # error means nothing under any arithmetic.  The pair is therefore compared as a vector, each component against the larger of the
    # two; the clamp test below, whose maps share one field (s = 0.76 .. 0.52), holds s and t each to 2^-23 of itself.
    for k, (s, t) in enumerate(fits, start=1):
        norm = max(abs(s), abs(t))
        ds, dt = abs(float(st[k, 0]) - s) / norm, abs(float(st[k, 1]) - t) / norm
        print(f"  window {k}: s {s:.7e} t {t:.7f}; difference {ds:.2e} / {dt:.2e} of the pair's scale")
        assert ds <= 2.0 ** -23 and dt <= 2.0 ** -23, f"window {k}"


# ---- 2. the clamp ------------------------------------------------------------------------------------------------------------------------
def test_clamp_zeros_where_the_restatement_has_them(cuda):
    h, w, K, n = 45, 67, 4, 80
    B = synth.uniform("stitch:clamp:base", (h, w), 0.0, 1.5)
    B[:10] = 0.0  # one field shared by all frames: the fit has a slope, and where B = 0 the aligned map straddles zero
    maps = []
    for k in range(K):
        m = (1 + 0.3 * k) * B[None] + 0.1 * k + synth.uniform(f"stitch:clamp:noise:{k}", (LEN, h, w), -0.05, 0.05)
        maps.append((np.maximum(m, 0.0) if k == 0 else m).astype(np.float32))
    ref, fits, margin = stitch_ref64(maps, n)
    zeros = ref[LEN:] == 0
    print(f"\n[clamp] exact zeros in frames >= 32 of the restatement: {zeros.mean():.2%}")
    assert 0.02 <= zeros.mean() <= 0.20
    dev, st, _ = device_stitch(maps, h, w, cuda)
    dev = dev[:n]
    _gate_a(dev, ref, "clamp")
    for k, (s, t) in enumerate(fits, start=1):  # a well-conditioned fit: each of s, t within one fp32 rounding of the restatement's
        ds, dt = abs(float(st[k, 0]) - s) / abs(s), abs(float(st[k, 1]) - t) / abs(t)
        print(f"  window {k}: s {s:.7f} t {t:.7f}; relative difference {ds:.2e} / {dt:.2e}")
        assert ds <= 2.0 ** -23 and dt <= 2.0 ** -23, f"window {k}"
    sure = margin > GATE_A * np.abs(ref).max()
    assert sure.mean() > 0.99
    assert np.array_equal((dev == 0)[sure], (ref == 0)[sure])
    assert (dev >= 0).all()


# ---- 3. det == 0 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0.0, 0.5])
def test_degenerate_fit_is_one_zero(cuda, value):
    """Constant maps: every sum is exact in fp64, det = 0 exactly, (s, t) = (1, 0) as the reference returns, and the result is the fade of
    the two constants with the fp32 weights of the host path."""
    h, w = 28, 42
    maps = [np.full((LEN, h, w), 0.25, np.float32), np.full((LEN, h, w), value, np.float32)]
    dev, st, _ = device_stitch(maps, h, w, cuda)
    assert st[1, 0] == 1.0 and st[1, 1] == 0.0
    step = 1.0 / (INTERP - 1)
    fade = [0.0] + [i * step for i in range(1, INTERP - 1)] + [1.0]
    want = np.empty((LEN + STEP, h, w), np.float32)
    want[:LEN - INTERP] = 0.25
    for i in range(INTERP):
        want[LEN - INTERP + i] = np.float32(0.25) * np.float32(1 - fade[i]) + np.float32(value) * np.float32(fade[i])
    want[LEN:] = value
    assert np.array_equal(dev, want)


# ---- 4. the public call against the reference goldens -----------------------------------------------------------------------------------
def _model(h, w, cuda, lora_type="none"):
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(h, w), lora_type=lora_type,
                            disable_conv_head=True).eval()
    synth.fill_module_(m)
    return m.to(cuda)


@pytest.mark.parametrize("name,case", [("video_stitch", VIDEO_CASE), ("video_stitch_long", VIDEO_LONG_CASE)])
def test_public_call_matches_reference_golden(cuda, name, case):
    g = H.load_golden(name)
    n, h, w = case["n_frames"], case["h"], case["w"]
    model = _model(h, w, cuda)
    frames = (synth.uniform("video:frames", (n, h, w, 3), 0.0, 1.0) * 255).astype(np.uint8) if name == "video_stitch" else long_video_frames(n, h, w)
    seen = []

    def recorder(x, lane=0):  # the stand-in forward the reference ran when the golden was made
        assert x.is_cuda and x.shape == (1, 32, 3, h, w)
        seen.append(x[0].mean(dim=(1, 2, 3)).double().cpu().numpy())
        return {("disp", 0): torch.from_numpy(fake_window_disp(len(seen) - 1, h, w)).to(x.device)}

    model.forward = recorder
    out = model.infer_video_depth(frames, device="cuda:0", stitch="device")
    assert out.shape == (n, h, w) and out.dtype == np.float32
    assert np.abs(np.stack(seen) - g["window_input_means"]).max() < 1e-6
    ref, _, _ = stitch_ref64([fake_window_disp(k, h, w)[:, 0] for k in range(len(seen))], n)
    gold = g["out"].astype(np.float64)
    own = np.abs(gold - ref).max()
    err = np.abs(out - gold).max()
    print(f"\n[{name}] golden vs fp64 restatement {own / np.abs(gold).max():.2e}; device vs golden {err / np.abs(gold).max():.2e} of the scale")
    assert err <= own + GATE_A * np.abs(gold).max()  # gate B


# ---- 5. the real runner, the real model -------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


def _window_maps(model, runner, sources, cuda):
    """Every window on its own through lane 0 with the runner's own conversion / pre-resize, brought to the frame size by edv_bilinear."""
    maps = []
    with torch.cuda.device(cuda), torch.no_grad():
        for src in sources:
            disp = model(runner.resized_clip(src))[("disp", 0)]
            maps.append(_upsampled(disp, runner.fh, runner.fw, cuda))
    return maps


class _LongVideo:
    """One model, 120 frames (6 windows), the host path's result and the restatement, computed once per frame size and only read afterwards."""

    def __init__(self, cuda, fh, fw):
        self.model = _model(NET_H, NET_W, cuda)
        self.frames = long_video_frames(120, fh, fw)
        self.runner = video.HipWindowRunner(self.model, self.frames, cuda)
        assert (self.runner.th, self.runner.tw) == (NET_H, NET_W)
        self.sources = video.window_sources(120)
        maps = _window_maps(self.model, self.runner, self.sources, cuda)
        self.host = self.model.infer_video_depth(self.frames, device="cuda:0")
        self.ref = stitch_ref64(maps, 120)[0]
        for a in (self.host, self.ref):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def long_videos(cuda):
    cache = {}

    def get(fh, fw):
        if (fh, fw) not in cache:
            cache[(fh, fw)] = _LongVideo(cuda, fh, fw)
        return cache[(fh, fw)]

    return get


@pytest.mark.parametrize("fh,fw", [(NET_H, NET_W), (60, 80)], ids=["native", "resized"])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_long_video_device_stitch_at_every_depth(cuda, long_videos, monkeypatch, depth, fh, fw):
    lv = long_videos(fh, fw)
    monkeypatch.setattr(ClipsInFlight, "auto_depth", staticmethod(lambda model, frames: depth))
    out = lv.model.infer_video_depth(lv.frames, device="cuda:0", stitch="device")
    assert out.shape == (120, fh, fw) and out.dtype == np.float32
    assert lv.model._video_flight.depth == depth
    assert np.array_equal(out[:LEN - INTERP], lv.host[:LEN - INTERP])  # pure upsample: bit-equal to edv_bilinear's
    _gate_a(out, lv.ref, f"runner depth {depth} {fh}x{fw}")
    again = lv.model.infer_video_depth(lv.frames, device="cuda:0", stitch="device")  # the cached lanes, mid round-robin
    assert np.array_equal(again, out)


@pytest.mark.parametrize("n", [1, 22, 23])
def test_short_videos_device_stitch(cuda, long_videos, n):
    lv = long_videos(NET_H, NET_W)
    frames = np.ascontiguousarray(lv.frames[:n])
    runner = video.HipWindowRunner(lv.model, frames, cuda)
    sources = video.window_sources(n)
    assert len(sources) == (1 if n <= 22 else 2)
    ref = stitch_ref64(_window_maps(lv.model, runner, sources, cuda), n)[0]
    out = lv.model.infer_video_depth(frames, device="cuda:0", stitch="device")
    assert out.shape == (n, NET_H, NET_W) and out.dtype == np.float32
    _gate_a(out, ref, f"n = {n}")


def test_dash_video_device_stitch_counts_one_call_per_window(cuda):
    n, start = 50, DashLinear.WARMUP - 1
    frames = long_video_frames(n, NET_H, NET_W)
    sources = video.window_sources(n)
    assert len(sources) == 3
    model, twin = _model(NET_H, NET_W, cuda, "dash"), _model(NET_H, NET_W, cuda, "dash")
    model._dash_calls = twin._dash_calls = start
    ref = stitch_ref64(_window_maps(twin, video.HipWindowRunner(twin, frames, cuda), sources, cuda), n)[0]
    assert twin._dash_calls == start + 3
    out = model.infer_video_depth(frames, device="cuda:0", stitch="device")
    assert model._dash_calls == start + 3 and all(m.FLAG == start + 3 for m in model._dash_layers())
    assert out.shape == (n, NET_H, NET_W)
    _gate_a(out, ref, "dash")


# ---- 6. run_stitched() orders itself after the caller's stream ---------------------------------------------------------------------------
def test_device_stitch_waits_for_weights_written_on_the_callers_stream(cuda):
    """As tests/test_video_gpu.py's stream-order test, with stitch="device": weights edited on the caller's stream behind queued work, the
    call made at once; the result must equal bit for bit that of a twin whose edit was synchronised first."""
    n = 50
    frames = long_video_frames(n, NET_H, NET_W)
    model, twin = _model(NET_H, NET_W, cuda, "dvlora"), _model(NET_H, NET_W, cuda, "dvlora")
    stream = torch.cuda.Stream(device=cuda)

    def edit(m):
        with torch.no_grad():
            m.pretrained.blocks[0].mlp.fc1.lora_B.mul_(1.5)
            m.head.scratch.output_conv2[2].bias.add_(0.01)

    def run(m):
        return m.infer_video_depth(frames, device="cuda:0", stitch="device")

    ev = lambda: torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        base = run(model)
        assert np.array_equal(run(twin), base)
        t0, t1 = ev(), ev()
        t0.record(stream)
        run(model)
        t1.record(stream)
        t1.synchronize()
        run_ms = t0.elapsed_time(t1)
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
        edit(model)        # queued behind the delay
        got = run(model)   # at once
        torch.cuda.synchronize()
        delay_ms = d0.elapsed_time(d1)
        print(f"\n[stream order, device stitch] one infer_video_depth {run_ms:.2f} ms; delay ahead of the edit {delay_ms:.2f} ms ({count} products)")
        assert delay_ms >= 2.0 * run_ms
        edit(twin)
        torch.cuda.synchronize()
        want = run(twin)
    assert not np.array_equal(want, base)
    assert np.array_equal(got, want)
