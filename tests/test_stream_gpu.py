"""model.stream_video_depth on MI355X: whatever the chunking, the frames push() and close() return, concatenated, equal
model.infer_video_depth(frames, stitch="device") bit for bit -- the same kernels in the same order, so no tolerance."""
import gc

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import synth, video
from endodav_amd.endodav import DashLinear
from tests.golden.make_golden import long_video_frames

pytestmark = pytest.mark.gpu

NET_H, NET_W = 42, 56
STEP = video.INFER_LEN - video.OVERLAP


def _model(cuda, lora_type="none"):
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type=lora_type,
                            disable_conv_head=True).eval()
    synth.fill_module_(m)
    return m.to(cuda)


class _Video:
    """One model, 150 frames and the offline result, computed once per frame size and only read afterwards."""

    def __init__(self, cuda, fh, fw):
        self.model = _model(cuda)
        self.frames = long_video_frames(150, fh, fw)
        self.frames.setflags(write=False)
        self.want = np.array(self.model.infer_video_depth(self.frames, device="cuda:0", stitch="device"))
        self.want.setflags(write=False)
        assert self.want.shape == (150, fh, fw)


@pytest.fixture(scope="module")
def videos(cuda):
    cache = {}

    def get(fh, fw):
        if (fh, fw) not in cache:
            cache[(fh, fw)] = _Video(cuda, fh, fw)
        return cache[(fh, fw)]

    return get


def _final(pushed):
    """Frames final after `pushed` frames and before close (the schedule of video.DepthStream)."""
    ran = sum(1 for k in range(pushed // STEP + 1) if video.stream_trigger(k) <= pushed)
    return video.stream_final(ran - 1) if ran else 0


def _sizes(n):
    sizes = [1] * 40 + [7, 22, 50]
    return sizes + [n - sum(sizes)]


@pytest.mark.parametrize("fh,fw", [(NET_H, NET_W), (60, 80)], ids=["native", "resized"])
def test_any_chunking_equals_the_offline_device_stitch(cuda, videos, fh, fw):
    v = videos(fh, fw)
    stream = v.model.stream_video_depth(frame_shape=(fh, fw), device="cuda:0")
    assert isinstance(stream, video.DepthStream)
    got, pos = [], 0
    for m in _sizes(150):
        out = stream.push(v.frames[pos:pos + m] if m > 1 else v.frames[pos])  # single frames without the leading axis
        pos += m
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape[1:] == (fh, fw)
        got.append(out)
        assert stream.pushed == pos and stream.emitted == sum(g.shape[0] for g in got) == _final(pos)
    assert stream.windows == 6 and stream.emitted == 134
    got.append(stream.close())
    assert got[-1].shape[0] == 16 and stream.pushed == stream.emitted == 150 and stream.windows == 7
    assert np.array_equal(np.concatenate(got), v.want)
    assert stream.close().shape == (0, fh, fw)


@pytest.mark.parametrize("n", [1, 22, 23, 32, 33, 44, 54])
def test_short_streams_pushed_whole(cuda, videos, n):
    """One padded window; the first length with two windows; window 0 eager and window 1 at close (32, 33, 44); window 1 eager and window
    2 at close (54)."""
    v = videos(NET_H, NET_W)
    frames = np.ascontiguousarray(v.frames[:n])
    want = v.model.infer_video_depth(frames, device="cuda:0", stitch="device")
    stream = v.model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0")
    first = stream.push(frames)
    assert first.shape[0] == _final(n) and stream.windows == sum(1 for k in range(3) if video.stream_trigger(k) <= n)
    rest = stream.close()
    assert stream.windows == len(video.window_sources(n))
    out = np.concatenate([first, rest])
    assert out.shape == (n, NET_H, NET_W) and np.array_equal(out, want)


def test_wait_false_returns_the_same_frames_without_gaps(cuda, videos):
    v = videos(60, 80)
    stream = v.model.stream_video_depth(frame_shape=(60, 80), device="cuda:0")
    got, pos = [], 0
    for m in _sizes(150):
        out = stream.push(v.frames[pos:pos + m], wait=False)
        pos += m
        got.append(out)
        assert stream.emitted == sum(g.shape[0] for g in got) <= _final(pos)
    got.append(stream.close())
    out = np.concatenate(got)  # every block continues where the previous one ended: any gap or repeat breaks the equality below
    assert out.shape[0] == 150 == stream.emitted
    assert np.array_equal(out, v.want)


def test_two_streams_of_one_model_pushed_alternately(cuda, videos):
    v = videos(NET_H, NET_W)
    a = np.ascontiguousarray(v.frames[:54])
    b = np.ascontiguousarray(v.frames[149:95:-1])
    want_a = v.model.infer_video_depth(a, device="cuda:0", stitch="device")
    want_b = v.model.infer_video_depth(b, device="cuda:0", stitch="device")
    assert not np.array_equal(want_a, want_b)
    sa = v.model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0")
    sb = v.model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0")
    got_a, got_b = [], []
    for pos in range(0, 54, 9):
        got_a.append(sa.push(a[pos:pos + 9]))
        got_b.append(sb.push(b[pos:pos + 9], wait=False))
    got_a.append(sa.close())
    got_b.append(sb.close())
    assert np.array_equal(np.concatenate(got_a), want_a)
    assert np.array_equal(np.concatenate(got_b), want_b)


def test_dash_stream_counts_one_call_per_window(cuda):
    """As infer_video_depth: one forward per window in window order on the model's one engine context; 50 frames are 3 windows, which from
    call count 99 straddle DashLinear's activation."""
    n, start = 50, DashLinear.WARMUP - 1
    frames = long_video_frames(n, NET_H, NET_W)
    model, twin = _model(cuda, "dash"), _model(cuda, "dash")
    model._dash_calls = twin._dash_calls = start
    want = twin.infer_video_depth(frames, device="cuda:0", stitch="device")
    assert twin._dash_calls == start + 3
    stream = model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0")
    got = [stream.push(frames[:33]), stream.push(frames[33:])]
    assert model._dash_calls == start + 1 and got[0].shape[0] == 24 and got[1].shape[0] == 0
    got.append(stream.close())
    assert model._dash_calls == start + 3 and all(m.FLAG == start + 3 for m in model._dash_layers())
    assert np.array_equal(np.concatenate(got), want)


def test_device_output_has_the_same_bits(cuda, videos):
    v = videos(60, 80)
    frames = v.frames[:54]
    stream = v.model.stream_video_depth(frame_shape=(60, 80), device="cuda:0", output="device")
    got = [stream.push(frames[:20]), stream.push(frames[20:]), stream.close()]
    assert [g.shape[0] for g in got] == [0, 46, 8]
    for g in got:
        assert isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float32 and g.shape[1:] == (60, 80)
    host = v.model.stream_video_depth(frame_shape=(60, 80), device="cuda:0")
    want = np.concatenate([host.push(frames), host.close()])
    assert np.array_equal(torch.cat(got).cpu().numpy(), want)
    # window 0 and 1 of the 150-frame video are the same windows: its first 46 frames are final after them
    assert np.array_equal(want[:46], v.want[:46])


def test_device_memory_does_not_grow_with_the_stream(cuda, videos):
    """A condition, not a measurement: once every lane has run (windows 0..2), what is allocated after a push is the stream's own buffers."""
    v = videos(NET_H, NET_W)
    stream = v.model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0")

    def allocated_after(upto, frm):
        out = stream.push(v.frames[frm:upto])
        assert out.shape[0] > 0
        del out
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated(cuda)

    at3 = allocated_after(video.stream_trigger(3), 0)
    assert stream.windows == 4
    at5 = allocated_after(video.stream_trigger(5), video.stream_trigger(3))
    assert stream.windows == 6
    assert at3 == at5
    stream.close()
