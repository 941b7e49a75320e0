"""Rendering on MI355X: the range kernels against numpy and the colouring against tests/render_ref.py, bit for bit (fp32 minimum, maximum and
order statistics are exact, and the colouring is the reference's float32 arithmetic in the reference's order, so nothing needs a
tolerance); then the coloured video and the coloured stream against ``render.colorize`` of the plain fp32 result."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, colormaps, render, synth, video
from endodav_amd.render import Render
from tests.golden.make_golden import long_video_frames
from tests.render_ref import colorize_ref, index_ref, ranges_ref

pytestmark = pytest.mark.gpu

# (3, 5, 7): frames of 35 elements, the scalar range path and the byte-per-store colouring; (2, 6, 8): the 16-byte loads and the dword
# stores; (4, 70, 98): E % 4 == 0 but w % 4 != 0 (vector ranges, byte colouring); (2, 130, 172): more than one block per frame
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 6, 8), (4, 70, 98), (2, 130, 172)]
KINDS = ["positive", "mixed", "negzero", "ties", "constant"]
NORMS = ["video", "frame", "fixed", "quantile"]
GUARD = 0xA5
# the range kernels: every shape under every kind, then 65 frames, one more than a chunk of 64: the second chunk's minima, maxima and select
# states live where the first chunk's did, and the select states must have been left cleared
RANGE_CASES = [pytest.param(s, k, id=f"{s}-{k}") for s in SHAPES for k in KINDS] + [pytest.param((65, 5, 7), k, id=f"(65, 5, 7)-{k}") for k in ("mixed", "ties")]


def _clip(shape, kind, seed=0):
    """No frame holds both -0.0 and +0.0: numpy leaves the choice between them open, the kernels order them."""
    rng = np.random.default_rng(seed + 17 * shape[2])
    n, h, w = shape
    if kind == "ties":
        x = np.array([-1.5, -0.0, 0.25, 1.0, 3.0], np.float32)[rng.integers(0, 5, size=shape)]
    else:
        x = rng.random(shape, dtype=np.float32)
        x = x * np.float32(3.0) + np.float32(0.05) if kind in ("positive", "constant") else x * np.float32(4.0) - np.float32(2.0)
    if kind == "negzero":
        x[0] = -np.abs(x[0])                      # frame 0 has no positive value: its maximum is -0.0
        x.reshape(-1)[::5] = np.float32(-0.0)
    if kind == "constant":
        x[n - 1] = np.float32(1.5)
    assert not (x == 0).any() or np.signbit(x[x == 0]).all()
    return np.ascontiguousarray(x, dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _st(cuda):
    return C.c_void_p(_lib.stream_ptr(cuda))


def _range(lib, cuda, x, mode, ranks=(0, 0)):
    n, h, w = x.shape
    xd = torch.from_numpy(x).to(cuda)
    out = torch.full((n, 2), float("nan"), dtype=torch.float32, device=cuda)
    ws = torch.empty(int(lib.edv_render_workspace(n)), dtype=torch.uint8, device=cuda)
    _lib.check(lib.edv_render_range(xd.data_ptr(), n, h, w, mode, ranks[0], ranks[1], out.data_ptr(), ws.data_ptr(), ws.numel(), _st(cuda)), "edv_render_range")
    return out.cpu().numpy()


# ---- 1. the range kernels against numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", RANGE_CASES)
def test_minimum_and_maximum_per_frame_and_per_video(lib, cuda, shape, kind):
    x = _clip(shape, kind)
    flat = x.reshape(shape[0], -1)
    got = _range(lib, cuda, x, 0)
    assert np.array_equal(_bits(got), _bits(np.stack([flat.min(axis=1), flat.max(axis=1)], axis=1)))
    got = _range(lib, cuda, x, 1)
    assert np.array_equal(_bits(got), _bits(np.tile(np.array([x.min(), x.max()], np.float32), (shape[0], 1))))


@pytest.mark.parametrize("shape,kind", RANGE_CASES)
def test_order_statistics_per_frame(lib, cuda, shape, kind):
    x = _clip(shape, kind)
    m = shape[1] * shape[2]
    s = np.sort(x.reshape(shape[0], -1), axis=1)
    # a pair inside one run of equal values of frame 0 (under "ties" a fifth of the frame; elsewhere it degenerates to one rank)
    mid = s[0, m // 2]
    run = np.flatnonzero(_bits(s[0]) == _bits(mid))
    inside = (int(run[0] + (run[-1] - run[0]) // 3), int(run[-1] - (run[-1] - run[0]) // 3))
    if kind == "ties" and m >= 35:
        assert inside[0] < inside[1] and s[0, inside[0]] == s[0, inside[1]]
    for ranks in [(0, m - 1), (0, int(np.floor(0.95 * (m - 1)))), (m // 3, m // 3), inside]:
        got = _range(lib, cuda, x, 2, ranks)
        assert np.array_equal(_bits(got), _bits(np.stack([s[:, ranks[0]], s[:, ranks[1]]], axis=1))), ranks


# ---- 2. the colouring against render_ref ---------------------------------------------------------------------------------------------------------
def _render(norm, **kw):
    if norm == "fixed":
        kw.setdefault("lo", 0.5)
        kw.setdefault("hi", 2.0)
    return Render(norm, **kw)


def _want(x, r, frames=None):
    return colorize_ref(x, r.norm, r.table(), r.lo, r.hi, r.q, frames)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_colorize_equals_the_reference_arithmetic(cuda, shape, norm):
    r = _render(norm)
    for kind in ("positive", "constant"):
        x = _clip(shape, kind, seed=3)
        got = render.colorize(x, r)                                           # from the host
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == shape + (3,)
        assert np.array_equal(got, _want(x, r)), kind
    dev = render.colorize(torch.from_numpy(x).to(cuda), r, output="device")   # from and to the device
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.uint8
    assert np.array_equal(dev.cpu().numpy(), got)


def test_ramp_reaches_every_index_and_the_maximum_reaches_255(cuda):
    x = ((np.arange(1024, dtype=np.float32) + np.float32(0.5)) / np.float32(64.0)).reshape(1, 32, 32)
    idx = index_ref(x[0], x.min(), x.max(), 0, False)
    assert np.array_equal(np.unique(idx), np.arange(256)) and idx.reshape(-1)[-1] == 255 and np.count_nonzero(idx == 255) == 1
    own = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], axis=1).astype(np.uint8)  # a caller's table: every row differs
    for r in (Render("frame", cmap=own), Render("quantile", q=(0.0, 1.0), cmap=own), Render("fixed", lo=float(x.min()), hi=float(x.max()), cmap=own)):
        got = render.colorize(x, r)
        assert np.array_equal(got[0, :, :, 0], idx), r.norm
        assert np.array_equal(got, _want(x, r)), r.norm
    got = render.colorize(x, Render("video", cmap=own))                       # (hi - lo) / (hi - lo + 1e-6) < 1: the maximum stays below 255
    assert np.array_equal(got, _want(x, Render("video", cmap=own))) and got[0, -1, -1, 0] == 254


@pytest.mark.parametrize("norm", ["video", "frame", "quantile"])
def test_constant_frames_take_the_first_colour(cuda, norm):
    x = np.full((2, 6, 8), 1.5, np.float32)
    got = render.colorize(x, Render(norm, cmap="viridis"))
    assert np.array_equal(got, np.broadcast_to(colormaps.TABLES["viridis"][0], (2, 6, 8, 3)))
    assert np.array_equal(got, _want(x, Render(norm, cmap="viridis")))


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 6, 8)], ids=str)
def test_fixed_clips_both_ways_and_bgr_reverses_the_channels(cuda, shape):
    x = _clip(shape, "mixed", seed=5)                                         # -2 .. 2 against the range 0.5 .. 1.0
    r = Render("fixed", lo=0.5, hi=1.0, cmap="magma")
    assert (x < 0.5).any() and (x > 1.0).any()
    got = render.colorize(x, r)
    assert np.array_equal(got, _want(x, r))
    assert np.array_equal(got[x < 0.5], np.broadcast_to(colormaps.TABLES["magma"][0], got[x < 0.5].shape))
    assert np.array_equal(got[x > 1.0], np.broadcast_to(colormaps.TABLES["magma"][255], got[x > 1.0].shape))
    bgr = render.colorize(x, Render("fixed", lo=0.5, hi=1.0, cmap="magma", order="bgr"))
    assert np.array_equal(bgr, got[..., ::-1]) and not np.array_equal(bgr, got)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 6, 8)], ids=str)
def test_side_by_side_puts_the_frame_left_of_its_colours(cuda, shape, norm):
    x = _clip(shape, "positive", seed=7)
    frames = np.random.default_rng(8).integers(0, 256, size=shape + (3,), dtype=np.uint8)
    r = _render(norm)
    got = render.colorize(x, r, frames=frames)
    assert got.shape == (shape[0], shape[1], 2 * shape[2], 3)
    assert np.array_equal(got, _want(x, r, frames))
    assert np.array_equal(got[:, :, :shape[2]], frames)
    dev = render.colorize(torch.from_numpy(x).to(cuda), r, frames=torch.from_numpy(frames).to(cuda), output="device")
    assert np.array_equal(dev.cpu().numpy(), got)


def _colorize_raw(lib, cuda, xd, shape, rng, table, beside, out_view):
    n, h, w = shape
    return lib.edv_render_colorize(xd.data_ptr(), n, h, w, rng.data_ptr(), 2, 0.0, 0, table.data_ptr(), _lib.ptr(beside), out_view.data_ptr(), _st(cuda))


@pytest.mark.parametrize("beside", [False, True], ids=["plain", "beside"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_nothing_is_written_outside_the_output(lib, cuda, shape, beside):
    """One guard row of 0xA5 before and one after the output: the dword stores must end with the last frame.  The output starts one row
    into the allocation, so it is 4-byte aligned exactly when the row is (the dword path at (2, 6, 8) and (2, 130, 172))."""
    n, h, w = shape
    x = _clip(shape, "positive", seed=9)
    frames = np.random.default_rng(10).integers(0, 256, size=shape + (3,), dtype=np.uint8) if beside else None
    row = w * 3 * (2 if beside else 1)
    buf = torch.full(((n * h + 2) * row,), GUARD, dtype=torch.uint8, device=cuda)
    xd = torch.from_numpy(x).to(cuda)
    rng = torch.from_numpy(ranges_ref(x, "frame")).to(cuda)
    table = torch.from_numpy(colormaps.TABLES["inferno"].copy()).to(cuda)
    side = torch.from_numpy(frames).to(cuda) if beside else None
    _lib.check(_colorize_raw(lib, cuda, xd, shape, rng, table, side, buf[row:]), "edv_render_colorize")
    got = buf.cpu().numpy()
    assert (got[:row] == GUARD).all() and (got[-row:] == GUARD).all()
    assert np.array_equal(got[row:-row].reshape(n, h, -1, 3), colorize_ref(x, "frame", colormaps.TABLES["inferno"], frames=frames))


@pytest.mark.parametrize("shape", [(2, 6, 8), (4, 70, 98)], ids=str)
def test_unaligned_bases_take_the_byte_path(lib, cuda, shape):
    """Depth sliced 4 bytes into its allocation (no 16-byte loads), and an output 1 byte into its own (no dword stores)."""
    n, h, w = shape
    x = _clip(shape, "mixed", seed=11)
    base = torch.zeros(x.size + 1, dtype=torch.float32, device=cuda)
    base[1:] = torch.from_numpy(x.reshape(-1)).to(cuda)
    xd = base[1:].view(n, h, w)
    assert xd.data_ptr() % 16 == 4
    for norm in NORMS:
        r = _render(norm)
        assert np.array_equal(render.colorize(xd, r), _want(x, r)), norm
    buf = torch.full((x.size * 3 + 2,), GUARD, dtype=torch.uint8, device=cuda)
    rng = torch.from_numpy(ranges_ref(x, "frame")).to(cuda)
    table = torch.from_numpy(colormaps.TABLES["inferno"].copy()).to(cuda)
    _lib.check(_colorize_raw(lib, cuda, torch.from_numpy(x).to(cuda), shape, rng, table, None, buf[1:]), "edv_render_colorize")
    got = buf.cpu().numpy()
    assert got[0] == GUARD and got[-1] == GUARD
    assert np.array_equal(got[1:-1].reshape(n, h, w, 3), colorize_ref(x, "frame", colormaps.TABLES["inferno"]))


# ---- 3. bad arguments ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(lib, cuda):
    n, h, w = 2, 6, 8
    x = torch.ones((n, h, w), dtype=torch.float32, device=cuda)
    rng = torch.full((n, 2), 7.0, dtype=torch.float32, device=cuda)
    ws = torch.zeros(int(lib.edv_render_workspace(n)), dtype=torch.uint8, device=cuda)
    table = torch.zeros((256, 3), dtype=torch.uint8, device=cuda)
    out = torch.full((n, h, w, 3), GUARD, dtype=torch.uint8, device=cuda)
    st = _st(cuda)
    X, R, W, T, O, B = x.data_ptr(), rng.data_ptr(), ws.data_ptr(), table.data_ptr(), out.data_ptr(), ws.numel()
    assert lib.edv_render_workspace(1) > 0 and lib.edv_render_workspace(10 ** 6) == lib.edv_render_workspace(64) >= lib.edv_render_workspace(32)
    bad_range = [
        (None, n, h, w, 0, 0, 0, R, W, B, st), (X, n, h, w, 0, 0, 0, None, W, B, st), (X, n, h, w, 0, 0, 0, R, None, B, st),   # null pointers
        (X, 0, h, w, 0, 0, 0, R, W, B, st), (X, -1, h, w, 1, 0, 0, R, W, B, st),                                               # n < 1
        (X, n, 0, w, 0, 0, 0, R, W, B, st), (X, n, h, -3, 2, 0, 0, R, W, B, st),                                               # sizes
        (X, n, h, w, 3, 0, 0, R, W, B, st), (X, n, h, w, -1, 0, 0, R, W, B, st),                                               # mode
        (X, n, h, w, 2, 5, 4, R, W, B, st), (X, n, h, w, 2, 0, h * w, R, W, B, st), (X, n, h, w, 2, -1, 3, R, W, B, st),       # ranks
        (X, n, h, w, 2, 0, 3, R, W, B // 2 - 1, st), (X, n, h, w, 0, 0, 0, R, W + 4, B, st),                                    # workspace
    ]
    for args in bad_range:
        assert lib.edv_render_range(*args) != 0, args
        assert lib.edv_last_error()
    bad_color = [
        (None, n, h, w, R, 2, 0.0, 0, T, None, O, st), (X, n, h, w, None, 2, 0.0, 0, T, None, O, st), (X, n, h, w, R, 2, 0.0, 0, None, None, O, st),
        (X, n, h, w, R, 2, 0.0, 0, T, None, None, st),
        (X, 0, h, w, R, 2, 0.0, 0, T, None, O, st), (X, n, 0, w, R, 2, 0.0, 0, T, None, O, st), (X, n, h, 0, R, 2, 0.0, 0, T, None, O, st),
        (X, n, h, w, R, 1, 0.0, 0, T, None, O, st), (X, n, h, w, R, -2, 0.0, 0, T, None, O, st),
    ]
    for args in bad_color:
        assert lib.edv_render_colorize(*args) != 0, args
        assert lib.edv_last_error()
    torch.cuda.synchronize()
    assert (out == GUARD).all() and (rng == 7.0).all() and (ws == 0).all()


# ---- 4. the coloured video and the coloured stream -------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56
STEP = video.INFER_LEN - video.OVERLAP


class _Video:
    """One model, 150 frames, the plain fp32 result and (per norm, on first use) the coloured one; computed once per frame size, then only read."""

    def __init__(self, cuda, fh, fw):
        m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
        synth.fill_module_(m)
        self.model = m.to(cuda)
        self.frames = long_video_frames(150, fh, fw)
        self.frames.setflags(write=False)
        self.depth = np.array(self.model.infer_video_depth(self.frames, device="cuda:0", stitch="device"))
        self.depth.setflags(write=False)
        lo, hi = (float(v) for v in np.quantile(self.depth, [0.2, 0.8]))   # a fifth of the pixels clip at either end
        assert lo < hi
        self.renders = {"video": Render("video"), "frame": Render("frame", cmap="viridis"), "fixed": Render("fixed", lo=lo, hi=hi, order="bgr"),
                        "quantile": Render("quantile", cmap="magma")}
        self._coloured = {}

    def coloured(self, norm):
        if norm not in self._coloured:
            got = np.array(self.model.infer_video_depth(self.frames, device="cuda:0", stitch="device", render=self.renders[norm]))
            got.setflags(write=False)
            self._coloured[norm] = got
        return self._coloured[norm]


@pytest.fixture(scope="module")
def videos(cuda):
    cache = {}

    def get(fh, fw):
        if (fh, fw) not in cache:
            cache[(fh, fw)] = _Video(cuda, fh, fw)
        return cache[(fh, fw)]

    return get


def _sizes(n):
    sizes = [1] * 40 + [7, 22, 50]
    return sizes + [n - sum(sizes)]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("fh,fw", [(NET_H, NET_W), (60, 80)], ids=["native", "resized"])
def test_coloured_video_equals_colorize_of_the_plain_video(cuda, videos, fh, fw, norm):
    v = videos(fh, fw)
    got = v.coloured(norm)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (150, fh, fw, 3)
    r = v.renders[norm]
    assert np.array_equal(got, render.colorize(v.depth, r))
    assert np.array_equal(got[:32], _want(v.depth, r)[:32] if norm == "video" else _want(v.depth[:32], r))   # and the yardstick, on one chunk


@pytest.mark.parametrize("norm", ["video", "quantile"])
def test_coloured_video_on_the_device_has_the_same_bytes(cuda, videos, norm):
    v = videos(NET_H, NET_W)
    frames = np.ascontiguousarray(v.frames[:54])
    r = v.renders[norm]
    host = v.model.infer_video_depth(frames, device="cuda:0", stitch="device", render=r)
    dev = v.model.infer_video_depth(frames, device="cuda:0", stitch="device", output="device", render=r)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.uint8 and dev.shape == (54, NET_H, NET_W, 3)
    assert np.array_equal(dev.cpu().numpy(), host)
    assert np.array_equal(host, render.colorize(v.model.infer_video_depth(frames, device="cuda:0", stitch="device"), r))


@pytest.mark.parametrize("norm", ["frame", "fixed", "quantile"])
def test_coloured_stream_equals_the_coloured_video_for_any_chunking(cuda, videos, norm):
    v = videos(60, 80)
    stream = v.model.stream_video_depth(frame_shape=(60, 80), device="cuda:0", render=v.renders[norm])
    got, pos = [], 0
    for m in _sizes(150):
        out = stream.push(v.frames[pos:pos + m] if m > 1 else v.frames[pos])
        pos += m
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape[1:] == (60, 80, 3)
        got.append(out)
        assert stream.pushed == pos and stream.emitted == sum(g.shape[0] for g in got)
    assert stream.windows == 6 and stream.emitted == 134
    got.append(stream.close())
    assert stream.pushed == stream.emitted == 150 and stream.windows == 7
    assert np.array_equal(np.concatenate(got), v.coloured(norm))
    last = stream.close()
    assert last.shape == (0, 60, 80, 3) and last.dtype == np.uint8


@pytest.mark.parametrize("norm", ["frame", "fixed", "quantile"])
def test_coloured_stream_without_waiting_returns_the_same_frames_without_gaps(cuda, videos, norm):
    v = videos(NET_H, NET_W)
    stream = v.model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0", render=v.renders[norm])
    got, pos = [], 0
    for m in _sizes(150):
        got.append(stream.push(v.frames[pos:pos + m], wait=False))
        pos += m
        assert stream.emitted == sum(g.shape[0] for g in got)
    got.append(stream.close())
    out = np.concatenate(got)
    assert out.shape[0] == 150 == stream.emitted and np.array_equal(out, v.coloured(norm))


@pytest.mark.parametrize("output", ["host", "device"])
@pytest.mark.parametrize("norm", ["frame", "fixed", "quantile"])
def test_device_memory_does_not_grow_with_the_coloured_stream(cuda, videos, norm, output):
    """A condition, not a measurement: once every lane has run (windows 0..2), what is allocated after a push is the stream's own buffers
    (with them the table, the range workspace and, for host results, the staging buffer)."""
    v = videos(NET_H, NET_W)
    stream = v.model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0", output=output, render=v.renders[norm])
    want = v.coloured(norm)

    def allocated_after(upto, frm):
        out = stream.push(v.frames[frm:upto])
        assert out.dtype == (torch.uint8 if output == "device" else np.uint8) and out.shape[0] > 0
        assert np.array_equal(out.cpu().numpy() if output == "device" else out, want[stream.emitted - out.shape[0]:stream.emitted])
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


def test_default_paths_keep_their_bits(cuda, videos):
    v = videos(NET_H, NET_W)
    again = v.model.infer_video_depth(v.frames, device="cuda:0", stitch="device", render=None)
    assert isinstance(again, np.ndarray) and again.dtype == np.float32 and np.array_equal(again, v.depth)
    stream = v.model.stream_video_depth(frame_shape=(NET_H, NET_W), device="cuda:0", render=None)
    got = [stream.push(v.frames[:100]), stream.push(v.frames[100:]), stream.close()]
    assert all(g.dtype == np.float32 and g.shape[1:] == (NET_H, NET_W) for g in got)
    assert np.array_equal(np.concatenate(got), v.depth)
    assert stream.close().shape == (0, NET_H, NET_W)
