"""CPU: the schedule, the ring bound and the argument checks of video.DepthStream, with a stub in place of the GPU backend."""
import numpy as np
import pytest

import endodav_amd
from endodav_amd import video

FH, FW = 4, 6
STEP = video.INFER_LEN - video.OVERLAP


class StubBackend:
    """Records what DepthStream asks for.  A "frame" of the result carries its own index, so order and gaps show.  ``late``: a window's
    block completes only ``late`` collects after it was enqueued (what wait=False sees of a busy GPU)."""

    def __init__(self, late=0):
        self.calls = []          # ("upload", first, m) / ("window", k, source, upto), in call order
        self.newest = -1
        self.done = 0
        self.blocks = []         # [first, upto, collects still to pass]
        self.late = late
        self.pushes = 0
        self.released = False

    def begin_push(self):
        self.pushes += 1

    def upload(self, first, frames):
        assert first == self.newest + 1 and frames.dtype == np.uint8 and frames.shape[1:] == (FH, FW, 3) and frames.shape[0] >= 1
        self.newest = first + frames.shape[0] - 1
        self.calls.append(("upload", first, frames.shape[0]))

    def window(self, k, source, upto):
        assert upto >= self.done                          # n = 23: window 1 runs (the offline path runs it too) and finalises nothing new
        self.calls.append(("window", k, np.array(source), upto, self.newest, self.pushes))
        self.blocks.append([self.done, upto, self.late])
        self.done = upto

    def collect(self, wait):
        got = []
        while self.blocks and (wait or self.blocks[0][2] <= 0):
            a, b, _ = self.blocks.pop(0)
            got.extend(range(a, b))
        for blk in self.blocks:
            blk[2] -= 1
        return np.broadcast_to(np.asarray(got, dtype=np.float32).reshape(-1, 1, 1), (len(got), FH, FW)).copy()

    def release(self):
        self.released = True


def _frames(n):
    return np.zeros((n, FH, FW, 3), dtype=np.uint8)


def _chunks(n, size):
    return [min(size, n - a) for a in range(0, n, size)]


def _windows(stub):
    return [c for c in stub.calls if c[0] == "window"]


@pytest.mark.parametrize("chunking", ["ones", "sevens", "whole"])
def test_schedule_runs_every_window_once_in_order_as_soon_as_it_is_due(chunking):
    for n in range(1, 201):
        stub = StubBackend()
        stream = video.DepthStream(None, (FH, FW), backend=stub)
        sizes = _chunks(n, {"ones": 1, "sevens": 7, "whole": n}[chunking])
        returned = []
        for i, m in enumerate(sizes):
            got = stream.push(_frames(m))
            returned.append(got)
            assert stream.pushed == sum(sizes[:i + 1])
            ran = len(_windows(stub))
            # before close: every window whose trigger has passed has run, and no other
            assert ran == sum(1 for k in range(len(video.window_sources(n))) if STEP * k + 32 <= stream.pushed), (n, stream.pushed)
            assert stream.emitted == (24 + STEP * (ran - 1) if ran else 0)
        before = len(_windows(stub))
        returned.append(stream.close())
        want = video.window_sources(n)
        wins = _windows(stub)
        assert [w[1] for w in wins] == list(range(len(want)))
        for w, src in zip(wins, want):
            assert np.array_equal(w[2], src), (n, w[1])
        for w in wins[:before]:                           # enqueued at the FIRST push with pushed >= 22 k + 32
            k, push_no = w[1], w[5]
            assert sum(sizes[:push_no]) >= STEP * k + 32 and sum(sizes[:push_no - 1]) < STEP * k + 32
        assert before < len(wins)                         # close always has a window left to run
        for w in wins[before:]:
            assert STEP * w[1] + 32 > n
        assert stream.emitted == n == stream.pushed and stub.released
        out = np.concatenate(returned)
        assert np.array_equal(out[:, 0, 0], np.arange(n, dtype=np.float32))  # every frame once, in order


def test_ring_holds_what_every_window_reads():
    """The bound on the ring derived from window_sources: at a window's trigger the ring holds frames newest - R + 1 .. newest, and the window
    reads back to min(source).  Then, with the stub, that no push before the trigger has gone past it."""
    R = video.STREAM_RING
    span = 0
    for n in range(1, 401):
        for k, src in enumerate(video.window_sources(n)):
            newest = min(STEP * k + 31, n - 1)            # at the trigger, or at close
            assert src.max() <= newest
            span = max(span, newest - int(src.min()) + 1)
    assert span == 48 and span <= R                       # slot 0 of window k is frame 22 k - 16: two hops of the key-frame chain
    for size in (1, 7, 200):
        stub = StubBackend()
        stream = video.DepthStream(None, (FH, FW), backend=stub)
        for m in _chunks(200, size):
            stream.push(_frames(m))
        stream.close()
        for w in _windows(stub):
            k, src, newest = w[1], w[2], w[4]
            assert newest <= STEP * k + 31                # no frame newer than the trigger is in the ring when the window is enqueued
            assert newest - int(src.min()) < R            # so frame min(source) has not been overwritten: j overwrites j - R
            assert len({int(j) % R for j in np.unique(src)}) == len(np.unique(src))


def test_eager_sources_do_not_depend_on_the_length():
    prev = None
    for k in range(12):
        prev = video.stream_next_source(k, prev)
        for n in (video.stream_trigger(k), video.stream_trigger(k) + 1, 400):
            assert np.array_equal(video.window_sources(n)[k], prev)


def test_argument_errors():
    mk = lambda: video.DepthStream(None, (FH, FW), backend=StubBackend())
    s = mk()
    with pytest.raises(ValueError):
        s.push(np.zeros((2, FH, FW, 3), dtype=np.float32))       # dtype
    with pytest.raises(ValueError):
        s.push(np.zeros((FH, FW), dtype=np.uint8))                # rank
    with pytest.raises(ValueError):
        s.push(np.zeros((1, 2, FH, FW, 3), dtype=np.uint8))       # rank
    with pytest.raises(ValueError):
        s.push(np.zeros((2, FH + 1, FW, 3), dtype=np.uint8))      # frame size
    with pytest.raises(ValueError):
        s.push(np.zeros((0, FH, FW, 3), dtype=np.uint8))          # no frame
    assert s.pushed == 0
    got = s.push(np.zeros((FH, FW, 3), dtype=np.uint8))          # one frame without the leading axis
    assert got.shape == (0, FH, FW) and s.pushed == 1
    assert s.close().shape == (1, FH, FW)
    again = s.close()
    assert again.shape == (0, FH, FW) and again.dtype == np.float32
    with pytest.raises(RuntimeError):
        s.push(_frames(1))
    s = mk()
    empty = s.close()                                             # nothing pushed
    assert empty.shape == (0, FH, FW) and s.pushed == s.emitted == 0
    with pytest.raises(ValueError):
        video.DepthStream(None, (FH, FW), output="pinned", backend=StubBackend())
    model = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(42, 56), disable_conv_head=True)
    with pytest.raises(RuntimeError):
        model.stream_video_depth(frame_shape=(42, 56), device="cpu")


def test_wait_false_returns_contiguous_prefixes_only():
    stub = StubBackend(late=2)
    stream = video.DepthStream(None, (FH, FW), backend=stub)
    nxt, sizes = 0, []
    for m in _chunks(150, 11):
        got = stream.push(_frames(m), wait=False)
        if got.shape[0]:
            assert got[0, 0, 0] == nxt and np.array_equal(np.diff(got[:, 0, 0]), np.ones(got.shape[0] - 1))
            nxt += got.shape[0]
        sizes.append(got.shape[0])
        assert stream.emitted == nxt <= max(stream.pushed - 8, 0)
    assert 0 in sizes[3:] and nxt < 24 + STEP * (len(_windows(stub)) - 1)  # the stub did complete late
    rest = stream.close()
    assert rest[0, 0, 0] == nxt and nxt + rest.shape[0] == 150 == stream.emitted
