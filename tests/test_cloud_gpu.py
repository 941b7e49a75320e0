"""Point clouds on MI355X: ``cloud.lift`` and the raw entry points against ``cloud.lift_host``, bit for bit (the kernels run the yardstick's
float32 and float64 operations in the yardstick's order, so nothing needs a tolerance); then ``model.video_point_cloud`` against
``lift_host`` of the stitched video."""
import ctypes as C

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, cloud, synth
from endodav_amd.cloud import Cloud
from tests import cloud_cases as cases
from tests.golden.make_golden import long_video_frames

pytestmark = pytest.mark.gpu

STEPS = [1, 2, 3, 8]
GUARD = 0xA5
PAD = 64  # guard bytes on either side of an output


def _shapes():
    """One pixel; less than a wave; several tiles with a ragged last one; exactly two tiles; a tile and one pixel; a pixel short of a wave and
    one more than a wave."""
    P = cloud.TILE_PIXELS
    return [(1, 1, 1), (2, 5, 7), (3, 70, 98), (2, 64, 2 * P // 64), (2, 1, P + 1), (3, 7, 9), (3, 5, 13)]


def pytest_generate_tests(metafunc):
    if "shape" in metafunc.fixturenames:
        metafunc.parametrize("shape", _shapes(), ids=str)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """Points, colours and offsets of a host or device result equal the yardstick's bits."""
    p, c = got.points, got.colors
    if isinstance(p, torch.Tensor):
        assert p.is_cuda and p.dtype == torch.float32 and (c is None or (c.is_cuda and c.dtype == torch.uint8))
        p, c = p.cpu().numpy(), None if c is None else c.cpu().numpy()
    assert isinstance(got.offsets, np.ndarray) and got.offsets.dtype == np.int64 and np.array_equal(got.offsets, want.offsets)
    assert p.shape == want.points.shape and p.dtype == np.float32 and np.array_equal(_bits(p), _bits(want.points))
    if want.colors is None:
        assert c is None
    else:
        assert c.shape == want.colors.shape and c.dtype == np.uint8 and np.array_equal(c, want.colors)


def _masks(shape, kind, seed=5):
    if kind == "none" or shape[1] * shape[2] == 1:   # the one pixel of a one-pixel frame is kept
        return None
    return np.random.default_rng(seed).random(shape[1:] if kind == "shared" else shape) < 0.7


# ---- a. bit equality --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", STEPS)
def test_lift_equals_the_host_mirror_on_every_shape(cuda, shape, step):
    """Every shape at every step, the options cycling with them: both sources, shared and per-frame cameras and masks, with colours."""
    i = _shapes().index(shape) + STEPS.index(step)
    source, per_frame, kind = cloud.SOURCES[i % 2], bool((i // 2) % 2), ("none", "shared", "per-frame")[i % 3]
    x, frames = cases.clip(shape, source, seed=i), cases.colours(shape, seed=i)
    spec = cases.spec_for(shape, source, step, per_frame, mask=_masks(shape, kind), seed=i, far=150.0 if shape == (1, 1, 1) else 3.0)
    want = cloud.lift_host(x, spec, frames)
    assert len(want) > 0
    _same(cloud.lift(x, spec, frames), want)


@pytest.mark.parametrize("kind", ["none", "shared", "per-frame"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["one-camera", "camera-per-frame"])
@pytest.mark.parametrize("source", cloud.SOURCES)
def test_lift_equals_the_host_mirror_under_every_option(cuda, source, per_frame, kind):
    shape = (3, 70, 98)
    x, frames = cases.clip(shape, source), cases.colours(shape)
    spec = cases.spec_for(shape, source, 2, per_frame, mask=_masks(shape, kind), gain=1.25)
    for rgb in (frames, None):
        want = cloud.lift_host(x, spec, rgb)
        assert 0 < len(want) < 3 * 35 * 49
        for output in ("host", "device"):
            _same(cloud.lift(x, spec, rgb, output=output), want)
        _same(cloud.lift(torch.from_numpy(x).to(cuda), spec, None if rgb is None else torch.from_numpy(rgb).to(cuda), output="device"), want)


@pytest.mark.parametrize("clip_shape", [(4100, 1, 3), (2050, 1, cloud.TILE_PIXELS + 1)], ids=str)
def test_lift_equals_the_host_mirror_beyond_one_round_of_the_scan(cuda, clip_shape):
    """The one-workgroup scan takes 4096 tile counts a round and carries their total into the next: with one tile a frame the frames from
    4096 on, with two tiles a frame (a full one and one pixel) the frames from 2048 on, take their offsets and tile bases from the carry."""
    n, h, w = clip_shape
    tiles_per_frame = -(-h * w // cloud.TILE_PIXELS)
    assert n * tiles_per_frame > 4096
    x, frames = cases.clip(clip_shape, "depth"), cases.colours(clip_shape)
    spec = cases.spec_for(clip_shape)
    want = cloud.lift_host(x, spec, frames)
    assert 0 < len(want) < x.size and want.offsets[4096 // tiles_per_frame] < want.offsets[n]
    _same(cloud.lift(x, spec, frames), want)


# ---- b. keep patterns ---------------------------------------------------------------------------------------------------------------------------
def _pattern(name, shape):
    """(depth, mask) of a "depth" clip whose kept set has the named form under near = 1e-3, far = 150."""
    n, h, w = shape
    P = cloud.TILE_PIXELS
    x = cases.clip(shape, "depth", seed=21)
    flat = np.zeros((n, h * w), bool)
    if name == "all":
        return x, None
    if name == "none":
        return x, flat.reshape(shape)
    if name == "last":
        flat[n - 1, h * w - 1] = True
    elif name == "half":
        flat[:] = np.random.default_rng(22).random(flat.shape) < 0.5
    elif name == "empty-waves-and-tiles":
        flat[:] = True
        flat[0, :P] = False                 # the first tile of frame 0
        flat[1, P:2 * P] = False            # a middle tile of frame 1
        flat[2, 64:128] = False             # whole waves
        flat[2, P + 256:P + 512] = False    # a whole iteration of the second tile
        flat[2, -(h * w % P):] = False      # the ragged last tile
    elif name == "odd-totals":
        rng = np.random.default_rng(23)
        for f, count in enumerate((3, 1001, 77)[:n]):
            flat[f, rng.choice(h * w, count, replace=False)] = True
    elif name == "nan-inf":
        x = x.copy()
        r = np.random.default_rng(24).random(shape)
        x[r < 0.1], x[(r >= 0.1) & (r < 0.2)], x[(r >= 0.2) & (r < 0.3)] = np.nan, np.inf, -np.inf
        x[(r >= 0.3) & (r < 0.35)], x[(r >= 0.35) & (r < 0.4)] = 0.0, 1e3
        return x, None
    return x, flat.reshape(shape)


@pytest.mark.parametrize("name", ["all", "none", "last", "half", "empty-waves-and-tiles", "odd-totals", "nan-inf"])
def test_keep_patterns(cuda, name):
    shape = (3, 70, 98)                      # 6860 pixels a frame: three full tiles and a ragged fourth
    assert 3 * cloud.TILE_PIXELS < 70 * 98 < 4 * cloud.TILE_PIXELS
    x, mask = _pattern(name, shape)
    frames = cases.colours(shape, seed=25)
    spec = cases.spec_for(shape, "depth", 1, True, mask=mask, far=150.0)
    want = cloud.lift_host(x, spec, frames)
    counts = np.diff(want.offsets)
    if name == "all":
        assert (counts == 70 * 98).all()
    if name == "none":
        assert len(want) == 0
    if name == "last":
        assert list(counts) == [0, 0, 1]
    if name == "odd-totals":
        assert list(counts) == [3, 1001, 77]   # frames 1 and 2 start at odd multiples of 12 and of 3 bytes
    if name == "nan-inf":
        assert 0 < len(want) < 0.7 * x.size and np.isfinite(want.points).all()
    for output in ("host", "device"):
        _same(cloud.lift(x, spec, frames, output=output), want)


# ---- c. guard bytes -------------------------------------------------------------------------------------------------------------------------------
def _raw(lib, cuda, x, spec, frames, capacity=None):
    """The two entry points on poisoned buffers: points start PAD bytes and colours PAD + 1 bytes into theirs.  Returns (offsets, points bytes,
    colour bytes) with the guards still attached."""
    n, h, w = x.shape
    st = C.c_void_p(_lib.stream_ptr(cuda))
    xd = torch.from_numpy(x).to(cuda)
    fd = None if frames is None else torch.from_numpy(frames).to(cuda)
    md = None if spec.mask is None else torch.from_numpy(spec.mask).to(cuda)
    cams = spec.cams(n)
    cd = torch.from_numpy(cams).to(cuda)
    sel = cloud.selection(xd, spec, md)
    ws = torch.empty(int(lib.edv_cloud_workspace(n, h, w, int(spec.step))), dtype=torch.uint8, device=cuda)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=cuda)
    _lib.check(lib.edv_cloud_count(C.byref(sel), off.data_ptr(), ws.data_ptr(), ws.numel(), st), "edv_cloud_count")
    offsets = off.cpu().numpy()
    room = int(offsets[n]) if capacity is None else capacity     # the buffers always hold the whole cloud, the capacity may be smaller
    total = max(int(offsets[n]), room)
    pbuf = torch.full((PAD + total * 12 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    cbuf = torch.full((PAD + 1 + total * 3 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    _lib.check(lib.edv_cloud_scatter(C.byref(sel), cd.data_ptr(), 21 if cams.shape[0] > 1 else 0, _lib.ptr(fd), off.data_ptr(), ws.data_ptr(), ws.numel(),
                                     pbuf.data_ptr() + PAD, cbuf.data_ptr() + PAD + 1 if frames is not None else None, room, st), "edv_cloud_scatter")
    torch.cuda.synchronize()
    assert np.array_equal(off.cpu().numpy(), offsets)
    return offsets, pbuf.cpu().numpy(), cbuf.cpu().numpy()


@pytest.mark.parametrize("step", [1, 3])
def test_nothing_is_written_outside_the_outputs(lib, cuda, shape, step):
    i = _shapes().index(shape)
    x, frames = cases.clip(shape, "depth", seed=30 + i), cases.colours(shape, seed=30 + i)
    spec = cases.spec_for(shape, "depth", step, True, mask=_masks(shape, "per-frame", seed=31 + i), far=150.0 if shape == (1, 1, 1) else 2.0)
    want = cloud.lift_host(x, spec, frames)
    total = len(want)
    assert total > 0
    offsets, pb, cb = _raw(lib, cuda, x, spec, frames)
    assert np.array_equal(offsets, want.offsets)
    assert (pb[:PAD] == GUARD).all() and (pb[PAD + total * 12:] == GUARD).all() and (cb[:PAD + 1] == GUARD).all() and (cb[PAD + 1 + total * 3:] == GUARD).all()
    assert np.array_equal(pb[PAD:PAD + total * 12].view(np.uint32).reshape(-1, 3), _bits(want.points))
    assert np.array_equal(cb[PAD + 1:PAD + 1 + total * 3].reshape(-1, 3), want.colors)
    # a capacity below the total: exactly the first `capacity` points, the rest of the buffers keeps its poison
    for cap in sorted({0, 1, total // 2, total - 1}):
        offsets, pb, cb = _raw(lib, cuda, x, spec, frames, capacity=cap)
        assert np.array_equal(offsets, want.offsets)
        assert np.array_equal(pb[PAD:PAD + cap * 12].view(np.uint32).reshape(-1, 3), _bits(want.points[:cap]))
        assert np.array_equal(cb[PAD + 1:PAD + 1 + cap * 3].reshape(-1, 3), want.colors[:cap])
        assert (pb[:PAD] == GUARD).all() and (pb[PAD + cap * 12:] == GUARD).all() and (cb[:PAD + 1] == GUARD).all() and (cb[PAD + 1 + cap * 3:] == GUARD).all()


def test_an_empty_cloud_writes_nothing(lib, cuda):
    shape = (3, 70, 98)
    x = cases.clip(shape, "depth")
    spec = cases.spec_for(shape, "depth", 1, False, mask=np.zeros(shape[1:], bool))
    offsets, pb, cb = _raw(lib, cuda, x, spec, cases.colours(shape), capacity=16)      # room for 16 points that never come
    assert np.array_equal(offsets, np.zeros(4, np.int64)) and (pb == GUARD).all() and (cb == GUARD).all()
    got = cloud.lift(x, spec, cases.colours(shape), output="device")
    assert len(got) == 0 and tuple(got.points.shape) == (0, 3) and tuple(got.colors.shape) == (0, 3) and np.array_equal(got.offsets, offsets)
    assert len(cloud.lift(np.zeros((0, 70, 98), np.float32), spec)) == 0      # no frames: the library is not called


# ---- d. determinism -----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes(lib, cuda):
    shape = (3, 70, 98)
    x, frames = cases.clip(shape, "disparity", seed=40), cases.colours(shape, seed=40)
    spec = cases.spec_for(shape, "disparity", 1, True, mask=_masks(shape, "per-frame", seed=41))
    first, second = _raw(lib, cuda, x, spec, frames), _raw(lib, cuda, x, spec, frames)
    assert first[0][-1] > 0
    for a, b in zip(first, second):
        assert np.array_equal(a, b)


# ---- e. zero-copy input -------------------------------------------------------------------------------------------------------------------------
def test_a_device_tensor_is_used_in_place(cuda):
    shape = (3, 70, 98)
    x, frames = cases.clip(shape, "disparity", seed=50), cases.colours(shape, seed=50)
    spec = cases.spec_for(shape, "disparity", 2, False)
    want = cloud.lift_host(x, spec, frames)
    base = torch.full((x.size + 8,), float("nan"), dtype=torch.float32, device=cuda)   # NaN around the clip: a read outside it would drop or add points
    base[1:1 + x.size] = torch.from_numpy(x.reshape(-1)).to(cuda)
    xd = base[1:1 + x.size].view(*shape)
    assert xd.data_ptr() % 16 == 4
    before = base.clone()
    _same(cloud.lift(xd, spec, torch.from_numpy(frames).to(cuda)), want)
    _same(cloud.lift(xd, spec, frames, output="device"), want)
    assert torch.equal(before.view(torch.int32), base.view(torch.int32))
    side = torch.cuda.Stream(device=cuda)                                                # on the caller's current stream, whichever it is
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        got = cloud.lift(xd, spec, frames, output="device")
    side.synchronize()
    _same(got, want)


# ---- f. / g. end to end --------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


@pytest.fixture(scope="module")
def video(cuda):
    """The small ViT-S of the video tests at its network size, 54 frames: two windows."""
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
    synth.fill_module_(m)
    frames = long_video_frames(54, NET_H, NET_W)
    frames.setflags(write=False)
    return m.to(cuda), frames


def test_video_point_cloud_equals_lifting_the_stitched_video(cuda, video, tmp_path):
    model, frames = video
    host_before = np.array(model.infer_video_depth(frames, device="cuda:0"))
    dev_before = np.array(model.infer_video_depth(frames, device="cuda:0", stitch="device"))
    spec = Cloud(K=cases.intrinsics(NET_H, NET_W), pose=cases.poses(54), step=2, mask=_masks((54, NET_H, NET_W), "shared"))
    want = cloud.lift_host(dev_before, spec, frames)
    assert 0 < len(want) and (np.diff(want.offsets) > 0).all()
    _same(model.video_point_cloud(frames, spec, device="cuda:0"), want)
    on_device = model.video_point_cloud(frames, spec, device="cuda:0", output="device")
    _same(on_device, want)
    # the .ply of a device cloud is the .ply of the host mirror, whole and one frame of it
    for frame in (None, 53):
        a, b = str(tmp_path / "device.ply"), str(tmp_path / "host.ply")
        cloud.write_ply(a, on_device, frame=frame)
        cloud.write_ply(b, want, frame=frame)
        assert open(a, "rb").read() == open(b, "rb").read()
    assert len(cloud.read_ply(a)) == want.offsets[54] - want.offsets[53]
    # the defaults keep their bits
    assert np.array_equal(_bits(model.infer_video_depth(frames, device="cuda:0")), _bits(host_before))
    assert np.array_equal(_bits(model.infer_video_depth(frames, device="cuda:0", stitch="device")), _bits(dev_before))
    with pytest.raises(ValueError, match="spec"):
        model.video_point_cloud(frames, None)
