"""Surface fusion on MI355X: ``fusion.Tsdf`` and the raw entry points against ``fusion.TsdfHost``, bit for bit (the kernels run the mirror's
float32 and float64 operations in the mirror's order, so nothing needs a tolerance); then ``model.video_surface`` against its three steps."""
import ctypes as C

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, cloud, fusion, synth
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Tsdf, TsdfHost, Volume
from tests import cloud_cases as cases
from tests import fusion_cases as fc
from tests.golden.make_golden import long_video_frames

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64  # guard bytes on either side of an output


def _both(vol, coloured, cuda):
    return Tsdf(vol, coloured=coloured, device=cuda), TsdfHost(vol, coloured=coloured)


def _same(dev, host, min_weights=(1.0,)):
    """State and surfaces of a device volume equal the mirror's bits, host and device output alike; returns the mirror's first surface."""
    fc.same_state(dev.arrays(), host.arrays())
    first = None
    for mw in min_weights:
        want = host.surface(min_weight=mw)
        first = want if first is None else first
        fc.same_cloud(dev.surface(min_weight=mw), want)
        got = dev.surface(min_weight=mw, output="device")
        assert got.points.is_cuda and got.points.dtype == torch.float32 and (got.colors is None or (got.colors.is_cuda and got.colors.dtype == torch.uint8))
        fc.same_cloud(cloud.PointCloud(got.points.cpu().numpy(), None if got.colors is None else got.colors.cpu().numpy(), got.offsets), want)
    return first


# ---- a. bit equality ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fc.CLIPS, ids=str)
@pytest.mark.parametrize("dims", fc.VOLUMES, ids=str)
def test_integrate_and_surface_equal_the_host_mirror_on_every_shape(cuda, dims, shape):
    """Every volume with every clip, the options cycling with them."""
    i = 2 * fc.VOLUMES.index(dims) + fc.CLIPS.index(shape)
    source, per_frame, kind, coloured = cloud.SOURCES[i % 2], bool((i // 2) % 2), ("none", "shared", "per-frame")[i % 3], i % 4 != 3
    vol, spec, depth, frames = fc.case(dims, shape, source, per_frame, kind, seed=i)
    dev, host = _both(vol, coloured, cuda)
    rgb = frames if coloured else None
    host.integrate(depth, spec, rgb)
    dev.integrate(depth, spec, rgb)
    weight = host.arrays()[1]
    assert 0 < (weight > 0).sum() < vol.voxels          # part of the volume is behind the camera or outside the image
    want = _same(dev, host, (1.0, float(shape[0])))
    assert len(want) > 0


@pytest.mark.parametrize("coloured", [True, False], ids=["coloured", "uncoloured"])
@pytest.mark.parametrize("kind", ["none", "shared", "per-frame"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["one-camera", "camera-per-frame"])
@pytest.mark.parametrize("source", cloud.SOURCES)
def test_integrate_and_surface_equal_the_host_mirror_under_every_option(cuda, source, per_frame, kind, coloured):
    shape, dims = (3, 37, 53), (67, 9, 5)
    vol, spec, depth, frames = fc.case(dims, shape, source, per_frame, kind, seed=11)
    dev, host = _both(vol, coloured, cuda)
    rgb = frames if coloured else None
    host.integrate(depth, spec, rgb)
    dev.integrate(torch.from_numpy(depth).to(cuda), spec, None if rgb is None else torch.from_numpy(rgb).to(cuda))
    weight = host.arrays()[1]
    assert 0 < (weight > 0).sum() < vol.voxels and (weight > 1).any()
    assert len(_same(dev, host, (1.0, 2.0))) > 0


# ---- b. edge inputs ---------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_and_zero_depth_is_skipped(cuda):
    shape, dims = (3, 37, 53), (67, 9, 5)
    vol, spec, depth, frames = fc.case(dims, shape, "depth", True, "shared", seed=12)
    depth = depth.copy()
    r = np.random.default_rng(13).random(shape)
    depth[r < 0.1], depth[(r >= 0.1) & (r < 0.2)], depth[(r >= 0.2) & (r < 0.3)], depth[(r >= 0.3) & (r < 0.4)] = np.nan, np.inf, -np.inf, 0.0
    for sp in (spec, Cloud(K=spec.K, pose=spec.pose, source="disparity", far=np.inf, mask=spec.mask)):
        dev, host = _both(vol, True, cuda)
        with np.errstate(all="ignore"):
            host.integrate(depth, sp, frames)
        dev.integrate(depth, sp, frames)
        state = host.arrays()
        assert all(np.isfinite(a).all() for a in state) and 0 < (state[1] > 0).sum()
        assert np.isfinite(_same(dev, host).points).all()


def test_weight_cap_split_calls_and_reset(cuda):
    shape, dims = (4, 37, 53), (67, 9, 5)
    vol, spec, depth, frames = fc.case(dims, shape, "depth", False, "none", seed=14, max_weight=2.0)
    dev, host = _both(vol, True, cuda)
    fresh = host.arrays()
    fc.same_state(dev.arrays(), fresh)
    host.integrate(depth, spec, frames)
    dev.integrate(depth, spec, frames)
    assert host.arrays()[1].max() == 2.0                 # four frames from one camera, capped at two
    want = _same(dev, host, (1.0, 2.0))
    # the halves one after the other are the whole clip
    dev.reset()
    fc.same_state(dev.arrays(), fresh)
    assert len(dev.surface()) == 0
    dev.integrate(depth[:2], spec, frames[:2])
    dev.integrate(depth[2:], spec, frames[2:])
    fc.same_state(dev.arrays(), host.arrays())
    fc.same_cloud(dev.surface(), want)


# ---- c. extract patterns ------------------------------------------------------------------------------------------------------------------------------
PATTERN_DIMS = (130, 7, 5)    # 4550 voxels: four full tiles and a ragged fifth


def _pattern(name):
    """(tsdf, weight) whose crossings have the named form."""
    nx, ny, nz = PATTERN_DIMS
    N, P = nx * ny * nz, fusion.TILE_VOXELS
    rng = np.random.default_rng(21)
    mag = (0.05 + 0.95 * rng.random(N)).astype(np.float32)
    a = np.arange(N)
    ix, iy, iz = a % nx, (a // nx) % ny, a // (nx * ny)
    weight = np.ones(N, np.float32)
    if name == "none":
        sign = np.ones(N)
    elif name == "every":
        sign = np.where((ix + iy + iz) % 2 == 0, 1.0, -1.0)
    elif name == "last":
        sign = np.ones(N)
        sign[N - 1] = -1.0
    else:
        sign = np.where(rng.random(N) < 0.5, 1.0, -1.0)
        if name == "weights":
            weight = rng.integers(0, 3, N).astype(np.float32)
        if name == "empty-waves-and-tiles":
            for lo, hi in ((0, P), (2 * P, 3 * P), (P + 64, P + 192), (3 * P + 256, 3 * P + 512), (4 * P, N)):
                sign[lo:hi] = 1.0
    return (mag * sign).astype(np.float32).reshape(nz, ny, nx), weight.reshape(nz, ny, nx)


@pytest.mark.parametrize("name", ["none", "every", "last", "half", "weights", "empty-waves-and-tiles"])
def test_extract_patterns(cuda, name):
    assert 4 * fusion.TILE_VOXELS < np.prod(PATTERN_DIMS) < 5 * fusion.TILE_VOXELS
    nx, ny, nz = PATTERN_DIMS
    vol = Volume(origin=(-1.0, 0.25, 3.0), voxel=0.03, dims=PATTERN_DIMS)
    dev, host = _both(vol, True, cuda)
    host.tsdf, host.weight = _pattern(name)
    host.color = (np.random.default_rng(22).random((nz, ny, nx, 3)) * 300.0 - 20.0).astype(np.float32)     # some outside 0..255: clamped
    dev.tsdf.copy_(torch.from_numpy(host.tsdf))
    dev.weight.copy_(torch.from_numpy(host.weight))
    dev.color.copy_(torch.from_numpy(host.color))
    want = _same(dev, host, (1.0, 2.0) if name == "weights" else (1.0,))
    if name == "none":
        assert len(want) == 0
    if name == "every":
        assert len(want) == (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    if name == "last":
        assert len(want) == 3
    if name in ("half", "weights", "empty-waves-and-tiles"):
        assert 0 < len(want) < 3 * vol.voxels // 2


# ---- d. guard bytes -------------------------------------------------------------------------------------------------------------------------------------
def _raw(lib, cuda, dev, min_weight=1.0, capacity=None):
    """The two extraction entry points on poisoned buffers: points start PAD bytes and colours PAD + 1 bytes into theirs.  Returns (total, points
    bytes, colour bytes) with the guards still attached."""
    st = C.c_void_p(_lib.stream_ptr(cuda))
    vol = dev.struct()
    ws = torch.empty(int(lib.edv_tsdf_workspace(*dev.volume.dims)), dtype=torch.uint8, device=cuda)
    tot = torch.full((3,), -7, dtype=torch.int64, device=cuda)
    _lib.check(lib.edv_tsdf_count(C.byref(vol), min_weight, tot.data_ptr() + 8, ws.data_ptr(), ws.numel(), st), "edv_tsdf_count")
    t = tot.cpu().numpy()
    assert t[0] == -7 and t[2] == -7
    total = int(t[1])
    room = total if capacity is None else capacity           # the buffers always hold the whole surface, the capacity may be smaller
    size = max(total, room)
    pbuf = torch.full((PAD + size * 12 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    cbuf = torch.full((PAD + 1 + size * 3 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    _lib.check(lib.edv_tsdf_extract(C.byref(vol), min_weight, ws.data_ptr(), ws.numel(), pbuf.data_ptr() + PAD, cbuf.data_ptr() + PAD + 1 if dev.coloured else None,
                                    room, st), "edv_tsdf_extract")
    torch.cuda.synchronize()
    return total, pbuf.cpu().numpy(), cbuf.cpu().numpy()


@pytest.fixture(scope="module")
def fused(cuda):
    """One integrated scene shared by the tests below, which only read it: (device volume, mirror, its surface)."""
    vol, spec, depth, frames = fc.case((67, 9, 5), (3, 37, 53), "disparity", True, "per-frame", seed=30)
    dev, host = _both(vol, True, cuda)
    host.integrate(depth, spec, frames)
    dev.integrate(depth, spec, frames)
    want = host.surface()
    assert len(want) > 8
    return dev, host, want


def test_nothing_is_written_outside_the_outputs(lib, cuda, fused):
    dev, host, want = fused
    total = len(want)
    for cap in [None] + sorted({0, 1, total // 2, total - 1}):
        got, pb, cb = _raw(lib, cuda, dev, capacity=cap)
        assert got == total
        cap = total if cap is None else cap
        assert np.array_equal(pb[PAD:PAD + cap * 12].view(np.uint32).reshape(-1, 3), fc.bits(want.points[:cap]))
        assert np.array_equal(cb[PAD + 1:PAD + 1 + cap * 3].reshape(-1, 3), want.colors[:cap])
        assert (pb[:PAD] == GUARD).all() and (pb[PAD + cap * 12:] == GUARD).all() and (cb[:PAD + 1] == GUARD).all() and (cb[PAD + 1 + cap * 3:] == GUARD).all()
    fc.same_state(dev.arrays(), host.arrays())           # extraction only reads the volume


def test_an_empty_surface_writes_nothing(lib, cuda):
    dev = Tsdf(Volume(origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(67, 9, 5)), device=cuda)
    total, pb, cb = _raw(lib, cuda, dev, capacity=16)     # room for 16 points that never come
    assert total == 0 and (pb == GUARD).all() and (cb == GUARD).all()
    got = dev.surface(output="device")
    assert len(got) == 0 and tuple(got.points.shape) == (0, 3) and tuple(got.colors.shape) == (0, 3) and np.array_equal(got.offsets, [0, 0])
    got = Tsdf(dev.volume, coloured=False, device=cuda).surface()
    assert len(got) == 0 and got.points.shape == (0, 3) and got.colors is None


# ---- e. determinism -----------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes(lib, cuda, fused):
    vol, spec, depth, frames = fc.case((67, 9, 5), (3, 37, 53), "disparity", True, "per-frame", seed=30)
    again = Tsdf(vol, device=cuda)
    again.integrate(depth, spec, frames)
    fc.same_state(again.arrays(), fused[0].arrays())
    first, second = _raw(lib, cuda, fused[0]), _raw(lib, cuda, again)
    assert first[0] > 0
    for a, b in zip(first, second):
        assert np.array_equal(a, b)


# ---- f. zero-copy input -----------------------------------------------------------------------------------------------------------------------------
def test_a_device_tensor_is_used_in_place(cuda):
    shape, dims = (3, 37, 53), (67, 9, 5)
    vol, spec, depth, frames = fc.case(dims, shape, "depth", False, "shared", seed=40)
    host = TsdfHost(vol)
    host.integrate(depth, spec, frames)
    base = torch.full((depth.size + 8,), float("nan"), dtype=torch.float32, device=cuda)   # NaN around the clip: a read outside it would skip a voxel
    base[1:1 + depth.size] = torch.from_numpy(depth.reshape(-1)).to(cuda)
    xd = base[1:1 + depth.size].view(*shape)
    assert xd.data_ptr() % 16 == 4
    before = base.clone()
    dev = Tsdf(vol, device=cuda)
    dev.integrate(xd, spec, torch.from_numpy(frames).to(cuda))
    _same(dev, host)
    assert torch.equal(before.view(torch.int32), base.view(torch.int32))
    side = torch.cuda.Stream(device=cuda)                                                  # on the caller's current stream, whichever it is
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        other = Tsdf(vol, device=cuda)
        other.integrate(xd, spec, frames)
        got = other.surface(output="device")
    side.synchronize()
    fc.same_cloud(cloud.PointCloud(got.points.cpu().numpy(), got.colors.cpu().numpy(), got.offsets), host.surface())
    with pytest.raises(ValueError, match="GPU"):
        dev.integrate(torch.from_numpy(depth), spec, frames)


# ---- g. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_and_leave_the_state_alone(lib, cuda, fused):
    dev, host, want = fused
    shape = (3, 37, 53)
    _, spec, depth, frames = fc.case((67, 9, 5), shape, "disparity", True, "per-frame", seed=30)
    st = C.c_void_p(_lib.stream_ptr(cuda))
    xd, fd, md = torch.from_numpy(depth).to(cuda), torch.from_numpy(frames).to(cuda), torch.from_numpy(spec.mask).to(cuda)
    cd = torch.from_numpy(fusion.cameras(spec, 3)).to(cuda)
    plain = Tsdf(dev.volume, coloured=False, device=cuda)
    need = int(lib.edv_tsdf_workspace(*dev.volume.dims))
    assert need == 8 * -(-dev.volume.voxels // fusion.TILE_VOXELS)
    assert lib.edv_tsdf_workspace(0, 4, 4) == 0 and lib.edv_tsdf_workspace(2048, 1024, 1024) == 0
    ws = torch.full((need + 8,), GUARD, dtype=torch.uint8, device=cuda)
    tot = torch.full((1,), -7, dtype=torch.int64, device=cuda)
    pts = torch.full((len(want) * 12,), GUARD, dtype=torch.uint8, device=cuda)
    cols = torch.full((len(want) * 3,), GUARD, dtype=torch.uint8, device=cuda)

    def vol(t=dev, **kw):
        v = t.struct()
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def sel(**kw):
        s = cloud.selection(xd, spec, md)
        for k, val in kw.items():
            setattr(s, k, val)
        return s

    def integrate(v=None, s=None, cams=cd.data_ptr(), stride=18, rgb=fd.data_ptr()):
        return lib.edv_tsdf_integrate(C.byref(v or vol()), C.byref(s or sel()), cams, stride, rgb, st)

    def count(v=None, total=tot.data_ptr(), w=ws.data_ptr(), nbytes=need):
        return lib.edv_tsdf_count(C.byref(v or vol()), 1.0, total, w, nbytes, st)

    def extract(v=None, w=ws.data_ptr(), nbytes=need, p=pts.data_ptr(), c=cols.data_ptr(), cap=len(want)):
        return lib.edv_tsdf_extract(C.byref(v or vol()), 1.0, w, nbytes, p, c, cap, st)

    geometry = [dict(tsdf_dev=None), dict(weight_dev=None), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=2048, ny=1024, nz=1024), dict(nx=2 ** 16, ny=2 ** 16, nz=1),
                dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(trunc=-1.0), dict(trunc=float("nan")), dict(max_weight=0.0),
                dict(max_weight=float("inf")), dict(max_weight=float("nan"))]
    refused = [integrate(v=vol(**kw)) for kw in geometry] + [count(v=vol(**kw)) for kw in geometry] + [extract(v=vol(**kw)) for kw in geometry]
    refused += [lib.edv_tsdf_integrate(None, C.byref(sel()), cd.data_ptr(), 18, fd.data_ptr(), st), lib.edv_tsdf_integrate(C.byref(vol()), None, cd.data_ptr(), 18, fd.data_ptr(), st),
                lib.edv_tsdf_count(None, 1.0, tot.data_ptr(), ws.data_ptr(), need, st), lib.edv_tsdf_extract(None, 1.0, ws.data_ptr(), need, pts.data_ptr(), cols.data_ptr(), 1, st)]
    refused += [integrate(s=sel(x_dev=None)), integrate(s=sel(step=2)), integrate(s=sel(n=0)), integrate(s=sel(n=65536)), integrate(s=sel(h=0)), integrate(s=sel(mode=2)),
                integrate(s=sel(mask_stride=5)), integrate(cams=None), integrate(stride=21), integrate(stride=1), integrate(rgb=None),
                integrate(v=vol(plain)), integrate(v=vol(color_dev=None))]
    refused += [count(total=None), count(w=None), count(nbytes=need - 8), count(nbytes=0), count(w=ws.data_ptr() + 4)]
    refused += [extract(w=None), extract(nbytes=need - 8), extract(w=ws.data_ptr() + 4), extract(p=None), extract(cap=-1), extract(v=vol(plain))]
    assert all(r != 0 for r in refused), refused
    assert lib.edv_last_error()
    torch.cuda.synchronize()
    fc.same_state(dev.arrays(), host.arrays())
    fc.same_state(plain.arrays(), TsdfHost(dev.volume, coloured=False).arrays())
    assert int(tot.cpu()[0]) == -7 and all((t.cpu().numpy() == GUARD).all() for t in (ws, pts, cols))
    # and the accepted forms of the same calls still work
    assert integrate(v=vol(plain), rgb=None) == 0 and count() == 0 and extract() == 0 and extract(c=None) == 0 and extract(cap=0) == 0
    torch.cuda.synchronize()
    assert int(tot.cpu()[0]) == len(want) and np.array_equal(pts.cpu().numpy().view(np.uint32).reshape(-1, 3), fc.bits(want.points))
    # the Python layer refuses before it reaches the library
    for args, match in [((depth, Cloud(K=spec.K, pose=spec.pose, step=2), frames), "step"), ((depth, spec, None), "coloured"), ((depth[:0], spec, frames[:0]), "frames per call")]:
        with pytest.raises(ValueError, match=match):
            dev.integrate(*args)
    with pytest.raises(ValueError):
        dev.surface(min_weight=float("nan"))
    with pytest.raises(ValueError, match="output"):
        dev.surface(output="disk")
    fc.same_state(dev.arrays(), host.arrays())


# ---- h. end to end ----------------------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


@pytest.fixture(scope="module")
def video(cuda):
    """The small ViT-S of the video tests at its network size, 54 frames: two windows."""
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
    synth.fill_module_(m)
    frames = long_video_frames(54, NET_H, NET_W)
    frames.setflags(write=False)
    return m.to(cuda), frames


def test_video_surface_equals_its_three_steps(cuda, video, tmp_path):
    model, frames = video
    depth = model.infer_video_depth(frames, device="cuda:0", stitch="device", output="device")
    assert depth.is_cuda and tuple(depth.shape) == (54, NET_H, NET_W)
    # the scene's own scale decides the camera path and the volume: the points of every ninth frame, out to twice the median depth
    z = cloud.lift_host(depth.cpu().numpy(), Cloud(K=np.eye(3)), None).points[:, 2]
    assert z.size and np.isfinite(z).all()
    scale = float(np.median(z))
    spec = Cloud(K=cases.intrinsics(NET_H, NET_W), pose=fc.nearby_poses(54, seed=1, scale=scale), far=2.0 * scale,
                 mask=np.random.default_rng(5).random((NET_H, NET_W)) < 0.9)
    points = cloud.lift_host(depth.cpu().numpy()[::9], Cloud(K=spec.K, pose=spec.pose[::9], far=spec.far), None).points
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    vol = Volume.bounding(points, extent / 40.0)
    assert max(vol.dims) <= 50
    steps = Tsdf(vol, coloured=True, device=cuda)
    steps.integrate(depth, spec, torch.from_numpy(frames.copy()).to(cuda))
    want = steps.surface(min_weight=2.0)
    assert len(want) > 0 and want.colors.shape == (len(want), 3)
    fc.same_cloud(model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0), want)
    on_device = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0, output="device")
    fc.same_cloud(cloud.PointCloud(on_device.points.cpu().numpy(), on_device.colors.cpu().numpy(), on_device.offsets), want)
    # the mirror agrees on the same stitched video
    host = TsdfHost(vol)
    host.integrate(depth.cpu().numpy(), spec, frames)
    fc.same_cloud(want, host.surface(min_weight=2.0))
    # a written .ply reads back equal
    path = str(tmp_path / "surface.ply")
    cloud.write_ply(path, on_device)
    fc.same_cloud(cloud.read_ply(path), want)
    with pytest.raises(ValueError, match="spec"):
        model.video_surface(frames, None, vol)
    with pytest.raises(ValueError, match="Volume"):
        model.video_surface(frames, spec, (4, 4, 4))
    with pytest.raises(ValueError, match="step"):
        model.video_surface(frames, Cloud(K=spec.K, pose=spec.pose, step=2), vol)
    with pytest.raises(ValueError, match="min_weight"):
        model.video_surface(frames, spec, vol, min_weight=-1.0)
    with pytest.raises(ValueError, match="output"):
        model.video_surface(frames, spec, vol, output="disk")
