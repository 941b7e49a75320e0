"""Views of the fused surface on MI355X: ``fusion.Tsdf.raycast`` and the raw entry point against ``fusion.TsdfHost.raycast``, bit for bit in depth,
normals and colours (the kernel runs the mirror's float32 and float64 operations in the mirror's order, so nothing needs a tolerance); then
``model.video_surface(surface="views")`` against its three steps."""
import ctypes as C

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, cloud, fusion, synth
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Raycast, Tsdf, TsdfHost, Views, Volume
from tests import cloud_cases as cases
from tests import fusion_cases as fc
from tests import mesh_cases as mc
from tests import raycast_cases as rc
from tests.golden.make_golden import long_video_frames

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64  # guard bytes on either side of an output


def _on_gpu(host, cuda):
    """A device volume with the mirror's state."""
    dev = Tsdf(host.volume, coloured=host.coloured, device=cuda)
    dev.tsdf.copy_(torch.from_numpy(host.tsdf))
    dev.weight.copy_(torch.from_numpy(host.weight))
    if host.coloured:
        dev.color.copy_(torch.from_numpy(host.color))
    return dev


def _to_host(result):
    return Raycast(*(None if p is None else p.cpu().numpy() for p in (result.depth, result.normals, result.colors)))


def _same(dev, host, views, min_weights=(1.0,), normals=(True, False)):
    """The views of a device volume equal the mirror's bits, host and device output alike; returns the mirror's first result."""
    first = None
    for mw in min_weights:
        for nrm in normals:
            with np.errstate(all="ignore"):
                want = host.raycast(views, min_weight=mw, normals=nrm)
            first = want if first is None else first
            rc.miss_is_zero(want)
            rc.same_raycast(dev.raycast(views, min_weight=mw, normals=nrm), want)
            got = dev.raycast(views, min_weight=mw, normals=nrm, output="device")
            assert all(p is None or (p.is_cuda and p.device == dev.device) for p in (got.depth, got.normals, got.colors))
            rc.same_raycast(_to_host(got), want)
    return first


# ---- 1. bit equality after integrate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fc.CLIPS, ids=str)
@pytest.mark.parametrize("dims", fc.VOLUMES, ids=str)
def test_raycast_equals_the_host_mirror_after_integrate(cuda, dims, shape):
    """Every volume with every clip, the options cycling with them as in tests/test_mesh_gpu.py; min_weight 1 and 2 after the three-frame clip.
    The views are the clip's own cameras and one more, at every size of raycast_cases.SIZES, a quarter of a voxel between two samples (the
    surface of these clips is rough, a few voxels of it observed on both sides; a whole voxel a step finds it in some of the scenes only).
    After the three-frame clips some ray of the 17 x 33 views finds the surface and some does not.  The one-frame clips are compared bit for
    bit alike, but leave so few observed voxels that a hit is not certain: in the (130, 7, 3) volume no cell with eight observed corners is
    crossed by the surface at all (its mesh is empty), and no view can hit there."""
    i = 2 * fc.VOLUMES.index(dims) + fc.CLIPS.index(shape)
    source, per_frame, kind, coloured = cloud.SOURCES[i % 2], shape[0] > 1, ("none", "shared", "per-frame")[i % 3], i % 4 != 3
    vol, spec, depth, frames = fc.case(dims, shape, source, per_frame, kind, seed=i)
    dev, host = Tsdf(vol, coloured=coloured, device=cuda), TsdfHost(vol, coloured=coloured)
    rgb = frames if coloured else None
    host.integrate(depth, spec, rgb)
    dev.integrate(depth, spec, rgb)
    fc.same_state(dev.arrays(), host.arrays())
    many = shape[0] > 1
    for size in rc.SIZES:
        views = rc.scene_views(spec, size, seed=i, step=vol.voxel / 4.0)
        assert views.count == spec.pose.shape[0] + 1
        want = _same(dev, host, views, (1.0, 2.0) if many else (1.0,), (True, False) if size == (17, 33) else (True,))
        assert (want.colors is not None) == coloured
        print(f"\n[{dims} {shape} {size}] {rc.hits(want)} hits of {want.depth.size}")
        if many and size == (17, 33):
            assert 0 < rc.hits(want) < want.depth.size
    fc.same_state(dev.arrays(), host.arrays())           # the views only read the volume


# ---- 2. hand-set volumes ----------------------------------------------------------------------------------------------------------------------------
def _looking_at(host, size=(17, 33), distance=None, **kw):
    """Two cameras that look at the centre of a hand-set volume from ``distance`` (default: 1.5 times its longest side), one along +z and one turned
    by 0.4 rad about y and 0.2 rad about x; the volume about fills the image."""
    vol = host.volume
    side = vol.voxel * np.asarray(vol.dims, np.float64)
    centre = np.asarray(vol.origin) + 0.5 * side
    distance = 1.5 * side.max() if distance is None else distance
    poses = []
    for ay, ax in ((0.0, 0.0), (0.4, 0.2)):
        cy, sy, cx, sx = np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
        T = np.eye(4)
        T[:3, :3] = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
        T[:3, 3] = centre - distance * T[:3, 2]
        poses.append(T)
    h, w = size
    focal = 0.9 * min(h, w) * distance / side.max()
    K = np.array([[focal, 0.0, 0.5 * w + 0.13], [0.0, focal, 0.5 * h + 0.21], [0.0, 0.0, 1.0]])
    kw.setdefault("step", vol.voxel / 2.0)
    return Views(K, np.stack(poses), size=size, near=max(distance - side.max(), 0.0), far=distance + side.max(), **kw)


def test_noise_and_sphere(cuda):
    for host in (mc.noise((6, 7, 9), seed=6), mc.noise((6, 7, 9), seed=6, coloured=False), mc.sphere(), mc.sphere(holes=0.03, seed=1, coloured=True)):
        want = _same(_on_gpu(host, cuda), host, _looking_at(host), (1.0, 2.0) if host.weight.max() > 1 else (1.0,))
        assert 0 < rc.hits(want) < want.depth.size
    ball = mc.sphere()
    want = _same(_on_gpu(ball, cuda), ball, rc.sphere_views())
    assert rc.hits(want) == 148                          # the view of tests/test_raycast_cpu.py


@pytest.mark.parametrize("name", mc.ONE_CELL)
def test_one_cell(cuda, name):
    host = mc.one_cell(name)
    want = _same(_on_gpu(host, cuda), host, _looking_at(host, step=host.volume.voxel / 8.0))
    if name in ("corner-5", "checker"):                  # an inside corner behind an outside one, seen from -z
        assert rc.hits(want) > 0
    if name in ("all-in", "all-out"):
        assert rc.hits(want) == 0


@pytest.mark.parametrize("dims", mc.NO_CELL, ids=str)
def test_a_volume_without_a_cell(cuda, dims):
    for coloured in (True, False):
        host = mc.noise(dims, seed=1, unobserved=0.0, coloured=coloured)
        want = _same(_on_gpu(host, cuda), host, _looking_at(host, size=(5, 7), step=host.volume.voxel))
        assert rc.hits(want) == 0


# ---- 3. the raw entry point -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused(cuda):
    """One integrated scene shared by the tests below, which only read it: (device volume, mirror, views, the mirror's result)."""
    vol, spec, depth, frames = fc.case((67, 9, 5), (3, 37, 53), "disparity", True, "per-frame", seed=30)
    dev, host = Tsdf(vol, device=cuda), TsdfHost(vol)
    host.integrate(depth, spec, frames)
    dev.integrate(depth, spec, frames)
    views = rc.scene_views(spec, (17, 33), seed=30, step=vol.voxel / 4.0)
    want = host.raycast(views)
    assert 0 < rc.hits(want) < want.depth.size
    return dev, host, views, want


def _raw(lib, cuda, dev, seen, min_weight=1.0, normals=True, colors=True, stream=None, **kw):
    """The entry point for the views ``seen`` on poisoned buffers: depth and normals start PAD bytes and colours PAD + 1 bytes into theirs.  Returns (the return value,
    the three buffers' bytes with the guards on)."""
    st = C.c_void_p(_lib.stream_ptr(cuda) if stream is None else stream.cuda_stream)
    vol = dev.struct()
    m, (h, w) = seen.count, seen.size
    px = m * h * w
    cams = torch.from_numpy(seen.cams().copy()).to(cuda)
    step, steps = seen.march(dev.volume.voxel)
    bufs = [torch.full((PAD + px * 4 + PAD,), GUARD, dtype=torch.uint8, device=cuda), torch.full((PAD + px * 12 + PAD,), GUARD, dtype=torch.uint8, device=cuda),
            torch.full((PAD + 1 + px * 3 + PAD,), GUARD, dtype=torch.uint8, device=cuda)]
    args = dict(vol=C.byref(vol), cams=cams.data_ptr(), views=m, h=h, w=w, near=seen.near, step=step, steps=steps, min_weight=min_weight,
                depth=bufs[0].data_ptr() + PAD, normals=bufs[1].data_ptr() + PAD, colors=bufs[2].data_ptr() + PAD + 1)
    for k, val in dict(normals=normals, colors=colors, **kw).items():      # True: as above; False or None: a null pointer; a function: of the pointer
        args[k] = args[k] if val is True else None if val is False else val(args[k]) if callable(val) else val
    ret = lib.edv_tsdf_raycast(*args.values(), st)
    torch.cuda.synchronize()
    return ret, [b.cpu().numpy() for b in bufs]


def _check_guarded(bufs, want, normals=True, colors=True):
    px = want.depth.size
    d, n, c = bufs
    assert np.array_equal(d[PAD:PAD + px * 4].view(np.uint32), fc.bits(want.depth).reshape(-1))
    assert (d[:PAD] == GUARD).all() and (d[PAD + px * 4:] == GUARD).all()
    if normals:
        assert np.array_equal(n[PAD:PAD + px * 12].view(np.uint32), fc.bits(want.normals).reshape(-1))
        assert (n[:PAD] == GUARD).all() and (n[PAD + px * 12:] == GUARD).all()
    else:
        assert (n == GUARD).all()
    if colors:
        assert np.array_equal(c[PAD + 1:PAD + 1 + px * 3], want.colors.reshape(-1))
        assert (c[:PAD + 1] == GUARD).all() and (c[PAD + 1 + px * 3:] == GUARD).all()
    else:
        assert (c == GUARD).all()


def test_every_pixel_is_written_and_nothing_else(lib, cuda, fused):
    """The outputs start as junk between guard bytes: every pixel comes back written, misses as zeros, and the guards are intact.  Without
    normals or colours their buffers stay as they were and the depth bits are the same."""
    dev, host, views, want = fused
    for normals, colors in ((True, True), (False, True), (True, False), (False, False)):
        ret, bufs = _raw(lib, cuda, dev, views, normals=normals, colors=colors)
        assert ret == 0, lib.edv_last_error()
        _check_guarded(bufs, want, normals, colors)
    for size in rc.SIZES:                                 # ragged tiles: the last row and column of workgroups write inside the image only
        ragged = Views(views.K, views.pose, size=size, near=views.near, far=views.far, step=views.step)
        ret, bufs = _raw(lib, cuda, dev, ragged)
        assert ret == 0, lib.edv_last_error()
        _check_guarded(bufs, host.raycast(ragged))
    fc.same_state(dev.arrays(), host.arrays())           # the views only read the volume


def test_two_calls_give_the_same_bytes_on_any_stream(lib, cuda, fused):
    dev, host, views, want = fused
    first, second = _raw(lib, cuda, dev, views), _raw(lib, cuda, dev, views)
    assert first[0] == 0 and second[0] == 0
    for a, b in zip(first[1], second[1]):
        assert np.array_equal(a, b)
    side = torch.cuda.Stream(device=cuda)                 # on the caller's current stream, whichever it is
    side.wait_stream(torch.cuda.current_stream(cuda))
    ret, bufs = _raw(lib, cuda, dev, views, stream=side)
    assert ret == 0
    _check_guarded(bufs, want)
    with torch.cuda.stream(side):
        other = _on_gpu(host, cuda)
        got = other.raycast(views, output="device")
    side.synchronize()
    assert got.depth.device == dev.device
    rc.same_raycast(_to_host(got), want)


def test_the_entry_point_refuses_and_leaves_everything_alone(lib, cuda, fused):
    dev, host, views, want = fused
    plain = Tsdf(dev.volume, coloured=False, device=cuda)

    def vol(t=dev, **kw):
        v = t.struct()
        for k, val in kw.items():
            setattr(v, k, val)
        return C.byref(v)

    geometry = [dict(tsdf_dev=None), dict(weight_dev=None), dict(tsdf_dev=dev.tsdf.data_ptr() + 2), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=2048, ny=1024, nz=1024),
                dict(voxel=0.0), dict(voxel=float("nan")), dict(trunc=-1.0), dict(max_weight=float("inf"))]
    bad = [dict(vol=vol(**kw)) for kw in geometry]
    bad += [dict(vol=None), dict(cams=None), dict(cams=lambda p: p + 4), dict(depth=None), dict(depth=lambda p: p + 2), dict(normals=lambda p: p + 1),
            dict(views=0), dict(h=0), dict(w=-1), dict(views=2 ** 16, h=2 ** 8, w=2 ** 7), dict(steps=0), dict(steps=65537), dict(steps=-1),
            dict(step=0.0), dict(step=-0.01), dict(step=float("nan")), dict(step=float("inf")), dict(near=float("nan")), dict(near=float("inf")),
            dict(vol=vol(plain))]                          # colours asked of an uncoloured volume
    for kw in bad:
        ret, bufs = _raw(lib, cuda, dev, views, **kw)
        assert ret != 0, kw
        assert lib.edv_last_error(), kw
        assert all((b == GUARD).all() for b in bufs), kw    # nothing was launched
    fc.same_state(dev.arrays(), host.arrays())
    fc.same_state(plain.arrays(), TsdfHost(dev.volume, coloured=False).arrays())
    # the accepted forms of the same calls still work
    ret, bufs = _raw(lib, cuda, dev, views, depth=lambda p: p + 4, normals=lambda p: p + 4, colors=lambda p: p + 1)
    assert ret == 0, lib.edv_last_error()
    assert np.array_equal(bufs[0][PAD + 4:PAD + 4 + want.depth.size * 4].view(np.uint32), fc.bits(want.depth).reshape(-1))
    ret, bufs = _raw(lib, cuda, dev, views, vol=vol(plain), colors=False)
    assert ret == 0 and (bufs[2] == GUARD).all() and not (bufs[0][PAD:-PAD] == GUARD).all()
    ret, bufs = _raw(lib, cuda, dev, views, steps=1)
    assert ret == 0 and (bufs[0][PAD:-PAD] == 0).all()      # one sample is never a hit
    # the Python layer refuses before it reaches the library
    for kw in (dict(min_weight=float("nan")), dict(min_weight=-1.0), dict(output="disk"), dict(normals="yes")):
        with pytest.raises(ValueError):
            dev.raycast(views, **kw)
    with pytest.raises(ValueError, match="Views"):
        dev.raycast(Cloud(K=views.K))
    with pytest.raises(ValueError, match="samples"):
        Tsdf(Volume(origin=(0.0, 0.0, 0.0), voxel=1e-6, dims=(2, 2, 2)), device=cuda).raycast(Views(views.K, size=(2, 2), near=0.0, far=1.0))
    fc.same_state(dev.arrays(), host.arrays())


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


@pytest.fixture(scope="module")
def video(cuda):
    """The small ViT-S of tests/test_mesh_gpu.py at its network size, 54 frames: two windows."""
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
    synth.fill_module_(m)
    frames = long_video_frames(54, NET_H, NET_W)
    frames.setflags(write=False)
    return m.to(cuda), frames


def test_video_surface_as_views_equals_its_three_steps(cuda, video):
    model, frames = video
    depth = model.infer_video_depth(frames, device="cuda:0", stitch="device", output="device")
    z = cloud.lift_host(depth.cpu().numpy(), Cloud(K=np.eye(3)), None).points[:, 2]
    scale = float(np.median(z))
    spec = Cloud(K=cases.intrinsics(NET_H, NET_W), pose=fc.nearby_poses(54, seed=1, scale=scale), far=2.0 * scale,
                 mask=np.random.default_rng(5).random((NET_H, NET_W)) < 0.9)
    points = cloud.lift_host(depth.cpu().numpy()[::9], Cloud(K=spec.K, pose=spec.pose[::9], far=spec.far), None).points
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    vol = Volume.bounding(points, extent / 40.0)
    assert max(vol.dims) <= 50
    views = Views(spec.K, spec.pose[::18], size=(NET_H, NET_W), near=0.0, far=2.0 * scale)      # three of the input cameras, a voxel a step
    steps = Tsdf(vol, coloured=True, device=cuda)
    steps.integrate(depth, spec, torch.from_numpy(frames.copy()).to(cuda))
    want = steps.raycast(views, min_weight=2.0)
    assert want.depth.shape == (3, NET_H, NET_W) and want.normals.shape == (3, NET_H, NET_W, 3) and want.colors.shape == (3, NET_H, NET_W, 3)
    assert 0 < rc.hits(want) < want.depth.size
    rc.miss_is_zero(want)
    rc.same_raycast(model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0, surface="views", views=views), want)
    on_device = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0, output="device", surface="views", views=views)
    assert isinstance(on_device, Raycast) and on_device.depth.is_cuda and on_device.normals.is_cuda and on_device.colors.is_cuda
    rc.same_raycast(_to_host(on_device), want)
    # the mirror agrees on the same stitched video
    host = TsdfHost(vol)
    host.integrate(depth.cpu().numpy(), spec, frames)
    rc.same_raycast(want, host.raycast(views, min_weight=2.0))
    # the hits, lifted as the cloud lifts a depth map, lie in the bounding box of the mesh's vertices: a hit lies in a cell the surface crosses or
    # next to one, so two voxels of margin
    back = cloud.lift_host(want.depth, Cloud(K=views.K, pose=views.pose, source="depth", near=0.0, far=4.0 * scale), None).points
    vertices = steps.mesh(min_weight=2.0).vertices
    assert back.shape[0] == rc.hits(want)
    assert (back >= vertices.min(axis=0) - 2.0 * vol.voxel).all() and (back <= vertices.max(axis=0) + 2.0 * vol.voxel).all()
    with pytest.raises(ValueError, match="views"):
        model.video_surface(frames, spec, vol, surface="views")
    with pytest.raises(ValueError, match="views"):
        model.video_surface(frames, spec, vol, surface="mesh", views=views)
