"""Triangle meshes on MI355X: ``fusion.Tsdf.mesh`` and the raw entry points against ``fusion.TsdfHost.mesh``, bit for bit in all four arrays
(the kernels run the mirror's float32 and float64 operations in the mirror's order, so nothing needs a tolerance); then
``model.video_surface(surface="mesh")`` against its three steps."""
import ctypes as C

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, cloud, fusion, synth
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Mesh, Tsdf, TsdfHost, Volume
from tests import cloud_cases as cases
from tests import fusion_cases as fc
from tests import mesh_cases as mc
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


def _to_host(mesh):
    return Mesh(*(None if p is None else p.cpu().numpy() for p in (mesh.vertices, mesh.normals, mesh.colors, mesh.triangles)))


def _same(dev, host, min_weights=(1.0,), normals=(True, False)):
    """The meshes of a device volume equal the mirror's bits, host and device output alike; returns the mirror's first mesh."""
    first = None
    for mw in min_weights:
        for nrm in normals:
            with np.errstate(all="ignore"):
                want = host.mesh(min_weight=mw, normals=nrm)
            first = want if first is None else first
            mc.same_mesh(dev.mesh(min_weight=mw, normals=nrm), want)
            got = dev.mesh(min_weight=mw, normals=nrm, output="device")
            assert all(p is None or (p.is_cuda and p.device == dev.device) for p in (got.vertices, got.normals, got.colors, got.triangles))
            mc.same_mesh(_to_host(got), want)
    return first


# ---- 10. bit equality --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fc.CLIPS, ids=str)
@pytest.mark.parametrize("dims", fc.VOLUMES, ids=str)
def test_mesh_equals_the_host_mirror_after_integrate(cuda, dims, shape):
    """Every volume with every clip, the options cycling with them; min_weight 1 and 2 after the three-frame clip, where validity and not only
    the sign decides."""
    i = 2 * fc.VOLUMES.index(dims) + fc.CLIPS.index(shape)
    source, per_frame, kind, coloured = cloud.SOURCES[i % 2], shape[0] > 1, ("none", "shared", "per-frame")[i % 3], i % 4 != 3
    vol, spec, depth, frames = fc.case(dims, shape, source, per_frame, kind, seed=i)
    dev, host = Tsdf(vol, coloured=coloured, device=cuda), TsdfHost(vol, coloured=coloured)
    rgb = frames if coloured else None
    host.integrate(depth, spec, rgb)
    dev.integrate(depth, spec, rgb)
    fc.same_state(dev.arrays(), host.arrays())
    weight = host.arrays()[1]
    assert 0 < (weight > 0).sum() < vol.voxels
    many = shape[0] > 1
    want = _same(dev, host, (1.0, 2.0) if many else (1.0,))
    if many:
        assert (weight > 1).any() and 0 < (weight == 1).sum()
        assert want.triangles.shape[0] > 0 and want.triangles.shape[0] > host.mesh(min_weight=2.0).triangles.shape[0]
    fc.same_state(dev.arrays(), host.arrays())           # the mesh only reads the volume


@pytest.mark.parametrize("dims", mc.NO_CELL, ids=str)
def test_a_volume_without_a_cell(cuda, dims):
    for coloured in (True, False):
        host = mc.noise(dims, seed=1, unobserved=0.0, coloured=coloured)
        want = _same(_on_gpu(host, cuda), host)
        assert want.vertices.shape == (0, 3) and want.triangles.shape == (0, 3)


@pytest.mark.parametrize("name", mc.ONE_CELL)
def test_one_cell(cuda, name):
    host = mc.one_cell(name)
    _same(_on_gpu(host, cuda), host)


def test_noise_sphere_and_zero_normals(cuda):
    for host in (mc.noise((6, 7, 9), seed=6), mc.noise((6, 7, 9), seed=6, coloured=False), mc.sphere(), mc.sphere(holes=0.03, seed=1, coloured=True),
                 mc.filled((4, 2, 2), np.tile(np.array([-0.5, 0.5, -0.5, 0.5]), 4))):
        want = _same(_on_gpu(host, cuda), host, (1.0, 2.0) if host.weight.max() > 1 else (1.0,))
        assert want.triangles.shape[0] > 0
    assert (want.normals == 0).all(axis=1).any()           # the last volume holds crossings with a zero gradient


# ---- 11. hand-set patterns ---------------------------------------------------------------------------------------------------------------------------
PATTERN_DIMS = (130, 7, 5)    # 4550 voxels: four full tiles and a ragged fifth


def _pattern(name):
    """(tsdf, weight) whose mesh has the named form."""
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
    elif name == "planes":
        sign = np.where(rng.random(N) < 0.5, 1.0, -1.0)
        weight = (iy % 2 == 0).astype(np.float32)                # every other y plane unobserved: crossings along x and z, no valid cell
    else:
        sign = np.where(rng.random(N) < 0.5, 1.0, -1.0)
        if name == "weights":
            weight = np.where(rng.random(N) < 0.05, 0.0, np.where(rng.random(N) < 0.1, 1.0, 2.0)).astype(np.float32)
        if name == "empty-waves-and-tiles":
            for lo, hi in ((0, P), (2 * P, 3 * P), (P + 64, P + 192), (3 * P + 256, 3 * P + 512), (4 * P, N)):
                sign[lo:hi] = 1.0
    return (mag * sign).astype(np.float32).reshape(nz, ny, nx), weight.reshape(nz, ny, nx)


@pytest.mark.parametrize("name", ["none", "every", "last", "planes", "half", "weights", "empty-waves-and-tiles"])
def test_mesh_patterns(cuda, name):
    assert 4 * fusion.TILE_VOXELS < np.prod(PATTERN_DIMS) < 5 * fusion.TILE_VOXELS
    nx, ny, nz = PATTERN_DIMS
    tsdf, weight = _pattern(name)
    color = np.random.default_rng(22).random((nz, ny, nx, 3)) * 300.0 - 20.0      # some outside 0..255: clamped
    host = mc.filled(PATTERN_DIMS, tsdf, weight, color, origin=(-1.0, 0.25, 3.0), voxel=0.03)
    want = _same(_on_gpu(host, cuda), host, (1.0, 2.0) if name == "weights" else (1.0,))
    V, F = want.vertices.shape[0], want.triangles.shape[0]
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    if name == "none":
        assert (V, F) == (0, 0)
    if name == "every":       # the checkerboard cuts every axis edge and every body diagonal, and no face diagonal: 12 triangles in every cell
        assert V == (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1) + cells and F == 12 * cells
    if name == "last":        # the last voxel is corner 7 of the last cell alone: the 7 edges into it, one triangle in each tetrahedron
        assert (V, F) == (7, 6) and want.triangles.max() == 6
    if name == "planes":
        assert (V, F) == (0, 0) and len(host.surface()) > 0
    if name in ("half", "weights", "empty-waves-and-tiles"):
        assert 0 < F <= 12 * cells and 0 < V < 7 * host.volume.voxels


# ---- 12. guard bytes ---------------------------------------------------------------------------------------------------------------------------------
def _raw(lib, cuda, dev, min_weight=1.0, capacity=None, normals=True):
    """The two mesh entry points on poisoned buffers; vertices, normals and triangles start PAD bytes and colours PAD + 1 bytes into theirs.
    ``capacity``: None for the totals, or (vertex capacity, triangle capacity).  Returns (totals, the four buffers' bytes with the guards on)."""
    st = C.c_void_p(_lib.stream_ptr(cuda))
    vol = dev.struct()
    ws = torch.empty(int(lib.edv_tsdf_mesh_workspace(*dev.volume.dims)), dtype=torch.uint8, device=cuda)
    tot = torch.full((4,), -7, dtype=torch.int64, device=cuda)
    _lib.check(lib.edv_tsdf_mesh_count(C.byref(vol), min_weight, tot.data_ptr() + 8, ws.data_ptr(), ws.numel(), st), "edv_tsdf_mesh_count")
    t = tot.cpu().numpy()
    assert t[0] == -7 and t[3] == -7
    nv, nt = int(t[1]), int(t[2])
    vcap, tcap = (nv, nt) if capacity is None else capacity
    vsize, tsize = max(nv, vcap), max(nt, tcap)            # the buffers always hold the whole mesh, the capacities may be smaller
    bufs = [torch.full((PAD + vsize * 12 + PAD,), GUARD, dtype=torch.uint8, device=cuda), torch.full((PAD + vsize * 12 + PAD,), GUARD, dtype=torch.uint8, device=cuda),
            torch.full((PAD + 1 + vsize * 3 + PAD,), GUARD, dtype=torch.uint8, device=cuda), torch.full((PAD + tsize * 12 + PAD,), GUARD, dtype=torch.uint8, device=cuda)]
    _lib.check(lib.edv_tsdf_mesh_extract(C.byref(vol), min_weight, ws.data_ptr(), ws.numel(), bufs[0].data_ptr() + PAD, bufs[1].data_ptr() + PAD if normals else None,
                                         bufs[2].data_ptr() + PAD + 1 if dev.coloured else None, vcap, bufs[3].data_ptr() + PAD, tcap, st), "edv_tsdf_mesh_extract")
    torch.cuda.synchronize()
    return (nv, nt), [b.cpu().numpy() for b in bufs]


@pytest.fixture(scope="module")
def fused(cuda):
    """One integrated scene shared by the tests below, which only read it: (device volume, mirror, its mesh)."""
    vol, spec, depth, frames = fc.case((67, 9, 5), (3, 37, 53), "disparity", True, "per-frame", seed=30)
    dev, host = Tsdf(vol, device=cuda), TsdfHost(vol)
    host.integrate(depth, spec, frames)
    dev.integrate(depth, spec, frames)
    want = host.mesh()
    assert want.vertices.shape[0] > 8 and want.triangles.shape[0] > 8
    return dev, host, want


def _check_guarded(bufs, want, vcap, tcap):
    v, n, c, t = bufs
    assert np.array_equal(v[PAD:PAD + vcap * 12].view(np.uint32).reshape(-1, 3), fc.bits(want.vertices[:vcap]))
    assert np.array_equal(n[PAD:PAD + vcap * 12].view(np.uint32).reshape(-1, 3), fc.bits(want.normals[:vcap]))
    assert np.array_equal(c[PAD + 1:PAD + 1 + vcap * 3].reshape(-1, 3), want.colors[:vcap])
    assert np.array_equal(t[PAD:PAD + tcap * 12].view(np.int32).reshape(-1, 3), want.triangles[:tcap])
    for b, lo, hi in ((v, PAD, PAD + vcap * 12), (n, PAD, PAD + vcap * 12), (c, PAD + 1, PAD + 1 + vcap * 3), (t, PAD, PAD + tcap * 12)):
        assert (b[:lo] == GUARD).all() and (b[hi:] == GUARD).all()


def test_nothing_is_written_outside_the_outputs(lib, cuda, fused):
    dev, host, want = fused
    nv, nt = want.vertices.shape[0], want.triangles.shape[0]
    for cap in [None, (0, nt), (nv, 0), (1, 1), (nv // 2, nt - 1), (nv - 1, nt // 2), (nv + 5, nt + 5)]:
        totals, bufs = _raw(lib, cuda, dev, capacity=cap)
        assert totals == (nv, nt)
        vcap, tcap = (nv, nt) if cap is None else (min(cap[0], nv), min(cap[1], nt))
        _check_guarded(bufs, want, vcap, tcap)
    totals, bufs = _raw(lib, cuda, dev, normals=False)      # without normals their buffer stays as it was
    assert (bufs[1] == GUARD).all() and np.array_equal(bufs[0][PAD:PAD + nv * 12].view(np.uint32).reshape(-1, 3), fc.bits(want.vertices))
    fc.same_state(dev.arrays(), host.arrays())           # the mesh only reads the volume


def test_an_empty_mesh_writes_nothing(lib, cuda):
    dev = Tsdf(Volume(origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(67, 9, 5)), device=cuda)
    totals, bufs = _raw(lib, cuda, dev, capacity=(16, 16))     # room for 16 vertices and triangles that never come
    assert totals == (0, 0) and all((b == GUARD).all() for b in bufs)
    got = dev.mesh(output="device")
    assert all(tuple(p.shape) == (0, 3) and p.is_cuda for p in (got.vertices, got.normals, got.colors, got.triangles))
    assert (got.vertices.dtype, got.normals.dtype, got.colors.dtype, got.triangles.dtype) == (torch.float32, torch.float32, torch.uint8, torch.int32)
    got = Tsdf(dev.volume, coloured=False, device=cuda).mesh(normals=False)
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and got.normals is None and got.colors is None


def test_two_calls_give_the_same_bytes_on_any_stream(lib, cuda, fused):
    dev, host, want = fused
    first, second = _raw(lib, cuda, dev), _raw(lib, cuda, dev)
    assert first[0] == second[0] and first[0][1] > 0
    for a, b in zip(first[1], second[1]):
        assert np.array_equal(a, b)
    side = torch.cuda.Stream(device=cuda)                 # on the caller's current stream, whichever it is
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        other = _on_gpu(host, cuda)
        got = other.mesh(output="device")
    side.synchronize()
    assert got.vertices.device == dev.device
    mc.same_mesh(_to_host(got), want)


# ---- 13. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_and_leave_everything_alone(lib, cuda, fused):
    dev, host, want = fused
    nv, nt = want.vertices.shape[0], want.triangles.shape[0]
    st = C.c_void_p(_lib.stream_ptr(cuda))
    plain = Tsdf(dev.volume, coloured=False, device=cuda)
    need = int(lib.edv_tsdf_mesh_workspace(*dev.volume.dims))
    assert need == 16 * -(-dev.volume.voxels // fusion.TILE_VOXELS) + 6 * dev.volume.voxels
    assert lib.edv_tsdf_mesh_workspace(0, 4, 4) == 0 and lib.edv_tsdf_mesh_workspace(4, -1, 4) == 0 and lib.edv_tsdf_mesh_workspace(2048, 1024, 1024) == 0
    assert lib.edv_tsdf_mesh_workspace(2 ** 16, 2 ** 16, 1) == 0
    ws = torch.full((need + 8,), GUARD, dtype=torch.uint8, device=cuda)
    tot = torch.full((2,), -7, dtype=torch.int64, device=cuda)
    outs = [torch.full((n,), GUARD, dtype=torch.uint8, device=cuda) for n in (nv * 12 + 4, nv * 12 + 4, nv * 3, nt * 12 + 4)]
    pv, pn, pc, pt = (o.data_ptr() for o in outs)

    def vol(t=dev, **kw):
        v = t.struct()
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def count(v=None, total=tot.data_ptr(), w=ws.data_ptr(), nbytes=need):
        return lib.edv_tsdf_mesh_count(C.byref(v or vol()), 1.0, total, w, nbytes, st)

    def extract(v=None, w=ws.data_ptr(), nbytes=need, p=pv, n=pn, c=pc, vcap=nv, t=pt, tcap=nt):
        return lib.edv_tsdf_mesh_extract(C.byref(v or vol()), 1.0, w, nbytes, p, n, c, vcap, t, tcap, st)

    geometry = [dict(tsdf_dev=None), dict(weight_dev=None), dict(tsdf_dev=dev.tsdf.data_ptr() + 2), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=2048, ny=1024, nz=1024),
                dict(nx=2 ** 16, ny=2 ** 16, nz=1), dict(voxel=0.0), dict(voxel=float("nan")), dict(trunc=-1.0), dict(max_weight=float("inf"))]
    refused = [count(v=vol(**kw)) for kw in geometry] + [extract(v=vol(**kw)) for kw in geometry]
    refused += [lib.edv_tsdf_mesh_count(None, 1.0, tot.data_ptr(), ws.data_ptr(), need, st), lib.edv_tsdf_mesh_extract(None, 1.0, ws.data_ptr(), need, pv, pn, pc, nv, pt, nt, st)]
    refused += [count(total=None), count(total=tot.data_ptr() + 4), count(w=None), count(nbytes=need - 1), count(nbytes=0), count(w=ws.data_ptr() + 4)]
    refused += [extract(w=None), extract(nbytes=need - 1), extract(w=ws.data_ptr() + 4), extract(p=None), extract(t=None), extract(p=pv + 2), extract(n=pn + 1),
                extract(t=pt + 2), extract(vcap=-1), extract(tcap=-1), extract(vcap=2 ** 31), extract(v=vol(plain)), extract(p=None, vcap=0), extract(t=None, tcap=0)]
    assert all(r != 0 for r in refused), refused
    assert lib.edv_last_error()
    torch.cuda.synchronize()
    fc.same_state(dev.arrays(), host.arrays())
    fc.same_state(plain.arrays(), TsdfHost(dev.volume, coloured=False).arrays())
    assert (tot.cpu().numpy() == -7).all() and all((t.cpu().numpy() == GUARD).all() for t in [ws] + outs)
    # and the accepted forms of the same calls still work
    assert count() == 0 and extract() == 0 and extract(n=None, c=None) == 0 and extract(vcap=0, tcap=0) == 0 and extract(v=vol(plain), c=None) == 0
    assert extract(p=pv + 4, n=pn + 4, t=pt + 4) == 0
    torch.cuda.synchronize()
    assert tot.cpu().tolist() == [nv, nt]
    assert np.array_equal(outs[0].cpu().numpy()[4:].view(np.uint32).reshape(-1, 3), fc.bits(want.vertices))
    assert np.array_equal(outs[3].cpu().numpy()[4:].view(np.int32).reshape(-1, 3), want.triangles)
    # the Python layer refuses before it reaches the library
    for kw in (dict(min_weight=float("nan")), dict(min_weight=-1.0), dict(output="disk"), dict(normals="yes")):
        with pytest.raises(ValueError):
            dev.mesh(**kw)
    fc.same_state(dev.arrays(), host.arrays())


# ---- 14. end to end ------------------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


@pytest.fixture(scope="module")
def video(cuda):
    """The small ViT-S of tests/test_fusion_gpu.py at its network size, 54 frames: two windows."""
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
    synth.fill_module_(m)
    frames = long_video_frames(54, NET_H, NET_W)
    frames.setflags(write=False)
    return m.to(cuda), frames


def test_video_surface_as_a_mesh_equals_its_three_steps(cuda, video, tmp_path):
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
    steps = Tsdf(vol, coloured=True, device=cuda)
    steps.integrate(depth, spec, torch.from_numpy(frames.copy()).to(cuda))
    want = steps.mesh(min_weight=2.0)
    V, F = want.vertices.shape[0], want.triangles.shape[0]
    assert V > 0 and F > 0 and want.colors.shape == (V, 3) and want.normals.shape == (V, 3)
    assert 0 <= want.triangles.min() and want.triangles.max() == V - 1 and np.unique(want.triangles).size == V
    mc.same_mesh(model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0, surface="mesh"), want)
    on_device = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0, output="device", surface="mesh")
    assert isinstance(on_device, Mesh) and on_device.triangles.is_cuda
    mc.same_mesh(_to_host(on_device), want)
    # the mirror agrees on the same stitched video
    host = TsdfHost(vol)
    host.integrate(depth.cpu().numpy(), spec, frames)
    mc.same_mesh(want, host.mesh(min_weight=2.0))
    # a written .ply reads back equal
    path = str(tmp_path / "mesh.ply")
    fusion.write_mesh_ply(path, on_device)
    mc.same_mesh(fusion.read_mesh_ply(path), want)
    # the default and surface="points" are the point list they were
    pts = steps.surface(min_weight=2.0)
    fc.same_cloud(model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0), pts)
    fc.same_cloud(model.video_surface(frames, spec, vol, device="cuda:0", min_weight=2.0, surface="points"), pts)
    with pytest.raises(ValueError, match="surface"):
        model.video_surface(frames, spec, vol, surface="cubes")
