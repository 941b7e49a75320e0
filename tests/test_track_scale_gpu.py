"""Camera tracking with the depth scale as a seventh unknown on MI355X: ``fusion.icp_sums(..., scale=True)`` and the raw entry point against
``fusion.icp_sums_host`` as 37 uint64 patterns (the kernel runs the mirror's float64 operations and additions in the mirror's order, so nothing
needs a tolerance), its 29 shared values against the 6-column kernel's, ``Tsdf.track`` and ``Tsdf.track_clip`` with ``Track(scale=True)`` against
the mirror's, and ``model.video_surface`` against its own steps.  What the tracker converges to is checked on the mirror alone
(tests/test_track_scale_cpu.py)."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, cloud, fusion, synth
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Raycast, Tracked, Tsdf, TsdfHost, Volume
from tests import cloud_cases as cases
from tests import fusion_cases as fc
from tests import track_cases as tc
from tests import track_scale_cases as sc
from tests.golden.make_golden import long_video_frames

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64  # guard bytes on either side of a buffer; a multiple of 8, so the buffers keep their alignment

SIZES = [(1, 1), (5, 7), (16, 16), (17, 33), (40, 56)]   # one pixel, inside a wave, exactly one tile, ragged tiles, the scene's nine tiles


def _guesses():
    truth = tc.pose(tc.ROTATION, tc.TRANSLATION)
    return {"truth": truth, "identity": np.eye(4), "beyond": fusion.apply_twist(truth, np.concatenate([tc.CLIP_ROTATION, tc.CLIP_TRANSLATION])), "away": tc.AWAY}


# ---- 1. the sums, bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_sums_equal_the_host_mirror(cuda, size, step):
    """Every size with both steps, and per case both gains, both sources, with and without a mask, the four guesses: the 37 sums from host arrays
    and from tensors equal the mirror's, and the 29 the 6-column kernel also has equal that kernel's, all as bit patterns."""
    shape = (2,) + size
    model, views = tc.model()
    on_device = Raycast(torch.from_numpy(model.depth.copy()).to(cuda), torch.from_numpy(model.normals.copy()).to(cuda), None)
    some = 0
    for i, (gain, source, kind) in enumerate(itertools.product((1.0, 1.02), cloud.SOURCES, ("none", "shared"))):
        depth, mask = tc.live(shape, source, kind, seed=100 + 8 * SIZES.index(size) + i)
        on_gpu = torch.from_numpy(depth).to(cuda)
        for name, T in _guesses().items():
            spec = dataclasses.replace(tc.live_spec(shape, T, step, source, mask), gain=gain)
            want = fusion.icp_sums_host(depth, spec, model, views, 0.1, 1, scale=True)
            got = fusion.icp_sums(depth, spec, model, views, 0.1, 1, scale=True)                       # host arrays in
            assert got.shape == (37,) and got.dtype == np.float64
            assert np.array_equal(tc.bits(got), tc.bits(want)), (gain, source, kind, name, got, want)
            again = fusion.icp_sums(on_gpu, spec, on_device, views, 0.1, frame=1, scale=True)          # tensors in: used in place
            assert np.array_equal(tc.bits(again), tc.bits(want)), (gain, source, kind, name)
            six = fusion.icp_sums(on_gpu, spec, on_device, views, 0.1, 1, scale=False)
            assert six.shape == (29,) and np.array_equal(tc.bits(got[sc.SHARED]), tc.bits(six)), (gain, source, kind, name)
            if name == "away":
                assert np.array_equal(tc.bits(want), tc.bits(np.zeros(37)))
            some += int(want[36])
    print(f"\n[{size} step {step}] {some} pairs over the cases")
    if size == (40, 56):
        assert some > 4000


# ---- 2. the raw entry point ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(cuda):
    """(a prepared ``fusion._IcpDevice`` with the seventh column, the estimate's 21 doubles, the mirror's sums) of the ragged 17 x 33 case, three
    frames, frame 2, a shared mask, gain 1.02."""
    shape = (3, 17, 33)
    depth, mask = tc.live(shape, "disparity", "shared", seed=40)
    model, views = tc.model()
    spec = dataclasses.replace(tc.live_spec(shape, np.eye(4), 1, "disparity", mask), gain=1.02)
    ctx = fusion._IcpDevice(depth, spec, model, views, 0.1, 2, device=cuda, scale=True)
    want = fusion.icp_sums_host(depth, spec, model, views, 0.1, 2, scale=True)
    assert want[36] > 100
    return ctx, fusion._estimate(ctx, spec, 2), want


def _raw(lib, cuda, ctx, estimate, stream=None, **kw):
    """The entry point on poisoned buffers: the sums and the workspace lie between PAD guard bytes, the workspace itself is filled with 0xFF
    (NaN patterns).  Returns (the return value, the two buffers' bytes with the guards on)."""
    st = C.c_void_p(_lib.stream_ptr(cuda) if stream is None else stream.cuda_stream)
    need = int(lib.edv_icp_scaled_workspace(ctx.sel.h, ctx.sel.w, ctx.sel.step))
    sums = torch.full((PAD + 37 * 8 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    ws = torch.full((PAD + need + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    ws[PAD:PAD + need] = 0xFF
    args = dict(sel=C.byref(ctx.sel), frame=ctx.frame, live=(C.c_double * 21)(*estimate), model=ctx.model_cam, depth=ctx.depth.data_ptr(), normals=ctx.normals.data_ptr(),
                mh=ctx.size[0], mw=ctx.size[1], max_dist2=ctx.max_dist2, sums=sums.data_ptr() + PAD, ws=ws.data_ptr() + PAD, ws_bytes=need)
    for k, val in kw.items():
        args[k] = val(args[k]) if callable(val) else val
    ret = lib.edv_icp_scaled_sums(*args.values(), st)
    torch.cuda.synchronize()
    return ret, sums.cpu().numpy(), ws.cpu().numpy()


def test_guards_stay_and_a_poisoned_workspace_changes_nothing(lib, cuda, scene):
    ctx, live, want = scene
    ret, sums, ws = _raw(lib, cuda, ctx, live)
    assert ret == 0, lib.edv_last_error()
    assert np.array_equal(sums[PAD:-PAD].view(np.uint64), tc.bits(want))
    assert (sums[:PAD] == GUARD).all() and (sums[-PAD:] == GUARD).all() and (ws[:PAD] == GUARD).all() and (ws[-PAD:] == GUARD).all()
    tiles = ws[PAD:-PAD].view(np.uint64).reshape(-1, 37)
    assert tiles.shape[0] == -(-17 * 33 // 256) and not (tiles == np.uint64(2 ** 64 - 1)).any()     # every slot was written
    assert np.ascontiguousarray(tiles[:, 36]).view(np.float64).sum() == want[36]
    ret2, sums2, ws2 = _raw(lib, cuda, ctx, live)                                                    # two calls, the same bytes
    assert ret2 == 0 and np.array_equal(sums, sums2) and np.array_equal(ws, ws2)
    side = torch.cuda.Stream(device=cuda)                                                            # on whichever stream it is given
    side.wait_stream(torch.cuda.current_stream(cuda))
    ret3, sums3, _ = _raw(lib, cuda, ctx, live, stream=side)
    assert ret3 == 0 and np.array_equal(sums, sums3)
    ret4, sums4, _ = _raw(lib, cuda, ctx, live, ws_bytes=lambda b: b + 8, sums=lambda p: p + 8)      # a larger workspace and any 8-byte alignment are accepted
    assert ret4 == 0 and np.array_equal(sums4[PAD + 8:PAD + 8 + 296], sums[PAD:-PAD]) and (sums4[:PAD + 8] == GUARD).all()


def test_the_entry_point_refuses_and_leaves_everything_alone(lib, cuda, scene):
    ctx, live, want = scene

    def sel(**kw):
        s = _lib.CloudSelection.from_buffer_copy(ctx.sel)
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    bad = [dict(sel=None), dict(live=None), dict(model=None), dict(depth=None), dict(normals=None), dict(sums=None), dict(ws=None), dict(frame=-1), dict(frame=3),
           dict(sel=sel(step=0)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)), dict(sel=sel(h=0)), dict(sel=sel(mode=2)), dict(sel=sel(mask_stride=5)),
           dict(mh=0), dict(mw=-1), dict(mh=2 ** 16, mw=2 ** 15), dict(max_dist2=-1.0), dict(max_dist2=float("nan")), dict(max_dist2=float("inf")),
           dict(ws_bytes=lambda b: b - 1), dict(ws=lambda p: p + 4), dict(sums=lambda p: p + 4), dict(depth=lambda p: p + 2)]
    for kw in bad:
        ret, sums, ws = _raw(lib, cuda, ctx, live, **kw)
        assert ret != 0, kw
        assert lib.edv_last_error(), kw
        assert (sums == GUARD).all() and (ws[:PAD] == GUARD).all() and (ws[-PAD:] == GUARD).all() and (ws[PAD:-PAD] == 0xFF).all(), kw    # nothing was launched
    ret, sums, _ = _raw(lib, cuda, ctx, live)                                                        # and the same call, unchanged, still works
    assert ret == 0 and np.array_equal(sums[PAD:-PAD].view(np.uint64), tc.bits(want))


# ---- 3. a track and a clip ----------------------------------------------------------------------------------------------------------------------
def test_track_equals_the_host_mirror(cuda):
    host = tc.fused()
    dev = Tsdf(tc.volume(), coloured=False, device=cuda)
    dev.integrate(tc.surface(), tc.spec())
    fc.same_state(dev.arrays(), host.arrays())
    for s in (1.0, 1.05):
        live, truth = sc.single(s)
        for spec, track in ((tc.spec(), tc.track(scale=True)), (tc.spec(), tc.track(scale=True, iterations=1)), (tc.spec(pose=tc.AWAY), tc.track(scale=True)),
                            (tc.spec(), tc.track(scale=True, max_scale_step=0.01))):
            want = host.track(live, spec, track)
            assert len(want) == 5
            for depth in (live, torch.from_numpy(live.copy()).to(cuda)):
                got = dev.track(depth, spec, track)
                assert len(got) == 5 and got[0].dtype == np.float64 and np.array_equal(tc.bits(got[0]), tc.bits(want[0]))
                assert got[1] == want[1] and np.array_equal(tc.bits(got[2]), tc.bits(want[2])) and got[3] is want[3]
                assert isinstance(got[4], float) and np.array_equal(tc.bits(got[4]), tc.bits(want[4]))
        want = host.track(live, tc.spec(), tc.track(scale=True))
        assert not want[3] and abs(want[4] / s - 1.0) <= 0.005                                       # the track the CPU test measures
        assert max(a / b for a, b in zip(tc.errors(want[0], truth), tc.errors(np.eye(4), truth))) <= 0.1
    assert host.track(sc.single(1.05)[0], tc.spec(pose=tc.AWAY), tc.track(scale=True))[3:] == (True, 1.0)
    assert len(dev.track(sc.single(1.0)[0], tc.spec(), tc.track())) == 4                            # without the option: the four values
    fc.same_state(dev.arrays(), host.arrays())                                                       # tracking only reads the volume


def test_track_clip_equals_the_host_mirror(cuda):
    depth, _, scales = sc.clip()
    track = tc.track(scale=True)
    host, dev = TsdfHost(tc.volume(), coloured=False), Tsdf(tc.volume(), coloured=False, device=cuda)
    want = host.track_clip(depth, tc.spec(), track)
    got = dev.track_clip(depth, tc.spec(), track)
    assert isinstance(got, Tracked)
    sc.same_tracked(got, want)
    assert not want.lost.any() and want.scales[0] == 1.0 and (np.abs(want.scales / scales - 1.0) <= 0.005).all()
    fc.same_state(dev.arrays(), host.arrays())
    # a coloured volume, a tensor clip, a mask per frame, and a frame that is lost on the way (it sees nothing: all zeros)
    rng = np.random.default_rng(8)
    holed = depth.copy()
    holed[2] = 0.0
    frames = rng.integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    spec = tc.spec(mask=rng.random(depth.shape) < 0.9)
    host, dev = TsdfHost(tc.volume()), Tsdf(tc.volume(), device=cuda)
    want = host.track_clip(holed, spec, track, frames)
    sc.same_tracked(dev.track_clip(torch.from_numpy(holed).to(cuda), spec, track, torch.from_numpy(frames).to(cuda)), want)
    assert list(want.lost) == [False, False, True, False, False] and np.array_equal(want.poses[2], want.poses[1]) and want.scales[2] == want.scales[1]
    fc.same_state(dev.arrays(), host.arrays())


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


@pytest.fixture(scope="module")
def video(cuda):
    """The video of tests/test_track_gpu.py: its small ViT-S at its network size, 54 frames (two windows) of one still frame whose brightness
    wanders by a few levels."""
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
    synth.fill_module_(m)
    still = long_video_frames(54, NET_H, NET_W)[:1].astype(np.int64)
    frames = np.clip(still + (np.arange(54) % 5)[:, None, None, None], 0, 255).astype(np.uint8)
    frames.setflags(write=False)
    return m.to(cuda), frames


def test_video_surface_with_a_scaled_track_equals_its_steps(cuda, video):
    """The plumbing, as in tests/test_track_gpu.py (the depth of synthetic weights is no surface): with ``Track(scale=True)`` the call does exactly
    what its steps do and hands back the scales; without it, what it did before."""
    model, frames = video
    depth = model.infer_video_depth(frames, device="cuda:0", stitch="device", output="device")
    z = cloud.lift_host(depth.cpu().numpy(), Cloud(K=np.eye(3)), None).points[:, 2]
    scale = float(np.median(z))
    spec = Cloud(K=cases.intrinsics(NET_H, NET_W), pose=fc.nearby_poses(1, seed=1, scale=scale)[0], far=2.0 * scale)
    points = cloud.lift_host(depth.cpu().numpy()[:1], spec, None).points
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    voxel = extent / 40.0
    vol = Volume.bounding(points, voxel, margin=0.25 * extent, trunc=12.0 * voxel)
    assert max(vol.dims) <= 64
    plain = dict(near=0.0, far=2.0 * scale, step=0.25 * voxel, max_dist=0.5 * scale, min_pairs=16)
    track = fusion.Track(**plain, scale=True, max_scale_step=0.5)                                    # at the default quarter every later frame of this depth is lost
    steps = Tsdf(vol, coloured=True, device=cuda)
    want_track = steps.track_clip(depth, spec, track, torch.from_numpy(frames.copy()).to(cuda))
    print(f"\n{int(want_track.lost.sum())} of 54 frames lost; pairs {want_track.pairs[1:].min()} .. {want_track.pairs.max()}; scales {want_track.scales.min():.4f} .. {want_track.scales.max():.4f}")
    assert want_track.poses.shape == (54, 4, 4) and not want_track.lost[0] and want_track.scales.shape == (54,) and want_track.scales[0] == 1.0
    assert np.isfinite(want_track.scales).all() and (want_track.scales > 0.0).all()
    assert not want_track.lost[1:].all() and (want_track.scales != 1.0).any()                        # some frame was found and integrated at a scale of its own
    want = steps.surface(min_weight=1.0)
    assert len(want) > 0
    got, tracked = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=1.0, track=track)
    fc.same_cloud(got, want)
    sc.same_tracked(tracked, want_track)
    steps = Tsdf(vol, coloured=True, device=cuda)                                                    # without the option: as before, and no scales
    want_track = steps.track_clip(depth, spec, fusion.Track(**plain), torch.from_numpy(frames.copy()).to(cuda))
    got, tracked = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=1.0, track=fusion.Track(**plain))
    assert tracked.scales is None and want_track.scales is None
    fc.same_cloud(got, steps.surface(min_weight=1.0))
    assert np.array_equal(tc.bits(tracked.poses), tc.bits(want_track.poses)) and np.array_equal(tracked.lost, want_track.lost)
    assert np.array_equal(tracked.pairs, want_track.pairs) and np.array_equal(tc.bits(tracked.rms), tc.bits(want_track.rms))
