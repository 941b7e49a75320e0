"""Camera tracking by colour too on MI355X: ``fusion.icp_colour_sums`` and the raw entry point against ``fusion.icp_colour_sums_host`` as 2 x 29 or
2 x 37 uint64 patterns (the kernel runs the mirror's float64 operations and additions in the mirror's order, so nothing needs a tolerance), its
geometric block against the kernels without colour, ``Tsdf.track`` and ``Tsdf.track_clip`` with ``Track(colour=...)`` against the mirror's, and
``model.video_surface`` end to end.  What the term computes and what the tracker converges to is checked on the mirror alone
(tests/test_track_colour_cpu.py)."""
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
from tests import track_colour_cases as cc
from tests.golden.make_golden import long_video_frames

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64  # guard bytes on either side of a buffer; a multiple of 8, so the buffers keep their alignment

# one partial tile, exactly one tile, the scene's nine tiles with a ragged last one, and at step 3 a grid of 6 x 8 from ragged frames
SHAPES = [((7, 9), 1), ((16, 16), 1), ((40, 56), 1), ((17, 23), 3)]


def _guesses():
    truth = tc.pose(tc.ROTATION, tc.TRANSLATION)
    return {"truth": truth, "identity": np.eye(4), "aside": tc.pose((0.0, 0.0, 0.0), (0.003, -0.003, 0.0)),
            "beyond": fusion.apply_twist(truth, np.concatenate([tc.CLIP_ROTATION, tc.CLIP_TRANSLATION])), "away": tc.AWAY}


def _models():
    """The model views of the CPU test's edges: the live camera's, one with a miss in the middle, one of another size and K, one whose K has
    skew, the middle of the view (hits up to its border) and one a pixel wide."""
    same, views = cc.model()
    depth = same.depth.copy()
    depth[0, 20, 30] = 0.0
    return {"same": (same, views), "holed": (Raycast(depth, same.normals, same.colors), views), "other": cc.model(size=tc.OTHER_SIZE, intrinsics=tc.OTHER_K),
            "skew": cc.model(intrinsics=cc.SKEW_K), "middle": cc.model(size=(30, 40), intrinsics=(60.0, 0.0, 20.0, 0.0, 60.0, 15.0, 0.0, 0.0, 1.0)),
            "narrow": cc.model(size=(tc.H, 1), intrinsics=(60.0, 0.0, 0.5, 0.0, 60.0, 20.0, 0.0, 0.0, 1.0))}


def _on(cuda, model):
    return Raycast(*(torch.from_numpy(a.copy()).to(cuda) for a in (model.depth, model.normals, model.colors)))


# ---- 1. the sums, bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,step", SHAPES, ids=str)
def test_sums_equal_the_host_mirror(cuda, size, step):
    """Frame 1 of a two-frame clip.  Per shape both sources, with and without a mask, both column counts and the five guesses against the live
    camera's model: the 2 T sums from host arrays and from tensors equal the mirror's, and the geometric block equals the kernel without
    colour, all as bit patterns."""
    shape = (2,) + size
    model, views = cc.model()
    on_device = _on(cuda, model)
    pairs = np.zeros(2, np.int64)
    for i, (source, kind, scale) in enumerate(itertools.product(cloud.SOURCES, ("none", "shared"), (False, True))):
        depth, mask, frames = cc.live(shape, source, kind, seed=300 + 8 * SHAPES.index((size, step)) + i)
        depth_d, frames_d = torch.from_numpy(depth).to(cuda), torch.from_numpy(frames).to(cuda)
        for name, T in _guesses().items():
            spec = dataclasses.replace(tc.live_spec(shape, T, step, source, mask), gain=1.02 if scale else 1.0)
            want = fusion.icp_colour_sums_host(depth, frames, spec, model, views, 0.1, 1, scale=scale)
            got = fusion.icp_colour_sums(depth, frames, spec, model, views, 0.1, 1, scale=scale)                   # host arrays in
            assert got.shape == (2, 37 if scale else 29) and got.dtype == np.float64
            assert np.array_equal(tc.bits(got), tc.bits(want)), (source, kind, scale, name, got, want)
            again = fusion.icp_colour_sums(depth_d, frames_d, spec, on_device, views, 0.1, frame=1, scale=scale)   # tensors in: used in place
            assert np.array_equal(tc.bits(again), tc.bits(want)), (source, kind, scale, name)
            alone = fusion.icp_sums(depth_d, spec, on_device, views, 0.1, 1, scale=scale)                          # the kernel without colour
            assert np.array_equal(tc.bits(got[0]), tc.bits(alone)), (source, kind, scale, name)
            if name == "away":
                assert np.array_equal(tc.bits(want), tc.bits(np.zeros_like(want)))
            pairs += want[:, -1].astype(np.int64)
    print(f"\n[{size} step {step}] {pairs[0]} pairs over the cases, {pairs[1]} with colour")
    assert pairs[0] > pairs[1] > 0
    if size == (40, 56):
        assert pairs[1] > 8000


@pytest.mark.parametrize("which", ["holed", "other", "skew", "middle", "narrow"])
def test_sums_equal_the_host_mirror_at_the_model_edges(cuda, which):
    """The model views of the CPU test's edges, at the scene's own size and at the ragged 17 x 23 with step 3, live depth with NaN, 0 and Inf."""
    model, views = _models()[which]
    on_device = _on(cuda, model)
    pairs, colour_pairs = 0, 0
    for (size, step), scale in itertools.product((((40, 56), 1), ((17, 23), 3)), (False, True)):
        shape = (2,) + size
        depth, mask, frames = cc.live(shape, "depth", "shared", seed=40 + step)
        depth[1, 2, 3:6], depth[1, 5, 1], depth[1, 6, 6] = np.nan, np.inf, 0.0
        for name in ("identity", "aside", "truth"):
            spec = tc.live_spec(shape, _guesses()[name], step, "depth", mask)
            want = fusion.icp_colour_sums_host(depth, frames, spec, model, views, 0.1, 1, scale=scale)
            got = fusion.icp_colour_sums(depth, frames, spec, on_device, views, 0.1, 1, scale=scale)
            assert np.array_equal(tc.bits(got), tc.bits(want)), (which, size, scale, name, got, want)
            assert np.isfinite(got).all()
            pairs, colour_pairs = pairs + int(want[0, -1]), colour_pairs + int(want[1, -1])
    assert pairs > 100 and (colour_pairs == 0) == (which == "narrow")


# ---- 2. the raw entry point ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(cuda):
    """(a prepared ``fusion._IcpDevice`` with colour and the seventh column, the estimate's 21 doubles, the mirror's sums) of the ragged 17 x 23
    case at step 1, three frames, frame 2, a shared mask, gain 1.02, disparity."""
    shape = (3, 17, 23)
    depth, mask, frames = cc.live(shape, "disparity", "shared", seed=41)
    model, views = cc.model()
    spec = dataclasses.replace(tc.live_spec(shape, tc.pose((0.0, 0.0, 0.0), (0.003, -0.003, 0.0)), 1, "disparity", mask), gain=1.02)
    ctx = fusion._IcpDevice(depth, spec, model, views, 0.1, 2, device=cuda, scale=True, frames=frames)
    want = fusion.icp_colour_sums_host(depth, frames, spec, model, views, 0.1, 2, scale=True)
    assert want[0, -1] > 100 and want[1, -1] > 100
    return ctx, fusion._estimate(ctx, spec, 2), want


def _raw(lib, cuda, ctx, estimate, stream=None, **kw):
    """The entry point on poisoned buffers: the sums and the workspace lie between PAD guard bytes, the workspace itself is filled with 0xFF
    (NaN patterns).  Returns (the return value, the two buffers' bytes with the guards on)."""
    st = C.c_void_p(_lib.stream_ptr(cuda) if stream is None else stream.cuda_stream)
    need = int(lib.edv_icp_colour_workspace(ctx.sel.h, ctx.sel.w, ctx.sel.step, 7))
    sums = torch.full((PAD + 74 * 8 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    ws = torch.full((PAD + need + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    ws[PAD:PAD + need] = 0xFF
    args = dict(sel=C.byref(ctx.sel), frame=ctx.frame, frames=ctx.frames.data_ptr(), live=(C.c_double * 21)(*estimate), model=ctx.model_cam, depth=ctx.depth.data_ptr(),
                normals=ctx.normals.data_ptr(), colors=ctx.colors.data_ptr(), mh=ctx.size[0], mw=ctx.size[1], max_dist2=ctx.max_dist2, cols=7, sums=sums.data_ptr() + PAD,
                ws=ws.data_ptr() + PAD, ws_bytes=need)
    for k, val in kw.items():
        args[k] = val(args[k]) if callable(val) else val
    ret = lib.edv_icp_colour_sums(*args.values(), st)
    torch.cuda.synchronize()
    return ret, sums.cpu().numpy(), ws.cpu().numpy()


def test_guards_stay_and_a_poisoned_workspace_changes_nothing(lib, cuda, scene):
    ctx, live, want = scene
    ret, sums, ws = _raw(lib, cuda, ctx, live)
    assert ret == 0, lib.edv_last_error()
    assert np.array_equal(sums[PAD:-PAD].view(np.uint64), tc.bits(want).reshape(-1))
    assert (sums[:PAD] == GUARD).all() and (sums[-PAD:] == GUARD).all() and (ws[:PAD] == GUARD).all() and (ws[-PAD:] == GUARD).all()
    tiles = ws[PAD:-PAD].view(np.uint64).reshape(-1, 74)
    assert tiles.shape[0] == -(-17 * 23 // 256) and not (tiles == np.uint64(2 ** 64 - 1)).any()     # every slot was written
    assert np.ascontiguousarray(tiles[:, 36]).view(np.float64).sum() == want[0, 36] and np.ascontiguousarray(tiles[:, 73]).view(np.float64).sum() == want[1, 36]
    ret2, sums2, ws2 = _raw(lib, cuda, ctx, live)                                                    # two calls, the same bytes
    assert ret2 == 0 and np.array_equal(sums, sums2) and np.array_equal(ws, ws2)
    side = torch.cuda.Stream(device=cuda)                                                            # on whichever stream it is given
    side.wait_stream(torch.cuda.current_stream(cuda))
    ret3, sums3, _ = _raw(lib, cuda, ctx, live, stream=side)
    assert ret3 == 0 and np.array_equal(sums, sums3)
    ret4, sums4, _ = _raw(lib, cuda, ctx, live, ws_bytes=lambda b: b + 8, sums=lambda p: p + 8)      # a larger workspace and any 8-byte alignment are accepted
    assert ret4 == 0 and np.array_equal(sums4[PAD + 8:PAD + 8 + 592], sums[PAD:-PAD]) and (sums4[:PAD + 8] == GUARD).all()
    ret5, sums5, ws5 = _raw(lib, cuda, ctx, live, cols=6)                                            # six columns in the same buffers: 58 sums, the rest untouched
    assert ret5 == 0 and (sums5[PAD + 58 * 8:] == GUARD).all() and (ws5[PAD + tiles.shape[0] * 58 * 8:-PAD] == 0xFF).all()
    six = sums5[PAD:PAD + 58 * 8].view(np.float64).reshape(2, 29)
    assert np.array_equal(six[:, -1], want[:, -1]) and np.array_equal(tc.bits(six[:, 24:27]), tc.bits(want[:, 31:34]))   # J_3..J_5 times the residual: positions 24..26 of 29, 31..33 of 37
    # and through the context's own buffers, which nothing ever cleared
    assert np.array_equal(ctx.sums(live).reshape(2, -1).view(np.uint64), tc.bits(want))


def test_the_entry_point_refuses_and_leaves_everything_alone(lib, cuda, scene):
    ctx, live, want = scene

    def sel(**kw):
        s = _lib.CloudSelection.from_buffer_copy(ctx.sel)
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    bad = [dict(sel=None), dict(frames=None), dict(live=None), dict(model=None), dict(depth=None), dict(normals=None), dict(colors=None), dict(sums=None), dict(ws=None),
           dict(cols=5), dict(cols=8), dict(cols=0), dict(frame=-1), dict(frame=3),
           dict(sel=sel(step=0)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)), dict(sel=sel(h=0)), dict(sel=sel(mode=2)), dict(sel=sel(mask_stride=5)),
           dict(mh=0), dict(mw=-1), dict(mh=2 ** 16, mw=2 ** 15), dict(max_dist2=-1.0), dict(max_dist2=float("nan")), dict(max_dist2=float("inf")),
           dict(ws_bytes=lambda b: b - 1), dict(ws=lambda p: p + 4), dict(sums=lambda p: p + 4), dict(depth=lambda p: p + 2)]
    for kw in bad:
        ret, sums, ws = _raw(lib, cuda, ctx, live, **kw)
        assert ret != 0, kw
        assert lib.edv_last_error(), kw
        assert (sums == GUARD).all() and (ws[:PAD] == GUARD).all() and (ws[-PAD:] == GUARD).all() and (ws[PAD:-PAD] == 0xFF).all(), kw    # nothing was launched
    ret, sums, _ = _raw(lib, cuda, ctx, live)                                                        # and the same call, unchanged, still works
    assert ret == 0 and np.array_equal(sums[PAD:-PAD].view(np.uint64), tc.bits(want).reshape(-1))


# ---- 3. a track and a clip ----------------------------------------------------------------------------------------------------------------------
def _same_track(got, want):
    assert len(got) == len(want) and got[0].dtype == np.float64 and np.array_equal(tc.bits(got[0]), tc.bits(want[0]))
    assert got[1] == want[1] and np.array_equal(tc.bits(got[2]), tc.bits(want[2])) and got[3] is want[3]
    if len(want) == 5:
        assert isinstance(got[4], float) and np.array_equal(tc.bits(got[4]), tc.bits(want[4]))


def test_track_equals_the_host_mirror(cuda):
    for kind in ("curved", "plane"):
        host = cc.fused(kind)
        dev = Tsdf(tc.volume(), device=cuda)
        dev.integrate(cc.shape_of(kind), tc.spec(), cc.texture())
        fc.same_state(dev.arrays(), host.arrays())
        motion = (tc.ROTATION, tc.TRANSLATION) if kind == "curved" else (cc.ROLL, cc.ROLL_SLIDE)
        live, frames, truth = cc.single(kind, *motion)
        for spec, track in ((tc.spec(), tc.track(colour=cc.WEIGHT)), (tc.spec(), tc.track(colour=cc.WEIGHT, scale=True)), (tc.spec(), tc.track(colour=0.01, iterations=1)),
                            (tc.spec(pose=tc.AWAY), tc.track(colour=cc.WEIGHT)), (tc.spec(), tc.track(colour=cc.WEIGHT, min_pairs=tc.H * tc.W))):
            want = host.track(live, spec, track, frames=frames)
            _same_track(dev.track(live, spec, track, frames=frames), want)
            _same_track(dev.track(torch.from_numpy(live.copy()).to(cuda), spec, track, frames=torch.from_numpy(frames.copy()).to(cuda)), want)
        want = host.track(live, tc.spec(), tc.track(colour=cc.WEIGHT), frames=frames)                # the track the CPU test measures
        assert not want[3] and max(a / b for a, b in zip(tc.errors(want[0], truth), tc.errors(np.eye(4), truth))) <= 0.1
        _same_track(dev.track(live, tc.spec(), tc.track(), frames=frames), host.track(live, tc.spec(), tc.track()))   # without the weight: the frames are not looked at
        with pytest.raises(ValueError):
            dev.track(live, tc.spec(), tc.track(colour=cc.WEIGHT))
        fc.same_state(dev.arrays(), host.arrays())                                                   # tracking only reads the volume
    with pytest.raises(ValueError):
        Tsdf(tc.volume(), coloured=False, device=cuda).track(live, tc.spec(), tc.track(colour=cc.WEIGHT), frames=frames)


@pytest.mark.parametrize("scale", [False, True])
def test_track_clip_equals_the_host_mirror(cuda, scale):
    depth, frames, _ = cc.clip()
    track = tc.track(colour=cc.WEIGHT, scale=scale)
    host, dev = TsdfHost(tc.volume()), Tsdf(tc.volume(), device=cuda)
    want = host.track_clip(depth, tc.spec(), track, frames)
    got = dev.track_clip(depth, tc.spec(), track, frames)
    assert isinstance(got, Tracked) and not want.lost.any()
    cc.same_tracked(got, want)
    fc.same_state(dev.arrays(), host.arrays())
    # a tensor clip, a mask per frame, and a frame that is lost on the way (it sees nothing: all zeros)
    rng = np.random.default_rng(8)
    holed = depth.copy()
    holed[2] = 0.0
    spec = tc.spec(mask=rng.random(depth.shape) < 0.9)
    host, dev = TsdfHost(tc.volume()), Tsdf(tc.volume(), device=cuda)
    want = host.track_clip(holed, spec, track, frames)
    cc.same_tracked(dev.track_clip(torch.from_numpy(holed).to(cuda), spec, track, torch.from_numpy(frames.copy()).to(cuda)), want)
    assert list(want.lost) == [False, False, True, False, False] and np.array_equal(want.poses[2], want.poses[1])
    fc.same_state(dev.arrays(), host.arrays())
    with pytest.raises(ValueError):
        Tsdf(tc.volume(), coloured=False, device=cuda).track_clip(depth, tc.spec(), track)


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


def test_video_surface_with_a_colour_track(cuda, video):
    """The plumbing, as in tests/test_track_gpu.py: with ``Track(colour=...)``, with and without the scale, the call does exactly what its steps
    do, and no frame is lost.  The depth of synthetic weights is no surface and changes from frame to frame: geometry alone loses 49 of the 54
    frames here (6 iterations; 31 with 2).  But the video is one still frame, and its colours say that the camera stands still: with the weight
    at a tenth of the scene's unit per level they hold it.  Measured: nothing lost with weights of 0.05, 0.1 and 0.2 units and 2 or 3 iterations,
    but for 4 frames at 0.05, 3 iterations and the scale; 46 lost at 0.001."""
    model, frames = video
    depth = model.infer_video_depth(frames, device="cuda:0", stitch="device", output="device")
    z = cloud.lift_host(depth.cpu().numpy(), Cloud(K=np.eye(3)), None).points[:, 2]
    unit = float(np.median(z))
    spec = Cloud(K=cases.intrinsics(NET_H, NET_W), pose=fc.nearby_poses(1, seed=1, scale=unit)[0], far=2.0 * unit)
    points = cloud.lift_host(depth.cpu().numpy()[:1], spec, None).points
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    voxel = extent / 40.0
    vol = Volume.bounding(points, voxel, margin=0.25 * extent, trunc=12.0 * voxel)
    assert max(vol.dims) <= 64
    for scale in (False, True):
        track = fusion.Track(near=0.0, far=2.0 * unit, step=0.25 * voxel, max_dist=0.5 * unit, min_pairs=16, iterations=2, colour=0.1 * unit, scale=scale, max_scale_step=0.5)
        steps = Tsdf(vol, coloured=True, device=cuda)
        want_track = steps.track_clip(depth, spec, track, torch.from_numpy(frames.copy()).to(cuda))
        print(f"\n[scale {scale}] {int(want_track.lost.sum())} of 54 frames lost; pairs {want_track.pairs[1:].min()} .. {want_track.pairs.max()}")
        want = steps.surface(min_weight=1.0)
        assert len(want) > 0
        got, tracked = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=1.0, track=track)
        assert isinstance(tracked, Tracked) and tracked.poses.shape == (54, 4, 4) and (tracked.scales is not None) == scale
        assert not tracked.lost.any()
        fc.same_cloud(got, want)
        cc.same_tracked(tracked, want_track)
