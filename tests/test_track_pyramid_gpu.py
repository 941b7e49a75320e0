"""Coarse-to-fine tracking on MI355X: ``fusion.depth_pyramid`` and ``fusion.rgb_pyramid`` against their numpy mirrors as bit patterns, the raw entry
points between guard bytes, ``Tsdf.track`` and ``Tsdf.track_clip`` with ``Track(pyramid=...)`` against ``TsdfHost`` (poses, pairs, rms, lost and
scales as bit patterns: the levels, the ray-casts and the sums all run the mirror's operations in the mirror's order, so nothing needs a
tolerance), and ``model.video_surface`` end to end.  What the rule computes and what the tracker gains is checked on the mirror alone
(tests/test_track_pyramid_cpu.py)."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import endodav_amd
from endodav_amd import _lib, cloud, fusion, synth
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Tracked, Tsdf, TsdfHost, Volume
from tests import cloud_cases as cases
from tests import fusion_cases as fc
from tests import pyramid_cases as pc
from tests import track_cases as tc
from tests import track_colour_cases as cc
from tests.golden.make_golden import long_video_frames

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 64  # guard bytes on either side of a buffer; a multiple of 4, so the buffers keep their alignment


def _sizes():
    """One output pixel; odd sizes over two levels; exactly one tile of the kernel with every level it can make; tiles crossed raggedly in both
    axes, again with every level; the scene's own size."""
    most = fusion.PYRAMID_MAX_LEVELS
    side = pc.tile(most)
    return [((2, 2), 1), ((7, 9), 2), ((side, side), most - 1), ((side + 1, 2 * side + 1), most - 1), ((tc.H, tc.W), 2)]


# ---- 8. the exports -------------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_pyramid(lib):
    for name in ("edv_depth_pyramid", "edv_rgb_pyramid", "edv_pyramid_max_levels", "edv_pyramid_pixels"):
        assert hasattr(lib, name)
    most = lib.edv_pyramid_max_levels()
    assert most >= 4 and fusion.PYRAMID_MAX_LEVELS == most
    offsets = (C.c_int64 * 3)()
    assert lib.edv_pyramid_pixels(40, 56, 3, offsets) == 20 * 28 + 10 * 14 + 5 * 7 and list(offsets) == [0, 560, 700]
    assert lib.edv_pyramid_pixels(7, 9, 2, None) == 3 * 4 + 1 * 2
    poisoned = (C.c_int64 * 3)(-7, -7, -7)
    for h, w, levels in ((0, 9, 1), (7, 0, 1), (7, 9, 0), (7, 9, most), (7, 9, 3), (1, 9, 1), (2 ** 16, 2 ** 15, 1)):
        assert lib.edv_pyramid_pixels(h, w, levels, poisoned) == 0 and list(poisoned) == [-7, -7, -7], (h, w, levels)


# ---- 6. the levels, bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_depth_levels_equal_the_host_mirror(cuda, case):
    """Both sources, with and without a mask, NaN, Inf, 0 and negative values among the inputs, ``jump`` in {0, 0.05, inf}, frame 1 of two: the
    levels from host arrays and from tensors, as numpy arrays and as tensors, equal the mirror's as bit patterns."""
    size, levels = _sizes()[case]
    shape = (2,) + size
    valid = split = 0
    for i, (source, kind, jump) in enumerate(itertools.product(cloud.SOURCES, ("none", "shared"), pc.JUMPS)):
        depth, mask = pc.frame(shape, source, kind, seed=20 * case + i)
        spec = dataclasses.replace(tc.live_spec(shape, np.eye(4), 1, source, mask), gain=1.02)
        want = fusion.depth_pyramid_host(depth, spec, levels, jump=jump, frame=1)
        got = fusion.depth_pyramid(depth, spec, levels, jump=jump, frame=1)                                          # a host array in, arrays out
        assert len(got) == levels and all(isinstance(g, np.ndarray) and g.dtype == np.float32 for g in got)
        again = fusion.depth_pyramid(torch.from_numpy(depth).to(cuda), spec, levels, jump=jump, frame=1, output="device")   # a tensor in, tensors out
        assert all(isinstance(g, torch.Tensor) and g.device == cuda and g.dtype == torch.float32 for g in again)
        for l, (g, a, w) in enumerate(zip(got, again, want)):
            assert g.shape == w.shape == tuple(a.shape) == (size[0] >> (l + 1), size[1] >> (l + 1))
            assert np.array_equal(pc.ubits(g), pc.ubits(w)), (source, kind, jump, l)
            assert np.array_equal(pc.ubits(a.cpu().numpy()), pc.ubits(w)), (source, kind, jump, l)
        if jump == 0.05:                                                                                             # and crossed: an array in, tensors out; a tensor in, arrays out
            crossed = fusion.depth_pyramid(depth, spec, levels, jump=jump, frame=1, output="device")
            back = fusion.depth_pyramid(torch.from_numpy(depth).to(cuda), spec, levels, jump=jump, frame=1)
            assert all(isinstance(c, torch.Tensor) and c.device == cuda for c in crossed) and all(isinstance(b, np.ndarray) for b in back)
            assert all(np.array_equal(pc.ubits(c.cpu().numpy()), pc.ubits(w)) and np.array_equal(pc.ubits(b), pc.ubits(w)) for c, b, w in zip(crossed, back, want))
        valid += int(sum((w != 0).sum() for w in want))
        if jump == 0.05:
            split += int(sum((a != b).sum() for a, b in zip(want, fusion.depth_pyramid_host(depth, spec, levels, jump=np.inf, frame=1))))
    print(f"\n[{size} x {levels}] {valid} valid pixels over the cases, {split} changed by jump = 0.05")
    assert valid >= 8 and (split > 0 or size == (2, 2))


@pytest.mark.parametrize("case", range(5))
def test_colour_levels_equal_the_host_mirror(cuda, case):
    size, levels = _sizes()[case]
    frames = pc.colours((3,) + size, seed=case)
    for frame in (0, 2):
        want = fusion.rgb_pyramid_host(frames, levels, frame=frame)
        got = fusion.rgb_pyramid(frames, levels, frame=frame)
        again = fusion.rgb_pyramid(torch.from_numpy(frames).to(cuda), levels, frame=frame, output="device")
        assert len(got) == len(again) == levels
        for l, (g, a, w) in enumerate(zip(got, again, want)):
            assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.shape == w.shape == (size[0] >> (l + 1), size[1] >> (l + 1), 3)
            assert isinstance(a, torch.Tensor) and a.device == cuda and a.dtype == torch.uint8
            assert np.array_equal(g, w) and np.array_equal(a.cpu().numpy(), w), (frame, l)
    crossed = fusion.rgb_pyramid(frames, levels, frame=2, output="device")                                          # an array in, tensors out; a tensor in, arrays out
    back = fusion.rgb_pyramid(torch.from_numpy(frames).to(cuda), levels, frame=2)
    assert all(isinstance(c, torch.Tensor) and c.device == cuda for c in crossed) and all(isinstance(b, np.ndarray) and b.dtype == np.uint8 for b in back)
    assert all(np.array_equal(c.cpu().numpy(), w) and np.array_equal(b, w) for c, b, w in zip(crossed, back, want))
    with pytest.raises(ValueError):
        fusion.rgb_pyramid(frames, levels, output="gpu")
    with pytest.raises(ValueError):
        fusion.rgb_pyramid(torch.from_numpy(frames), levels)
    with pytest.raises(ValueError):
        fusion.depth_pyramid(torch.zeros((1,) + size), tc.spec(), levels)


def test_a_tall_frame_has_more_rows_of_tiles_than_a_grid_axis_holds(cuda):
    """2 x 16 x 65537 rows of two pixels: 65537 rows of tiles, one more than the y axis of a grid takes; the tiles run along x alone."""
    h = 2 * 16 * 65537
    depth = (0.5 + 0.25 * np.random.default_rng(5).random((1, h, 2))).astype(np.float32)
    depth[0, -4:, :] = 0.0                                                                                           # the last row of level 1: one valid pixel of four
    depth[0, -1, 1] = 0.625
    spec = Cloud(K=np.eye(3), source="depth", far=10.0)
    want = fusion.depth_pyramid_host(depth, spec, 1)[0]
    got = fusion.depth_pyramid(depth, spec, 1)[0]
    assert got.shape == want.shape == (h // 2, 1) and np.array_equal(pc.ubits(got), pc.ubits(want))
    assert got[-1, 0] == np.float32(0.625) and got[-2, 0] == 0 and (got[:-2] != 0).all()
    rgb = pc.colours((1, h, 2), seed=6)
    assert np.array_equal(fusion.rgb_pyramid(rgb, 1)[0], fusion.rgb_pyramid_host(rgb, 1)[0])


# ---- the raw entry points -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(cuda):
    """Two frames that cross the kernel's tiles raggedly, disparity with a mask per frame and a gain, and their colours; frame 1 and every level."""
    most = fusion.PYRAMID_MAX_LEVELS
    side = pc.tile(most)
    shape = (2, side + 1, 2 * side + 1)
    depth, _ = pc.frame(shape, "disparity", "none", seed=77)
    mask = np.random.default_rng(78).random(shape) < 0.8
    spec = dataclasses.replace(tc.live_spec(shape, np.eye(4), 1, "disparity", mask), gain=1.02)
    frames = pc.colours(shape, seed=79)
    x, m, rgb = torch.from_numpy(depth).to(cuda), torch.from_numpy(spec.mask.copy()).to(cuda), torch.from_numpy(frames).to(cuda)
    levels = most - 1
    want = np.concatenate([w.reshape(-1) for w in fusion.depth_pyramid_host(depth, spec, levels, frame=1)])
    want_rgb = np.concatenate([w.reshape(-1) for w in fusion.rgb_pyramid_host(frames, levels, frame=1)])
    assert (want != 0).sum() > 500
    return dict(x=x, mask=m, rgb=rgb, sel=cloud.selection(x, spec, m), shape=shape, levels=levels, want=want, want_rgb=want_rgb)


def _raw_depth(lib, cuda, r, stream=None, **kw):
    st = C.c_void_p(_lib.stream_ptr(cuda) if stream is None else stream.cuda_stream)
    out = torch.full((PAD + r["want"].size * 4 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    args = dict(sel=C.byref(r["sel"]), frame=1, levels=r["levels"], one_plus_jump=float(np.float32(1.05)), out=out.data_ptr() + PAD)
    for k, val in kw.items():
        args[k] = val(args[k]) if callable(val) else val
    ret = lib.edv_depth_pyramid(*args.values(), st)
    torch.cuda.synchronize()
    return ret, out.cpu().numpy()


def _raw_rgb(lib, cuda, r, stream=None, **kw):
    st = C.c_void_p(_lib.stream_ptr(cuda) if stream is None else stream.cuda_stream)
    out = torch.full((PAD + r["want_rgb"].size + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    n, h, w = r["shape"]
    args = dict(frames=r["rgb"].data_ptr(), n=n, h=h, w=w, frame=1, levels=r["levels"], out=out.data_ptr() + PAD)
    for k, val in kw.items():
        args[k] = val(args[k]) if callable(val) else val
    ret = lib.edv_rgb_pyramid(*args.values(), st)
    torch.cuda.synchronize()
    return ret, out.cpu().numpy()


def test_the_depth_entry_writes_its_levels_and_nothing_else(lib, cuda, ragged):
    ret, out = _raw_depth(lib, cuda, ragged)
    assert ret == 0, lib.edv_last_error()
    assert np.array_equal(out[PAD:-PAD].view(np.uint32), pc.ubits(ragged["want"]))                   # every pixel of every level written, zeros included
    assert (out[:PAD] == GUARD).all() and (out[-PAD:] == GUARD).all()
    side = torch.cuda.Stream(device=cuda)                                                            # on whichever stream it is given
    side.wait_stream(torch.cuda.current_stream(cuda))
    ret, again = _raw_depth(lib, cuda, ragged, stream=side)
    assert ret == 0 and np.array_equal(again, out)
    n, h, w = ragged["shape"]
    for levels in (1, 2):                                                                            # fewer levels: the front of the same buffer, the rest untouched
        ret, part = _raw_depth(lib, cuda, ragged, levels=levels)
        used = 4 * int(lib.edv_pyramid_pixels(h, w, levels, None))
        assert ret == 0 and np.array_equal(part[PAD:PAD + used], out[PAD:PAD + used]) and (part[PAD + used:] == GUARD).all(), levels
    ret, other = _raw_depth(lib, cuda, ragged, frame=0)
    assert ret == 0 and not np.array_equal(other, out)

    def sel(**kw):
        s = _lib.CloudSelection.from_buffer_copy(ragged["sel"])
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    nan = float("nan")
    bad = [dict(sel=None), dict(out=None), dict(out=lambda p: p + 2), dict(frame=-1), dict(frame=2), dict(levels=0), dict(levels=-1), dict(levels=ragged["levels"] + 1),
           dict(one_plus_jump=0.5), dict(one_plus_jump=nan), dict(one_plus_jump=-1.0), dict(sel=sel(step=2)), dict(sel=sel(step=0)), dict(sel=sel(near_z=-0.1)),
           dict(sel=sel(near_z=nan)), dict(sel=sel(gain=0.0)), dict(sel=sel(gain=-1.0)), dict(sel=sel(gain=nan)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)),
           dict(sel=sel(mode=2)), dict(sel=sel(mask_stride=5)), dict(sel=sel(h=1)), dict(sel=sel(w=8))]                   # h = 1: no level 1; w = 8: no level 4
    for kw in bad:
        ret, out = _raw_depth(lib, cuda, ragged, **kw)
        assert ret != 0 and lib.edv_last_error(), kw
        assert (out == GUARD).all(), kw                                                              # nothing was launched
    ret, out = _raw_depth(lib, cuda, ragged, one_plus_jump=float("inf"))                             # inf is a jump
    assert ret == 0 and (out[:PAD] == GUARD).all() and (out[-PAD:] == GUARD).all()


def test_the_colour_entry_writes_its_levels_and_nothing_else(lib, cuda, ragged):
    ret, out = _raw_rgb(lib, cuda, ragged)
    assert ret == 0, lib.edv_last_error()
    assert np.array_equal(out[PAD:-PAD], ragged["want_rgb"]) and (out[:PAD] == GUARD).all() and (out[-PAD:] == GUARD).all()
    ret, odd = _raw_rgb(lib, cuda, ragged, out=lambda p: p + 1)                                      # bytes: any alignment
    assert ret == 0 and np.array_equal(odd[PAD + 1:-PAD + 1], ragged["want_rgb"]) and (odd[:PAD + 1] == GUARD).all() and (odd[-PAD + 1:] == GUARD).all()
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    ret, again = _raw_rgb(lib, cuda, ragged, stream=side)
    assert ret == 0 and np.array_equal(again, out)
    n, h, w = ragged["shape"]
    ret, part = _raw_rgb(lib, cuda, ragged, levels=1)
    used = 3 * int(lib.edv_pyramid_pixels(h, w, 1, None))
    assert ret == 0 and np.array_equal(part[PAD:PAD + used], out[PAD:PAD + used]) and (part[PAD + used:] == GUARD).all()
    bad = [dict(frames=None), dict(out=None), dict(n=0), dict(frame=-1), dict(frame=2), dict(levels=0), dict(levels=ragged["levels"] + 1), dict(h=0), dict(w=0), dict(h=1),
           dict(w=8), dict(h=2 ** 16, w=2 ** 15)]
    for kw in bad:
        ret, out = _raw_rgb(lib, cuda, ragged, **kw)
        assert ret != 0 and lib.edv_last_error(), kw
        assert (out == GUARD).all(), kw


# ---- 7. a track and a clip ------------------------------------------------------------------------------------------------------------------------
VARIANTS = {"alone": {}, "scale": dict(scale=True), "colour": dict(colour=cc.WEIGHT), "robust": dict(min_cos=0.985, huber=0.005)}


def _same_track(got, want):
    assert len(got) == len(want) and got[0].dtype == np.float64 and np.array_equal(tc.bits(got[0]), tc.bits(want[0]))
    assert got[1] == want[1] and np.array_equal(tc.bits(got[2]), tc.bits(want[2])) and got[3] is want[3]
    if len(want) == 5:
        assert isinstance(got[4], float) and np.array_equal(tc.bits(got[4]), tc.bits(want[4]))


@pytest.mark.parametrize("plan", pc.PLANS, ids=str)
def test_track_equals_the_host_mirror(cuda, plan):
    """The four variants from host arrays, and everything together from tensors; a frame at five times the scene's motion, which only the pyramid
    finds; a guess that sees nothing and a level that is lost for want of pairs."""
    host = cc.fused()
    dev = Tsdf(tc.volume(), device=cuda)
    dev.integrate(cc.shape_of("curved"), tc.spec(), cc.texture())
    fc.same_state(dev.arrays(), host.arrays())
    live, frames, truth = cc.single()
    for name, options in VARIANTS.items():
        track = tc.track(pyramid=plan, min_pairs=16, **options)
        want = host.track(live, tc.spec(), track, frames=frames)
        _same_track(dev.track(live, tc.spec(), track, frames=frames), want)
        assert not want[3]
        print(f"\n[{plan} {name}] rotation {tc.errors(want[0], truth)[0]:.3e} rad, translation {tc.errors(want[0], truth)[1]:.3e}; {want[1]} pairs")
    track = tc.track(pyramid=plan, min_pairs=16, scale=True, colour=cc.WEIGHT, huber_colour=8.0, min_cos=0.985, huber=0.005, jump=0.0)
    spec = tc.spec(gain=1.01, mask=np.random.default_rng(3).random((tc.H, tc.W)) < 0.9)
    want = host.track(live, spec, track, frames=frames)
    _same_track(dev.track(torch.from_numpy(live.copy()).to(cuda), spec, track, frames=torch.from_numpy(frames.copy()).to(cuda)), want)   # tensors in
    assert not want[3]
    far_truth = tc.pose(tc.ROTATION, tc.TRANSLATION, 5.0)
    far_live = cc.seen_from(far_truth)[0]
    want = host.track(far_live, tc.spec(), tc.track(pyramid=(10, 5, 4), min_pairs=16))
    _same_track(dev.track(far_live, tc.spec(), tc.track(pyramid=(10, 5, 4), min_pairs=16)), want)
    assert not want[3] and tc.errors(want[0], far_truth)[0] < 5e-3
    lost = 0
    for spec, track in ((tc.spec(pose=tc.AWAY), tc.track(pyramid=plan)), (tc.spec(), tc.track(pyramid=plan, min_pairs=10 * 14 + 1, scale=True))):
        want = host.track(live, spec, track, frames=frames)
        _same_track(dev.track(live, spec, track, frames=frames), want)
        lost += int(want[3])
    assert lost == 2
    fc.same_state(dev.arrays(), host.arrays())                                                       # tracking only reads the volume


@pytest.mark.parametrize("plan", pc.PLANS, ids=str)
def test_track_clip_equals_the_host_mirror(cuda, plan):
    """The five-frame clip of tests/track_cases.py in colour, the four variants: poses, pairs, rms, lost and scales as bit patterns, and the volumes
    after the clip bit for bit."""
    depth, frames, truth = cc.clip()
    for name, options in VARIANTS.items():
        track = tc.track(pyramid=plan, min_pairs=16, **options)
        host, dev = TsdfHost(tc.volume()), Tsdf(tc.volume(), device=cuda)
        want = host.track_clip(depth, tc.spec(), track, frames)
        got = dev.track_clip(depth, tc.spec(), track, frames) if name != "robust" else dev.track_clip(torch.from_numpy(depth.copy()).to(cuda), tc.spec(), track,
                                                                                                      torch.from_numpy(frames.copy()).to(cuda))
        assert isinstance(got, Tracked) and not want.lost.any()
        cc.same_tracked(got, want)
        fc.same_state(dev.arrays(), host.arrays())
        worst = max(tc.errors(want.poses[i], truth[i])[0] for i in range(5))
        print(f"\n[{plan} {name}] worst rotation error {worst:.3e} rad; pairs {want.pairs[1:].min()} .. {want.pairs.max()}")
        assert worst < 2e-2
    with pytest.raises(ValueError):
        Tsdf(tc.volume(), device=cuda).track_clip(depth, tc.spec(near=-0.1), tc.track(pyramid=plan), frames)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


def test_video_surface_with_a_pyramid(cuda):
    """The plumbing, with the scene of tests/test_track_robust_gpu.py: ``video_surface(track=Track(pyramid=...))`` does exactly what its steps do on
    the GPU, and its first frames are the mirror's to the bit (``TsdfHost.track_clip`` on the same depth; a tracked clip is causal, so the first
    six frames of the 54 are a clip of six).  The depth of synthetic weights is no surface, so how many frames are kept says nothing; it is printed.
    Two levels, not three: with ``pyramid=(1, 1, 1)``, ``min_pairs=16`` and ``min_cos=0.5`` the same comparisons held to the bit, but the 10 x 14
    level found 4 to 6 pairs and 53 of the 54 frames were lost there, so the run showed little beyond a lost frame."""
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
    synth.fill_module_(m)
    still = long_video_frames(54, NET_H, NET_W)[:1].astype(np.int64)
    frames = np.clip(still + (np.arange(54) % 5)[:, None, None, None], 0, 255).astype(np.uint8)
    model = m.to(cuda)
    depth = model.infer_video_depth(frames, device="cuda:0", stitch="device", output="device")
    z = cloud.lift_host(depth.cpu().numpy(), Cloud(K=np.eye(3)), None).points[:, 2]
    unit = float(np.median(z))
    spec = Cloud(K=cases.intrinsics(NET_H, NET_W), pose=fc.nearby_poses(1, seed=1, scale=unit)[0], far=2.0 * unit)
    points = cloud.lift_host(depth.cpu().numpy()[:1], spec, None).points
    extent = float((points.max(axis=0) - points.min(axis=0)).max())
    voxel = extent / 40.0
    vol = Volume.bounding(points, voxel, margin=0.25 * extent, trunc=12.0 * voxel)
    assert max(vol.dims) <= 64
    track = fusion.Track(near=0.0, far=2.0 * unit, step=0.5 * voxel, max_dist=0.5 * unit, min_pairs=8, pyramid=(1, 1), colour=0.1 * unit, huber=0.1 * unit)
    steps = Tsdf(vol, coloured=True, device=cuda)
    want_track = steps.track_clip(depth, spec, track, torch.from_numpy(frames.copy()).to(cuda))
    print(f"\n{int(want_track.lost.sum())} of 54 frames lost; pairs {want_track.pairs[1:].min()} .. {want_track.pairs.max()}")
    want = steps.surface(min_weight=1.0)
    assert len(want) > 0
    got, tracked = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=1.0, track=track)
    assert isinstance(tracked, Tracked) and tracked.poses.shape == (54, 4, 4) and tracked.scales is None
    fc.same_cloud(got, want)
    cc.same_tracked(tracked, want_track)
    mirror = TsdfHost(vol, coloured=True).track_clip(depth[:6].cpu().numpy(), spec, track, frames[:6])
    cc.same_tracked(Tracked(tracked.poses[:6], tracked.pairs[:6], tracked.rms[:6], tracked.lost[:6]), mirror)
