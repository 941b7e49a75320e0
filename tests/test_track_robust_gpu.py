"""Robust camera tracking on MI355X: ``fusion.frame_normals`` against ``fusion.frame_normals_host`` as uint32 patterns, ``fusion.icp_robust_sums`` and
the raw entry points against ``fusion.icp_robust_sums_host`` as uint64 patterns (the kernels run the mirror's float64 operations and additions in
the mirror's order, so nothing needs a tolerance), the sums with every option off against the kernels without the options, ``Tsdf.track`` and
``Tsdf.track_clip`` with ``Track(min_cos=..., huber=..., huber_colour=...)`` against the mirror's, and ``model.video_surface`` end to end.  What
the rule computes and what the tracker gains from it is checked on the mirror alone (tests/test_track_robust_cpu.py)."""
import ctypes as C
import dataclasses
import itertools
import math

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
from tests import track_robust_cases as rc
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
    """The model views of tests/test_track_colour_gpu.py: one with a miss in the middle, one of another size and K, one whose K has skew, the
    middle of the view (hits up to its border) and one a pixel wide."""
    same, views = cc.model()
    depth = same.depth.copy()
    depth[0, 20, 30] = 0.0
    return {"holed": (Raycast(depth, same.normals, same.colors), views), "other": cc.model(size=tc.OTHER_SIZE, intrinsics=tc.OTHER_K), "skew": cc.model(intrinsics=cc.SKEW_K),
            "middle": cc.model(size=(30, 40), intrinsics=(60.0, 0.0, 20.0, 0.0, 60.0, 15.0, 0.0, 0.0, 1.0)),
            "narrow": cc.model(size=(tc.H, 1), intrinsics=(60.0, 0.0, 0.5, 0.0, 60.0, 20.0, 0.0, 0.0, 1.0))}


def _on(cuda, model):
    return Raycast(*(torch.from_numpy(a.copy()).to(cuda) for a in (model.depth, model.normals, model.colors)))


def _per_frame(spec, mask=None):
    """``spec`` with a K per frame (two frames), and optionally a mask per frame."""
    K = np.stack([spec.K[0], spec.K[0] * np.array([[1.1, 1.0, 0.95], [1.0, 0.9, 1.05], [1.0, 1.0, 1.0]])])
    return dataclasses.replace(spec, K=K, mask=spec.mask if mask is None else np.stack([mask, mask[::-1, ::-1]]))


# ---- 1. the live normals, bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,step", SHAPES, ids=str)
def test_normals_equal_the_host_mirror(cuda, size, step):
    """Two frames.  Both sources, with and without a mask, one K or one per frame, NaN, Inf and 0 among the depths: the map from host arrays and
    from tensors, as a numpy array and as a tensor, equals the mirror's as bit patterns."""
    shape = (2,) + size
    found = 0
    for i, (source, kind, per_frame) in enumerate(itertools.product(cloud.SOURCES, ("none", "shared"), (False, True))):
        depth, mask = tc.live(shape, source, kind, seed=500 + 8 * SHAPES.index((size, step)) + i)
        depth[1, size[0] // 2, size[1] // 2], depth[0, 1, 1], depth[1, 2, 5] = np.nan, np.inf, 0.0
        spec = dataclasses.replace(tc.live_spec(shape, np.eye(4), step, source, mask), gain=1.02 if per_frame else 1.0)
        if per_frame:
            spec = _per_frame(spec, mask)
        want = fusion.frame_normals_host(depth, spec)
        got = fusion.frame_normals(depth, spec)                                                             # a host array in, one out
        assert isinstance(got, np.ndarray) and got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(rc.ubits(got), rc.ubits(want)), (source, kind, per_frame)
        again = fusion.frame_normals(torch.from_numpy(depth).to(cuda), spec, output="device")               # a tensor in, used in place, one out
        assert isinstance(again, torch.Tensor) and again.device == cuda and again.dtype == torch.float32
        assert np.array_equal(rc.ubits(again.cpu().numpy()), rc.ubits(want)), (source, kind, per_frame)
        found += int(want.any(axis=-1).sum())
    print(f"\n[{size} step {step}] {found} normals over the cases")
    assert found > (5000 if size == (40, 56) else 20)


def test_normals_of_frames_too_small_for_a_neighbourhood(cuda):
    K = np.array([[5.0, 0.0, 1.5], [0.0, 5.0, 1.5], [0.0, 0.0, 1.0]])
    spec = Cloud(K=K, source="depth", far=10.0)
    for shape in ((1, 1, 9), (1, 2, 2), (3, 3, 3), (1, 5, 7)):
        depth = np.full(shape, 0.5, np.float32)
        got, want = fusion.frame_normals(depth, spec), fusion.frame_normals_host(depth, spec)
        assert np.array_equal(rc.ubits(got), rc.ubits(want))
        assert int(got.any(axis=-1).sum()) == shape[0] * max(shape[1] - 2, 0) * max(shape[2] - 2, 0)
    assert np.array_equal(fusion.frame_normals(np.full((1, 3, 3), 0.5, np.float32), spec)[0, 1, 1], [0.0, 0.0, -1.0])
    with pytest.raises(ValueError):
        fusion.frame_normals(np.zeros((1, 3, 3), np.float32), spec, output="gpu")
    with pytest.raises(ValueError):
        fusion.frame_normals(torch.zeros((1, 3, 3)), spec)


@pytest.fixture(scope="module")
def clip3(cuda):
    """(depth tensor, mask tensor, cams tensor [3, 21], selection, the mirror's normals [3, 6, 8, 3]) of three ragged 17 x 23 frames at step 3 with a K
    per frame, a mask and disparity."""
    shape = (3, 17, 23)
    depth, mask = tc.live(shape, "disparity", "shared", seed=61)
    base = tc.live_spec(shape, np.eye(4), 3, "disparity", mask)
    spec = dataclasses.replace(base, K=np.stack([base.K[0] * (1.0 + 0.05 * f * np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, 0.0]])) for f in range(3)]), gain=1.02)
    x, m = torch.from_numpy(depth).to(cuda), torch.from_numpy(spec.mask.copy()).to(cuda)
    cams = torch.from_numpy(spec.cams(3)).to(cuda)
    want = fusion.frame_normals_host(depth, spec)
    assert want.shape == (3, 6, 8, 3) and all(want[f].any() for f in range(3))
    return x, m, cams, cloud.selection(x, spec, m), want


def _raw_normals(lib, cuda, clip3, stream=None, **kw):
    x, m, cams, sel, _ = clip3
    st = C.c_void_p(_lib.stream_ptr(cuda) if stream is None else stream.cuda_stream)
    out = torch.full((PAD + 3 * 6 * 8 * 3 * 4 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    args = dict(sel=C.byref(sel), cams=cams.data_ptr(), stride=21, first=0, count=3, normals=out.data_ptr() + PAD)
    for k, val in kw.items():
        args[k] = val(args[k]) if callable(val) else val
    ret = lib.edv_frame_normals(*args.values(), st)
    torch.cuda.synchronize()
    return ret, out.cpu().numpy()


def test_the_normals_entry_writes_its_range_and_nothing_else(lib, cuda, clip3):
    want = clip3[4]
    frame = 6 * 8 * 3 * 4
    ret, out = _raw_normals(lib, cuda, clip3)
    assert ret == 0, lib.edv_last_error()
    assert np.array_equal(out[PAD:-PAD].view(np.uint32), rc.ubits(want).reshape(-1)) and (out[:PAD] == GUARD).all() and (out[-PAD:] == GUARD).all()
    for first, count in ((1, 1), (2, 1), (1, 2), (0, 2)):                                            # a range of frames: that many maps from the buffer's start
        ret, part = _raw_normals(lib, cuda, clip3, first=first, count=count)
        assert ret == 0 and np.array_equal(part[PAD:PAD + count * frame].view(np.uint32), rc.ubits(want[first:first + count]).reshape(-1)), (first, count)
        assert (part[:PAD] == GUARD).all() and (part[PAD + count * frame:] == GUARD).all(), (first, count)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    ret, again = _raw_normals(lib, cuda, clip3, stream=side)
    assert ret == 0 and np.array_equal(again, out)
    ret, shared = _raw_normals(lib, cuda, clip3, stride=0)                                           # one camera for all: frame 0's
    assert ret == 0 and np.array_equal(shared[PAD:PAD + frame], out[PAD:PAD + frame]) and not np.array_equal(shared[PAD + frame:-PAD], out[PAD + frame:-PAD])

    def sel(**kw):
        s = _lib.CloudSelection.from_buffer_copy(clip3[3])
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    bad = [dict(sel=None), dict(cams=None), dict(normals=None), dict(cams=lambda p: p + 4), dict(normals=lambda p: p + 2), dict(stride=7), dict(first=-1), dict(first=3, count=1),
           dict(count=0), dict(count=4), dict(first=2, count=2), dict(sel=sel(step=0)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)), dict(sel=sel(mode=2)),
           dict(sel=sel(mask_stride=5))]
    for kw in bad:
        ret, out = _raw_normals(lib, cuda, clip3, **kw)
        assert ret != 0 and lib.edv_last_error(), kw
        assert (out == GUARD).all(), kw                                                              # nothing was launched


# ---- 2. the sums, bit for bit -------------------------------------------------------------------------------------------------------------------
COMBOS = list(itertools.product((False, True), (False, True), (False, True), (math.inf, rc.HUBER)))   # scale, colour, normals, huber


def _options(colour, normals, huber):
    kw = dict(min_cos=rc.MIN_COS if normals else None, huber=huber)
    if colour:
        kw["huber_colour"] = math.inf if huber == math.inf else rc.HUBER_COLOUR
    return kw


@pytest.mark.parametrize("size,step", SHAPES, ids=str)
def test_sums_equal_the_host_mirror(cuda, size, step):
    """Frame 1 of a two-frame clip against the live camera's model.  The sixteen combinations of the column count, the colour block, the normal
    test and the Huber weights, each with a source and a mask of its own, and the five guesses: the sums from host arrays and from tensors equal
    the mirror's as bit patterns; with every option off they equal the kernels without the options."""
    shape = (2,) + size
    model, views = cc.model()
    on_device = _on(cuda, model)
    count = {c: np.zeros(2, np.int64) for c in itertools.product((False, True), (math.inf, rc.HUBER))}
    weighed = 0
    variants = list(itertools.product(cloud.SOURCES, ("none", "shared")))
    for i, (scale, colour, normals, huber) in enumerate(COMBOS):
        source, kind = variants[i % 4]
        depth, mask, frames = cc.live(shape, source, kind, seed=700 + 16 * SHAPES.index((size, step)) + i)
        depth_d, frames_d = torch.from_numpy(depth).to(cuda), torch.from_numpy(frames).to(cuda)
        kw = _options(colour, normals, huber)
        for name, T in _guesses().items():
            spec = dataclasses.replace(tc.live_spec(shape, T, step, source, mask), gain=1.02 if scale else 1.0)
            want = fusion.icp_robust_sums_host(depth, spec, model, views, 0.1, 1, scale=scale, frames=frames if colour else None, **kw)
            got = fusion.icp_robust_sums(depth, spec, model, views, 0.1, 1, scale=scale, frames=frames if colour else None, **kw)              # host arrays in
            assert got.shape == ((2,) if colour else ()) + (37 if scale else 29,) and got.dtype == np.float64
            assert np.array_equal(tc.bits(got), tc.bits(want)), (scale, colour, normals, huber, name, got, want)
            again = fusion.icp_robust_sums(depth_d, spec, on_device, views, 0.1, frame=1, scale=scale, frames=frames_d if colour else None, **kw)   # tensors in
            assert np.array_equal(tc.bits(again), tc.bits(want)), (scale, colour, normals, huber, name)
            if not normals and huber == math.inf:                                                      # the kernels without the options
                plain = fusion.icp_colour_sums(depth_d, frames_d, spec, on_device, views, 0.1, 1, scale=scale) if colour else fusion.icp_sums(depth_d, spec, on_device, views, 0.1, 1, scale=scale)
                assert np.array_equal(tc.bits(got), tc.bits(plain)), (scale, colour, name)
            if name == "away":
                assert np.array_equal(tc.bits(want), tc.bits(np.zeros_like(want)))
            off = fusion.icp_robust_sums_host(depth, spec, model, views, 0.1, 1, scale=scale, frames=frames if colour else None)
            geometric, plain_block = want.reshape(-1, want.shape[-1])[0], off.reshape(-1, off.shape[-1])[0]
            count[(normals, huber)] += np.array([geometric[-1], plain_block[-1]], np.int64)
            if huber != math.inf and not normals:
                assert geometric[-1] == plain_block[-1] and np.array_equal(tc.bits(geometric[-2]), tc.bits(plain_block[-2]))       # weights touch neither the count nor e e
                weighed += int(geometric[0] < plain_block[0])
    for (normals, huber), (with_options, without) in count.items():
        print(f"\n[{size} step {step}] normals {normals}, huber {huber}: {with_options} pairs over the cases, {without} without the options")
        assert (with_options < without) if normals else (with_options == without)
        if size == (40, 56):
            assert with_options > 1000                                                              # an option never removes every pair
    if size == (40, 56):
        assert weighed >= 8                                                                         # the weights bit: of the four combinations with them alone, four guesses see the surface


@pytest.mark.parametrize("which", ["holed", "other", "skew", "middle", "narrow"])
def test_sums_equal_the_host_mirror_at_the_model_edges(cuda, which):
    """The model views of the colour test's edges, at the scene's own size and at the ragged 17 x 23 with step 3, live depth with NaN, 0 and Inf,
    everything on."""
    model, views = _models()[which]
    on_device = _on(cuda, model)
    pairs = 0
    for (size, step), scale, colour in itertools.product((((40, 56), 1), ((17, 23), 3)), (False, True), (False, True)):
        shape = (2,) + size
        depth, mask, frames = cc.live(shape, "depth", "shared", seed=40 + step)
        depth[1, 2, 3:6], depth[1, 5, 1], depth[1, 6, 6] = np.nan, np.inf, 0.0
        kw = dict(_options(colour, True, rc.HUBER), frames=frames if colour else None, scale=scale)
        for name in ("identity", "aside", "truth"):
            spec = tc.live_spec(shape, _guesses()[name], step, "depth", mask)
            want = fusion.icp_robust_sums_host(depth, spec, model, views, 0.1, 1, **kw)
            got = fusion.icp_robust_sums(depth, spec, on_device, views, 0.1, 1, **kw)
            assert np.array_equal(tc.bits(got), tc.bits(want)), (which, size, scale, colour, name, got, want)
            assert np.isfinite(got).all()
            pairs += int(want.reshape(-1, want.shape[-1])[0, -1])
    print(f"\n[{which}] {pairs} pairs over the cases")
    assert pairs > (20 if which == "narrow" else 1000)                                               # a view one pixel wide sees a column of the frame


# ---- 3. the raw entry point ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(cuda):
    """(a prepared ``fusion._IcpDevice`` with every option, colour and the seventh column, the estimate's 21 doubles, the mirror's sums) of the
    ragged 17 x 23 case at step 1, three frames, frame 2, a shared mask, gain 1.02, disparity."""
    shape = (3, 17, 23)
    depth, mask, frames = cc.live(shape, "disparity", "shared", seed=41)
    model, views = cc.model()
    spec = dataclasses.replace(tc.live_spec(shape, tc.pose((0.0, 0.0, 0.0), (0.003, -0.003, 0.0)), 1, "disparity", mask), gain=1.02)
    options = dict(min_cos=0.9, huber=0.002, huber_colour=2.0)
    ctx = fusion._IcpDevice(depth, spec, model, views, 0.1, 2, device=cuda, scale=True, frames=frames, robust=options)
    want = fusion.icp_robust_sums_host(depth, spec, model, views, 0.1, 2, scale=True, frames=frames, **options)
    off = fusion.icp_colour_sums_host(depth, frames, spec, model, views, 0.1, 2, scale=True)
    assert 50 < want[0, -1] < off[0, -1] and 50 < want[1, -1] and ctx.live_normals.shape == (1, 17, 23, 3)
    return ctx, fusion._estimate(ctx, spec, 2), want, options


def _raw(lib, cuda, ctx, estimate, options, stream=None, **kw):
    """The entry point on poisoned buffers: the sums and the workspace lie between PAD guard bytes, the workspace itself is filled with 0xFF
    (NaN patterns).  Returns (the return value, the two buffers' bytes with the guards on)."""
    st = C.c_void_p(_lib.stream_ptr(cuda) if stream is None else stream.cuda_stream)
    need = int(lib.edv_icp_robust_workspace(ctx.sel.h, ctx.sel.w, ctx.sel.step, 7, 1))
    sums = torch.full((PAD + 74 * 8 + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    ws = torch.full((PAD + need + PAD,), GUARD, dtype=torch.uint8, device=cuda)
    ws[PAD:PAD + need] = 0xFF
    args = dict(sel=C.byref(ctx.sel), frame=ctx.frame, frames=ctx.frames.data_ptr(), live=(C.c_double * 21)(*estimate), model=ctx.model_cam, depth=ctx.depth.data_ptr(),
                normals=ctx.normals.data_ptr(), colors=ctx.colors.data_ptr(), mh=ctx.size[0], mw=ctx.size[1], max_dist2=ctx.max_dist2, cols=7,
                live_normals=ctx.live_normals.data_ptr(), min_cos=options["min_cos"], huber=options["huber"], huber_colour=options["huber_colour"], sums=sums.data_ptr() + PAD,
                ws=ws.data_ptr() + PAD, ws_bytes=need)
    for k, val in kw.items():
        args[k] = val(args[k]) if callable(val) else val
    ret = lib.edv_icp_robust_sums(*args.values(), st)
    torch.cuda.synchronize()
    return ret, sums.cpu().numpy(), ws.cpu().numpy()


def test_guards_stay_and_a_poisoned_workspace_changes_nothing(lib, cuda, scene):
    ctx, live, want, options = scene
    ret, sums, ws = _raw(lib, cuda, ctx, live, options)
    assert ret == 0, lib.edv_last_error()
    assert np.array_equal(sums[PAD:-PAD].view(np.uint64), tc.bits(want).reshape(-1))
    assert (sums[:PAD] == GUARD).all() and (sums[-PAD:] == GUARD).all() and (ws[:PAD] == GUARD).all() and (ws[-PAD:] == GUARD).all()
    tiles = ws[PAD:-PAD].view(np.uint64).reshape(-1, 74)
    assert tiles.shape[0] == -(-17 * 23 // 256) and not (tiles == np.uint64(2 ** 64 - 1)).any()     # every slot was written
    assert np.ascontiguousarray(tiles[:, 36]).view(np.float64).sum() == want[0, 36] and np.ascontiguousarray(tiles[:, 73]).view(np.float64).sum() == want[1, 36]
    ret2, sums2, ws2 = _raw(lib, cuda, ctx, live, options)                                           # two calls, the same bytes
    assert ret2 == 0 and np.array_equal(sums, sums2) and np.array_equal(ws, ws2)
    side = torch.cuda.Stream(device=cuda)                                                            # on whichever stream it is given
    side.wait_stream(torch.cuda.current_stream(cuda))
    ret3, sums3, _ = _raw(lib, cuda, ctx, live, options, stream=side)
    assert ret3 == 0 and np.array_equal(sums, sums3)
    ret4, sums4, _ = _raw(lib, cuda, ctx, live, options, ws_bytes=lambda b: b + 8, sums=lambda p: p + 8)   # a larger workspace and any 8-byte alignment are accepted
    assert ret4 == 0 and np.array_equal(sums4[PAD + 8:PAD + 8 + 592], sums[PAD:-PAD]) and (sums4[:PAD + 8] == GUARD).all()
    for kw, width in ((dict(cols=6), 58), (dict(frames=None), 37), (dict(colors=None), 37), (dict(cols=6, frames=None, colors=None), 29)):
        ret5, sums5, ws5 = _raw(lib, cuda, ctx, live, options, **kw)                                 # fewer sums in the same buffers: the rest untouched
        assert ret5 == 0 and (sums5[PAD + width * 8:] == GUARD).all() and (ws5[PAD + tiles.shape[0] * width * 8:-PAD] == 0xFF).all(), kw
        block = sums5[PAD:PAD + width * 8].view(np.float64).reshape(-1, 29 if width in (29, 58) else 37)
        assert np.array_equal(block[:, -1], want[:block.shape[0], -1]), kw                           # the same pairs
        if block.shape[1] == 37:
            assert np.array_equal(tc.bits(block[0]), tc.bits(want[0])), kw                           # without the colour block the geometric one keeps its bits
    ret6, sums6, _ = _raw(lib, cuda, ctx, live, options, live_normals=None, min_cos=-1.0)            # no normal test: more pairs
    assert ret6 == 0 and sums6[PAD:-PAD].view(np.float64)[36] > want[0, 36]
    # and through the context's own buffers, which nothing ever cleared
    assert np.array_equal(ctx.sums(live).reshape(2, -1).view(np.uint64), tc.bits(want))


def test_the_entry_point_refuses_and_leaves_everything_alone(lib, cuda, scene):
    ctx, live, want, options = scene

    def sel(**kw):
        s = _lib.CloudSelection.from_buffer_copy(ctx.sel)
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    nan = float("nan")
    bad = [dict(sel=None), dict(live=None), dict(model=None), dict(depth=None), dict(normals=None), dict(sums=None), dict(ws=None),
           dict(cols=5), dict(cols=8), dict(cols=0), dict(frame=-1), dict(frame=3),
           dict(sel=sel(step=0)), dict(sel=sel(x_dev=None)), dict(sel=sel(n=0)), dict(sel=sel(h=0)), dict(sel=sel(mode=2)), dict(sel=sel(mask_stride=5)),
           dict(mh=0), dict(mw=-1), dict(mh=2 ** 16, mw=2 ** 15), dict(max_dist2=-1.0), dict(max_dist2=nan), dict(max_dist2=math.inf),
           dict(min_cos=1.5), dict(min_cos=-1.5), dict(min_cos=nan), dict(min_cos=math.inf), dict(min_cos=nan, live_normals=None),
           dict(huber=0.0), dict(huber=-1.0), dict(huber=nan), dict(huber_colour=0.0), dict(huber_colour=nan), dict(huber_colour=-math.inf),
           dict(live_normals=lambda p: p + 2),
           dict(ws_bytes=lambda b: b - 1), dict(ws=lambda p: p + 4), dict(sums=lambda p: p + 4), dict(depth=lambda p: p + 2)]
    for kw in bad:
        ret, sums, ws = _raw(lib, cuda, ctx, live, options, **kw)
        assert ret != 0, kw
        assert lib.edv_last_error(), kw
        assert (sums == GUARD).all() and (ws[:PAD] == GUARD).all() and (ws[-PAD:] == GUARD).all() and (ws[PAD:-PAD] == 0xFF).all(), kw    # nothing was launched
    ret, sums, _ = _raw(lib, cuda, ctx, live, options)                                               # and the same call, unchanged, still works
    assert ret == 0 and np.array_equal(sums[PAD:-PAD].view(np.uint64), tc.bits(want).reshape(-1))


# ---- 4. a track and a clip ----------------------------------------------------------------------------------------------------------------------
def _same_track(got, want):
    assert len(got) == len(want) and got[0].dtype == np.float64 and np.array_equal(tc.bits(got[0]), tc.bits(want[0]))
    assert got[1] == want[1] and np.array_equal(tc.bits(got[2]), tc.bits(want[2])) and got[3] is want[3]
    if len(want) == 5:
        assert isinstance(got[4], float) and np.array_equal(tc.bits(got[4]), tc.bits(want[4]))


TRACKS = [dict(huber=rc.HUBER), dict(min_cos=rc.MIN_COS), rc.OPTIONS["both"]]


def test_track_equals_the_host_mirror(cuda):
    """Each option and all together, with and without ``scale`` and ``colour``, on the untouched frame and on the two spoilt ones, a guess that
    sees nothing and a frame that is lost for want of pairs: pose, pairs, rms, the lost flag and the scale as bits."""
    host = cc.fused()
    dev = Tsdf(tc.volume(), device=cuda)
    dev.integrate(cc.shape_of("curved"), tc.spec(), cc.texture())
    fc.same_state(dev.arrays(), host.arrays())
    frames = cc.single()[1]
    lost = 0
    for kind in ("untouched", "shift", "tilt"):
        live, truth = rc.scene(kind)
        for options, scale, colour in itertools.product(TRACKS, (False, True), (False, True)):
            extra = dict(colour=cc.WEIGHT, huber_colour=rc.HUBER_COLOUR) if colour else {}
            track = tc.track(scale=scale, **options, **extra)
            want = host.track(live, tc.spec(), track, frames=frames)
            _same_track(dev.track(live, tc.spec(), track, frames=frames), want)
            lost += int(want[3])
        track = tc.track(colour=cc.WEIGHT, huber_colour=rc.HUBER_COLOUR, **rc.OPTIONS["both"])
        want = host.track(live, tc.spec(), track, frames=frames)
        _same_track(dev.track(torch.from_numpy(live.copy()).to(cuda), tc.spec(), track, frames=torch.from_numpy(frames.copy()).to(cuda)), want)   # tensors in
        print(f"\n[{kind}] everything on: rotation {tc.errors(want[0], truth)[0]:.3e} rad, translation {tc.errors(want[0], truth)[1]:.3e}; {want[1]} pairs")
    assert lost == 0
    live = rc.scene("shift")[0]
    for spec, track in ((tc.spec(pose=tc.AWAY), tc.track(**rc.OPTIONS["both"])), (tc.spec(), tc.track(min_pairs=tc.H * tc.W, scale=True, **rc.OPTIONS["both"])),
                        (tc.spec(), tc.track(iterations=1, huber=rc.HUBER)), (tc.spec(step=3), tc.track(min_cos=0.9, min_pairs=16))):
        want = host.track(live, spec, track, frames=frames)
        _same_track(dev.track(live, spec, track, frames=frames), want)
        lost += int(want[3])
    assert lost == 2
    with pytest.raises(ValueError):
        dev.track(live, tc.spec(), tc.track(colour=cc.WEIGHT, huber_colour=rc.HUBER_COLOUR))        # no frames
    fc.same_state(dev.arrays(), host.arrays())                                                       # tracking only reads the volume


@pytest.mark.parametrize("scale", [False, True])
def test_track_clip_equals_the_host_mirror(cuda, scale):
    depth, frames, _ = cc.clip()
    spoilt = depth.copy()
    spoilt[2, rc.ROWS, rc.COLS] -= np.float32(rc.SHIFT)
    spoilt[3, rc.ROWS, rc.COLS] = (spoilt[3, 15, 40] + rc.TILT * (np.arange(rc.COLS.start, rc.COLS.stop) + 0.5 - 40)).astype(np.float32)[None, :]
    track = tc.track(colour=cc.WEIGHT, huber_colour=rc.HUBER_COLOUR, scale=scale, **rc.OPTIONS["both"])
    host, dev = TsdfHost(tc.volume()), Tsdf(tc.volume(), device=cuda)
    want = host.track_clip(spoilt, tc.spec(), track, frames)
    got = dev.track_clip(spoilt, tc.spec(), track, frames)
    assert isinstance(got, Tracked) and not want.lost.any()
    cc.same_tracked(got, want)
    fc.same_state(dev.arrays(), host.arrays())
    # without colour on an uncoloured volume: a tensor clip, a mask per frame, and a frame that is lost on the way (it sees nothing: all zeros)
    rng = np.random.default_rng(8)
    holed = depth.copy()
    holed[2] = 0.0
    spec = tc.spec(mask=rng.random(depth.shape) < 0.9)
    track = tc.track(scale=scale, **rc.OPTIONS["both"])
    host, dev = TsdfHost(tc.volume(), coloured=False), Tsdf(tc.volume(), coloured=False, device=cuda)
    want = host.track_clip(holed, spec, track)
    cc.same_tracked(dev.track_clip(torch.from_numpy(holed).to(cuda), spec, track), want)
    assert list(want.lost) == [False, False, True, False, False] and np.array_equal(want.poses[2], want.poses[1])
    fc.same_state(dev.arrays(), host.arrays())


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 42, 56


@pytest.fixture(scope="module")
def video(cuda):
    """The video of tests/test_track_colour_gpu.py: its small ViT-S at its network size, 54 frames (two windows) of one still frame whose brightness
    wanders by a few levels."""
    m = endodav_amd.endodav(encoder="vits", features=32, out_channels=[32, 32, 64, 64], image_shape=(NET_H, NET_W), lora_type="none", disable_conv_head=True).eval()
    synth.fill_module_(m)
    still = long_video_frames(54, NET_H, NET_W)[:1].astype(np.int64)
    frames = np.clip(still + (np.arange(54) % 5)[:, None, None, None], 0, 255).astype(np.uint8)
    frames.setflags(write=False)
    return m.to(cuda), frames


def test_video_surface_with_a_robust_track(cuda, video):
    """The plumbing, as in tests/test_track_colour_gpu.py and with its scene and its ``Track``: with ``huber``, ``min_cos`` and ``huber_colour`` the
    call does exactly what its steps do.  The depth of synthetic weights is no surface and changes from frame to frame, so how many frames such a
    tracker keeps says nothing; it is printed (measured: none of the 54 lost, 82 to 392 pairs a frame)."""
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
    track = fusion.Track(near=0.0, far=2.0 * unit, step=0.25 * voxel, max_dist=0.5 * unit, min_pairs=16, iterations=2, colour=0.1 * unit, huber=0.1 * unit, min_cos=0.5,
                         huber_colour=10.0)
    steps = Tsdf(vol, coloured=True, device=cuda)
    want_track = steps.track_clip(depth, spec, track, torch.from_numpy(frames.copy()).to(cuda))
    print(f"\n{int(want_track.lost.sum())} of 54 frames lost; pairs {want_track.pairs[1:].min()} .. {want_track.pairs.max()}")
    want = steps.surface(min_weight=1.0)
    assert len(want) > 0
    got, tracked = model.video_surface(frames, spec, vol, device="cuda:0", min_weight=1.0, track=track)
    assert isinstance(tracked, Tracked) and tracked.poses.shape == (54, 4, 4) and tracked.scales is None
    fc.same_cloud(got, want)
    cc.same_tracked(tracked, want_track)
