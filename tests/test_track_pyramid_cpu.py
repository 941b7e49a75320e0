"""Coarse-to-fine tracking on the numpy mirror (module docstring of ``fusion``, "pyramid"): the levels of the depth and colour pyramids against
values worked out by hand, a stored level consumed as an ordinary clip, what ``Track(pyramid=..., jump=...)`` and the pyramid functions refuse,
the default path unchanged, and what the pyramid buys on the scene of tests/track_cases.py.  The kernels are held to these mirrors bit for bit in
tests/test_track_pyramid_gpu.py."""
import dataclasses

import numpy as np
import pytest

from endodav_amd import fusion
from endodav_amd.cloud import Cloud
from endodav_amd.fusion import Track, TsdfHost
from tests import pyramid_cases as pc
from tests import track_cases as tc


# ---- 1. the levels, by hand ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jump", pc.JUMPS, ids=str)
def test_depth_levels_equal_the_values_worked_out_by_hand(jump):
    """The four kinds of block (all valid, one valid, none valid, split by ``jump``), two equal minima and a masked pixel; ``jump=inf`` uses every
    valid value and ``jump=0`` only those equal to the smallest.  The gain decides what is valid and stays out of what is stored."""
    got = fusion.depth_pyramid_host(pc.HAND, pc.hand_spec(), 2, jump=jump)
    assert [g.shape for g in got] == [(2, 3), (1, 1)] and all(g.dtype == np.float32 for g in got)
    assert np.array_equal(pc.ubits(got[0]), pc.ubits(pc.HAND_LEVEL1[jump])), (got[0], pc.HAND_LEVEL1[jump])
    assert np.array_equal(pc.ubits(got[1]), pc.ubits(pc.HAND_LEVEL2[jump]).reshape(1, 1)), (got[1], pc.HAND_LEVEL2[jump])
    assert not np.signbit(got[0][0, 2])                                                             # nothing valid: +0
    one = fusion.depth_pyramid_host(pc.HAND, pc.hand_spec(), 1, jump=jump)                          # fewer levels: the same level 1
    assert len(one) == 1 and np.array_equal(pc.ubits(one[0]), pc.ubits(got[0]))


def test_validity_follows_the_gain_and_the_frame_is_chosen():
    spec = dataclasses.replace(pc.hand_spec(), gain=1.0)                                            # now 6 * 1 lies inside far = 10: the block (0, 1) has two valid values
    got = fusion.depth_pyramid_host(pc.HAND, spec, 1)[0]
    assert got[0, 1] == np.float32(0.75) and fusion.depth_pyramid_host(pc.HAND, spec, 1, jump=np.inf)[0][0, 1] == np.float32(6.75) / np.float32(2)
    clip = np.concatenate([np.zeros_like(pc.HAND), pc.HAND])
    assert np.array_equal(pc.ubits(fusion.depth_pyramid_host(clip, pc.hand_spec(), 1, frame=1)[0]), pc.ubits(pc.HAND_LEVEL1[0.05]))
    assert not fusion.depth_pyramid_host(clip, pc.hand_spec(), 1, frame=0)[0].any()


def test_disparity_is_turned_into_depth_before_it_is_averaged():
    """``source="disparity"``: d = 1 / (lo + span * x) in float32, the cloud's rule without the gain; the mean is of depths, not of disparities."""
    spec = Cloud(K=np.eye(3), gain=3.0, near=0.0, far=1000.0)
    lo, span = spec.scalars()[:2]
    x = np.array([[0.5, 0.51], [0.505, 0.2]], np.float32)[None]
    d = [np.float32(1.0) / (lo + span * v) for v in x.reshape(-1)]
    want = ((d[0] + d[1]) + d[2]) / np.float32(3)                                                   # the fourth is far behind
    got = fusion.depth_pyramid_host(x, spec, 1)[0]
    assert got.shape == (1, 1) and np.array_equal(pc.ubits(got[0, 0]), pc.ubits(want))
    assert np.array_equal(pc.ubits(fusion.depth_pyramid_host(x, spec, 1, jump=np.inf)[0][0, 0]), pc.ubits((((d[0] + d[1]) + d[2]) + d[3]) / np.float32(4)))


def test_colour_levels_equal_the_values_worked_out_by_hand():
    got = fusion.rgb_pyramid_host(pc.HAND_RGB, 2)
    assert [g.shape for g in got] == [(2, 3, 3), (1, 1, 3)] and all(g.dtype == np.uint8 for g in got)
    assert np.array_equal(got[0], pc.HAND_RGB_LEVEL1), got[0]
    assert np.array_equal(got[1][0, 0], [(2 + 255 + 2 + 1 + 2) >> 2, (253 + 0 + 254 + 255 + 2) >> 2, 10])
    assert np.array_equal(fusion.rgb_pyramid_host(np.concatenate([pc.HAND_RGB, 255 - pc.HAND_RGB]), 1, frame=1)[0][..., 2], np.full((2, 3), 245))


def test_odd_sizes_drop_the_last_row_and_column():
    depth = np.arange(1, 5 * 7 + 1, dtype=np.float32).reshape(1, 5, 7)
    spec = Cloud(K=np.eye(3), source="depth", near=0.0, far=1000.0)
    got = fusion.depth_pyramid_host(depth, spec, 2, jump=np.inf)
    assert [g.shape for g in got] == [(2, 3), (1, 1)]
    assert np.array_equal(got[0], np.array([[5.0, 7.0, 9.0], [19.0, 21.0, 23.0]], np.float32))     # the means of rows 0..3 and columns 0..5: row 4 and column 6 are not read
    assert got[1][0, 0] == np.float32(13.0)
    changed = depth.copy()
    changed[0, 4, :], changed[0, :, 6] = 500.0, 700.0
    assert all(np.array_equal(a, b) for a, b in zip(fusion.depth_pyramid_host(changed, spec, 2, jump=np.inf), got))
    rgb = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(1, 5, 7, 3)
    assert [g.shape for g in fusion.rgb_pyramid_host(rgb, 2)] == [(2, 3, 3), (1, 1, 3)]
    assert fusion.rgb_pyramid_host(rgb, 1)[0][1, 2, 0] == (3 * (2 * 7 + 4) + 3 * (2 * 7 + 5) + 3 * (3 * 7 + 4) + 3 * (3 * 7 + 5) + 2) >> 2


# ---- 2. a stored level is an ordinary clip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
def test_a_level_is_consumed_as_a_clip(scale):
    """``icp_sums_host`` on the stored level 1 with K_1 and the gain of level 0 against a clip built by hand that holds the same z with gain 1: the
    same sums to the bit.  The zeros of the level fall to ``near``."""
    gain = 1.02
    live = (tc.single()[0] / np.float32(gain)).astype(np.float32)
    live[0, 10:14, 20:30] = 0.0                                                                     # a hole: zeros at level 1
    spec = tc.spec(gain=gain)
    level = fusion.depth_pyramid_host(live, spec, 1)[0]
    assert level.shape == (tc.H // 2, tc.W // 2) and (level[5:7, 10:15] == 0).all() and (level != 0).sum() > 200
    K1 = pc.level_K(tc.K, 1)
    assert np.array_equal(K1, [[30.0, 0.0, 14.0], [0.0, 30.0, 10.0], [0.0, 0.0, 1.0]])
    model, views = tc.model(size=level.shape, intrinsics=tuple(K1.reshape(-1)))
    T = tc.pose((0.0, 0.0, 0.0), (0.003, -0.003, 0.0))
    as_level = Cloud(K=K1, pose=T, source="depth", gain=gain, near=spec.near, far=spec.far)
    z = level * np.float32(gain)                                                                    # what the sums see of the level
    by_hand = Cloud(K=K1, pose=T, source="depth", gain=1.0, near=spec.near, far=spec.far)
    got = fusion.icp_sums_host(level[None], as_level, model, views, 0.1, scale=scale)
    want = fusion.icp_sums_host(z[None], by_hand, model, views, 0.1, scale=scale)
    assert np.array_equal(tc.bits(got), tc.bits(want)) and got[-1] > 200
    assert got[-1] <= (level != 0).sum()                                                            # no zero became a pair


# ---- 3. what is refused ---------------------------------------------------------------------------------------------------------------------------
def test_track_validates_pyramid_and_jump():
    most = fusion.PYRAMID_MAX_LEVELS
    assert isinstance(most, int) and most >= 4
    for bad in ((-1, 2), (2, -1), (0, 0), (0,), (), (1,) * (most + 1), (1.0, 2), (True, 1), 3, "12", ((1, 2),)):
        with pytest.raises(ValueError):
            tc.track(pyramid=bad)
    for bad in (-0.05, float("nan"), "0.05", None, True):
        with pytest.raises(ValueError):
            tc.track(jump=bad)
    ok = tc.track(pyramid=[0, np.int64(3), 2], jump=np.inf)
    assert ok.pyramid == (0, 3, 2) and all(type(i) is int for i in ok.pyramid) and ok.jump == np.inf
    assert tc.track(pyramid=(1,) * most).pyramid == (1,) * most and tc.track(jump=0).jump == 0.0
    assert tc.track().pyramid is None and tc.track().jump == 0.05


def test_the_tracker_refuses_a_pyramid_the_frame_cannot_have():
    host, live = tc.fused(), tc.single()[0]
    track = tc.track(pyramid=(1, 1, 1), min_pairs=16)
    with pytest.raises(ValueError):
        host.track(np.full((1, 2, 3), 0.6, np.float32), tc.spec(), track)                           # level 2 of 2 x 3 holds no pixel
    with pytest.raises(ValueError):
        host.track(np.full((1, 2, 3), 0.6, np.float32), tc.spec(), tc.track(pyramid=(1, 0, 0)))     # also when that level is not run
    for spec in (tc.spec(step=2), tc.spec(near=-0.1), tc.spec(gain=0.0), tc.spec(gain=-1.0)):
        with pytest.raises(ValueError):
            host.track(live, spec, track)
        with pytest.raises(ValueError):
            host.track(live, spec, tc.track(pyramid=(2,)))
        with pytest.raises(ValueError):
            fusion.depth_pyramid_host(live, spec, 1)
    fresh = TsdfHost(tc.volume(), coloured=False)
    with pytest.raises(ValueError):
        fresh.track_clip(tc.clip()[0], tc.spec(near=-0.1), track)
    assert not fresh.weight.any()                                                                   # refused before frame 0 was integrated
    for levels in (0, -1, fusion.PYRAMID_MAX_LEVELS, 1.0, True, None):
        with pytest.raises(ValueError):
            fusion.depth_pyramid_host(live, tc.spec(), levels)
        with pytest.raises(ValueError):
            fusion.rgb_pyramid_host(np.zeros((1, 40, 56, 3), np.uint8), levels)
    with pytest.raises(ValueError):
        fusion.depth_pyramid_host(live, tc.spec(), 1, jump=-1.0)
    with pytest.raises(ValueError):
        fusion.depth_pyramid_host(live, tc.spec(), 1, frame=1)
    with pytest.raises(ValueError):
        fusion.depth_pyramid_host(np.ones((1, 1, 8), np.float32), tc.spec(), 1)                     # a level of size 0
    with pytest.raises(ValueError):
        fusion.rgb_pyramid_host(np.zeros((1, 4, 4), np.uint8), 1)
    with pytest.raises(ValueError):
        fusion.rgb_pyramid_host(np.zeros((1, 4, 4, 3), np.float32), 1)


# ---- 4. the default is unchanged ------------------------------------------------------------------------------------------------------------------
def _same(got, want):
    assert len(got) == len(want) and np.array_equal(tc.bits(got[0]), tc.bits(want[0])) and got[1] == want[1]
    assert np.array_equal(tc.bits(got[2]), tc.bits(want[2])) and got[3] is want[3]
    if len(want) == 5:
        assert np.array_equal(tc.bits(got[4]), tc.bits(want[4]))


@pytest.mark.parametrize("options", [{}, dict(scale=True), dict(min_cos=0.985, huber=0.005)], ids=str)
def test_without_a_pyramid_nothing_changes(options):
    """``Track(pyramid=None)`` gives the bits of a ``Track`` that names no new field, and ``pyramid=(n,)`` those of ``iterations=n``: one level, the
    finest, no pyramid formed.  Both sides run the present ``_track``; that its results are those of before the pyramid is what the untouched
    tracking tests and their goldens hold, not this test."""
    host, (live, _) = tc.fused(), tc.single()
    before = {**tc.TRACK, "iterations": 4, "min_pairs": 16, **options}                              # no new field is named
    want = host.track(live, tc.spec(), Track(**before))
    assert not want[3]
    _same(host.track(live, tc.spec(), Track(**before, pyramid=None)), want)
    _same(host.track(live, tc.spec(), Track(**before, pyramid=None, jump=0.5)), want)               # jump alone does nothing
    _same(host.track(live, tc.spec(), Track(**{**before, "iterations": 1}, pyramid=(4,))), want)    # iterations is not used
    depth, _ = tc.clip()
    clip_want = TsdfHost(tc.volume(), coloured=False).track_clip(depth, tc.spec(), Track(**before))
    for track in (Track(**before, pyramid=None), Track(**before, pyramid=(4,))):
        got = TsdfHost(tc.volume(), coloured=False).track_clip(depth, tc.spec(), track)
        assert np.array_equal(tc.bits(got.poses), tc.bits(clip_want.poses)) and np.array_equal(got.pairs, clip_want.pairs)
        assert np.array_equal(tc.bits(got.rms), tc.bits(clip_want.rms)) and np.array_equal(got.lost, clip_want.lost)
        assert (got.scales is None) == (clip_want.scales is None) and (got.scales is None or np.array_equal(tc.bits(got.scales), tc.bits(clip_want.scales)))


# ---- 5. what it buys ------------------------------------------------------------------------------------------------------------------------------
def test_the_pyramid_reaches_a_pose_the_plain_tracker_does_not():
    """The scene of ``tc.single()`` at five times its motion (0.195 rad, 0.135 of length: some 8 pixels at level 0), the guess the identity,
    ``min_pairs=16``.  The bounds are the issue's: the plain tracker with 19 steps must end more than 0.1 rad from the truth, ``pyramid=(10, 5, 4)``
    within 5e-3 rad and 5e-3 of length.  Measured on the mirror: plain 6.833e-01 rad / 4.986e-01 with 1397 pairs; pyramid 9.230e-04 rad /
    5.531e-04 with 1378 pairs.  At the scene's own motion the pyramid must end no farther from the truth than the plain tracker with as many
    steps: measured 7.077e-05 rad / 1.318e-05 against 9.366e-04 / 4.521e-04."""
    host = tc.fused()
    truth = tc.pose(tc.ROTATION, tc.TRANSLATION, 5.0)
    live = tc.seen_from(truth)
    plain = host.track(live, tc.spec(), tc.track(iterations=19, min_pairs=16))
    coarse = host.track(live, tc.spec(), tc.track(pyramid=(10, 5, 4), min_pairs=16))
    (pr, pt), (cr, ct) = tc.errors(plain[0], truth), tc.errors(coarse[0], truth)
    print(f"\n5x: plain {pr:.3e} rad / {pt:.3e}, {plain[1]} pairs, lost {plain[3]}; pyramid {cr:.3e} rad / {ct:.3e}, {coarse[1]} pairs, lost {coarse[3]}")
    assert pr > 0.1
    assert not coarse[3] and cr < 5e-3 and ct < 5e-3
    live, truth = tc.single()
    plain = host.track(live, tc.spec(), tc.track(iterations=19, min_pairs=16))
    coarse = host.track(live, tc.spec(), tc.track(pyramid=(10, 5, 4), min_pairs=16))
    (pr, pt), (cr, ct) = tc.errors(plain[0], truth), tc.errors(coarse[0], truth)
    print(f"1x: plain {pr:.3e} rad / {pt:.3e}; pyramid {cr:.3e} rad / {ct:.3e}")
    assert not plain[3] and not coarse[3] and cr <= pr and ct <= pt


def test_a_level_without_steps_is_skipped_and_a_lost_level_loses_the_frame():
    host, (live, truth) = tc.fused(), tc.single()
    casts = []
    real = host.raycast

    class Counting:
        """The volume with its ray-casts counted: what ``_track`` asks of it is ``raycast``, ``volume`` and ``coloured``."""
        volume, coloured = host.volume, host.coloured

        def raycast(self, views, **kw):
            casts.append(views.size)
            return real(views, **kw)

    got = fusion._track(Counting(), fusion._IcpHost, live, tc.spec(), tc.track(pyramid=(0, 3, 2), min_pairs=16), 0)
    assert casts == [(10, 14), (20, 28)] and not got[3]                                             # the coarsest first, and level 0 never cast
    assert tc.errors(got[0], truth)[0] < 5e-3
    assert np.allclose(got[0][:3, :3].T @ got[0][:3, :3], np.eye(3), rtol=0.0, atol=1e-15)          # re-orthonormalised after the last level
    lost = host.track(live, tc.spec(), tc.track(pyramid=(2, 2, 2), min_pairs=10 * 14 + 1))          # level 2 cannot have that many pairs
    assert lost[3] and np.array_equal(lost[0], np.eye(4)) and lost[1] <= 140
