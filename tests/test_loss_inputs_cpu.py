"""What tests/test_loss_edges_gpu.py takes for granted, checked without a GPU on the cases of tests/loss_inputs.py:

  reach        every case hits what its table row claims, measured on the float64 definition: the share of clipped samples, the share with Z < 0 and
               the distance of the nearest pixel from Z = 0, the corners of the depth samples that fall outside, the depth-consistency counts, the SSIM
               tiles and idle sum chunks
  passable     the definition itself, evaluated in float32 (losses.photometric_loss / losses.trainer_losses on the CPU), passes every gate the kernels
               are held to, with zero violations: a gate that float32 arithmetic cannot pass would be a wrong gate or a wrong case
  narrow       the band decides under 20 % of the elements of every tensor loss_inputs.band_capped names (a coarse disparity map sums a block of frame
               pixels, so one kink pixel in the block puts it in the band: those maps are held by the gate without the cap)
  closed form  the formulas of loss_inputs.*_closed_form agree with the float64 definition to 1e-12 relative, before a kernel sees either
  structure    the exact zeros the GPU test asserts are exact zeros of the definition"""
import pytest
import torch

from endodav_amd import losses
from tests import loss_inputs as L

PHOTO_IDS = [c.name for c in L.PHOTO_CASES]
TRAINER_IDS = [c.name for c in L.TRAINER_CASES]


# ---- reach ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PHOTO_IDS)
def test_photometric_case_reaches_what_its_row_claims(name):
    c, inp, r = L.PHOTO[name], L.photo_inputs(name), L.photo_reach(name)
    print(f"\n[{name}] {c.reaches}: {r}")
    if c.camera == "out_of_view":
        assert r["clip_x"] == 1.0 and r["clip_y"] == 1.0
    elif c.camera == "half_out_x":
        assert 0.2 < r["clip_x"] < 0.45 and r["on_last"] > 0.05
    elif c.camera == "half_out_y":
        assert 0.2 < r["clip_y"] < 0.45 and r["on_last"] > 0.05
    if c.camera == "behind":
        assert 0.05 < r["neg_z"] < 0.6 and r["min_abs_z"] >= 1e-3, r  # near pixels behind, far ones not, none within 1e-3 of Z = 0
    else:
        assert r["neg_z"] == 0.0 and r["min_abs_z"] > 0.05
    for s, (h, w) in enumerate(c.sizes):
        d = inp["disps"][("disp", s)]
        assert d.shape == (c.B * c.T, 1, h, w) and d.dtype == torch.float32 and float(d.min()) >= 0.0 and float(d.max()) <= 1.0
        if c.disparity == "with_0_and_1" and h * w >= 100:
            assert int((d == 0).sum()) > 0 and int((d == 1).sum()) > 0
        if c.disparity == "zero_frame":
            assert float(d[1].abs().max()) == 0.0 and float(d[0].min()) > 0.0
        if c.disparity == "ramp" and w > 1:
            step = d[..., 1:] - d[..., :-1]
            assert float(step.min()) == float(step.max()) == L.ramp_span_mean(w)[0] and abs(float(d.double().mean()) - L.ramp_span_mean(w)[1]) < 1e-15
    fr = inp["frames"]
    assert float(fr.min()) >= 0.0 and float(fr.max()) <= 1.0
    if c.image == "constant":
        assert all(float(fr[f, ch].min()) == float(fr[f, ch].max()) for f in range(fr.shape[0]) for ch in range(3))
    ty, tx = L.tiles(c.H, c.W)
    if name.endswith("33x65"):
        assert (ty, tx) == (2, 3) and c.H % 32 == 1 and c.W % 32 == 1  # the last tile row / column is one pixel thick
    if name == "two_frames_64x32":
        assert (ty, tx) == (2, 1) and c.T == 2
    if name == "tiny_3x3":
        assert (1, 1) in c.sizes and (1, 2) in c.sizes and lib_accepts(c)
    if name == "larger_maps_20x28":
        assert all(h >= c.H and w >= c.W and (h, w) != (c.H, c.W) for h, w in c.sizes)


def lib_accepts(c):
    return c.T >= 2 and c.H >= 3 and c.W >= 3  # edv_photometric_loss's own limits


@pytest.mark.parametrize("name", TRAINER_IDS)
def test_trainer_case_reaches_what_its_row_claims(name):
    c, r = L.TRAINER[name], L.trainer_reach(name)
    inp, disps = L.trainer_inputs(name)
    w = c.wts()
    print(f"\n[{name}] {c.reaches}: {r}")
    if c.camera == "out_of_view":
        assert r["clip"] == 1.0
    if c.camera == "behind":
        assert 0.05 < r["neg_z"] < 0.6 and r["min_abs_z"] >= 1e-3, r
    else:
        assert r["neg_z"] == 0.0
    if w.tune_temporal and w.depth_reproj:
        assert len(r["drp_count"]) == 8 and min(r["drp_count"]) > 0, r["drp_count"]  # every scale, both neighbours: a mean of something
    if w.tune_temporal and w.depth_flow:
        assert len(r["dfl_count"]) == 8 and min(r["dfl_count"]) > 0, r["dfl_count"]
    if c.flow == "outward":
        k = r["flow_corners"]
        # 0, 2 (one coordinate out), 3 (both out by less than a pixel) and 4 corners outside; exactly one corner outside cannot happen on a rectangle
        assert k[0] > 0 and k[2] > 0 and k[3] > 0 and k[4] > 0 and k[1] == 0, k
        assert 0.3 < k[4] / sum(k) < 0.7, k
        assert max(r["dfl_count"]) < 0.6 * (c.n - 1) * c.H * c.W
    if c.flow == "collide":
        fl = inp[("position", "high", 0, 1)].double()
        ys, xs = torch.meshgrid(torch.arange(c.H, dtype=torch.float64), torch.arange(c.W, dtype=torch.float64), indexing="ij")
        ty, tx = ys + fl[:, 0], xs + fl[:, 1]
        assert float(ty.max() - ty.min()) < 1e-5 and float(tx.max() - tx.min()) < 1e-5 and 0 < float(tx.mean()) % 1 and 0 < float(ty.mean()) % 1
    for fid in losses.FIDS:
        m = inp[("occu_mask_backward", 0, fid)]
        assert set(m.unique().tolist()) <= {0.0, 1.0}
        if c.mask == "single_pixel":
            assert float(m.sum()) == 1.0 and float(m[:, :, :, :-1].sum()) == 1.0 and float(m[:, :, :-1, :].sum()) == 1.0
        if c.mask == "one_frame_only":
            assert float(m[0].sum()) == 0.0 and float(m[2].sum()) == 0.0 and float(m[1].sum()) > 0.5 * c.H * c.W
        if c.mask == "border_band":
            assert float(m[:, :, 2:-2, 2:-2].sum()) == 0.0 and float(m.sum()) == c.n * (c.H * c.W - (c.H - 4) * (c.W - 4))
    same = [tuple(disps[("disp", s)].shape[-2:]) == (c.H, c.W) for s in range(4)]
    same_c = [tuple(disps[("disp", s)].shape[-2:]) == (c.H >> s, c.W >> s) for s in range(4)]
    if name.endswith("16x16"):
        assert (c.H >> 3) * (c.W >> 3) == 4 and 64 - (c.H >> 3) * (c.W >> 3) == 60 and L.tiles(c.H, c.W) == (1, 1)  # 60 idle chunks of frame_sum_kernel's 64
    if name == "behind_33x65" or name == "rotated_33x65":
        assert not any(same) and not any(same_c)  # both resize paths at every scale
    if name.endswith("32x32"):
        assert all(same_c) and L.tiles(c.H, c.W) == (1, 1)
    if name.endswith("32x64"):
        assert all(same)
    if name.endswith("17x33"):
        assert L.tiles(c.H, c.W) == (1, 2) and c.W % 32 == 1


def test_an_emptied_selection_is_nan_in_the_definition():
    val, _ = L.trainer_eval("depth_16x16", flow="empty_next")
    r = L.trainer_reach("depth_16x16", flow="empty_next")
    assert min(r["dfl_count"][1::2]) == max(r["dfl_count"][1::2]) == 0 and min(r["dfl_count"][0::2]) > 0  # the next-frame neighbour only
    assert all(val[f"loss/loss_depth_flow/{s}"] != val[f"loss/loss_depth_flow/{s}"] for s in range(4))
    assert all(val[f"loss/loss_depth_reproj/{s}"] == val[f"loss/loss_depth_reproj/{s}"] for s in range(4))


# ---- the gate is passable and narrow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PHOTO_IDS)
def test_float32_torch_passes_the_photometric_gate(name):
    val, g, moved = L.photo_reference(name)
    v32, g32 = L.photo_eval(name, torch.float32)
    assert not L.check_gate(L.PHOTO[name], v32, g32, val, g, moved, "fp32 torch")


@pytest.mark.parametrize("name", TRAINER_IDS)
def test_float32_torch_passes_the_trainer_gate(name):
    val, g, moved = L.trainer_reference(name)
    v32, g32 = L.trainer_eval(name, torch.float32)
    assert not L.check_gate(L.TRAINER[name], v32, g32, val, g, moved, "fp32 torch")


@pytest.mark.parametrize("name,flow", [("depth_16x16", "collide"), ("rotated_33x65", "outward")])
def test_float32_torch_passes_the_trainer_gate_with_the_other_flow(name, flow):
    val, g, moved = L.trainer_reference(name, flow)
    v32, g32 = L.trainer_eval(name, torch.float32, flow=flow)
    assert not L.check_gate(L.TRAINER[name], v32, g32, val, g, moved, f"fp32 torch, {flow} flow")


# ---- closed forms -------------------------------------------------------------------------------------------------------------------------------
def test_photometric_closed_form_is_the_definition():
    val, g, _ = L.photo_reference("constant_33x65")
    cf = L.photo_closed_form("constant_33x65")
    assert abs(cf - val) <= 1e-12 * abs(val), (cf, val)
    # and the reprojection term has no disparity gradient: a constant neighbour looks the same wherever it is sampled
    _, g0 = L.photo_eval("constant_33x65", smooth=0.0)
    assert all(float(v.abs().max()) == 0.0 for v in g0.values())
    v32, g32 = L.photo_eval("constant_33x65", torch.float32)
    assert L.value_ok(v32, cf)
    for k in g:  # float32 torch meets the GPU test's bound on the same comparison
        assert float((g32[k].double() - g[k]).abs().max()) <= 1e-6 * float(g[k].abs().max()), k


def test_trainer_closed_form_is_the_definition():
    val, g, _ = L.trainer_reference("constant_32x32")
    cf = L.trainer_closed_form("constant_32x32")
    for k, v in cf.items():
        assert abs(v - val[k]) <= 1e-12 * abs(val[k]), (k, v, val[k])
    v32, g32 = L.trainer_eval("constant_32x32", torch.float32)
    assert all(L.value_ok(v32[k], v) for k, v in cf.items())
    _, g0 = L.trainer_eval("constant_32x32", wts=L.TRAINER["constant_32x32"].wts(disparity_smoothness=0.0))
    assert all(float(g0[("disp", s)].abs().max()) == 0.0 for s in range(4))
    for s in range(4):
        k = ("disp", s)
        assert float((g32[k].double() - g[k]).abs().max()) <= 1e-6 * float(g[k].abs().max()), k


# ---- the exact zeros of the definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_structure_of_the_definition(dtype):
    _, g = L.photo_eval("out_of_view_20x28", dtype)
    assert all(float(v.abs().max()) == 0.0 for v in g.values())
    _, g = L.photo_eval("zero_frame_20x28", dtype, smooth=1.0)
    _, g0 = L.photo_eval("zero_frame_20x28", dtype, smooth=0.0)
    for k in g:  # the zero frame's smoothness gradient is exactly zero: with and without the term its gradient is the same
        assert bool(torch.isfinite(g[k]).all()) and torch.equal(g[k][1], g0[k][1]) and not torch.equal(g[k][0], g0[k][0]), k
    _, g = L.trainer_eval("out_of_view_32x32", dtype)
    for k, v in g.items():
        if k in ("K", "inv_K") or k[0] in ("disp", "cam_T_cam"):
            assert float(v.abs().max()) == 0.0, k
    _, g = L.trainer_eval("one_frame_17x33", dtype)
    for k, v in g.items():
        if isinstance(k, tuple) and k[0] in ("refined", "transform"):
            assert float(v[0].abs().max()) == 0.0 and float(v[2].abs().max()) == 0.0 and float(v[1].abs().max()) > 0.0, k
    c = L.TRAINER["single_pixel_32x32"]
    _, g = L.trainer_eval("single_pixel_32x32", dtype)
    for fid in losses.FIDS:
        y, x = L.SINGLE_PIXEL(c.H, c.W, fid)
        for s in range(4):
            nz = g[("transform", "high", s, fid)].abs().amax(1).nonzero().tolist()
            assert sorted(nz) == sorted([[0, y, x], [0, y, x + 1], [0, y + 1, x]]), (s, fid, nz)
