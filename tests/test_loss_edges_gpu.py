"""edv_photometric_loss (csrc/loss.hip) and edv_trainer_loss (csrc/loss_trainer.hip) on the cases of tests/loss_inputs.py: clipped, behind-the-camera
and rotated projections, disparities with exact 0.0 and 1.0 and a whole zero frame, constant and affine images, masks with empty frames or a single
pixel, flow that leaves the map or collides on one cell, and the smallest and tile-edge shapes.  tests/test_loss_inputs_cpu.py shows that every case
reaches its edge and that float32 torch passes every gate used here.  Reference: the float64 definition on the CPU.

  (a) every element   value to 5e-6, every gradient element to max(2e-4 of its frame's scale, 3 x the float64 spread under +-8-ulp inputs); no percentile
  (b) structure       exact zeros, no tolerance: all samples clipped, a zero-disparity frame, masked-out frames, a single-pixel mask
  (c) closed forms    constant images and a ramp disparity against formulas that use neither the PyTorch definition nor autograd
  (d) depth terms     the disparity-only call with the depth terms on against the all-leaves call; outward and colliding flow; an emptied selection
  (e) workspace       results do not depend on what the cached workspace held; outputs and an exactly-sized workspace between guard bands"""
import ctypes as C

import pytest
import torch

from endodav_amd import _lib, losses
from tests import loss_inputs as L

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64  # floats on either side of every output and workspace (a multiple of 4: what lies between stays 16-byte aligned)
DISP = [("disp", s) for s in range(4)]


def run_photo(name, cuda, smooth=None):
    c, inp = L.PHOTO[name], L.photo_inputs(name)
    dev = {k: v.to(cuda).requires_grad_(True) for k, v in inp["disps"].items()}
    loss = losses.photometric_loss_hip(dev, inp["frames"].to(cuda), inp["K"].to(cuda), inp["inv_K"].to(cuda), inp["T_prev"].to(cuda), inp["T_next"].to(cuda),
                                       clips=c.B, disparity_smoothness=c.smooth if smooth is None else smooth)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), {k: v.grad.cpu() for k, v in dev.items()}


def run_trainer(name, cuda, want=None, flow="", wts=None):
    c = L.TRAINER[name]
    inp, disps = L.trainer_inputs(name, flow)
    keys = L.trainer_leaves(inp, disps)
    want = set(keys) if want is None else want
    leaves = {k: v.to(cuda).clone().requires_grad_(k in want) for k, v in keys.items()}
    inp_d = {k: v.to(cuda) for k, v in inp.items()}
    inp_d.update({k: v for k, v in leaves.items() if k not in DISP})
    out = losses.trainer_losses_hip({k: leaves[k] for k in DISP}, inp_d, wts or c.wts())
    if bool(torch.isfinite(out["loss"])):
        out["loss"].backward()
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, {k: (None if v.grad is None else v.grad.cpu()) for k, v in leaves.items()}


# ---- (a) every element --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in L.PHOTO_CASES])
def test_photometric_loss_every_element(lib, cuda, name):
    val, g, moved = L.photo_reference(name)
    loss, got = run_photo(name, cuda)
    print()
    bad = L.check_gate(L.PHOTO[name], float(loss), got, val, g, moved, "kernel")
    L.check_gate(L.PHOTO[name], *L.photo_eval(name, torch.float32), val, g, moved, "fp32 torch")  # printed for comparison; asserted in test_loss_inputs_cpu.py
    assert not bad, bad


@pytest.mark.parametrize("name", [c.name for c in L.TRAINER_CASES])
def test_trainer_loss_every_element(lib, cuda, name):
    val, g, moved = L.trainer_reference(name)
    out, got = run_trainer(name, cuda)
    print()
    bad = L.check_gate(L.TRAINER[name], out, got, val, g, moved, "kernel")
    L.check_gate(L.TRAINER[name], *L.trainer_eval(name, torch.float32), val, g, moved, "fp32 torch")
    assert not bad, bad


# ---- (b) exact structure --------------------------------------------------------------------------------------------------------------------------
def test_all_samples_clipped_gives_exactly_zero_gradients(lib, cuda):
    _, got = run_photo("out_of_view_20x28", cuda)
    assert L.PHOTO["out_of_view_20x28"].smooth == 0.0 and all(float(v.abs().max()) == 0.0 for v in got.values())
    assert not L.TRAINER["out_of_view_32x32"].wts().disparity_smoothness and not L.TRAINER["out_of_view_32x32"].wts().tune_temporal
    _, got = run_trainer("out_of_view_32x32", cuda)
    for k, v in got.items():
        if k in ("K", "inv_K") or k[0] in ("disp", "cam_T_cam"):  # whatever reaches them comes through the colour samples
            assert float(v.abs().max()) == 0.0, k
        else:
            assert float(v.abs().max()) > 0.0, k


def test_a_zero_disparity_frame_is_finite_and_has_exactly_no_smoothness_gradient(lib, cuda):
    loss, strong = run_photo("zero_frame_20x28", cuda, smooth=1.0)
    _, none = run_photo("zero_frame_20x28", cuda, smooth=0.0)
    assert bool(torch.isfinite(loss))
    for k in strong:  # sign(0) = 0 and S = sum g D = 0: the term adds exactly nothing on the zero frame, and something on the others
        assert bool(torch.isfinite(strong[k]).all()) and torch.equal(strong[k][1], none[k][1]) and not torch.equal(strong[k][0], none[k][0]), k
    out, got = run_trainer("one_frame_17x33", cuda)
    assert all(bool(torch.isfinite(v).all()) for v in out.values()) and all(bool(torch.isfinite(v).all()) for v in got.values())


def test_masked_out_frames_get_exactly_zero_gradients(lib, cuda):
    _, got = run_trainer("one_frame_17x33", cuda)
    for k, v in got.items():
        if isinstance(k, tuple) and k[0] in ("refined", "transform"):
            assert float(v[0].abs().max()) == 0.0 and float(v[2].abs().max()) == 0.0 and float(v[1].abs().max()) > 0.0, k


def test_a_single_pixel_mask_reaches_three_pixels_of_transform(lib, cuda):
    c = L.TRAINER["single_pixel_32x32"]
    _, got = run_trainer("single_pixel_32x32", cuda)
    for fid in losses.FIDS:
        y, x = L.SINGLE_PIXEL(c.H, c.W, fid)
        for s in range(4):
            nz = got[("transform", "high", s, fid)].abs().amax(1).nonzero().tolist()
            assert sorted(nz) == sorted([[0, y, x], [0, y, x + 1], [0, y + 1, x]]), (s, fid, nz)


# ---- (c) closed forms -------------------------------------------------------------------------------------------------------------------------------
def smooth_gradient_of_a_ramp(case, s, n, h, w, hc, wc, weight):
    """d (weight / 4 / 2^s (mean |d_x norm| + mean |d_y norm|)) / d disp of the ramp whose colour image is constant, by hand: norm = D / (m + 1e-7),
    every x pair has the same sign, no y pair differs.  d/dD_p = (g_p - sum_q g_q D_q / (m + 1e-7) / P) / (m + 1e-7) with g = -1/Nx on the first
    column, +1/Nx on the last one (the inner pixels' two pairs cancel)."""
    assert (h, w) == (hc, wc)
    step, mean = L.ramp_span_mean(w)
    den = mean + 1e-7
    D = (0.125 + torch.arange(w, dtype=torch.float64) * step).view(1, 1, 1, w).expand(n, 1, h, w)
    g = torch.zeros(n, 1, h, w, dtype=torch.float64)
    g[..., 0], g[..., -1] = -1.0 / (n * h * (w - 1)), 1.0 / (n * h * (w - 1))
    S = (g * D).sum((1, 2, 3), keepdim=True)
    return weight / 4 / 2 ** s * (g / den - S / (den * den) / (h * w))


def test_photometric_closed_form(lib, cuda):
    c = L.PHOTO["constant_33x65"]
    loss, got = run_photo(c.name, cuda)
    cf = L.photo_closed_form(c.name)
    print(f"\n[{c.name}] kernel {float(loss)!r}, closed form {cf!r}: {abs(float(loss) - cf) / cf:.2e} relative")
    assert L.value_ok(float(loss), cf)
    for s, (h, w) in enumerate(c.sizes):
        want = smooth_gradient_of_a_ramp(c, s, c.B * c.T, h, w, c.H, c.W, c.smooth)  # the reprojection term adds nothing: a constant neighbour
        err = float((got[("disp", s)].double() - want).abs().max()) / float(want.abs().max())
        print(f"  disp_{s}: {err:.2e} of the smoothness gradient's scale")
        assert err <= 1e-6, (s, err)
    _, got0 = run_photo(c.name, cuda, smooth=0.0)
    assert all(float(v.abs().max()) == 0.0 for v in got0.values())


def test_trainer_closed_form(lib, cuda):
    c = L.TRAINER["constant_32x32"]
    out, got = run_trainer(c.name, cuda)
    cf = L.trainer_closed_form(c.name)
    print()
    for k, v in cf.items():
        print(f"  [{c.name}] {k}: kernel {float(out[k])!r}, closed form {v!r}: {abs(float(out[k]) - v) / v:.2e} relative")
        assert L.value_ok(float(out[k]), v), k
    for s, (h, w) in enumerate(c.sizes):
        want = smooth_gradient_of_a_ramp(c, s, c.n, h, w, c.H >> s, c.W >> s, c.wts().disparity_smoothness)
        err = float((got[("disp", s)].double() - want).abs().max()) / float(want.abs().max())
        print(f"  disp_{s}: {err:.2e} of the smoothness gradient's scale")
        assert err <= 1e-6, (s, err)


# ---- (d) the missing instantiation and the depth terms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in L.TRAINER_CASES if c.wts().tune_temporal and c.wts().depth_reproj and c.flow != "collide"])
def test_disparity_only_gradients_with_the_depth_terms_on(lib, cuda, name):
    """What a user who freezes poses and intrinsics gets with the depth-reprojection term on, on every table row that has it (the colliding flow
    apart: its atomics alone move a call by more than the bound).  The bound is the one the existing test holds the default weights to, 1e-6 of the
    tensor's scale.

    This test found that geom_bwd_kernel<POSE = false, DREPROJ = true> -- the same arithmetic as <true, true>, contracted differently by the compiler
    -- moved disp_0 by 1.06e-6 of scale on depth_16x16 (and 1.24e-6 on rotated_33x65 with outward flow); the host code now launches <true, true>
    whenever the term is on and leaves the pose partials unfinished, so that the two calls differ by the order of their atomics only."""
    w = L.TRAINER[name].wts()
    assert w.tune_temporal and w.depth_reproj
    full, gf = run_trainer(name, cuda)
    only, go = run_trainer(name, cuda, want=set(DISP))
    assert all(go[k] is None for k in go if k not in DISP)
    assert abs(float(only["loss"]) - float(full["loss"])) <= 1e-6 * abs(float(full["loss"]))
    for k in DISP:
        scale = float(gf[k].abs().max())
        err = float((go[k] - gf[k]).abs().max())
        print(f"\n[{name}] {k}: {err / scale:.2e} of scale between the disparity-only and the all-leaves call")
        assert err <= 1e-6 * scale, (k, err / scale)


@pytest.mark.parametrize("name,flow", [("depth_16x16", "collide"), ("rotated_33x65", "outward")])
def test_trainer_loss_every_element_with_the_other_flow(lib, cuda, name, flow):
    val, g, moved = L.trainer_reference(name, flow)
    for call in range(2):  # atomics: two calls may differ in the last bits; each is held to the reference, they are not compared
        out, got = run_trainer(name, cuda, flow=flow)
        print()
        bad = L.check_gate(L.TRAINER[name], out, got, val, g, moved, f"kernel, {flow} flow, call {call}")
        assert not bad, bad


def test_depth_terms_stay_finite_and_an_emptied_selection_is_nan(lib, cuda):
    for name in ("depth_16x16", "behind_33x65"):
        out, _ = run_trainer(name, cuda)
        ref = L.trainer_reference(name)[0]
        for s in range(4):
            for k in (f"loss/loss_depth_reproj/{s}", f"loss/loss_depth_flow/{s}"):
                assert bool(torch.isfinite(out[k])) and ref[k] > 0 and L.value_ok(float(out[k]), ref[k]), (name, k, float(out[k]), ref[k])
    out, _ = run_trainer("depth_16x16", cuda, flow="empty_next")
    ref, _ = L.trainer_eval("depth_16x16", flow="empty_next")
    for s in range(4):
        k = f"loss/loss_depth_flow/{s}"
        assert ref[k] != ref[k] and bool(torch.isnan(out[k])), (k, ref[k], float(out[k]))
        k = f"loss/loss_depth_reproj/{s}"
        assert L.value_ok(float(out[k]), ref[k]), (k, float(out[k]), ref[k])
    assert bool(torch.isnan(out["loss"])) and ref["loss"] != ref["loss"]


# ---- (e) workspace hygiene ----------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def refill_workspaces(value):
    assert losses._WS
    for ws in losses._WS.values():
        ws.fill_(value)


def guarded(n, cuda, init=None):
    """(buffer, view of n floats between two NaN guard bands); the view starts as NaN or as `init`."""
    big = torch.full((n + 2 * GUARD,), NAN, device=cuda)
    if init is not None:
        big[GUARD:GUARD + n] = init.reshape(-1).to(cuda)
    return big, big[GUARD:GUARD + n]


def guards_intact(big, n):
    return bool(torch.isnan(big[:GUARD]).all() and torch.isnan(big[GUARD + n:]).all())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def photo_direct(lib, cuda, name, fill):
    """edv_photometric_loss with the loss, the four gradients and a workspace of exactly edv_photometric_loss_workspace bytes between guard bands."""
    c, inp = L.PHOTO[name], L.photo_inputs(name)
    n = c.B * c.T
    d = [inp["disps"][k].to(cuda).contiguous() for k in DISP]
    fr, K, iK, Tp, Tn = (inp[k].to(cuda).contiguous() for k in ("frames", "K", "inv_K", "T_prev", "T_next"))
    nbytes = lib.edv_photometric_loss_workspace(c.B, c.T, c.H, c.W)
    assert nbytes > 0 and nbytes % 16 == 0
    ws_big, ws = guarded(nbytes // 4, cuda, torch.full((nbytes // 4,), fill))
    loss_big, loss = guarded(4, cuda)
    gr = [guarded(x.numel(), cuda) for x in d]
    dptr, gptr = (C.c_void_p * 4)(*[x.data_ptr() for x in d]), (C.c_void_p * 4)(*[b[1].data_ptr() for b in gr])
    dh, dw = (C.c_int32 * 4)(*[x.shape[-2] for x in d]), (C.c_int32 * 4)(*[x.shape[-1] for x in d])
    _lib.check(lib.edv_photometric_loss(fr.data_ptr(), dptr, dh, dw, c.B, c.T, c.H, c.W, K.data_ptr(), iK.data_ptr(), Tp.data_ptr(), Tn.data_ptr(), losses.MIN_DEPTH,
                                        losses.MAX_DEPTH, c.smooth, loss.data_ptr(), gptr, ws.data_ptr(), nbytes, st()), "edv_photometric_loss")
    torch.cuda.synchronize()
    assert guards_intact(ws_big, nbytes // 4), "a write outside the workspace"
    assert bool(torch.isnan(loss_big[GUARD + 1:]).all() and torch.isnan(loss_big[:GUARD]).all()), "a write beside the loss"
    for s, (big, view) in enumerate(gr):
        assert guards_intact(big, d[s].numel()), f"a write outside the gradient of disp_{s}"
    return loss[0].cpu(), {k: gr[s][1].view(d[s].shape).cpu() for s, k in enumerate(DISP)}


@pytest.mark.parametrize("name", ["benign_33x65", "two_frames_64x32"])
def test_photometric_loss_reads_only_workspace_it_has_written(lib, cuda, name):
    first = run_photo(name, cuda)
    for value in (NAN, 1e30):
        refill_workspaces(value)
        again = run_photo(name, cuda)
        assert same_bits(first[0], again[0]) and all(same_bits(first[1][k], again[1][k]) for k in DISP), f"the result depends on a workspace filled with {value}"
    for value in (NAN, 1e30, 0.0):  # exactly the advertised bytes, between guard bands, whatever they held
        direct = photo_direct(lib, cuda, name, value)
        assert same_bits(first[0], direct[0]) and all(same_bits(first[1][k], direct[1][k]) for k in DISP), f"exact-size workspace filled with {value}"


def trainer_direct(lib, cuda, name, fill):
    """edv_trainer_loss with the 29 values, every gradient buffer and a workspace of exactly edv_trainer_loss_workspace bytes between guard bands."""
    c = L.TRAINER[name]
    inp, disps = L.trainer_inputs(name)
    w = c.wts()
    t = {k: v.to(cuda).contiguous() for k, v in inp.items()}
    d = {k: v.to(cuda).contiguous() for k, v in disps.items()}
    a, g, wt = _lib.TrainerLossInputs(), _lib.TrainerLossGrads(), _lib.TrainerLossWeights()
    bufs = {}

    def gbuf(key, like):
        bufs[key] = guarded(like.numel(), cuda) + (like.shape,)
        return bufs[key][1].data_ptr()

    for s in range(4):
        a.color[s] = t[("color", 0, s)].data_ptr()
        a.disp[s], a.disp_h[s], a.disp_w[s] = d[("disp", s)].data_ptr(), d[("disp", s)].shape[-2], d[("disp", s)].shape[-1]
        g.disp[s] = gbuf(("disp", s), d[("disp", s)])
        for i, fid in enumerate(losses.FIDS):
            a.refined[s][i], a.transform[s][i] = t[("refined", s, fid)].data_ptr(), t[("transform", "high", s, fid)].data_ptr()
            a.registration[s][i], a.position[s][i] = t[("registration", s, fid)].data_ptr(), None
            g.refined[s][i] = gbuf(("refined", s, fid), t[("refined", s, fid)])
            g.transform[s][i] = gbuf(("transform", "high", s, fid), t[("transform", "high", s, fid)])
    for i, fid in enumerate(losses.FIDS):
        a.color_nb[i], a.T[i], a.mask[i] = t[("color", fid, 0)].data_ptr(), t[("cam_T_cam", 0, fid)].data_ptr(), t[("occu_mask_backward", 0, fid)].data_ptr()
        g.T[i] = gbuf(("cam_T_cam", 0, fid), t[("cam_T_cam", 0, fid)])
    a.K, a.invK = t["K"].data_ptr(), t["inv_K"].data_ptr()
    g.K, g.invK = gbuf("K", t["K"]), gbuf("inv_K", t["inv_K"])
    wt.disparity_smoothness, wt.transform_constraint, wt.transform_smoothness = w.disparity_smoothness, w.transform_constraint, w.transform_smoothness
    wt.depth_reproj, wt.depth_flow, wt.tune_temporal, wt.min_depth, wt.max_depth = w.depth_reproj, w.depth_flow, int(w.tune_temporal), w.min_depth, w.max_depth
    assert not wt.tune_temporal  # the options' defaults: no flow input, no atomics
    nbytes = lib.edv_trainer_loss_workspace(c.n, c.H, c.W)
    assert nbytes > 0 and nbytes % 16 == 0
    ws_big, ws = guarded(nbytes // 4, cuda, torch.full((nbytes // 4,), fill))
    val_big, values = guarded(29, cuda)
    _lib.check(lib.edv_trainer_loss(C.byref(a), c.n, c.H, c.W, C.byref(wt), values.data_ptr(), C.byref(g), ws.data_ptr(), nbytes, st()), "edv_trainer_loss")
    torch.cuda.synchronize()
    assert guards_intact(ws_big, nbytes // 4), "a write outside the workspace"
    assert guards_intact(val_big, 29), "a write outside the 29 values"
    for k, (big, view, shape) in bufs.items():
        assert guards_intact(big, view.numel()), f"a write outside the gradient of {k}"
    return values.cpu(), {k: view.view(shape).cpu() for k, (big, view, shape) in bufs.items()}


@pytest.mark.parametrize("name", ["border_17x33", "benign_16x16"])
def test_trainer_loss_reads_only_workspace_it_has_written(lib, cuda, name):
    assert not L.TRAINER[name].weights  # the default weights: bit-reproducible
    first = run_trainer(name, cuda)
    for value in (NAN, 1e30):
        refill_workspaces(value)
        again = run_trainer(name, cuda)
        assert all(same_bits(first[0][k], again[0][k]) for k in first[0]) and all(same_bits(first[1][k], again[1][k]) for k in first[1]), \
            f"the result depends on a workspace filled with {value}"
    for value in (NAN, 1e30, 0.0):
        values, grads = trainer_direct(lib, cuda, name, value)
        assert same_bits(values[28], first[0]["loss"]) and all(same_bits(grads[k], first[1][k]) for k in grads), f"exact-size workspace filled with {value}"
