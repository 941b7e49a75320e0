"""What tests/test_conv_edges_gpu.py relies on, checked without a GPU: the input classes of tests/conv_inputs.py are what they claim (the integer
operands are exact in fp32 in any order, the cancelling ones cancel, the scaled ones stay far from the ends of the exponent range), torch's own
fp32 operators pass the gates the kernels are held to, the integer operands cannot hide the classical indexing mistakes, and every shape reaches
the kernel variant its route names (the dispatch is restated in Python beside the shapes and compared with the library's own planner)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from . import conv_inputs as V

CONV = 2  # edv_split_plan kind
FWD = V.fwd_cases()
FWD_IDS = [f"{route}-{'x'.join(map(str, shape))}" for route, shape, _ in FWD]
U = V.U


def plan(lib, tiles, k_tiles):
    out = (C.c_int64 * 8)()
    assert lib.edv_split_plan(CONV, tiles, V.CONV_SLOTS, k_tiles, out) == 0
    return dict(zip(("split", "grid", "whole_rounds", "chunk", "nsplit", "stride", "units", "ws"), out))


def in_u(err):
    return f"rms {err[0] / U:.2f}u max {err[1] / U:.2f}u"


# ---- 1. the classes are what they claim --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,admitted", FWD, ids=FWD_IDS)
def test_exact_int_forward_is_exact_in_fp32(route, shape, admitted):
    for ep in admitted:
        ops = V.fwd_operands("exact_int", shape, ep)
        ref = V.fwd_reference("exact_int", shape, ep)[0]
        assert V.fwd_exact_bound(shape, ep) < V.EXACT_LIMIT
        assert torch.equal(ref, ref.round()) and ref.abs().max() <= V.fwd_exact_bound(shape, ep)
        assert torch.equal(V.fwd_apply(*ops, ep, shape[5], torch.float32).long(), ref.long())
        assert ref.abs().max() > 100  # not a degenerate problem


@pytest.mark.parametrize("shape", V.DOT_SHAPES)
def test_exact_int_dot_is_exact_in_fp32(shape):
    assert V.dot_exact_bound(shape) < V.EXACT_LIMIT and V.dot_exact_bound(V.DOT_SHAPES[1]) < 1.25e6
    for ep in V.DOT_EPILOGUES:
        for act2 in V.DOT_ACT2:
            ops, ref = V.dot_operands("exact_int", shape, ep), V.dot_reference("exact_int", shape, ep, act2)[0]
            assert ref.abs().max() <= V.dot_exact_bound(shape)
            assert torch.equal(V.dot_apply(ops, ep, act2, torch.float32).long(), ref.long())


def test_exact_int_backward_is_exact_in_fp32():
    for shape in V.BWD_DATA_SHAPES + tuple((Fr, H, W, Cc, Cc) for Fr, H, W, Cc in V.S2_BWD_SHAPES):
        stride = 1 if shape in V.BWD_DATA_SHAPES else 2
        dy, w, ref, mag, err = V.bwd_data_class("exact_int", shape, stride)
        assert 9 * shape[4] * 16 < V.EXACT_LIMIT and err == (0.0, 0.0) and torch.equal(ref, ref.round())
        # the transposed convolution is the gradient autograd takes
        x = torch.zeros(shape[0], shape[3], shape[1], shape[2], dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(x, w.double(), None, stride=stride, padding=1), [x], dy.double())
        assert torch.equal(V.nhwc(g), ref)
    for shape in V.WGRAD_SHAPES:
        x, dy, base, ref, mag, err = V.wgrad_class("exact_int", shape)
        pixels = shape[0] * shape[1] * shape[2]
        assert pixels <= 1560 and pixels * 32 + 16 < V.EXACT_LIMIT and err == (0.0, 0.0) and torch.equal(ref, ref.round())
        wt = torch.zeros(shape[4], shape[3], 3, 3, dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(x.double(), wt, padding=1), [wt], dy.double())
        assert torch.equal(g + (0 if base is None else base.double()), ref)
    for shape in V.CONVT_SHAPES:
        x, wt, b, dy, y, dx = V.convT_class(shape)
        Cc, s = shape[3], shape[4]
        assert Cc * 32 + 16 < V.EXACT_LIMIT and s * s * Cc * 16 < V.EXACT_LIMIT
        assert torch.equal(V.nhwc(F.conv_transpose2d(x, wt, b, stride=s)).long(), y.long())
        xs = x.double().requires_grad_(True)
        (g,) = torch.autograd.grad(F.conv_transpose2d(xs, wt.double(), b.double(), stride=s), [xs], dy.double())
        assert torch.equal(V.nhwc(g), dx) and torch.equal(V.nhwc(F.conv2d(dy, wt, None, stride=s)).long(), dx.long())


def cancelling_median(ref, mag):
    return (ref.abs() / mag).median().item()


@pytest.mark.parametrize("index", range(len(FWD)), ids=FWD_IDS)
def test_cancelling_operands_cancel(index):
    """A condition on the input, not a measurement: the median |ref| / mag is at most 1e-5."""
    route, shape, admitted = FWD[index]
    ep = V.cycled_epilogue(index, "cancelling", admitted)
    ref, mag, _ = V.fwd_reference("cancelling", shape, ep)
    m = cancelling_median(ref, mag)
    print(f"\n[cancelling {route} {shape} {ep}] median |ref| / mag = {m:.2e}")
    assert m <= 1e-5


def test_cancelling_operands_cancel_on_the_other_routes():
    for shape in V.DOT_SHAPES:
        for ep in V.DOT_EPILOGUES:
            ref, mag, _ = V.dot_reference("cancelling", shape, ep, "none")
            assert cancelling_median(ref, mag) <= 1e-5
    for shape in V.BWD_DATA_SHAPES:
        dy, w, ref, mag, _ = V.bwd_data_class("cancelling", shape)
        assert cancelling_median(ref, mag) <= 1e-5, shape
    for shape in V.WGRAD_SHAPES:
        if V.wgrad_has_class("cancelling", shape):
            ref, mag = V.wgrad_class("cancelling", shape)[3:5]
            assert cancelling_median(ref, mag) <= 1e-5, shape


LO, HI = 2.0 ** -100, 2.0 ** 100


def _inside(*tensors):
    for t in tensors:
        if t is not None:
            a = t.double().abs()
            a = a[a != 0]  # a ReLU's zeros are exact at every scale
            assert a.numel() and a.min() >= LO and a.max() <= HI


SCALINGS = [(p, 0) for p in V.BITWISE_SCALES] + [(0, -40), (0, 0)]


@pytest.mark.parametrize("route,shape,admitted", FWD, ids=FWD_IDS)
def test_scaled_operands_stay_inside_the_exponent_range(route, shape, admitted):
    """No operand, product or reference leaves [2^-100, 2^100] at any scaling the GPU tests assert bit for bit."""
    ep = admitted[-1]  # the epilogue with the most operands
    for px, pw in SCALINGS:
        x, w, b, R1, R2 = V.fwd_scaled(shape, ep, px, pw)
        _inside(x, w, R1, R2, V.fwd_apply(x, w, b, R1, R2, ep, shape[5], torch.float64))
        xa, wa = x.abs().double(), w.abs().double()
        assert xa.min() * wa.min() >= LO and xa.max() * wa.max() * 9 * shape[3] <= HI
    if shape in V.DOT_SHAPES:
        for px, pw in SCALINGS:
            ops = V.dot_operands("scaled", shape, "post")
            x, w = ops[0] * 2.0 ** px, ops[1] * 2.0 ** pw
            z = V.dot_apply((x, w) + ops[2:], "post", "none", torch.float64)
            _inside(z, ops[5])
            assert (ops[5].abs().min() * x.abs().min() * w.abs().min()).item() >= LO


def test_scaled_wgrad_operands_stay_inside_the_exponent_range():
    for shape in V.WGRAD_SHAPES:
        for px, pdy in SCALINGS:
            x, dy, base = V.wgrad_scaled(shape, px, pdy)
            g = V._wgrad(x, dy, torch.float64)
            _inside(x, dy, base, g, g if base is None else g + base.double())
            assert x.abs().min().double() * dy.abs().min().double() >= LO


# ---- 2. the reference alone is inside the gates ------------------------------------------------------------------------------------------
def gates(err, terms):
    """Bound (a) and gate (b) of tests/test_conv_edges_gpu.py for an error (rms, max) against torch's own `err`."""
    bad = V.gate_failures(*err, err, floor=V.FLOOR)
    if not err[1] <= (terms + 4) * U:
        bad.append(f"max {err[1] / U:.2f}u > ({terms} + 4) u")
    return bad


@pytest.mark.parametrize("cls", V.ACCURACY_CLASSES)
@pytest.mark.parametrize("index", range(len(FWD)), ids=FWD_IDS)
def test_torch_fp32_forward_passes_the_gates(index, cls):
    route, shape, admitted = FWD[index]
    ep = V.cycled_epilogue(index, cls, admitted)
    ref, mag, err = V.fwd_reference(cls, shape, ep)
    print(f"\n[{cls} {route} {shape} {ep}] torch fp32 on the CPU: {in_u(err)}; K u = {9 * shape[3]}u")
    assert not gates(err, 9 * shape[3])


@pytest.mark.parametrize("cls", V.ACCURACY_CLASSES)
def test_torch_fp32_passes_the_gates_on_the_other_routes(cls):
    for shape in V.DOT_SHAPES:
        for i, ep in enumerate(V.DOT_EPILOGUES):
            act2 = tuple(V.DOT_ACT2)[i]
            err = V.dot_reference(cls, shape, ep, act2)[2]
            print(f"\n[{cls} dot {shape} {ep} {act2}] torch fp32 on the CPU: {in_u(err)}")
            assert not gates(err, V.dot_terms(shape) - 4)
    for shape in V.BWD_DATA_SHAPES:
        err = V.bwd_data_class(cls, shape)[4]
        print(f"\n[{cls} bwd_data {shape}] torch fp32 on the CPU: {in_u(err)}")
        assert not gates(err, 9 * shape[4])
    for shape in V.WGRAD_SHAPES:
        if V.wgrad_has_class(cls, shape):
            err = V.wgrad_class(cls, shape)[5]
            print(f"\n[{cls} wgrad {shape}] torch fp32 on the CPU: {in_u(err)}")
            assert not gates(err, V.wgrad_terms(shape))


# ---- 3. the inputs discriminate ----------------------------------------------------------------------------------------------------------
def touches_padding(shape):
    """[OH, OW] bool: the window of this output pixel reaches into the zero padding."""
    Fr, H, W, Cin, Cout, stride = shape
    live = F.conv2d(torch.ones(1, 1, H, W), torch.ones(1, 1, 3, 3), stride=stride, padding=1)[0, 0]
    return live < 9


@pytest.mark.parametrize("route,shape,admitted", FWD, ids=FWD_IDS)
def test_integer_operands_show_the_classical_mistakes(route, shape, admitted):
    """Deliberately wrong references, computed by torch on the exact_int operands, differ from the right answer wherever the mistake acts and
    nowhere else: none of them can hide behind these inputs.  `most`: two different sums of hundreds of integer products coincide at a few
    elements in a thousand, never at a tenth of them."""
    Fr, H, W, Cin, Cout, stride = shape
    x, w, b, _, _ = (t.double() if t is not None else None for t in V.fwd_operands("exact_int", shape, "bias"))
    right = V.fwd_reference("exact_int", shape, "bias")[0]
    differs = lambda wrong: V.nhwc(wrong) != right
    most = lambda d: d.double().mean().item() >= 0.9
    # 1. ky / kx swapped in the weight
    assert most(differs(F.conv2d(x, w.transpose(2, 3), b, stride=stride, padding=1)))
    # 2. replicate padding instead of zero padding: border outputs only, and every one of them
    d = differs(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, b, stride=stride))
    border = touches_padding(shape)
    assert not d[:, ~border].any() and d[:, border].any(-1).all() and most(d[:, border])
    # 3. window origin off by one for stride 2 (rows / columns 2 o .. 2 o + 2 instead of 2 o - 1 .. 2 o + 1)
    if stride == 2:
        OH, OW = V.out_hw(H, W, 2)
        assert most(differs(F.conv2d(F.pad(x, (0, 2, 0, 2)), w, b, stride=2)[:, :, :OH, :OW]))
    # 4. the last 32 input channels dropped
    if Cin > 32:
        assert most(differs(F.conv2d(x[:, :Cin - 32], w[:, :Cin - 32], b, stride=stride, padding=1)))
    # 5. pre_relu applied after the convolution instead of before
    xr, wr, br, R1, R2 = (t.double() for t in V.fwd_operands("exact_int", shape, "rcu"))
    wrong = F.relu(F.conv2d(xr, wr, br, stride=stride, padding=1)) + R1 + R2
    assert most(V.nhwc(wrong) != V.fwd_reference("exact_int", shape, "rcu")[0])


# ---- 4. the dispatch is restated, not assumed --------------------------------------------------------------------------------------------
TABLE = {  # route -> (tiles, k-tiles) per shape, as the routes' table states them
    "dma64": [(4, 18)], "dma64_s2": [(4, 27)], "dma64_split": [(17, 18), (17, 54)], "dma128": [(3, 9), (2, 18)], "dma128_split": [(17, 18)],
}


def test_shapes_reach_the_kernels_their_routes_name(lib):
    for route, counts in TABLE.items():
        for shape, want in zip(V.FWD_ROUTES[route], counts):
            Fr, H, W, Cin, Cout, stride = shape
            assert V.takes_dma_loader(Cin) and (Cout <= 32) == route.startswith("dma128")
            assert not V.halo_in_automatic_mode(shape)  # automatic mode: fewer than 4096 patches stay with conv3_dma_kernel
            assert V.dma_tiles(shape) == want, (shape, V.dma_tiles(shape))
            p = plan(lib, *want)
            assert p["split"] == int(route.endswith("_split")), (shape, p)
            if p["split"]:
                assert p["units"] == want[0] * want[1] and p["nsplit"] > want[0]  # more runs than tiles: tiles are cut along k
    assert V.out_hw(13, 10, 2) == (7, 5)
    for shape in V.FWD_ROUTES["halo"]:
        assert V.halo_supported(shape) and V.takes_dma_loader(shape[3]) and V.halo_patches(shape) < V.HALO_PAYS_TILES
    # one pixel past an 8 x 16 patch in both directions
    assert [(s[1] % V.HALO_TH, s[2] % V.HALO_TW) for s in V.FWD_ROUTES["halo"]] == [(1, 1), (0, 1)] and V.FWD_ROUTES["halo"][1][1] == 5 * V.HALO_TH
    for shape in V.FWD_ROUTES["reg"]:
        assert not V.takes_dma_loader(shape[3]) and shape[3] % 4 == 0
    assert [V.takes_dma_loader(s[4]) for s in V.BWD_DATA_SHAPES] == [True, False]  # the input gradient contracts over Cout
    assert all(s in V.FWD_ROUTES["halo"] for s in V.DOT_SHAPES)


def test_mismatch_report_names_the_place():
    """The report the GPU tests print on an exact_int failure, on a reference with two corrupted elements."""
    ref = V.fwd_reference("exact_int", V.FWD_ROUTES["dma64"][0], "bias")[0]  # [2, 9, 11, 48]
    assert V.describe_mismatch(ref.float(), ref, 64) == "no mismatch"
    y = ref.float().clone()
    y[0, 5, 9, 40] += 1   # pixel 64 of frame 0: the first row of the second 64-row tile
    y[1, 8, 3, 33] += 1   # the bottom border of frame 1
    msg = V.describe_mismatch(y, ref, 64)
    assert "2 of 9504 differ" in msg and "first at (frame, y, x, channel) = (0, 5, 9, 40)" in msg, msg
    assert "all on the image border: False" in msg and "32-channel blocks hit: [1]" in msg and "row tiles hit: [1, 2]" in msg, msg
    assert "all on the image border: True" in V.describe_mismatch(y[1:], ref[1:], 64)


def test_outlier_indices_are_inside_range():
    assert V.outlier_indices(64) == [5, 35, 60] and V.outlier_indices(192) == [5, 99, 188]
    for Cc in (4, 8, 16, 20, 32, 48, 96):
        idx = V.outlier_indices(Cc)
        assert 2 <= len(idx) <= 3 and all(0 <= i < Cc for i in idx)


def test_wgrad_pieces_match_the_workspace(lib):
    """wgrad_pieces restates wgrad_plan: the workspace the library asks for is pieces x column groups x Cout blocks x 3 x 1024 floats."""
    for Fr, H, W, Cin, Cout, acc in V.WGRAD_SHAPES:
        n_cg, n_cb = -(-(-(-9 * Cin // 32)) // 3), -(-Cout // 32)
        assert lib.edv_conv3x3_wgrad_workspace(Fr, H, W, Cin, Cout) == V.wgrad_pieces(Fr, H, Cin, Cout) * n_cg * n_cb * 3 * 1024 * 4
