"""The halo-tiled 3x3 convolution (csrc/conv_halo.hip), the 1x1-to-one-channel epilogue fused into both convolution kernels (edv_conv3x3_dot,
gemm_common.hpp) and the process-wide switch edv_set_conv_impl.  Reference everywhere: the existing edv_conv3x3 without a workspace under
edv_set_conv_impl(1); candidate: mode 2 (halo kernel and fused epilogue wherever supported; other shapes fall through to conv3_dma_kernel)."""
import contextlib
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

from endodav_amd import _lib
from tests import helpers as H

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
RAGGED = [(3, 9, 17), (2, 23, 37), (1, 40, 33)]  # one pixel past a 8x16 / 128-row tile in both directions, ragged sizes
ACT2 = {"none": 0, "relu": 2, "sigmoid": 3, "sigmoid_neg": 4}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def conv_impl(lib, mode):
    _lib.check(lib.edv_set_conv_impl(mode), "edv_set_conv_impl")
    try:
        yield
    finally:
        _lib.check(lib.edv_set_conv_impl(0), "edv_set_conv_impl")


@contextlib.contextmanager
def env(name, value):
    """EDV_CONV_HALO / EDV_CONV_DOT are read at every call (conv_halo.hip, conv_dma.hip), so a test can switch them."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def problem(cuda, Fr, Hh, Ww, Cin, Cout):
    """Operands on the device: x [F,H,W,Cin], packed weight, bias, w2 [Cout], b2 [1]."""
    x = rnd(Fr, Hh, Ww, Cin, seed=1).to(cuda)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=1 / math.sqrt(9 * Cin)).to(cuda)
    b = rnd(Cout, seed=3, scale=0.1).to(cuda)
    w2 = rnd(Cout, seed=6, scale=1.5).to(cuda)
    b2 = rnd(1, seed=7, scale=0.3).to(cuda)
    wp = torch.empty(Cout * 9 * Cin, device=cuda)
    lib = _lib.load()
    _lib.check(lib.edv_pack_conv3x3(w.data_ptr(), wp.data_ptr(), Cout, Cin, st()))
    return x, w, wp, b, w2, b2


def reference_conv(lib, cuda, x, wp, b, Cout, post):
    """The parent's path: edv_conv3x3 without a workspace, mode 1."""
    Fr, Hh, Ww, Cin = x.shape
    o = torch.full((Fr, Hh, Ww, Cout), float("nan"), device=cuda)
    with conv_impl(lib, 1):
        _lib.check(lib.edv_conv3x3(x.data_ptr(), wp.data_ptr(), b.data_ptr(), o.data_ptr(), Fr, Hh, Ww, Cin, Cout, 1, 0, int(post), None, None, st()), "edv_conv3x3")
    torch.cuda.synchronize()
    return o


def fused(lib, x, wp, b, Cout, post, w2, b2, act2, y):
    Fr, Hh, Ww, Cin = x.shape
    with conv_impl(lib, 2):
        _lib.check(lib.edv_conv3x3_dot(x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), Fr, Hh, Ww, Cin, Cout, 1, 0, int(post), w2.data_ptr(),
                                       _lib.ptr(b2), act2, st()), "edv_conv3x3_dot")
    torch.cuda.synchronize()


def act2_ref(z, name):
    if name == "relu":
        return z.clamp_min(0)
    if name == "sigmoid":
        return torch.sigmoid(z)
    if name == "sigmoid_neg":
        return torch.sigmoid(-z)
    return z


def dot_bound(o, w2, b2, name):
    """The issue's bound: 33 * 2^-24 * (sum |w2 o| + |b2|) for a 32-term sum plus bias in any order; the sigmoids (slope <= 1/4, outputs in [0, 1])
    a quarter of it plus 4 * 2^-24."""
    mag = (o.double().abs() * w2.double().abs()).sum(-1) + b2.double().abs()
    bound = 33 * EPS * mag
    return bound / 4 + 4 * EPS if name.startswith("sigmoid") else bound


@pytest.mark.parametrize("act2", list(ACT2))
@pytest.mark.parametrize("post", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("Cin,Cout", [(32, 32), (64, 32), (32, 8)])
@pytest.mark.parametrize("Fr,Hh,Ww", RAGGED)
@pytest.mark.parametrize("kernel", ["halo", "dma"])
def test_fused_epilogue_within_the_rounding_of_a_32_term_sum(lib, cuda, kernel, Fr, Hh, Ww, Cin, Cout, post, act2):
    """y = act2(sum_c w2[c] act(conv + bias)[c] + b2) against the float64 sum over the reference path's fp32 convolution output, every element; and
    edv_dot_channels on the same tensor at the same bound.  (Cout = 8: 24 of a wave's 32 column lanes must add nothing.)  Both kernels that carry
    the epilogue: conv3_halo_kernel (mode 2) and conv3_dma_kernel (mode 2 with EDV_CONV_HALO=0)."""
    x, w, wp, b, w2, b2 = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    o = reference_conv(lib, cuda, x, wp, b, Cout, post)
    ref = act2_ref((o.double() * w2.double()).sum(-1) + b2.double(), act2)
    bound = dot_bound(o, w2, b2, act2)
    y = torch.full((Fr, Hh, Ww), float("nan"), device=cuda)
    with env("EDV_CONV_HALO", "1" if kernel == "halo" else "0"):
        fused(lib, x, wp, b, Cout, post, w2, b2, ACT2[act2], y)
    ratio = ((y.double() - ref).abs() / bound).max().item()
    print(f"fused 1x1 ({kernel}) {Fr}x{Hh}x{Ww} {Cin}->{Cout} post={post} {act2}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"fused epilogue: worst error / bound {ratio:.3f}"
    yd = torch.full((Fr, Hh, Ww), float("nan"), device=cuda)
    _lib.check(lib.edv_dot_channels(o.data_ptr(), w2.data_ptr(), b2.data_ptr(), yd.data_ptr(), Fr * Hh * Ww, Cout, ACT2[act2], st()), "edv_dot_channels")
    torch.cuda.synchronize()
    r2 = ((y.double() - yd.double()).abs() / bound).max().item()
    assert r2 <= 1.0, f"fused epilogue vs edv_dot_channels: worst difference / bound {r2:.3f}"


def test_fused_epilogue_without_b2_and_against_fp64_conv(lib, cuda):
    """b2 = NULL adds nothing; the whole chain against float64 conv2d at the 3e-6 scale-relative gate of test_kernels_gpu.py."""
    Fr, Hh, Ww, Cin, Cout = 2, 23, 37, 64, 32
    x, w, wp, b, w2, b2 = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    y = torch.full((Fr, Hh, Ww), float("nan"), device=cuda)
    fused(lib, x, wp, b, Cout, 1, w2, None, 0, y)
    ref = F.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1))
    ref = (ref * w2.double().view(1, -1, 1, 1)).sum(1)
    err = ((y.double() - ref).abs().max() / ref.abs().max()).item()
    assert err <= 3e-6, f"fused chain vs float64: scale-relative error {err:.3e}"


GUARD = 16 * 1024


def _guarded(t, cuda, fill):
    big = torch.full((t.numel() + 2 * GUARD,), fill, device=cuda)
    big[GUARD:GUARD + t.numel()] = t.reshape(-1).to(cuda)
    return big, big[GUARD:GUARD + t.numel()].view(t.shape)


@pytest.mark.parametrize("Fr,Hh,Ww,Cin,Cout", [(3, 9, 17, 32, 32), (1, 40, 33, 64, 8)])
@pytest.mark.parametrize("kernel", ["halo", "dma"])
def test_fused_output_stays_inside_guard_bands(lib, cuda, kernel, Fr, Hh, Ww, Cin, Cout):
    """x and the one-float-per-pixel output are slices of NaN / sentinel-filled allocations: rows past M of the last tile are dropped by the
    descriptor, a padding tap reads zeros and never the memory around x."""
    x, w, wp, b, w2, b2 = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    o = reference_conv(lib, cuda, x, wp, b, Cout, 1)
    bigx, xg = _guarded(x, cuda, float("nan"))
    SENT = -4321.0
    bigy, y = _guarded(torch.full((Fr, Hh, Ww), float("nan")), cuda, SENT)
    with env("EDV_CONV_HALO", "1" if kernel == "halo" else "0"):
        fused(lib, xg, wp, b, Cout, 1, w2, b2, 0, y)
    n = y.numel()
    assert bool((bigy[:GUARD] == SENT).all()) and bool((bigy[GUARD + n:] == SENT).all()), "a store escaped the output descriptor"
    assert bool(torch.isfinite(y).all())
    ref = (o.double() * w2.double()).sum(-1) + b2.double()
    assert bool(((y.double() - ref).abs() <= dot_bound(o, w2, b2, "none")).all())


def test_fused_epilogue_beside_another_stream(lib, cuda):
    """20 launches while a second stream runs edv_conv3x3 of another shape: every result identical to the quiet run, bit for bit."""
    Fr, Hh, Ww, Cin, Cout = 2, 23, 37, 32, 32
    x, w, wp, b, w2, b2 = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    quiet = torch.empty((Fr, Hh, Ww), device=cuda)
    fused(lib, x, wp, b, Cout, 1, w2, b2, 2, quiet)
    x2 = rnd(4, 40, 40, 64, seed=11).to(cuda)
    w2nd = rnd(64, 64, 3, 3, seed=12, scale=0.05).to(cuda)
    wp2 = torch.empty(64 * 9 * 64, device=cuda)
    _lib.check(lib.edv_pack_conv3x3(w2nd.data_ptr(), wp2.data_ptr(), 64, 64, st()))
    y2 = torch.empty((4, 40, 40, 64), device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = [torch.full((Fr, Hh, Ww), float("nan"), device=cuda) for _ in range(20)]
    _lib.check(lib.edv_set_conv_impl(2))
    try:
        for y in outs:
            for _ in range(3):
                _lib.check(lib.edv_conv3x3(x2.data_ptr(), wp2.data_ptr(), None, y2.data_ptr(), 4, 40, 40, 64, 64, 1, 1, 0, None, None, C.c_void_p(side.cuda_stream)))
            _lib.check(lib.edv_conv3x3_dot(x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), Fr, Hh, Ww, Cin, Cout, 1, 0, 1, w2.data_ptr(), b2.data_ptr(), 2, st()))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.edv_set_conv_impl(0))
    assert all(torch.equal(y, quiet) for y in outs)


def test_switch_and_unsupported_shapes_are_errors(lib, cuda):
    """Mode 1 switches the fused entry off; Cout > 32 and Cin % 32 != 0 have no fused kernel: an error, never another path."""
    x, w, wp, b, w2, b2 = problem(cuda, 1, 8, 16, 32, 32)
    y = torch.empty((1, 8, 16), device=cuda)
    args = lambda Cin, Cout: (x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 8, 16, Cin, Cout, 1, 0, 0, w2.data_ptr(), b2.data_ptr(), 0, st())
    with conv_impl(lib, 1):
        assert lib.edv_conv3x3_dot(*args(32, 32)) != 0
    assert lib.edv_set_conv_impl(3) != 0
    with conv_impl(lib, 2):
        assert lib.edv_conv3x3_dot(*args(32, 64)) != 0
        assert lib.edv_conv3x3_dot(*args(16, 32)) != 0
        assert lib.edv_conv3x3_dot(*args(32, 32)) == 0
    torch.cuda.synchronize()


# ---- the halo kernel against conv3_dma_kernel, bit for bit -----------------------------------------------------------------------------------------
SHAPES = [(1, 3, 5), (2, 8, 16), (3, 9, 17), (2, 23, 37), (1, 40, 33)]  # below a patch, exactly one, one pixel past it both ways, ragged
CHANNELS = [(32, 32), (64, 32), (64, 64), (96, 64), (32, 8)]            # (64, 64) and (96, 64) have no halo kernel: they must fall through unchanged
# (pre_relu, post_relu, residuals, bias): every value of every axis, with every shape and every channel pair
OPTIONS = [(0, 0, 0, True), (1, 1, 1, False), (0, 1, 2, True), (1, 0, 2, False), (1, 1, 0, True), (0, 0, 1, True)]


def conv(lib, cuda, mode, x, wp, b, Cout, pre, post, r1, r2, y=None, stream=None):
    Fr, Hh, Ww, Cin = x.shape
    if y is None:
        y = torch.full((Fr, Hh, Ww, Cout), float("nan"), device=cuda)
    with conv_impl(lib, mode):
        _lib.check(lib.edv_conv3x3(x.data_ptr(), wp.data_ptr(), _lib.ptr(b), y.data_ptr(), Fr, Hh, Ww, Cin, Cout, 1, int(pre), int(post), _lib.ptr(r1), _lib.ptr(r2),
                                   stream or st()), "edv_conv3x3")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("pre,post,res,use_bias", OPTIONS)
@pytest.mark.parametrize("Cin,Cout", CHANNELS)
@pytest.mark.parametrize("Fr,Hh,Ww", SHAPES)
def test_halo_kernel_is_bit_identical(lib, cuda, Fr, Hh, Ww, Cin, Cout, pre, post, res, use_bias):
    x, w, wp, b, _, _ = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    r1 = rnd(Fr, Hh, Ww, Cout, seed=4).to(cuda) if res >= 1 else None
    r2 = rnd(Fr, Hh, Ww, Cout, seed=5).to(cuda) if res >= 2 else None
    bias = b if use_bias else None
    ref = conv(lib, cuda, 1, x, wp, bias, Cout, pre, post, r1, r2)
    got = conv(lib, cuda, 2, x, wp, bias, Cout, pre, post, r1, r2)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(got, ref)


def test_halo_kernel_against_fp64(lib, cuda):
    """One case against float64 conv2d at the 3e-6 scale-relative gate of test_kernels_gpu.py."""
    Fr, Hh, Ww, Cin, Cout = 2, 23, 37, 64, 32
    x, w, wp, b, _, _ = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    got = conv(lib, cuda, 2, x, wp, b, Cout, 0, 1, None, None)
    ref = F.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    assert err <= 3e-6, f"halo conv vs float64: scale-relative error {err:.3e}"


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (64, 32)])
def test_halo_never_reads_a_neighbouring_frame(lib, cuda, Cin, Cout):
    """Frames 0 and 2 are NaN: the halo rows above row 0 and below row H - 1 of frame 1 are those frames' memory and must read as zeros."""
    Hh, Ww = 9, 17
    x, w, wp, b, _, _ = problem(cuda, 3, Hh, Ww, Cin, Cout)
    alone = conv(lib, cuda, 2, x[1:2].contiguous(), wp, b, Cout, 0, 0, None, None)
    x[0] = float("nan")
    x[2] = float("nan")
    got = conv(lib, cuda, 2, x, wp, b, Cout, 0, 0, None, None)
    assert bool(torch.isfinite(got[1]).all())
    assert torch.equal(got[1], alone[0])


@pytest.mark.parametrize("Fr,Hh,Ww,Cin,Cout", [(3, 9, 17, 32, 32), (1, 40, 33, 64, 8)])
def test_halo_stays_inside_guard_bands(lib, cuda, Fr, Hh, Ww, Cin, Cout):
    """x, y and R1 are slices of NaN / sentinel-filled allocations."""
    x, w, wp, b, _, _ = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    r1 = rnd(Fr, Hh, Ww, Cout, seed=4).to(cuda)
    ref = conv(lib, cuda, 1, x, wp, b, Cout, 0, 1, r1, None)
    SENT = -4321.0
    bigx, xg = _guarded(x, cuda, float("nan"))
    bigr, rg = _guarded(r1, cuda, float("nan"))
    bigy, y = _guarded(torch.full((Fr, Hh, Ww, Cout), float("nan")), cuda, SENT)
    conv(lib, cuda, 2, xg, wp, b, Cout, 0, 1, rg, None, y=y)
    n = y.numel()
    assert bool((bigy[:GUARD] == SENT).all()) and bool((bigy[GUARD + n:] == SENT).all()), "a store escaped the output descriptor"
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, ref)


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (64, 32)])
def test_halo_padding_is_written_not_assumed(lib, cuda, Cin, Cout):
    """Two launches back to back: the first leaves large values in every LDS byte the patch uses, the second must see zeros in its padding."""
    Fr, Hh, Ww = 3, 9, 17
    x, w, wp, b, _, _ = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    ref = conv(lib, cuda, 1, x, wp, b, Cout, 0, 0, None, None)
    big = torch.full_like(x, 3.0e18)
    y = torch.empty((Fr, Hh, Ww, Cout), device=cuda)
    with conv_impl(lib, 2):
        for src in (big, x):
            _lib.check(lib.edv_conv3x3(src.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), Fr, Hh, Ww, Cin, Cout, 1, 0, 0, None, None, st()))
        torch.cuda.synchronize()
    assert torch.equal(y, ref)


def test_halo_beside_another_stream(lib, cuda):
    """20 launches while a second stream runs edv_conv3x3 of another shape: every result identical to the quiet run (the project's barrier-race check)."""
    Fr, Hh, Ww, Cin, Cout = 2, 23, 37, 64, 32
    x, w, wp, b, _, _ = problem(cuda, Fr, Hh, Ww, Cin, Cout)
    quiet = conv(lib, cuda, 1, x, wp, b, Cout, 0, 1, None, None)
    x2 = rnd(4, 40, 40, 64, seed=11).to(cuda)
    wb = rnd(64, 64, 3, 3, seed=12, scale=0.05).to(cuda)
    wp2 = torch.empty(64 * 9 * 64, device=cuda)
    _lib.check(lib.edv_pack_conv3x3(wb.data_ptr(), wp2.data_ptr(), 64, 64, st()))
    y2 = torch.empty((4, 40, 40, 64), device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = [torch.full((Fr, Hh, Ww, Cout), float("nan"), device=cuda) for _ in range(20)]
    with conv_impl(lib, 2):
        for y in outs:
            for _ in range(3):
                _lib.check(lib.edv_conv3x3(x2.data_ptr(), wp2.data_ptr(), None, y2.data_ptr(), 4, 40, 40, 64, 64, 1, 1, 0, None, None, C.c_void_p(side.cuda_stream)))
            _lib.check(lib.edv_conv3x3(x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), Fr, Hh, Ww, Cin, Cout, 1, 0, 1, None, None, st()))
        torch.cuda.synchronize()
    assert all(torch.equal(y, quiet) for y in outs)


# ---- engine level ------------------------------------------------------------------------------------------------------------------------------
# The smallest golden configuration of test_forward_gpu.py whose head these kernels serve: the micro cases have features = 32, i.e. 16-channel head
# convolutions, which neither the halo kernel nor the fused epilogue covers (Cin % 32 == 0) -- under any mode they run the parent's path.
NAME = "vits_224x280_t2"


def _forward(lib, cuda, mode):
    model, kwargs, shape, kind, store = H.build_model(NAME)
    model = model.to(cuda)
    x = H.case_input(NAME).to(cuda)
    with conv_impl(lib, mode):
        with torch.no_grad():
            out = model(x)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}, model.launch_count(), model.device_bytes()


def test_engine_inference(lib, cuda):
    """Mode 2 without the fused epilogue: the halo kernel alone, four maps bit-identical to mode 1.  With it: the dot_channels launch and the
    32-channel buffer of the output head are gone and the maps stay inside the golden's gate."""
    from tests.test_forward_gpu import check_against_golden

    out1, n1, bytes1 = _forward(lib, cuda, 1)
    with env("EDV_CONV_DOT", "0"):
        out_h, n_h, _ = _forward(lib, cuda, 2)
    assert n_h == n1
    assert all(torch.equal(out_h[k], out1[k]) for k in out1)
    out2, n2, bytes2 = _forward(lib, cuda, 2)
    assert n2 == n1 - 1, (n1, n2)
    assert bytes2 < bytes1, (bytes1, bytes2)
    check_against_golden(NAME, out2, "strided", all_pixels=True)


def test_engine_training_keeps_two_steps(lib, cuda):
    """A training forward never fuses (the backward reads the 32-channel tensor): outputs and gradients under mode 2 are mode 1's, bit for bit."""
    import endodav_amd

    def grads(mode):
        model, kwargs, shape, kind, store = H.build_model(NAME)
        model = model.to(cuda)
        endodav_amd.mark_only_part_as_trainable(model, warm_up=True)
        model.train()
        x = H.case_input(NAME).to(cuda)
        params = [p for p in model.parameters() if p.requires_grad]
        with conv_impl(lib, mode):
            out = model(x)
            sum(o.mean() for o in out.values()).backward()
            torch.cuda.synchronize()
        return [o.detach().clone() for o in out.values()], [p.grad.clone() for p in params]

    o1, g1 = grads(1)
    o2, g2 = grads(2)
    assert len(g1) > 0
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
