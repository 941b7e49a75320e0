"""The convolution kernels on the operands of tests/conv_inputs.py: integer operands whose answer is exactly known (any summation order gives the
int64 result, so a wrong tap, a padding lane that reads memory or a swapped index in a pack kernel cannot hide inside a tolerance), operands
scaled by 2^+-40 bit for bit, and outlier, heavy-tailed, cancelling and offset operands against fp64 with a per-element yardstick and two gates:
(a) the theorem (K + 4) u sum |x w| for K fp32 products summed in any order plus four epilogue roundings, (b) 4 x torch's own fp32 error.
Every route of the table in tests/conv_inputs.py is run; tests/test_conv_inputs_cpu.py shows that the shapes reach the kernels named there."""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import time

import pytest
import torch

from endodav_amd import _lib
from tests import conv_inputs as V

pytestmark = pytest.mark.gpu

U = V.U
COUNTER_FLOATS = 4096  # SPLIT_MAX_COUNTERS: the arrival counters at the head of the stream-K workspace
CHILD = "EDV_TEST_CONV_FLAT_CHILD"  # set in the child process of the flat-address test
NAN = float("nan")


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sid(shape):
    return "x".join(str(int(v)) for v in shape)


@contextlib.contextmanager
def conv_impl(lib, mode):
    _lib.check(lib.edv_set_conv_impl(mode), "edv_set_conv_impl")
    try:
        yield
    finally:
        _lib.check(lib.edv_set_conv_impl(0), "edv_set_conv_impl")


@contextlib.contextmanager
def env(name, value):
    """EDV_CONV_HALO is read at every call (conv_halo.hip), so a test can switch it."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


_WS = {}


def workspace(lib, cuda):
    """The stream-K workspace, its piece slots poisoned: a piece nobody wrote shows as NaN.  Only the arrival counters are zeroed, once."""
    if "ws" not in _WS:
        nbytes = lib.edv_gemm_workspace()
        w = torch.full((nbytes // 4,), NAN, device=cuda)
        w[:COUNTER_FLOATS] = 0
        _WS["ws"] = (w, nbytes)
    return _WS["ws"]


def counters_are_zero(ws):
    return int(ws[:COUNTER_FLOATS].view(torch.int32).abs().sum()) == 0


def pack(lib, cuda, w, bwd=False):
    Cout, Cin = w.shape[:2]
    wd, wp = w.to(cuda), torch.empty(w.numel(), device=cuda)
    _lib.check((lib.edv_pack_conv3x3_bwd if bwd else lib.edv_pack_conv3x3)(wd.data_ptr(), wp.data_ptr(), Cout, Cin, st()), "pack")
    torch.cuda.synchronize()
    return wp


def conv(lib, cuda, route, shape, ops, ep, launches=1):
    """The forward convolution of `route` on CPU operands (x, w, b, R1, R2) in torch layout -> list of outputs [F, OH, OW, Cout], one per launch."""
    Fr, H, W, Cin, Cout, stride = shape
    pre, post, _ = V.EPILOGUES[ep]
    x, w, b, R1, R2 = ops
    d = lambda t: None if t is None else t.to(cuda)
    xd, bd, r1, r2, wp = d(V.nhwc(x)), d(b), d(V.nhwc(R1)), d(V.nhwc(R2)), pack(lib, cuda, w)
    OH, OW = V.out_hw(H, W, stride)
    outs = []
    with conv_impl(lib, 2 if route == "halo" else 0):
        for _ in range(launches):
            y = torch.full((Fr, OH, OW, Cout), NAN, device=cuda)
            if route.endswith("_split"):
                ws, nbytes = workspace(lib, cuda)
                _lib.check(lib.edv_conv3x3_ws(xd.data_ptr(), wp.data_ptr(), _lib.ptr(bd), y.data_ptr(), Fr, H, W, Cin, Cout, stride, pre, post, _lib.ptr(r1),
                                              _lib.ptr(r2), ws.data_ptr(), nbytes, st()), "edv_conv3x3_ws")
                torch.cuda.synchronize()
                assert counters_are_zero(ws), "a launch left an arrival counter set"
            else:
                _lib.check(lib.edv_conv3x3(xd.data_ptr(), wp.data_ptr(), _lib.ptr(bd), y.data_ptr(), Fr, H, W, Cin, Cout, stride, pre, post, _lib.ptr(r1),
                                           _lib.ptr(r2), st()), "edv_conv3x3")
                torch.cuda.synchronize()
            outs.append(y)
    return outs


def conv_dot(lib, cuda, kernel, shape, ops, ep, act2):
    """edv_conv3x3_dot on the halo kernel or, with EDV_CONV_HALO=0, on conv3_dma_kernel<4, 8 + act> -> [F, H, W]."""
    Fr, H, W, Cin, Cout, stride = shape
    pre, post, _ = V.EPILOGUES[ep]
    x, w, b, _, _, w2, b2 = ops
    d = lambda t: None if t is None else t.to(cuda)
    xd, bd, w2d, b2d, wp = d(V.nhwc(x)), d(b), d(w2), d(b2), pack(lib, cuda, w)
    y = torch.full((Fr, H, W), NAN, device=cuda)
    with env("EDV_CONV_HALO", "1" if kernel == "halo" else "0"), conv_impl(lib, 2):
        _lib.check(lib.edv_conv3x3_dot(xd.data_ptr(), wp.data_ptr(), _lib.ptr(bd), y.data_ptr(), Fr, H, W, Cin, Cout, 1, pre, post, w2d.data_ptr(), _lib.ptr(b2d),
                                       V.DOT_ACT2[act2], st()), "edv_conv3x3_dot")
        torch.cuda.synchronize()
    return y


def bwd_data(lib, cuda, shape, dy, w):
    """Stride-1 input gradient: edv_pack_conv3x3_bwd + edv_conv3x3 on dy -> [F, H, W, Cin]."""
    Fr, H, W, Cin, Cout = shape
    wp, gd = pack(lib, cuda, w, bwd=True), V.nhwc(dy).to(cuda)
    dx = torch.full((Fr, H, W, Cin), NAN, device=cuda)
    _lib.check(lib.edv_conv3x3(gd.data_ptr(), wp.data_ptr(), None, dx.data_ptr(), Fr, H, W, Cout, Cin, 1, 0, 0, None, None, st()), "edv_conv3x3")
    torch.cuda.synchronize()
    return dx


def wgrad(lib, cuda, shape, x, dy, base):
    Fr, H, W, Cin, Cout, acc = shape
    xd, gd = V.nhwc(x).to(cuda), V.nhwc(dy).to(cuda)
    nb = lib.edv_conv3x3_wgrad_workspace(Fr, H, W, Cin, Cout)
    ws = torch.full((nb // 4,), NAN, device=cuda)
    dw = base.to(cuda) if acc else torch.full((Cout, Cin, 3, 3), NAN, device=cuda)
    _lib.check(lib.edv_conv3x3_wgrad(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), Fr, H, W, Cin, Cout, ws.data_ptr(), nb, int(acc), st()), "edv_conv3x3_wgrad")
    torch.cuda.synchronize()
    return dw


def tile_rows(route, shape):
    return None if route == "halo" else V.dma_tile(shape[4])[0]  # the register-staged kernel has the same 64 x 64 / 128 x 32 tiles


def assert_exact(y, ref, what, rows=None):
    assert not bool(torch.isnan(y).any()), f"{what}: NaN in the output"
    assert torch.equal(y.long().cpu(), ref.long()), f"{what}: {V.describe_mismatch(y.cpu(), ref, rows)}"
    print(f"\n[exact_int {what}] all {ref.numel()} elements exact, largest |ref| {int(ref.abs().max())}")


def check_gates(y, ref, mag, torch_err, terms, what):
    """Bound (a): max <= (terms + 4) u, and gate (b): within 4 x torch fp32 (floor 4 u), both per element of sum |x w|."""
    rms, mx = V.elem_error(y, ref, mag)
    print(f"\n[{what}] {V.ratios(rms, mx, torch_err)} | max {mx / U:.2f}u of ({terms} + 4)u")
    bad = V.gate_failures(rms, mx, torch_err, floor=V.FLOOR)
    if not mx <= (terms + 4) * U:
        bad.append(f"max {mx / U:.2f}u > ({terms} + 4) u")
    assert not bad, f"{what}: {bad}"


FWD = V.fwd_cases()
FWD_EXACT = [pytest.param(route, shape, ep, id=f"{route}-{sid(shape)}-{ep}") for route, shape, admitted in FWD for ep in admitted]
FWD_INDEX = [pytest.param(i, id=f"{FWD[i][0]}-{sid(FWD[i][1])}") for i in range(len(FWD))]
DOT = [pytest.param(kernel, shape, id=f"dot_{kernel}-{sid(shape)}") for kernel in V.DOT_KERNELS for shape in V.DOT_SHAPES]


# ---- exact integers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,shape,ep", FWD_EXACT)
def test_exact_int_forward(lib, cuda, route, shape, ep):
    """Every partial sum in any order is an integer below 2^24: the kernel must give the int64 answer exactly.  On the split routes a second launch
    repeats the first bit for bit and both leave the arrival counters at zero."""
    split = route.endswith("_split")
    outs = conv(lib, cuda, route, shape, V.fwd_operands("exact_int", shape, ep), ep, launches=2 if split else 1)
    ref = V.fwd_reference("exact_int", shape, ep)[0]
    assert_exact(outs[0], ref, f"{route} {shape} {ep}", tile_rows(route, shape))
    if split:
        assert torch.equal(V.bits(outs[1]), V.bits(outs[0])), "the second stream-K launch differs from the first"


@pytest.mark.parametrize("kernel,shape", DOT)
def test_exact_int_dot(lib, cuda, kernel, shape):
    for ep in V.DOT_EPILOGUES:
        for act2 in V.DOT_ACT2:
            y = conv_dot(lib, cuda, kernel, shape, V.dot_operands("exact_int", shape, ep), ep, act2)
            ref = V.dot_reference("exact_int", shape, ep, act2)[0]
            assert_exact(y[..., None], ref[..., None], f"dot ({kernel}) {shape} {ep} act2 = {act2}", 128 if kernel == "dma" else None)


@pytest.mark.parametrize("shape", V.BWD_DATA_SHAPES, ids=lambda s: "bwd_data-" + sid(s))
def test_exact_int_bwd_data(lib, cuda, shape):
    dy, w, ref, _, _ = V.bwd_data_class("exact_int", shape)
    assert_exact(bwd_data(lib, cuda, shape, dy, w), ref, f"bwd_data {shape}", V.dma_tile(shape[3])[0])


@pytest.mark.parametrize("shape", V.S2_BWD_SHAPES, ids=lambda s: "s2_bwd-" + sid(s))
def test_exact_int_s2_bwd(lib, cuda, shape):
    """edv_conv3x3_s2_bwd on the forward's packed weight, and the engine's route: edv_dilate2 + the stride-1 input-gradient convolution."""
    Fr, H, W, Cc = shape
    dy, w, ref, _, _ = V.s2_bwd_class(shape)
    gd = V.nhwc(dy).to(cuda)
    dx = torch.full((Fr, H, W, Cc), NAN, device=cuda)
    wp = pack(lib, cuda, w)
    _lib.check(lib.edv_conv3x3_s2_bwd(gd.data_ptr(), wp.data_ptr(), dx.data_ptr(), Fr, H, W, Cc, Cc, st()), "edv_conv3x3_s2_bwd")
    torch.cuda.synchronize()
    assert_exact(dx, ref, f"s2_bwd {shape}")
    z = torch.full((Fr, H, W, Cc), NAN, device=cuda)
    _lib.check(lib.edv_dilate2(gd.data_ptr(), z.data_ptr(), Fr, H, W, Cc, st()), "edv_dilate2")
    torch.cuda.synchronize()
    OH, OW = V.out_hw(H, W, 2)
    want = torch.zeros(Fr, H, W, Cc)
    want[:, ::2, ::2] = V.nhwc(dy)[:, :OH, :OW]
    assert_exact(z, want, f"dilate2 {shape}")
    wb = pack(lib, cuda, w, bwd=True)
    dx2 = torch.full((Fr, H, W, Cc), NAN, device=cuda)
    _lib.check(lib.edv_conv3x3(z.data_ptr(), wb.data_ptr(), None, dx2.data_ptr(), Fr, H, W, Cc, Cc, 1, 0, 0, None, None, st()), "edv_conv3x3")
    torch.cuda.synchronize()
    assert_exact(dx2, ref, f"s2_bwd via dilation {shape}", V.dma_tile(Cc)[0])


@pytest.mark.parametrize("shape", V.WGRAD_SHAPES, ids=lambda s: "wgrad-" + sid(s))
def test_exact_int_wgrad(lib, cuda, shape):
    x, dy, base, ref, _, _ = V.wgrad_class("exact_int", shape)
    dw = wgrad(lib, cuda, shape, x, dy, base)
    # [Cout, Cin, 3, 3] read as [frame = Cout, y = Cin, x = ky, channel = kx] by the mismatch report
    assert_exact(dw, ref, f"wgrad {shape} (report: frame = Cout index, y = Cin index, x = ky, channel = kx)")


@pytest.mark.parametrize("shape", V.CONVT_SHAPES, ids=lambda s: "convT-" + sid(s))
def test_exact_int_conv_transpose(lib, cuda, shape):
    """edv_conv_transpose, and its input gradient through edv_pixel_unshuffle + edv_transpose_scale + edv_gemm."""
    Fr, h, w_, Cc, s = shape
    x, wt, b, dy, yref, dxref = V.convT_class(shape)
    xd, wd, bd = V.nhwc(x).to(cuda), wt.to(cuda), b.to(cuda)
    wp, bp = torch.full((s * s * Cc * Cc,), NAN, device=cuda), torch.full((s * s * Cc,), NAN, device=cuda)
    y = torch.full((Fr, h * s, w_ * s, Cc), NAN, device=cuda)
    _lib.check(lib.edv_conv_transpose(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), wp.data_ptr(), bp.data_ptr(), y.data_ptr(), Fr, h, w_, Cc, s, st()), "edv_conv_transpose")
    torch.cuda.synchronize()
    assert_exact(y, yref, f"convT {shape}")
    gd = V.nhwc(dy).to(cuda)
    A = torch.full((Fr * h * w_, s * s * Cc), NAN, device=cuda)
    _lib.check(lib.edv_pixel_unshuffle(gd.data_ptr(), A.data_ptr(), Fr, h, w_, Cc, s, st()), "edv_pixel_unshuffle")
    wpt = torch.full((Cc, s * s * Cc), NAN, device=cuda)  # packed weight [s*s*C, C] -> [C, s*s*C]
    _lib.check(lib.edv_transpose_scale(wp.data_ptr(), None, wpt.data_ptr(), s * s * Cc, Cc, st()), "edv_transpose_scale")
    dx = torch.full((Fr * h * w_, Cc), NAN, device=cuda)
    _lib.check(lib.edv_gemm(A.data_ptr(), wpt.data_ptr(), dx.data_ptr(), Fr * h * w_, Cc, s * s * Cc, None, 0, None, None, None, 0, st()), "edv_gemm")
    torch.cuda.synchronize()
    assert_exact(dx.view(Fr, h, w_, Cc), dxref, f"convT input gradient {shape}")


# ---- scaling by a power of two, bit for bit ----------------------------------------------------------------------------------------------
def assert_scales(y, y0, p, what):
    assert not bool(torch.isnan(y0).any()) and bool((y0 != 0).any()), f"{what}: NaN or an all-zero output"
    assert torch.equal(V.bits(y), V.bits(y0 * 2.0 ** p)), f"{what}: not the unscaled result x 2^{p} bit for bit"


@pytest.mark.parametrize("index", FWD_INDEX)
def test_scaled_forward(lib, cuda, index):
    """y(2^p x) == 2^p y(x) for p = +-40, and y(x, 2^-40 w) == 2^-40 y(x, w), residuals scaled alike: no term of the sum may see the exponent."""
    route, shape, admitted = FWD[index]
    ep = V.cycled_epilogue(index, "scaled", admitted)
    run = lambda px, pw: conv(lib, cuda, route, shape, V.fwd_scaled(shape, ep, px, pw), ep)[0]
    y0 = run(0, 0)
    for p in V.BITWISE_SCALES:
        assert_scales(run(p, 0), y0, p, f"{route} {shape} {ep} x 2^{p}")
    assert_scales(run(0, -40), y0, -40, f"{route} {shape} {ep} w 2^-40")


@pytest.mark.parametrize("kernel,shape", DOT)
def test_scaled_dot(lib, cuda, kernel, shape):
    ep, act2 = "post", "relu"
    ops = V.dot_operands("scaled", shape, ep)
    run = lambda px, pw: conv_dot(lib, cuda, kernel, shape, (ops[0] * 2.0 ** px, ops[1] * 2.0 ** pw) + ops[2:], ep, act2)
    y0 = run(0, 0)
    for p in V.BITWISE_SCALES:
        assert_scales(run(p, 0), y0, p, f"dot ({kernel}) {shape} x 2^{p}")
    assert_scales(run(0, -40), y0, -40, f"dot ({kernel}) {shape} w 2^-40")


@pytest.mark.parametrize("shape", V.WGRAD_SHAPES, ids=lambda s: "wgrad-" + sid(s))
def test_scaled_wgrad(lib, cuda, shape):
    run = lambda px, pdy: wgrad(lib, cuda, shape, *V.wgrad_scaled(shape, px, pdy))
    d0 = run(0, 0)
    for p in V.BITWISE_SCALES:
        assert_scales(run(p, 0), d0, p, f"wgrad {shape} x 2^{p}")
    assert_scales(run(0, -40), d0, -40, f"wgrad {shape} dy 2^-40")


# ---- accuracy classes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", FWD_INDEX)
@pytest.mark.parametrize("cls", V.ACCURACY_CLASSES)
def test_accuracy_forward(lib, cuda, cls, index):
    route, shape, admitted = FWD[index]
    ep = V.cycled_epilogue(index, cls, admitted)
    y = conv(lib, cuda, route, shape, V.fwd_operands(cls, shape, ep), ep)[0]
    check_gates(y, *V.fwd_reference(cls, shape, ep), 9 * shape[3], f"{cls} {route} {shape} {ep}")


@pytest.mark.parametrize("kernel,shape", DOT)
@pytest.mark.parametrize("cls", V.ACCURACY_CLASSES)
def test_accuracy_dot(lib, cuda, cls, kernel, shape):
    """The bound of test_conv_halo_gpu.dot_bound -- 33 u for the 32-term sum plus b2 -- on top of the convolution's own (9 Cin + 4) u, because the
    reference here is the fp64 convolution and not the other kernel's fp32 output; per pixel of sum_c |w2| (sum |x w| + |bias|) + |b2|."""
    for ep, act2 in zip(V.DOT_EPILOGUES, V.DOT_ACT2):
        y = conv_dot(lib, cuda, kernel, shape, V.dot_operands(cls, shape, ep), ep, act2)
        check_gates(y, *V.dot_reference(cls, shape, ep, act2), V.dot_terms(shape) - 4, f"{cls} dot ({kernel}) {shape} {ep} act2 = {act2}")


@pytest.mark.parametrize("shape", V.BWD_DATA_SHAPES, ids=lambda s: "bwd_data-" + sid(s))
@pytest.mark.parametrize("cls", V.ACCURACY_CLASSES)
def test_accuracy_bwd_data(lib, cuda, cls, shape):
    dy, w, ref, mag, terr = V.bwd_data_class(cls, shape)
    check_gates(bwd_data(lib, cuda, shape, dy, w), ref, mag, terr, 9 * shape[4], f"{cls} bwd_data {shape}")


WGRAD = [pytest.param(cls, shape, id=f"{cls}-wgrad-{sid(shape)}") for cls in V.WGRAD_CLASSES for shape in V.WGRAD_SHAPES if V.wgrad_has_class(cls, shape)]


@pytest.mark.parametrize("cls,shape", WGRAD)
def test_accuracy_wgrad(lib, cuda, cls, shape):
    x, dy, base, ref, mag, terr = V.wgrad_class(cls, shape)
    check_gates(wgrad(lib, cuda, shape, x, dy, base), ref, mag, terr, V.wgrad_terms(shape), f"{cls} wgrad {shape}")


# ---- the flat-address route of conv3_dma_kernel ------------------------------------------------------------------------------------------
FLAT_CASES = "(exact_int_forward or (accuracy_forward and outlier_ch)) and (dma64 or dma128)"
FLAT_TIMEOUT = 120  # seconds.  Measured on the MI355X: the 35 cases take 0.4 s in this process and the child 4 s in all, nearly all of it start-up
#                     (torch, the HIP runtime, the library); 30 x that for a loaded machine.  The test does not wait: it ends when the child does.


def test_flat_address_route_in_a_fresh_process(lib, cuda):
    """BUF = false of conv3_dma_kernel (64-bit DMA sources, the zero page for padding taps) is the automatic route once an input reaches 2 GB; at
    test sizes only EDV_CONV_BUF=0 reaches it, and that flag is read once per process.  One fresh child runs the exact_int and outlier_ch cases of
    the dma routes under it while this process keeps the GPU idle."""
    if os.environ.get(CHILD):
        pytest.skip("this is the child process")
    torch.cuda.synchronize()
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", FLAT_CASES],
                       env={**os.environ, "EDV_CONV_BUF": "0", CHILD: "1"}, timeout=FLAT_TIMEOUT, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
    print(f"\n[flat addresses] child exit {r.returncode} after {time.time() - t0:.1f} s: {tail.splitlines()[-1] if tail else ''}")
    assert r.returncode == 0, f"the child failed under EDV_CONV_BUF=0:\n{tail}"
