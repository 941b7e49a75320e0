"""Per-kernel parity on MI355X: every C-ABI kernel entry point against the plain PyTorch fp32/fp64 op
the reference calls.  All calls go through ctypes -> libendodav_hip.so."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from endodav_amd import _lib

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def close(a, b, rtol, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    assert err <= rtol, f"{what}: scale-relative error {err:.3e} > {rtol:.1e}"
    return err


# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", [(1000, 384), (777, 1024), (513, 64), (129, 32), (5, 768), (300, 192)])
def test_layernorm(lib, cuda, rows, dim):
    x, w, b = rnd(rows, dim, seed=1, scale=3) + 0.5, rnd(dim, seed=2) + 1.0, rnd(dim, seed=3, scale=0.1)
    ref = F.layer_norm(x.double(), (dim,), w.double(), b.double(), 1e-6)
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    y = torch.empty_like(xd)
    _lib.check(lib.edv_layernorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), rows, dim, 1e-6, None, 0, 0, st()))
    close(y, ref, 2e-6, "layernorm")


def test_layernorm_with_temporal_pe(lib, cuda):
    Bc, T, P, Cc = 2, 5, 37, 64
    rows = Bc * T * P
    x, w, b, pe = rnd(rows, Cc, seed=1), rnd(Cc, seed=2) + 1, rnd(Cc, seed=3, scale=0.1), rnd(32, Cc, seed=4)
    ref = F.layer_norm(x, (Cc,), w, b, 1e-5).reshape(Bc, T, P, Cc) + pe[:T].reshape(1, T, 1, Cc)
    xd, wd, bd, ped = (t.to(cuda) for t in (x, w, b, pe))
    y = torch.empty_like(xd)
    _lib.check(lib.edv_layernorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), rows, Cc, 1e-5, ped.data_ptr(), P, T, st()))
    close(y, ref.reshape(rows, Cc), 2e-6, "layernorm+pe")


# ----------------------------------------------------------------------------------------------
_WS = {}


COUNTER_FLOATS = 4096  # MAX_COUNTERS of gemm_dma.hip


def gemm_ws(lib, cuda):
    """The stream-K workspace edv_gemm_workspace() asks for.  The contract is "zero-filled once"; here only the arrival counters
    at its head (COUNTER_FLOATS 32-bit words, gemm_dma.hip) are zeroed and the piece slots are poisoned, so that a piece nobody
    wrote would show as NaN."""
    if "ws" not in _WS:
        nbytes = lib.edv_gemm_workspace()
        assert nbytes > 0 and nbytes % 16 == 0
        w = torch.full((nbytes // 4,), float("nan"), device=cuda)
        w[:COUNTER_FLOATS] = 0
        _WS["ws"] = (w, nbytes)
    return _WS["ws"]


@pytest.mark.parametrize("M,N,K,act,use_bias,use_gamma,use_res", [
    (300, 384, 384, 0, True, False, False),
    (2 * 1370, 1152, 384, 0, True, False, False),     # qkv
    (2 * 1370, 384, 1536, 0, True, True, True),       # fc2 + LayerScale + residual
    (1370, 1536, 384, 1, True, False, False),         # fc1 + GELU
    (8 * 1370, 1536, 384, 1, True, False, False),     # 128x128 tile path
    (2 * 1369, 384, 588, 0, True, False, True),       # patch-embed (K tail: 588 = 18*32 + 12)
    (257, 48, 384, 0, True, False, False),            # N not a multiple of 32
    (1000, 32, 144, 2, True, False, False),           # N = 32 tile, ReLU
    (999, 16, 64, 0, False, False, False),            # N < 32
    (3, 96, 96, 0, True, False, False),               # tiny M
    (5000, 768, 48, 0, True, False, False),           # ConvT-like
    (8 * 1370, 384, 384, 0, True, True, True),        # proj at T=8: 1032 tiles, one round + 8 tiles split along K
    (8 * 1370, 384, 1536, 0, True, True, True),       # fc2 at T=8: 48 k-tiles per split tile
    (700 * 64, 64, 64, 2, True, False, True),         # 2 k-tiles per tile: pieces of a single k-tile
    (8 * 1370, 1152, 384, 0, True, False, False),     # qkv at T=8: three whole rounds + 24 tiles split
    (4 * 1370, 1152, 384, 0, True, False, False),     # one frame group of the encoder: 524 leftover tiles, runs straddle tile boundaries
    (4 * 1370, 384, 1536, 0, True, True, True),       # 516 tiles, no whole round: every tile is split
    (4 * 1370, 1536, 384, 1, True, False, False),     # fc1 + GELU applied by the last piece to arrive
])
@pytest.mark.parametrize("split", [False, True], ids=["plain", "streamk"])
def test_gemm(lib, cuda, M, N, K, act, use_bias, use_gamma, use_res, split):
    A, W = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    bias = rnd(N, seed=3, scale=0.1) if use_bias else None
    gamma = rnd(N, seed=4) + 1.2 if use_gamma else None
    R = rnd(M, N, seed=5) if use_res else None
    ref = A.double() @ W.double().T
    if bias is not None:
        ref = ref + bias.double()
    if act == 1:
        ref = F.gelu(ref)
    elif act == 2:
        ref = F.relu(ref)
    if gamma is not None:
        ref = ref * gamma.double()
    if R is not None:
        ref = ref + R.double()
    d = lambda t: None if t is None else t.to(cuda)
    Ad, Wd, bd, gd, Rd = d(A), d(W), d(bias), d(gamma), d(R)
    Cd = torch.full((M, N), float("nan"), device=cuda)
    ws, nbytes = gemm_ws(lib, cuda) if split else (None, 0)
    _lib.check(lib.edv_gemm(Ad.data_ptr(), Wd.data_ptr(), Cd.data_ptr(), M, N, K, _lib.ptr(bd), act, _lib.ptr(gd), _lib.ptr(Rd), _lib.ptr(ws), nbytes, st()),
               "edv_gemm")
    close(Cd, ref, 3e-6, f"gemm {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,expect_buffer", [(400_030, 1600, True), (700_030, 1600, False)], ids=["2.6GB-buffer-offsets", "4.5GB-flat-addresses"])
def test_gemm_output_beyond_two_gigabytes(lib, cuda, M, N, expect_buffer):
    """The buffer epilogue addresses C and the residual with 32-bit byte offsets in SCALAR registers (gemm_common.hpp, gemm_epilogue_buf): an
    output of 2.6 GB exercises offsets past 2^31, one of 4.5 GB must take the flat-address instantiation (fits_buffer).  Checked on row blocks
    at the start, around the 2^31 / 2^32 byte marks and at the ragged end (M % 64 != 0) against an fp64 product of the same rows."""
    K = 32
    g = torch.Generator(device=cuda).manual_seed(7)
    A = torch.randn(M, K, device=cuda, generator=g)
    W = torch.randn(N, K, device=cuda, generator=g) / math.sqrt(K)
    bias = torch.randn(N, device=cuda, generator=g) * 0.1
    R = torch.randn(M, N, device=cuda, generator=g)
    C = torch.full((M, N), float("nan"), device=cuda)
    assert (M * N * 4 < 2 ** 32 - 2 ** 20) == expect_buffer and M % 64 != 0
    _lib.check(lib.edv_gemm(A.data_ptr(), W.data_ptr(), C.data_ptr(), M, N, K, bias.data_ptr(), 0, None, R.data_ptr(), None, 0, st()), "edv_gemm")
    marks = [0, 2 ** 31 // (N * 4) - 100, min(2 ** 32 // (N * 4), M) - 200, M - 300]
    for r0 in marks:
        rows = slice(r0, min(r0 + 300, M))
        ref = A[rows].double() @ W.double().T + bias.double() + R[rows].double()
        close(C[rows], ref.cpu(), 3e-6, f"rows {r0}..")
    assert torch.isfinite(C).all()  # every row was written exactly where it belongs (the buffer was NaN-filled)


@pytest.mark.parametrize("M,split", [(1370, False), (8 * 1370, True)], ids=["plain", "streamk"])
def test_gemm_inplace_residual(lib, cuda, M, split):
    """proj / fc2 write the residual stream in place (C aliases R)."""
    N, K = 384, 384
    ws, nbytes = gemm_ws(lib, cuda) if split else (None, 0)
    A, W, X = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05), rnd(M, N, seed=3)
    ref = X.double() + A.double() @ W.double().T
    Ad, Wd, Xd = A.to(cuda), W.to(cuda), X.to(cuda)
    _lib.check(lib.edv_gemm(Ad.data_ptr(), Wd.data_ptr(), Xd.data_ptr(), M, N, K, None, 0, None, Xd.data_ptr(), _lib.ptr(ws), nbytes, st()))
    close(Xd, ref, 3e-6, "in-place residual")


def test_gemm_streamk_is_reproducible_and_leaves_counters_zero(lib, cuda):
    """The in-kernel merge sums a tile's pieces in run order whatever order they arrived in: two launches give identical bits;
    every launch leaves the arrival counters at zero (the next launch depends on it)."""
    ws, nbytes = gemm_ws(lib, cuda)
    for M, N, K in ((8 * 1370, 384, 1536), (4 * 1370, 1152, 384), (8 * 1370, 1536, 384)):
        A, W = rnd(M, K, seed=1).to(cuda), rnd(N, K, seed=2, scale=1 / math.sqrt(K)).to(cuda)
        outs = []
        for _ in range(3):
            Cd = torch.full((M, N), float("nan"), device=cuda)
            _lib.check(lib.edv_gemm(A.data_ptr(), W.data_ptr(), Cd.data_ptr(), M, N, K, None, 0, None, None, ws.data_ptr(), nbytes, st()), "edv_gemm")
            torch.cuda.synchronize()
            assert int(ws[:COUNTER_FLOATS].view(torch.int32).abs().sum()) == 0
            outs.append(Cd)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        plain = torch.empty_like(outs[0])
        _lib.check(lib.edv_gemm(A.data_ptr(), W.data_ptr(), plain.data_ptr(), M, N, K, None, 0, None, None, None, 0, st()), "edv_gemm")
        close(outs[0], plain.double().cpu(), 2e-6, "stream-K vs plain")


def test_gemm_rejects_bad_k(lib, cuda):
    a = torch.zeros(8, 6, device=cuda)
    assert lib.edv_gemm(a.data_ptr(), a.data_ptr(), a.data_ptr(), 8, 8, 6, None, 0, None, None, None, 0, st()) != 0
    assert b"multiple of 4" in lib.edv_last_error()


# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fr,H,W,Cin,Cout,stride,pre,post,res", [
    (2, 19, 23, 48, 64, 1, False, False, 0),
    (2, 37, 37, 384, 384, 2, False, False, 0),   # resize_layers[3]
    (3, 20, 16, 64, 64, 1, True, False, 2),      # ResidualConvUnit conv2 + both skip adds
    (1, 74, 74, 64, 32, 1, False, False, 0),     # output_conv1
    (1, 70, 98, 32, 32, 1, False, True, 0),      # output_conv2.0 + ReLU
    (2, 5, 7, 16, 32, 1, False, True, 0),        # micro head
    (2, 1, 2, 64, 64, 2, False, False, 1),       # degenerate grid
    (8, 19, 19, 384, 64, 1, False, False, 0),    # layer4_rn: 46 tiles of 108 k-tiles -> split along K with a workspace
    (8, 37, 37, 192, 64, 1, False, False, 0),    # layer3_rn: 172 tiles of 54 k-tiles
    (8, 37, 37, 384, 384, 2, False, False, 0),   # resize_layers[3] at T=8: 276 tiles of 108 k-tiles
    (8, 37, 37, 64, 64, 1, True, False, 2),      # ResidualConvUnit at 37x37: 172 tiles of 18 k-tiles, both residual adds in the merged epilogue
    (4, 74, 74, 64, 64, 1, True, True, 1),       # 343 tiles
])
@pytest.mark.parametrize("split", [False, True], ids=["plain", "streamk"])
def test_conv3x3(lib, cuda, Fr, H, W, Cin, Cout, stride, pre, post, res, split):
    x = rnd(Fr, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=1 / math.sqrt(9 * Cin))
    b = rnd(Cout, seed=3, scale=0.1)
    xin = F.relu(x) if pre else x
    ref = F.conv2d(xin.double(), w.double(), b.double(), stride=stride, padding=1)
    if post:
        ref = F.relu(ref)
    OH, OW = ref.shape[-2:]
    R1 = rnd(Fr, Cout, OH, OW, seed=4) if res >= 1 else None
    R2 = rnd(Fr, Cout, OH, OW, seed=5) if res >= 2 else None
    for r in (R1, R2):
        if r is not None:
            ref = ref + r.double()
    nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(cuda)
    xd, wd, bd, r1, r2 = nhwc(x), w.to(cuda), b.to(cuda), nhwc(R1), nhwc(R2)
    wp = torch.empty(Cout * 9 * Cin, device=cuda)
    _lib.check(lib.edv_pack_conv3x3(wd.data_ptr(), wp.data_ptr(), Cout, Cin, st()))
    y = torch.full((Fr, OH, OW, Cout), float("nan"), device=cuda)
    if split:
        ws, nbytes = gemm_ws(lib, cuda)
        for _ in range(2):  # twice: the second launch depends on the first leaving the arrival counters at zero
            y.fill_(float("nan"))
            _lib.check(lib.edv_conv3x3_ws(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr(), Fr, H, W, Cin, Cout, stride, int(pre), int(post),
                                          _lib.ptr(r1), _lib.ptr(r2), ws.data_ptr(), nbytes, st()), "edv_conv3x3_ws")
            torch.cuda.synchronize()
            assert int(ws[:COUNTER_FLOATS].view(torch.int32).abs().sum()) == 0
            close(y.permute(0, 3, 1, 2), ref, 3e-6, "conv3x3 stream-K")
        return
    _lib.check(lib.edv_conv3x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr(), Fr, H, W, Cin, Cout, stride, int(pre), int(post),
                               _lib.ptr(r1), _lib.ptr(r2), st()), "edv_conv3x3")
    close(y.permute(0, 3, 1, 2), ref, 3e-6, "conv3x3")


# ---- guard bands: the buffer epilogue masks ragged edges ONLY through descriptor range checks (rows >= M dropped because
# voffset + soffset is checked as one non-wrapping sum, columns >= N through a per-lane offset near 2^32).  Here C, R1 and R2 are slices of
# larger sentinel-filled allocations: a store that escapes the descriptor lands in a guard and is seen.
GUARD = 64 * 1024  # floats on either side: more than 63 rows x ld of every case below


def _guarded(t, cuda, fill):
    big = torch.full((t.numel() + 2 * GUARD,), fill, device=cuda)
    big[GUARD:GUARD + t.numel()] = t.reshape(-1).to(cuda)
    return big, big[GUARD:GUARD + t.numel()].view(t.shape)


def _guards_intact(big, n, fill):
    return bool((big[:GUARD] == fill).all()) and bool((big[GUARD + n:] == fill).all())


@pytest.mark.parametrize("M,N,K,act,use_gamma,use_res", [
    (64 * 5 + 1, 384 - 7, 384, 0, True, True),     # one row and 25 columns into the last tiles
    (64 * 40 + 63, 32 * 9 + 1, 96, 1, False, False),
    (1370, 48, 384, 0, False, True),
    (8 * 1370 + 13, 384 - 31, 1536, 0, True, True),  # stream-K: the merged epilogue of a ragged tile
])
@pytest.mark.parametrize("split", [False, True], ids=["plain", "streamk"])
def test_gemm_ragged_edges_stay_inside_guard_bands(lib, cuda, M, N, K, act, use_gamma, use_res, split):
    A, W = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    bias, gamma = rnd(N, seed=3, scale=0.1), (rnd(N, seed=4) + 1.2 if use_gamma else None)
    R = rnd(M, N, seed=5) if use_res else None
    ref = A.double() @ W.double().T + bias.double()
    if act == 1:
        ref = F.gelu(ref)
    if gamma is not None:
        ref = ref * gamma.double()
    if R is not None:
        ref = ref + R.double()
    SENT = 12345.0
    bigC, Cd = _guarded(torch.full((M, N), float("nan")), cuda, SENT)
    bigR, Rd = _guarded(R, cuda, float("nan")) if R is not None else (None, None)  # a read past the residual's end would put a NaN into C
    ws, nbytes = gemm_ws(lib, cuda) if split else (None, 0)
    g = None if gamma is None else gamma.to(cuda)
    Ad, Wd, bd = A.to(cuda), W.to(cuda), bias.to(cuda)  # (named: a temporary would be freed -- and its block reused -- before the kernel runs)
    _lib.check(lib.edv_gemm(Ad.data_ptr(), Wd.data_ptr(), Cd.data_ptr(), M, N, K, bd.data_ptr(), act, _lib.ptr(g), _lib.ptr(Rd), _lib.ptr(ws), nbytes, st()),
               "edv_gemm")
    torch.cuda.synchronize()
    assert _guards_intact(bigC, M * N, SENT), "a store escaped the C descriptor"
    close(Cd, ref, 3e-6, f"gemm {M}x{N}x{K} in guard bands")


@pytest.mark.parametrize("Fr,H,W,Cin,Cout,stride,res", [
    (1, 9, 7, 32, 48, 1, 2),     # 63 pixels: one ragged 64-row tile; Cout not a multiple of 64
    (3, 13, 11, 64, 96, 1, 1),   # 429 pixels
    (2, 37, 37, 64, 64, 2, 0),   # stride 2: 19 x 19 outputs
    (8, 19, 19, 384, 64, 1, 2),  # split along K with a workspace
])
@pytest.mark.parametrize("split", [False, True], ids=["plain", "streamk"])
def test_conv3x3_ragged_edges_stay_inside_guard_bands(lib, cuda, Fr, H, W, Cin, Cout, stride, res, split):
    x = rnd(Fr, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=1 / math.sqrt(9 * Cin))
    b = rnd(Cout, seed=3, scale=0.1)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1)
    OH, OW = ref.shape[-2:]
    Rs = [rnd(Fr, Cout, OH, OW, seed=4 + i) for i in range(res)]
    for r in Rs:
        ref = ref + r.double()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    SENT = -4321.0
    bigY, y = _guarded(torch.full((Fr, OH, OW, Cout), float("nan")), cuda, SENT)
    # the input sits in guard bands of NaN as well: a padding tap that read real memory instead of zeros would poison the border outputs
    bigX, xd = _guarded(nhwc(x), cuda, float("nan"))
    rd = [_guarded(nhwc(r), cuda, float("nan"))[1] for r in Rs] + [None, None]
    wd, bd = w.to(cuda), b.to(cuda)
    wp = torch.empty(Cout * 9 * Cin, device=cuda)
    _lib.check(lib.edv_pack_conv3x3(wd.data_ptr(), wp.data_ptr(), Cout, Cin, st()))
    if split:
        ws, nbytes = gemm_ws(lib, cuda)
        _lib.check(lib.edv_conv3x3_ws(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr(), Fr, H, W, Cin, Cout, stride, 0, 0, _lib.ptr(rd[0]), _lib.ptr(rd[1]),
                                      ws.data_ptr(), nbytes, st()), "edv_conv3x3_ws")
    else:
        _lib.check(lib.edv_conv3x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr(), Fr, H, W, Cin, Cout, stride, 0, 0, _lib.ptr(rd[0]), _lib.ptr(rd[1]), st()),
                   "edv_conv3x3")
    torch.cuda.synchronize()
    assert _guards_intact(bigY, y.numel(), SENT), "a store escaped the output descriptor"
    close(y.permute(0, 3, 1, 2), ref, 3e-6, "conv3x3 in guard bands")


@pytest.mark.parametrize("Fr,h,w,Cc,s", [(2, 37, 37, 48, 4), (2, 16, 20, 96, 2), (1, 3, 4, 32, 4)])
def test_conv_transpose(lib, cuda, Fr, h, w, Cc, s):
    x, wt, b = rnd(Fr, Cc, h, w, seed=1), rnd(Cc, Cc, s, s, seed=2, scale=1 / math.sqrt(Cc)), rnd(Cc, seed=3, scale=0.1)
    ref = F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=s)
    xd = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    wd, bd = wt.to(cuda), b.to(cuda)
    wp, bp = torch.empty(s * s * Cc * Cc, device=cuda), torch.empty(s * s * Cc, device=cuda)
    y = torch.full((Fr, h * s, w * s, Cc), float("nan"), device=cuda)
    _lib.check(lib.edv_conv_transpose(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), wp.data_ptr(), bp.data_ptr(), y.data_ptr(), Fr, h, w, Cc, s, st()))
    close(y.permute(0, 3, 1, 2), ref, 3e-6, "convT")


# ----------------------------------------------------------------------------------------------
def attn_spatial(lib, cuda, qd, o, Fr, N, heads):
    """edv_attn_spatial with the split workspace the planner asks for (poisoned, so a piece nobody wrote shows)."""
    nbytes = lib.edv_attn_spatial_workspace(Fr, N, heads)
    ws = torch.full((max(nbytes // 4, 4),), float("nan"), device=cuda)
    _lib.check(lib.edv_attn_spatial(qd.data_ptr(), o.data_ptr(), Fr, N, heads, ws.data_ptr(), nbytes, None, st()), "edv_attn_spatial")
    return nbytes


# (8, 1370, 6) is the bench shape: 528 tasks on 512 resident slots = one whole round + 16 tasks split by keys;
# (24, 1370, 1) leaves 264 tasks, all split; (40, 300, 16) runs several whole rounds with a long split tail.
@pytest.mark.parametrize("Fr,N,heads", [(2, 1370, 6), (1, 64, 2), (3, 10, 1), (1, 129, 12), (2, 321, 6), (1, 1369, 16), (8, 1370, 6), (24, 1370, 1),
                                        (40, 300, 16), (1, 4096, 1)])
def test_attn_spatial(lib, cuda, Fr, N, heads):
    D = heads * 64
    qkv = rnd(Fr * N, 3 * D, seed=1, scale=2.0)
    t = qkv.double().reshape(Fr, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * 64 ** -0.5, t[1], t[2]
    ref = ((q @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(Fr * N, D)
    qd = qkv.to(cuda)
    o = torch.full((Fr * N, D), float("nan"), device=cuda)
    attn_spatial(lib, cuda, qd, o, Fr, N, heads)
    close(o, ref, 5e-6, "attn_spatial")


def test_attention_on_poisoned_lds(lib, cuda):
    """Key / value rows past the sequence end (N % 64 != 0) reach LDS as zeros written by the DMA itself (out-of-range lanes of buffer_load ... lds,
    scratch/ubench/lds_dma_oob.hip); the kernel no longer clears its stages first.  With every CU's LDS full of NaN beforehand a stale byte entering
    the PV product (0 x NaN) would show in the output."""
    for Fr, N, heads in [(2, 1370, 6), (3, 10, 1), (1, 129, 12), (8, 1370, 6)]:
        D = heads * 64
        qkv = rnd(Fr * N, 3 * D, seed=1, scale=2.0)
        t = qkv.double().reshape(Fr, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
        q, k, v = t[0] * 64 ** -0.5, t[1], t[2]
        ref = ((q @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(Fr * N, D)
        qd = qkv.to(cuda)
        o = torch.full((Fr * N, D), float("nan"), device=cuda)
        _lib.check(lib.edv_debug_fill_lds(float("nan"), st()), "edv_debug_fill_lds")
        attn_spatial(lib, cuda, qd, o, Fr, N, heads)
        close(o, ref, 5e-6, f"attn_spatial after an LDS poison, N={N}")


def test_attn_spatial_workspace_contract(lib, cuda):
    """A split plan without (enough) workspace is refused, never run unsplit or out of bounds."""
    Fr, N, heads = 1, 1370, 6
    need = lib.edv_attn_spatial_workspace(Fr, N, heads)
    assert need > 0 and need % 16 == 0
    qd = torch.zeros(Fr * N, 3 * heads * 64, device=cuda)
    o = torch.empty(Fr * N, heads * 64, device=cuda)
    small = torch.empty(need // 4 - 4, device=cuda)
    assert lib.edv_attn_spatial(qd.data_ptr(), o.data_ptr(), Fr, N, heads, None, 0, None, st()) != 0
    assert lib.edv_attn_spatial(qd.data_ptr(), o.data_ptr(), Fr, N, heads, small.data_ptr(), need - 16, None, st()) != 0
    assert "workspace" in lib.edv_last_error().decode()


def test_attn_spatial_peaked_rows(lib, cuda):
    """Online-softmax rescale path: one key dominates, and it sits in a LATE tile for some rows."""
    Fr, N, heads, D = 1, 300, 1, 64
    qkv = rnd(Fr * N, 3 * D, seed=7, scale=0.5)
    qkv[:, :64] *= 6.0
    qkv[250, 64:128] *= 12.0  # key 250 (4th tile) gets very large scores against many queries
    t = qkv.double().reshape(Fr, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref = (((t[0] * 0.125) @ t[1].transpose(-2, -1)).softmax(-1) @ t[2]).transpose(1, 2).reshape(Fr * N, D)
    qd = qkv.to(cuda)
    o = torch.empty((Fr * N, D), device=cuda)
    attn_spatial(lib, cuda, qd, o, Fr, N, heads)
    close(o, ref, 5e-6, "attn_spatial peaked")


# T <= 8: all-queries-per-thread kernel (d = C/8 < 24) or pixel-per-workgroup kernel (d >= 24); T > 8: per-query kernel
@pytest.mark.parametrize("Bc,T,P,Cc", [(1, 8, 37 * 37, 192), (2, 3, 50, 64), (1, 16, 19 * 19, 384), (1, 32, 41, 32), (1, 1, 9, 64), (2, 32, 30, 256),
                                       (1, 8, 19 * 19, 384), (2, 5, 100, 192), (1, 8, 74 * 74, 64), (3, 4, 77, 64), (1, 1, 33, 384),
                                       (1, 16, 19 * 19, 768), (1, 16, 300, 128), (1, 32, 100, 1024), (1, 32, 200, 256), (2, 12, 50, 512),
                                       (1, 48, 40, 64), (1, 64, 25, 192), (2, 40, 9, 32), (1, 64, 7, 256), (1, 56, 13, 1024)])  # round 3: num_frames > 32
def test_attn_temporal(lib, cuda, Bc, T, P, Cc):
    heads, d = 8, Cc // 8
    qkv = rnd(Bc * T * P, 3 * Cc, seed=1, scale=1.5)
    t = qkv.double().reshape(Bc, T, P, 3, heads, d).permute(3, 0, 2, 4, 1, 5)  # [3, B, P, h, T, d]
    a = ((t[0] @ t[1].transpose(-1, -2)) * d ** -0.5).softmax(-1)
    ref = (a @ t[2]).permute(0, 3, 1, 2, 4).reshape(Bc * T * P, Cc)  # [B, T, P, h, d]
    qd = qkv.to(cuda)
    o = torch.full((Bc * T * P, Cc), float("nan"), device=cuda)
    _lib.check(lib.edv_attn_temporal(qd.data_ptr(), o.data_ptr(), Bc, T, P, Cc, heads, st()), "edv_attn_temporal")
    close(o, ref, 3e-6, "attn_temporal")


@pytest.mark.parametrize("Bc,T,P,Cc", [(1, 8, 361, 384), (2, 5, 33, 64), (1, 32, 17, 192)])
def test_rope_qk(lib, cuda, Bc, T, P, Cc):
    """pe="rope" (attention.py:402-429, restated with torch complex arithmetic as the reference does it): q and k rotated in place,
    v untouched; the transposed launch is the adjoint, so <R x, y> == <x, R^T y> and R^T R x == x."""
    from endodav_amd.endodav import _rope_table

    table = _rope_table(Cc, 32)  # [32, C/2, 2]
    fc = torch.view_as_complex(table)[:T]  # [T, C/2]
    qkv = rnd(Bc * T * P, 3 * Cc, seed=1, scale=1.5)
    t = qkv.reshape(Bc, T, P, 3, Cc)
    ref = t.clone()
    for j in range(2):
        z = torch.view_as_complex(t[:, :, :, j].reshape(Bc, T, P, Cc // 2, 2).contiguous()) * fc[None, :, None, :]
        ref[:, :, :, j] = torch.view_as_real(z).flatten(-2)
    ref = ref.reshape(Bc * T * P, 3 * Cc)
    qd, td = qkv.to(cuda), table.to(cuda)
    _lib.check(lib.edv_rope_qk(qd.data_ptr(), td.data_ptr(), Bc, T, P, Cc, 0, st()), "edv_rope_qk")
    close(qd, ref, 1e-6, "rope")
    assert torch.equal(qd[:, 2 * Cc:].cpu(), qkv[:, 2 * Cc:])
    y = rnd(Bc * T * P, 3 * Cc, seed=2)
    yd = y.to(cuda)
    _lib.check(lib.edv_rope_qk(yd.data_ptr(), td.data_ptr(), Bc, T, P, Cc, 1, st()), "edv_rope_qk^T")
    lhs, rhs = (qd.double().cpu() * y.double()).sum().item(), (qkv.double() * yd.double().cpu()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0)
    _lib.check(lib.edv_rope_qk(qd.data_ptr(), td.data_ptr(), Bc, T, P, Cc, 1, st()), "edv_rope_qk^T")
    close(qd, qkv, 1e-6, "rope round trip")


def test_attn_temporal_rejects_clips_beyond_64_frames(lib, cuda):
    z = torch.zeros(65 * 8 * 3 * 64, device=cuda)
    assert lib.edv_attn_temporal(z.data_ptr(), z.data_ptr(), 1, 65, 8, 64, 8, st()) != 0
    assert b"64" in lib.edv_last_error()


# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fr,P,Cc", [(3, 25, 64), (2, 1369, 192), (2, 361, 384), (4, 6, 32), (1, 5476, 64), (2, 33, 1024), (3, 100, 96), (8, 5476, 64)])
@pytest.mark.parametrize("two_stage", [False, True], ids=["strided", "two_stage"])
def test_groupnorm(lib, cuda, Fr, P, Cc, two_stage):
    x = rnd(Fr, P, Cc, seed=1, scale=2) + 3.0  # mean >> std: one-pass E[x^2]-E[x]^2 would lose digits
    w, b = rnd(Cc, seed=2) + 1, rnd(Cc, seed=3, scale=0.1)
    ref = F.group_norm(x.double().permute(0, 2, 1), 32, w.double(), b.double(), 1e-6).permute(0, 2, 1)
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    y, stats = torch.full_like(xd, float("nan")), torch.empty(Fr * 32 * 2, device=cuda)
    nb = lib.edv_groupnorm_workspace(Fr, P, Cc) if two_stage else 0
    ws = torch.full((max(nb // 4, 4),), float("nan"), device=cuda)
    _lib.check(lib.edv_groupnorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), stats.data_ptr(), Fr, P, Cc, 32, 1e-6,
                                 ws.data_ptr() if two_stage else None, nb, st()))
    close(y, ref, 5e-6, "groupnorm")


def test_geglu(lib, cuda):
    M, inner = 777, 256
    x = rnd(M, 2 * inner, seed=1, scale=3)
    ref = x[:, :inner].double() * F.gelu(x[:, inner:].double())
    xd = x.to(cuda)
    y = torch.empty(M, inner, device=cuda)
    _lib.check(lib.edv_geglu(xd.data_ptr(), y.data_ptr(), M, inner, st()))
    close(y, ref, 2e-6, "geglu")


@pytest.mark.parametrize("Fr,H,W,Cc,OH,OW", [(2, 19, 19, 64, 37, 37), (1, 296, 296, 32, 518, 518), (2, 518, 518, 1, 259, 259), (2, 129, 129, 1, 64, 64),
                                             (1, 16, 20, 64, 32, 40), (2, 1, 2, 32, 3, 4), (1, 7, 9, 4, 7, 9), (3, 37, 37, 1, 480, 640)])
def test_bilinear(lib, cuda, Fr, H, W, Cc, OH, OW):
    x = rnd(Fr, Cc, H, W, seed=1)
    ref = F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=True)
    xd = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    y = torch.empty(Fr, OH, OW, Cc, device=cuda)
    _lib.check(lib.edv_bilinear(xd.data_ptr(), y.data_ptr(), Fr, H, W, Cc, OH, OW, st()))
    close(y.permute(0, 3, 1, 2), ref, 2e-6, "bilinear")


@pytest.mark.parametrize("act", [0, 2, 3, 4])
def test_dot_channels(lib, cuda, act):
    M, Cc = 12345, 32
    x, w, b = rnd(M, Cc, seed=1), rnd(Cc, seed=2), rnd(1, seed=3)
    ref = x.double() @ w.double() + b.double()
    ref = {0: ref, 2: F.relu(ref), 3: torch.sigmoid(ref), 4: torch.sigmoid(-ref)}[act]
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    y = torch.empty(M, device=cuda)
    _lib.check(lib.edv_dot_channels(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, Cc, act, st()))
    close(y, ref, 2e-6, "dot_channels")


@pytest.mark.parametrize("H,W,ih,iw", [(518, 518, 518, 518), (256, 320, 224, 280), (64, 80, 42, 56), (30, 50, 42, 42)])
def test_patchify(lib, cuda, H, W, ih, iw):
    Fr = 2
    x = torch.rand(Fr, 3, H, W, generator=torch.Generator().manual_seed(3))
    xr = F.interpolate(x, size=(ih, iw), mode="bilinear", align_corners=True)
    xn = (xr - torch.tensor([0.485, 0.456, 0.406])[None, :, None, None]) / torch.tensor([0.229, 0.224, 0.225])[None, :, None, None]
    ref = F.unfold(xn, kernel_size=14, stride=14).transpose(1, 2).reshape(-1, 588)  # rows (f, py, px), cols (c, ky, kx)
    xd = x.to(cuda)
    cols = torch.empty(ref.shape, device=cuda)
    _lib.check(lib.edv_patchify(xd.data_ptr(), cols.data_ptr(), Fr, H, W, ih, iw, st()))
    close(cols, ref, 2e-6, "patchify")


@pytest.mark.parametrize("S,oh,ow", [(37, 16, 20), (16, 37, 37), (37, 3, 4), (16, 3, 4), (37, 37, 37)])
def test_bicubic_pos(lib, cuda, S, oh, ow):
    D = 64
    g = rnd(S, S, D, seed=1)
    sh, sw = (oh + 0.1) / math.sqrt(S * S), (ow + 0.1) / math.sqrt(S * S)
    ref = F.interpolate(g.permute(2, 0, 1)[None], scale_factor=(sh, sw), mode="bicubic")[0].permute(1, 2, 0)
    assert ref.shape[:2] == (oh, ow)
    gd = g.to(cuda)
    out = torch.empty(oh, ow, D, device=cuda)
    _lib.check(lib.edv_bicubic_pos(gd.data_ptr(), out.data_ptr(), S, D, oh, ow, sh, sw, st()))
    close(out, ref, 3e-6, "bicubic_pos")


@pytest.mark.parametrize("H,W,OH,OW", [(480, 640, 518, 686), (1024, 1280, 518, 644), (50, 60, 100, 120)])
def test_resize_bicubic(lib, cuda, H, W, OH, OW):
    # fp64 reference: ATen's fp32 bicubic evaluates the source coordinate in fp32 and is itself 4e-5 .. 9e-5 of the range away from the fp64
    # result at these sizes (test_resize_bicubic_against_fp64 prints it); the kernel splits the coordinate in integers
    x = torch.rand(3, 1, H, W, generator=torch.Generator().manual_seed(5))
    ref = F.interpolate(x.double(), size=(OH, OW), mode="bicubic", align_corners=False)
    xd = x.to(cuda)
    y = torch.empty(3, 1, OH, OW, device=cuda)
    _lib.check(lib.edv_resize_bicubic(xd.data_ptr(), y.data_ptr(), 3, H, W, OH, OW, st()))
    close(y, ref, 3e-6, "resize_bicubic")


# what infer_video_depth's pre-resize sees (video.HipWindowRunner), then the edges of the kernel: all four taps clamped, identity, up-scale
RESIZE_VIDEO_SHAPES = [
    (1080, 1920, 518, 924),  # a full-HD frame at image_shape 518 x 518 (lower_bound_size)
    (1024, 1280, 224, 280),  # the endoscopy frame at the reference's 224 x 280
    (61, 83, 42, 56),        # odd sizes, no multiple of anything
    (20, 30, 60, 90),        # 3x up-scale: negative source coordinates at the border
    (1, 7, 5, 9), (7, 1, 9, 5), (2, 3, 7, 8), (3, 2, 5, 6), (1, 1, 4, 4), (37, 53, 1, 1), (3, 3, 2, 2),  # height / width 1, 2, 3: every tap clamps
]


def _frames_u8(planes, H, W, seed=5):
    """Values k / 255 in [0, 1], as the runner feeds the kernel (uint8 frames converted on the device)."""
    return torch.randint(0, 256, (planes, 1, H, W), generator=torch.Generator().manual_seed(seed)).float() / 255.0


@pytest.mark.parametrize("H,W,OH,OW", RESIZE_VIDEO_SHAPES)
def test_resize_bicubic_against_fp64(lib, cuda, H, W, OH, OW):
    """edv_resize_bicubic against the published algorithm in fp64 (Keys cubic a = -0.75, half-pixel centres, clamped borders, no antialiasing:
    F.interpolate(bicubic, align_corners=False) on doubles = cv2.INTER_CUBIC on float images), on 8-bit image values.  ATen's own fp32 result
    is printed beside it: it evaluates the source coordinate in fp32, whose ulp at row 1000 is 6e-5, and ends 1e-4 of the range away from
    the fp64 result on a full-HD frame; the kernel splits the coordinate in integers and stays at fp32 rounding of the sum at every size."""
    x = _frames_u8(3, H, W)
    ref = F.interpolate(x.double(), size=(OH, OW), mode="bicubic", align_corners=False)
    aten = F.interpolate(x, size=(OH, OW), mode="bicubic", align_corners=False)
    xd = x.to(cuda)
    y = torch.full((3, 1, OH, OW), float("nan"), device=cuda)
    _lib.check(lib.edv_resize_bicubic(xd.data_ptr(), y.data_ptr(), 3, H, W, OH, OW, st()))
    scale = ref.abs().max().item()
    err = (y.double().cpu() - ref).abs().max().item() / scale
    aten_err = (aten.double() - ref).abs().max().item() / scale
    print(f"\n[resize_bicubic] {H}x{W} -> {OH}x{OW}: scale-relative error {err:.2e} (ATen fp32 {aten_err:.2e})")
    close(y, ref, 3e-6, "resize_bicubic vs fp64")


@pytest.mark.parametrize("H,W", [(224, 280), (42, 56), (1, 1), (3, 5)])
def test_resize_bicubic_identity_is_exact(lib, cuda, H, W):
    """Same size in and out: the source coordinate is the pixel itself, the weights are (0, 1, 0, 0), the input comes back bit for bit."""
    xd = _frames_u8(3, H, W, seed=6).to(cuda)
    y = torch.full((3, 1, H, W), float("nan"), device=cuda)
    _lib.check(lib.edv_resize_bicubic(xd.data_ptr(), y.data_ptr(), 3, H, W, H, W, st()))
    assert torch.equal(y, xd)


@pytest.mark.parametrize("dv", [False, True])
def test_fold_lora(lib, cuda, dv):
    nout, nin, r = 1536, 384, 4
    W, A, Bm = rnd(nout, nin, seed=1, scale=0.05), rnd(r, nin, seed=2, scale=0.1), rnd(nout, r, seed=3)
    U, V = (rnd(r, 1, seed=4) + 1, rnd(nout, 1, seed=5) + 1) if dv else (None, None)
    scale = 1.0 if dv else 2.0
    ref = W.double() + scale * ((Bm * V).double() @ (A * U).double() if dv else Bm.double() @ A.double())
    d = lambda t: None if t is None else t.to(cuda)
    Wd, Ad, Bd, Ud, Vd = d(W), d(A), d(Bm), d(U), d(V)
    out = torch.empty(nout, nin, device=cuda)
    _lib.check(lib.edv_fold_lora(Wd.data_ptr(), Ad.data_ptr(), Bd.data_ptr(), _lib.ptr(Ud), _lib.ptr(Vd), scale, out.data_ptr(), nout, nin, r, st()))
    close(out, ref, 2e-6, "fold_lora")
    # the fold is equivalent to the reference's side product x A^T B^T (mylora/layers.py:152-155)
    x = rnd(64, nin, seed=9)
    side = x.double() @ W.double().T + scale * (x.double() @ ((A * U) if dv else A).double().T @ ((Bm * V) if dv else Bm).double().T)
    close(x.double() @ out.double().cpu().T, side, 1e-6, "fold == side product")


def test_gelu_accuracy(lib, cuda):
    """The erf-form GELU of every epilogue (common.hpp gelu_erf, the device library's erff) against the fp64 function over |x| <= 8:
    fp32 rounding level, like ATen's own fp32 GELU (1.2e-6 over the same range).  (Round 2 tried Abramowitz & Stegun 7.1.26 for erf -- 16
    VALU instructions instead of ~35, 4.7e-7 absolute -- to shorten fc1's epilogue: +0.5 % on the ViT-S step, 0 on ViT-B, and its 1e-7
    shift flipped one ReLU mask in a micro gradient case past the 2e-4 gate, so the exact form stayed.)"""
    x = torch.linspace(-8.0, 8.0, 1 << 20, dtype=torch.float32)
    out = torch.empty_like(x, device=cuda)
    xd = x.to(cuda)
    _lib.check(lib.edv_ew_bwd(xd.data_ptr(), None, None, out.data_ptr(), x.numel(), 3, _lib.stream_ptr()))
    ref = torch.nn.functional.gelu(x.double())
    err = (out.cpu().double() - ref).abs()
    aten = (torch.nn.functional.gelu(x).double() - ref).abs()
    print(f"\n[gelu] max abs error {err.max().item():.2e} (ATen fp32 {aten.max().item():.2e}); over |x| <= 3: {err[x.abs() <= 3].max().item():.2e}")
    assert err.max().item() <= 1.5e-6 and err[x.abs() <= 3].max().item() <= 5e-7


@pytest.mark.parametrize("M,C", [(8 * 361, 384), (1000, 64), (8 * 1369, 192), (77, 32), (43808, 64)])
def test_gemm_geglu_epilogue(lib, cuda, M, C):
    """ff.net.0 of a motion module + GEGLU in one launch (edv_gemm_geglu on the weight interleaved by edv_pack_geglu) against
    x, gate = F.linear(h, W, b).chunk(2, -1); x * F.gelu(gate) in fp64 (motion_module.py GEGLU.forward); ragged M, all four module widths."""
    N, K = 8 * C, C
    h, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K)), rnd(N, seed=3, scale=0.2)
    y = h.double() @ W.double().T + b.double()
    val, gate = y.chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    hd, Wd, bd = h.to(cuda), W.to(cuda), b.to(cuda)
    Wi, bi = torch.empty_like(Wd), torch.empty_like(bd)
    _lib.check(lib.edv_pack_geglu(Wd.data_ptr(), bd.data_ptr(), Wi.data_ptr(), bi.data_ptr(), N, K, st()), "edv_pack_geglu")
    # the packing is a permutation of rows: block b of 64 = value rows 32b.., then gate rows N/2 + 32b..
    perm = torch.cat([torch.cat([torch.arange(32 * k, 32 * k + 32), N // 2 + torch.arange(32 * k, 32 * k + 32)]) for k in range(N // 64)])
    assert torch.equal(Wi.cpu(), W[perm]) and torch.equal(bi.cpu(), b[perm])
    out = torch.full((M, N // 2), float("nan"), device=cuda)
    _lib.check(lib.edv_gemm_geglu(hd.data_ptr(), Wi.data_ptr(), bi.data_ptr(), out.data_ptr(), M, N, K, st()), "edv_gemm_geglu")
    close(out, ref, 3e-6, f"geglu {M}x{N}x{K}")


def test_attention_beside_other_kernels(lib, cuda):
    """Two chains LayerNorm -> qkv GEMM -> spatial attention -> proj GEMM (+ residual) on two streams, the way the two-frame-group encoder runs
    them: every buffer of every round must be bit-identical to the chain run alone.  (Round 2's attention kernel left an LDS read in flight
    across its tile barrier; alone on the GPU that never showed, beside another stream's kernels one wave in a few hundred launches read the
    next tile's V rows.)"""
    Fr, N, heads = 2, 1370, 6
    D, M = heads * 64, Fr * N
    g = torch.Generator(device=cuda).manual_seed(3)
    r = lambda *s, scale=1.0: torch.randn(*s, device=cuda, generator=g) * scale
    Wq, bq, Wp, bp = r(3 * D, D, scale=0.05), r(3 * D, scale=0.1), r(D, D, scale=0.05), r(D, scale=0.1)
    lw, lb = r(D, scale=0.1) + 1, r(D, scale=0.1)
    nb, gb = lib.edv_attn_spatial_workspace(Fr, N, heads), lib.edv_gemm_workspace()

    class Lane:
        def __init__(self):
            self.x0 = r(M, D)
            self.x, self.xn, self.qkv, self.att = self.x0.clone(), torch.empty(M, D, device=cuda), torch.empty(M, 3 * D, device=cuda), torch.empty(M, D, device=cuda)
            self.ws, self.gws, self.s = torch.zeros(max(nb // 4, 4), device=cuda), torch.zeros(gb // 4, device=cuda), torch.cuda.Stream()

        def run(self, blocks=2):
            s = self.s.cuda_stream
            with torch.cuda.stream(self.s):
                self.x.copy_(self.x0)
            for _ in range(blocks):
                _lib.check(lib.edv_layernorm(self.x.data_ptr(), lw.data_ptr(), lb.data_ptr(), self.xn.data_ptr(), M, D, 1e-6, None, 0, 0, s))
                _lib.check(lib.edv_gemm(self.xn.data_ptr(), Wq.data_ptr(), self.qkv.data_ptr(), M, 3 * D, D, bq.data_ptr(), 0, None, None, self.gws.data_ptr(), gb, s))
                _lib.check(lib.edv_attn_spatial(self.qkv.data_ptr(), self.att.data_ptr(), Fr, N, heads, self.ws.data_ptr(), nb, None, s))
                _lib.check(lib.edv_gemm(self.att.data_ptr(), Wp.data_ptr(), self.x.data_ptr(), M, D, D, bp.data_ptr(), 0, None, self.x.data_ptr(), self.gws.data_ptr(), gb, s))

        def snap(self):
            return [t.clone() for t in (self.qkv, self.att, self.x)]

    a, b = Lane(), Lane()
    torch.cuda.synchronize()
    refs = []
    for lane in (a, b):
        lane.run()
        torch.cuda.synchronize()
        refs.append(lane.snap())
    for it in range(300):
        a.run()
        b.run()
        torch.cuda.synchronize()
        for lane, ref in zip((a, b), refs):
            for name, got, want in zip(("qkv", "attention", "x"), lane.snap(), ref):
                assert torch.equal(got, want), f"round {it}: {name} differs from the solo run by {float((got - want).abs().max()):.3e}"
