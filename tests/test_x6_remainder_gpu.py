"""The remainder plan of the bf16 x 6 GEMM (gemm_x6.hip, streamk_plan.hpp: plan_remainder) through edv_gemm_x6: the few tiles past a whole number
of rounds of CUs are cut along k, their pieces run first, every other tile stays whole.  edv_set_x6_remainder(2, 8) plans for 8 CUs wherever the
walk is supported, so ten-tile problems take the path; one shape is sized from the device's CU count so that the default policy triggers.

Gates: those of tests/test_gemm_x6_gpu.py.  Every epilogue: 3e-6 of the output scale against fp64.  The product itself (no epilogue, as in that
file): error relative to sum |a w|, against edv_gemm on the same operands rms <= 1.05 x, maximum <= max(1.25 x, 4 u), and 8 u absolute, u = 2^-24.
Every epilogue is also held to the two relative gates against edv_gemm with the same epilogue; there the error is taken relative to sum |a w|
carried through the epilogue (+ |bias|, x |gamma|, + |R|), since an element whose product cancels would otherwise measure the bias's rounding."""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

from endodav_amd import _lib

from .test_gemm_x6_gpu import planes_of
from .test_kernels_gpu import COUNTER_FLOATS, close, rnd, st

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64          # NaN guard rows on both sides of C
WS_GUARD = 4096     # NaN guard floats on both sides of the workspace
GROUP_M = 8         # launch_x6's tile order: groups of 8 row blocks swept column by column
WGS = 2             # resident workgroups per CU of gemm_x6_kernel (2 x 72 KB of LDS)
EPILOGUES = ("bias", "gelu", "gamma_res")
SMALL = [(640, 256, 48),     # 10 tiles = 8 + 2, three k-steps: a run is a whole tile, no piece is handed off
         (600, 200, 384),    # ragged M and N, 24 k-steps: 12 runs of 4, the ragged corner tile is split
         (1100, 384, 64)]    # 27 tiles = 3 x 8 + 3, 4 k-steps: runs of 3 cross tile boundaries


@pytest.fixture(autouse=True)
def restore_mode(lib):
    assert "EDV_X6_GROUP_M" not in os.environ and "EDV_GEMM_PLAIN" not in os.environ
    yield
    _lib.check(lib.edv_set_x6_remainder(1, 0))


def remainder_plan(lib, tiles, cus, nkt, mode):
    out = (C.c_int64 * 8)()
    out[0], out[1] = WGS, mode
    assert lib.edv_split_plan(4, tiles, cus, nkt, out) == 0
    return tuple(out)


def split_mask(M, N, first_split, cuda):
    """[M, N] bool: the elements of the tiles with index >= first_split in launch_x6's tile order."""
    tiles_m, tiles_n = (M + 127) // 128, (N + 127) // 128
    mask = torch.zeros(M, N, dtype=torch.bool, device=cuda)
    for tile in range(first_split, tiles_m * tiles_n):
        gidx = tile // (GROUP_M * tiles_n)
        first = gidx * GROUP_M
        rows = min(GROUP_M, tiles_m - first)
        r = tile - gidx * GROUP_M * tiles_n
        tn, tm = r // rows, first + r % rows
        mask[tm * 128:(tm + 1) * 128, tn * 128:(tn + 1) * 128] = True
    return mask


_OPERANDS = {}


def operands(lib, cuda, M, N, K):
    """Operands, fp64 product and sum |a w| of one shape, made once and left unchanged."""
    if (M, N, K) not in _OPERANDS:
        _OPERANDS.clear()  # one shape at a time on the device
        A, W = (rnd(M, K, seed=11) * 2).to(cuda), rnd(N, K, seed=12, scale=1 / math.sqrt(K)).to(cuda)
        bias, gamma, R = rnd(N, seed=3, scale=0.1).to(cuda), (rnd(N, seed=4) + 1.2).to(cuda), rnd(M, N, seed=5).to(cuda)
        _OPERANDS[(M, N, K)] = dict(A=A, W=W, bias=bias, gamma=gamma, R=R, planes=planes_of(lib, W, N, K), prod=A.double() @ W.double().T,
                                    mag=A.double().abs() @ W.double().abs().T)
    return _OPERANDS[(M, N, K)]


def check_shape(lib, cuda, M, N, K, epi, mode, cus):
    o = operands(lib, cuda, M, N, K)
    act = 1 if epi == "gelu" else 0
    gamma, R = (o["gamma"], o["R"]) if epi == "gamma_res" else (None, None)
    ref, scale = o["prod"] + o["bias"].double(), o["mag"] + o["bias"].double().abs()
    if act:
        ref = F.gelu(ref)
    if gamma is not None:
        ref, scale = ref * gamma.double() + R.double(), scale * gamma.double().abs() + R.double().abs()
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    dev_cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    rem, grid, first_split, chunk, nsplit, split_tiles, units, ws_floats = remainder_plan(lib, tiles, cus or dev_cus, K // 16, mode)
    assert rem == 1 and split_tiles == tiles % (cus or dev_cus) and split_tiles > 0, "the shape does not take the remainder plan"

    nbytes = lib.edv_gemm_workspace()
    assert ws_floats * 4 <= nbytes
    wsbuf = torch.full((nbytes // 4 + 2 * WS_GUARD,), float("nan"), device=cuda)  # poisoned slots: a piece nobody wrote would show as NaN
    ws = wsbuf[WS_GUARD:WS_GUARD + nbytes // 4]
    ws[:COUNTER_FLOATS] = 0

    def launch(fn, out, mode_, cus_, epilogue=True):
        _lib.check(lib.edv_set_x6_remainder(mode_, cus_))
        w = o["planes"] if fn is lib.edv_gemm_x6 else o["W"]
        b, a, g, r = (o["bias"], act, gamma, R) if epilogue else (None, 0, None, None)
        _lib.check(fn(o["A"].data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, _lib.ptr(b), a, _lib.ptr(g), _lib.ptr(r), ws.data_ptr(), nbytes, st()),
                   f"{M}x{N}x{K} {epi}")
        torch.cuda.synchronize()
        assert int(ws[:COUNTER_FLOATS].view(torch.int32).abs().sum()) == 0, "the arrival counters are not left at zero"

    bufs = [torch.full((M + 2 * GUARD, N), float("nan"), device=cuda) for _ in range(5)]
    off, first, second, third, c32 = (b[GUARD:GUARD + M] for b in bufs)
    launch(lib.edv_gemm_x6, off, 0, 0)
    launch(lib.edv_gemm_x6, first, mode, cus)
    launch(lib.edv_gemm_x6, second, mode, cus)
    launch(lib.edv_gemm_x6, third, mode, cus)
    # the launch did take the remainder walk: run 0 starts at unit 0, so where a run is shorter than a tile its slot 0 is a piece that was written;
    # where every run is a whole tile no slot is touched
    slots = ws[COUNTER_FLOATS:COUNTER_FLOATS + nsplit * 2 * 128 * 128]
    if chunk < K // 16:
        assert not torch.isnan(slots[:128 * 128]).any(), "run 0 left no piece: the launch did not take the remainder walk"
    else:
        assert torch.isnan(slots).all()
    launch(lib.edv_gemm, c32, 0, 0)

    # 4, 5. every element up to row M - 1 and column N - 1 is stored, nothing outside C or the workspace is
    for b in bufs:
        assert torch.isnan(b[:GUARD]).all() and torch.isnan(b[GUARD + M:]).all(), "a launch wrote outside C's rows"
        assert not torch.isnan(b[GUARD:GUARD + M]).any(), "an element of C was not stored"
    assert torch.isnan(wsbuf[:WS_GUARD]).all() and torch.isnan(wsbuf[WS_GUARD + nbytes // 4:]).all(), "a launch wrote outside the workspace"
    # 3, 4. the same bits from every launch on the same workspace
    assert torch.equal(first, second) and torch.equal(first, third)
    # 2. a tile that was not split keeps the bits of the plain grid
    mask = split_mask(M, N, first_split, cuda)
    assert mask[M - 1, N - 1], "the last tile is a split tile"
    assert torch.equal(first[~mask], off[~mask]), "a whole tile differs from mode 0"
    if chunk >= K // 16 and (K // 16) % chunk == 0:
        assert torch.equal(first, off)  # every run is a whole tile: nothing is merged
    # 1. the gates of test_gemm_x6_gpu.py
    close(first, ref, 3e-6, f"gemm_x6 remainder {M}x{N}x{K} {epi}")
    e6, e32 = (first.double() - ref).abs() / scale, (c32.double() - ref).abs() / scale
    gates(e6, e32, mask, f"{M}x{N}x{K} {epi}", absolute=False)
    if epi == "bias":  # once per shape: the product itself, exactly as test_gemm_x6_gpu.py measures it
        p6, p32 = bufs[1][GUARD:GUARD + M], bufs[4][GUARD:GUARD + M]
        launch(lib.edv_gemm_x6, p6, mode, cus, epilogue=False)
        launch(lib.edv_gemm, p32, 0, 0, epilogue=False)
        gates((p6.double() - o["prod"]).abs() / o["mag"], (p32.double() - o["prod"]).abs() / o["mag"], mask, f"{M}x{N}x{K} product", absolute=True)


def gates(e6, e32, mask, what, absolute):
    """rms and maximum no worse than the fp32 pipe's, over all tiles and over the split tiles alone (they are few: the whole tiles must not hide them)."""
    for sel, which in ((slice(None), "all tiles"), (mask, "split tiles")):
        a, b = e6[sel], e32[sel]
        rms6, rms32 = a.pow(2).mean().sqrt().item(), b.pow(2).mean().sqrt().item()
        print(f"{what} {which}: rms {rms6 / U:.3f} u against {rms32 / U:.3f} u, max {a.max().item() / U:.2f} u against {b.max().item() / U:.2f} u")
        assert rms6 <= rms32 * 1.05, (what, which, rms6, rms32)
        assert a.max().item() <= max(b.max().item() * 1.25, 4 * U), (what, which, a.max().item(), b.max().item())
        if absolute:
            assert a.max().item() <= 8 * U, (what, which, a.max().item())


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("M,N,K", SMALL)
def test_remainder_wherever_supported(lib, cuda, M, N, K, epi):
    check_shape(lib, cuda, M, N, K, epi, 2, 8)


@pytest.mark.parametrize("epi", EPILOGUES)
def test_remainder_by_default_policy(lib, cuda, epi):
    """CUs + 4 tiles of three k-steps: the policy itself routes it (asserted through edv_split_plan inside)."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    check_shape(lib, cuda, (cus + 4) * 128 - 48, 128, 48, epi, 1, 0)
