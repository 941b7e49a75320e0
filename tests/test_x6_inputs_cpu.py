"""What tests/test_x6_edges_gpu.py relies on, checked without a GPU: every input class of tests/x6_inputs.py is inside the domain of the bf16 x 6
construction (a CPU emulation of it meets the gates the kernels are held to), the cancelling operands do cancel, the operands of the bit-for-bit
scaling tests keep every term a normal number, the shapes get the stream-K plans their comments claim, and the split of a non-finite or nearly
overflowing value is what include/endodav_hip.h says it is."""
import ctypes as C

import pytest
import torch

from . import x6_inputs as X

GEMM_X6, ATTN = 1, 3  # edv_split_plan kinds


def plan(lib, kind, n, slots, k_tiles):
    out = (C.c_int64 * 8)()
    assert lib.edv_split_plan(kind, n, slots, k_tiles, out) == 0
    return dict(zip(("split", "grid", "whole_rounds", "chunk", "nsplit", "stride", "units", "ws"), out))


def test_gemm_shapes_get_the_plans_the_gpu_test_names(lib):
    """An MI355X keeps 2 x 256 workgroups of gemm_x6_kernel resident (two per CU)."""
    (M, N, K), (M2, N2, K2) = X.GEMM_SHAPES
    tiles = -(-M // 128) * -(-N // 128)
    assert tiles == 20 and K // 16 == 48
    p = plan(lib, GEMM_X6, tiles, 512, K // 16)
    assert p["split"] == 1 and p["whole_rounds"] == 0 and p["units"] == tiles * 48  # every tile is cut along k
    assert p["nsplit"] > tiles                                                      # into more runs than tiles: no tile runs whole
    tiles2 = -(-M2 // 128) * -(-N2 // 128)
    assert tiles2 == 6 and plan(lib, GEMM_X6, tiles2, 512, K2 // 16)["split"] == 0  # plain grid, workspace or not


def test_attention_shapes_get_the_plans_the_gpu_test_names(lib):
    """attn_x6_kernel: 256 queries per task, 64 keys per tile, one resident workgroup per CU."""
    tasks = lambda Fr, N, heads: Fr * heads * -(-N // 256)
    p = plan(lib, ATTN, tasks(2, 321, 2), 256, -(-321 // 64))
    assert tasks(2, 321, 2) == 8 and p["whole_rounds"] == 0 and p["stride"] == 8 and p["nsplit"] > 8   # all 8 tasks split by keys
    p = plan(lib, ATTN, tasks(1, 257, 1), 256, -(-257 // 64))
    assert p["whole_rounds"] == 0 and p["stride"] == 2 and p["nsplit"] > 2
    p = plan(lib, ATTN, tasks(3, 300, 43), 256, -(-300 // 64))
    assert tasks(3, 300, 43) == 258 and p["whole_rounds"] == 1 and p["stride"] == 2 and p["nsplit"] > 2  # one whole round + two split tasks


@pytest.mark.parametrize("M,N,K", X.GEMM_SHAPES)
def test_cancelling_operands_cancel(M, N, K):
    """A condition on the input, not a measurement: |A W^T| <= 1e-4 |A| |W|^T at 99 % of the elements or more."""
    _, _, ref, mag = X.gemm_class("cancelling", M, N, K)
    share = (ref.abs() <= 1e-4 * mag).double().mean().item()
    assert share >= 0.99, share


@pytest.mark.parametrize("M,N,K", X.GEMM_SHAPES)
def test_bitwise_scaling_operands_stay_normal(M, N, K):
    """For every exponent the GPU tests assert bit for bit, no split term of A or W and no kept product term is non-zero and below 2^-126: the
    scaling then moves every term by exactly that power of two, whatever the hardware does with subnormals."""
    A, W = X.gemm_bounded(M, N, K)
    lowest = float("inf")
    for sa, sw in [(s, 0) for s in X.BITWISE_SCALES] + [(40, -40), (0, 0)]:
        a, w = X.split3(A * 2.0 ** sa), X.split3(W * 2.0 ** sw)
        assert all(torch.isfinite(p).all() for p in a + w)
        nz = lambda t: t[t != 0].abs().min().item() if (t != 0).any() else float("inf")
        lowest = min([lowest] + [nz(p.double()) for p in a + w])
        colmin = lambda p: torch.where(p != 0, p.abs().double(), torch.full(p.shape, float("inf"), dtype=torch.float64)).amin(0)
        for pa, pb in X.KEPT:
            # the smallest non-zero |a_pa[m, k] w_pb[n, k]| over m, n at each k is the product of the two column minima
            lowest = min(lowest, (colmin(a[pa]) * colmin(w[pb])).min().item())
    assert lowest >= X.FP32_MIN_NORMAL, lowest


@pytest.mark.parametrize("M,N,K", X.GEMM_SHAPES)
@pytest.mark.parametrize("name", X.GEMM_CLASSES)
def test_emulated_x6_meets_the_gpu_gates(name, M, N, K):
    A, W, ref, mag = X.gemm_class(name, M, N, K)
    rms6, max6 = X.rel_error(X.emulate_x6(A, W), ref, mag)
    rms32, max32 = X.rel_error(X.emulate_f32(A, W), ref, mag)
    print(f"\n[{name} {M}x{N}x{K}] emulated x6 rms {rms6 / X.U:.3f}u max {max6 / X.U:.3f}u | f32 rms {rms32 / X.U:.3f}u max {max32 / X.U:.3f}u")
    assert not X.gemm_gate_failures(rms6, max6, rms32, max32, K)


def test_emulated_scaling_is_exact():
    M, N, K = X.GEMM_SHAPES[1]
    A, W = X.gemm_bounded(M, N, K)
    c = X.emulate_x6(A, W)
    for s in X.BITWISE_SCALES:
        assert torch.equal(X.emulate_x6(A * 2.0 ** s, W), c * 2.0 ** s)
    assert torch.equal(X.emulate_x6(A * 2.0 ** 40, W * 2.0 ** -40), c)


def test_split_of_non_finite_and_nearly_overflowing_values():
    """+Inf, NaN and any finite |x| >= 3.3962e38 (which rounds to bf16 Inf) leave a non-finite p0 or p1 -- NaN in the bf16 x 6 products, where the
    fp32 kernels give +-Inf / NaN.  The largest value whose bf16 rounding is finite splits cleanly."""
    p0, p1, p2 = X.split3(torch.tensor([float("inf"), float("nan"), 3.4e38, -3.3962e38, 3.3895e38]))
    bad = ~(torch.isfinite(p0) & torch.isfinite(p1))
    assert bad.tolist() == [True, True, True, True, False]
    assert torch.isnan(p1[0])                                       # Inf - Inf
    assert p0[2] == float("inf") and p1[2] == float("-inf") and torch.isnan(p2[2])  # a0 w + a1 w = Inf - Inf: NaN in the accumulator all the same
    assert (p0[4].double() + p1[4].double() + p2[4].double()) == float(torch.tensor(3.3895e38))


def test_attention_reference_matches_the_existing_one():
    from .test_attn_x6_gpu import reference

    qkv = X.uniform((2 * 50, 3 * 2 * 64), 1, 2.0)
    assert torch.equal(X.attn_reference(qkv, 2, 50, 2), reference(qkv, 2, 50, 2))
