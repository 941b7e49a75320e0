"""The bf16 x 6 GEMM and attention (gemm_x6.hip, attn_x6_kernel) at the numeric edges of their accuracy claim, next to the fp32-MFMA kernels on the
same operands: outlier channels, heavy tails, cancellation, operands scaled to 2^+-100, exact power-of-two scaling, graceful degradation below the
supported range, and where a NaN / Inf in one operand row may and may not show in the output.  The input classes come from tests/x6_inputs.py;
tests/test_x6_inputs_cpu.py checks them (and the stream-K plans named below) without a GPU.

None of the accuracy gates here is close(): it divides by the largest output, so with three channels scaled by 1e3 an error a thousand times too
large in an ordinary column would pass.  The GEMM yardstick is per element, |C - ref| / sum_k |a_k w_k|, the attention's per output column."""
import pytest
import torch

from endodav_amd import _lib

from . import x6_inputs as X
from .test_gemm_x6_gpu import planes_of
from .test_kernels_gpu import COUNTER_FLOATS, attn_spatial, gemm_ws, st
from .test_attn_x6_gpu import attn_x6

pytestmark = pytest.mark.gpu

U = X.U
# (600, 512, 768): 20 tiles of 48 k-steps; edv_split_plan (tests/test_x6_inputs_cpu.py) confirms that gemm_x6_split_policy cuts every one of them along
# k when the workspace is given, so "streamk" runs pieces and merges only, "plain" whole tiles only.  (257, 200, 64) never splits: plain only.
GEMM_CASES = [pytest.param(*X.GEMM_SHAPES[0], False, id="600x512x768-plain"), pytest.param(*X.GEMM_SHAPES[0], True, id="600x512x768-streamk"),
              pytest.param(*X.GEMM_SHAPES[1], False, id="257x200x64-plain")]


def bits(t):
    return t.contiguous().view(torch.int32)


def gemm_pair(lib, cuda, A, W, split, bias=None, act=0, R=None):
    """(edv_gemm_x6, edv_gemm) on the same operands -> two CPU tensors."""
    M, K = A.shape
    N = W.shape[0]
    d = lambda t: None if t is None else t.to(cuda)
    Ad, Wd, bd, Rd = d(A), d(W), d(bias), d(R)
    planes = planes_of(lib, Wd, N, K)
    ws, nbytes = gemm_ws(lib, cuda) if split else (None, 0)
    C6, C32 = torch.full((M, N), 7.0, device=cuda), torch.full((M, N), 7.0, device=cuda)
    _lib.check(lib.edv_gemm_x6(Ad.data_ptr(), planes.data_ptr(), C6.data_ptr(), M, N, K, _lib.ptr(bd), act, None, _lib.ptr(Rd), _lib.ptr(ws), nbytes, st()),
               "edv_gemm_x6")
    _lib.check(lib.edv_gemm(Ad.data_ptr(), Wd.data_ptr(), C32.data_ptr(), M, N, K, _lib.ptr(bd), act, None, _lib.ptr(Rd), _lib.ptr(ws), nbytes, st()), "edv_gemm")
    torch.cuda.synchronize()
    if split:
        assert int(ws[:COUNTER_FLOATS].view(torch.int32).abs().sum()) == 0
    return C6.cpu(), C32.cpu()


# ---- GEMM -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,split", GEMM_CASES)
@pytest.mark.parametrize("name", X.GEMM_CLASSES)
def test_gemm_edges_accuracy(lib, cuda, name, M, N, K, split):
    """Error relative to sum |a w| against fp64, bf16 x 6 next to the fp32-MFMA kernel: rms6 <= 1.05 rms32, max6 <= max(1.25 max32, 4 u) (the margins of
    test_gemm_x6_is_as_accurate_as_the_fp32_pipe), and both <= K u, the classical bound on a length-K fp32 dot product (the bf16 x 6 path rounds
    fewer than K times per element and drops 2^-26 + 2^-27).

    Measured on an MI355X (u = 2^-24), rms6/rms32 and max6/max32 per shape; the largest errors are those of 600x512x768 plain:
    class          600x512x768 plain   600x512x768 stream-K   257x200x64 plain    largest error (x6 | fp32, in u)
    outlier_A        0.639  0.604         0.650  0.454         0.687  0.848        22.3 | 36.9
    outlier_AW       0.630  0.719         0.641  0.682         0.705  0.790        28.2 | 39.2
    lognormal_A      0.752  0.627         0.773  0.567         0.792  0.826        16.8 | 26.9
    cancelling       0.830  0.954         0.659  0.993         0.837  0.754         2.7 |  2.9
    A_2p100          0.837  0.813         0.813  0.942         0.760  0.715         4.0 |  4.9
    A_2m100, W_2m100: the bits of A_2p100's error (the scaling is exact)
    No class needs more than the project's margins; on the outlier and heavy-tailed classes the flat 8 u gate of the uniform test would fail BOTH
    kernels, the error there is that of correct fp32 arithmetic."""
    A, W, ref, mag = X.gemm_class(name, M, N, K)
    C6, C32 = gemm_pair(lib, cuda, A, W, split)
    rms6, max6 = X.rel_error(C6, ref, mag)
    rms32, max32 = X.rel_error(C32, ref, mag)
    print(f"\n[gemm {name} {M}x{N}x{K} {'streamk' if split else 'plain'}] x6 rms {rms6 / U:.3f}u max {max6 / U:.3f}u | f32 rms {rms32 / U:.3f}u max {max32 / U:.3f}u"
          f" | rms6/rms32 {rms6 / rms32:.3f} max6/max32 {max6 / max32:.3f}")
    bad = X.gemm_gate_failures(rms6, max6, rms32, max32, K)
    assert not bad, f"{name} {M}x{N}x{K}: " + "; ".join(bad)


@pytest.mark.parametrize("M,N,K,split", GEMM_CASES)
def test_gemm_edges_power_of_two_scaling_is_exact(lib, cuda, M, N, K, split):
    """Both kernels: C(A 2^s, W) is ldexp(C(A, W), s) bit for bit at s = +-40, and C(A 2^40, W 2^-40) is C(A, W).  The operands are bounded away
    from zero, so no split term and no product leaves the normal range (tests/test_x6_inputs_cpu.py): whatever differs is the kernel's doing."""
    A, W = X.gemm_bounded(M, N, K)
    base = gemm_pair(lib, cuda, A, W, split)
    for s in X.BITWISE_SCALES:
        got = gemm_pair(lib, cuda, A * 2.0 ** s, W, split)
        for which, g, b in zip(("x6", "f32"), got, base):
            assert torch.equal(bits(g), bits(b * 2.0 ** s)), f"{which}: A 2^{s} is not an exact scaling"
    got = gemm_pair(lib, cuda, A * 2.0 ** 40, W * 2.0 ** -40, split)
    for which, g, b in zip(("x6", "f32"), got, base):
        assert torch.equal(bits(g), bits(b)), f"{which}: A 2^40, W 2^-40 changes the result"


def test_gemm_edges_degrades_gracefully_below_the_domain(lib, cuda):
    """A 2^-120 is 20 binades under the supported range: the second and third bf16 terms of A are subnormal or zero there, but the leading term alone
    keeps the result finite and within 2^-8 of sum |a w| (2^-9 per operand), subnormal bf16 flushed or not.

    Sweep on an MI355X, 600x512x768 stream-K, uniform |a| < 2 scaled by 2^s, |w| < 0.05 (rms error in u = 2^-24, and their ratio):
    s             0, -100 .. -108    -112      -116      -120      -124
    bf16 x 6           0.166         0.203     1.55      24.7      395      (largest: 1.24, 1.31, 7.5, 114, 1928)
    fp32 kernel        0.204         0.204     0.204     0.204     0.254
    ratio              0.81          1.00      7.6       121       1553
    The figures equal the CPU emulation with bf16 subnormals KEPT (0.269 / 1.56 / 24.7 / 395 u at -112 .. -124 in its own summation order; with them
    flushed it would be 6.1 / 246 / 1313 / 35724 u, and 1.0 u already at -108): gfx950's fp32 -> bf16 conversion and its bf16 MFMA both keep
    subnormals.  Directly: edv_gemm_x6_split returns 2^-133 as the bf16 subnormal 2^-133, and A = 2^-120 (1 + 2^-8), whose second term 2^-128 is
    a subnormal bf16, times W = 2^20 comes out exact.  The third term (2^-18 |a|) starts to lose bits when |a| < 2^-108 or so."""
    M, N, K = X.GEMM_SHAPES[0]
    A, W = X.gemm_bounded(M, N, K)
    A = A * 2.0 ** -120
    ref, mag = X.gemm_reference(A, W)
    for split in (False, True):
        C6, _ = gemm_pair(lib, cuda, A, W, split)
        assert torch.isfinite(C6).all()
        rms6, max6 = X.rel_error(C6, ref, mag)
        print(f"\n[gemm A 2^-120 {'streamk' if split else 'plain'}] x6 rms {rms6 / U:.1f}u max {max6 / U:.1f}u")
        assert max6 <= 2.0 ** -8, max6


def _contained(got, clean, rows=(), cols=()):
    """The listed output rows / columns are non-finite everywhere; everything else has the clean run's bits."""
    keep_r = torch.ones(got.shape[0], dtype=torch.bool)
    keep_c = torch.ones(got.shape[1], dtype=torch.bool)
    keep_r[list(rows)] = False
    keep_c[list(cols)] = False
    return (not torch.isfinite(got[~keep_r]).any() and not torch.isfinite(got[:, ~keep_c]).any(),
            torch.equal(bits(got[keep_r][:, keep_c]), bits(clean[keep_r][:, keep_c])) and bool(torch.isfinite(clean).all()))


@pytest.mark.parametrize("M,N,K,split", GEMM_CASES)
@pytest.mark.parametrize("operand", ["A", "W"])
def test_gemm_edges_non_finite_stays_in_its_row_or_column(lib, cuda, operand, M, N, K, split):
    """Both kernels, with bias and residual.  A NaN in an interior row of A and a +Inf in row M - 1 (the row the clamped loads of a ragged tile's
    padding rows duplicate) make those two output rows non-finite in every column and leave every other row bit for bit what it is with 1.0 in
    their place; the same for a NaN in row N - 1 and in an interior row of W and the output columns."""
    A, W = X.gemm_base(M, N, K)
    bias, R = X.uniform((N,), 3, 0.1), X.uniform((M, N), 5)
    if operand == "A":
        hit, spots = A, ((131, 17, float("nan")), (M - 1, K - 3, float("inf")))
    else:
        hit, spots = W, ((N - 1, 5, float("nan")), (70, K - 2, float("nan")))
    for r, k, _ in spots:
        hit[r, k] = 1.0
    clean = gemm_pair(lib, cuda, A, W, split, bias=bias, R=R)
    for r, k, val in spots:
        hit[r, k] = val
    got = gemm_pair(lib, cuda, A, W, split, bias=bias, R=R)
    where = [r for r, _, _ in spots]
    for which, g, c in zip(("x6", "f32"), got, clean):
        marked, untouched = _contained(g, c, rows=where) if operand == "A" else _contained(g, c, cols=where)
        assert marked, f"{which}: a finite value in an output {'row' if operand == 'A' else 'column'} that holds a NaN / Inf operand"
        assert untouched, f"{which}: a NaN / Inf in {operand} changed other output {'rows' if operand == 'A' else 'columns'}"


@pytest.mark.parametrize("M,N,K,split", GEMM_CASES)
def test_gemm_edges_non_finite_with_gelu_leaves_other_rows_alone(lib, cuda, M, N, K, split):
    """The same with the GELU epilogue, where the marked rows need not stay non-finite (gelu(-Inf) may be 0): only the untouched rows are held."""
    A, W = X.gemm_base(M, N, K)
    bias = X.uniform((N,), 3, 0.1)
    spots = ((131, 17, float("nan")), (M - 1, K - 3, float("inf")))
    for r, k, _ in spots:
        A[r, k] = 1.0
    clean = gemm_pair(lib, cuda, A, W, split, bias=bias, act=1)
    for r, k, val in spots:
        A[r, k] = val
    got = gemm_pair(lib, cuda, A, W, split, bias=bias, act=1)
    keep = torch.ones(M, dtype=torch.bool)
    keep[[r for r, _, _ in spots]] = False
    for which, g, c in zip(("x6", "f32"), got, clean):
        assert torch.isfinite(c).all() and torch.equal(bits(g[keep]), bits(c[keep])), f"{which}: a NaN / Inf in A changed other output rows"


# ---- attention --------------------------------------------------------------------------------------------------------------------------
# (2, 321, 2): ragged query block and key tile, all 8 tasks split by keys; (1, 257, 1): one query in the second block; (3, 300, 43): 258 tasks on 256
# resident workgroups, one whole round plus a split tail (planner: tests/test_x6_inputs_cpu.py)
ATTN_CASES = [pytest.param(*s, id="F{}xN{}xh{}".format(*s)) for s in X.ATTN_SHAPES]


def attn_pair(lib, cuda, qkv, Fr, N, heads):
    """(edv_attn_spatial_x6, edv_attn_spatial) on the same q | k | v -> two CPU tensors."""
    qd = qkv.to(cuda)
    o6, o32 = torch.full((Fr * N, heads * 64), 7.0, device=cuda), torch.full((Fr * N, heads * 64), 7.0, device=cuda)
    attn_x6(lib, cuda, qd, o6, Fr, N, heads)
    attn_spatial(lib, cuda, qd, o32, Fr, N, heads)
    torch.cuda.synchronize()
    return o6.cpu(), o32.cpu()


@pytest.mark.parametrize("Fr,N,heads", ATTN_CASES)
@pytest.mark.parametrize("name", X.ATTN_CLASSES)
def test_attn_edges_accuracy(lib, cuda, name, Fr, N, heads):
    """Error per output column, |o - ref| / max_rows |ref[:, c]|, against the fp64 attention: rms6 <= 1.10 rms32, max6 <= max(1.5 max32, 1e-6) (the margins
    of test_attn_x6_is_as_accurate_as_the_fp32_kernel), and both kernels within 4 x the error of the same attention evaluated by torch in fp32 on
    the CPU.  No flat gate: on the q / k outlier class torch's own fp32 attention is 9.4e-6 from fp64.

    Measured on an MI355X at (2, 321, 2), rms6/rms32, max6/max32, max6 / torch fp32, max32 / torch fp32:
    class         rms6/rms32  max6/max32  max6/torch  max32/torch   (largest error: x6 | fp32 kernel | torch fp32)
    qk_outlier      0.719       0.730       1.03        1.41          9.5e-6 | 1.3e-5 | 9.2e-6
    v_outlier       0.747       0.471       0.51        1.08          6.3e-7 | 1.3e-6 | 1.2e-6
    shifted         0.707       0.910       0.71        0.78          8.5e-5 | 9.4e-5 | 1.2e-4
    v_2p100/2m100   0.748       0.471       0.51        1.08          (v_outlier's plain operands, exactly scaled)
    q_2m100         0.505       0.460       0.27        0.58          6.0e-7 | 1.3e-6 | 2.3e-6
    Over all three shapes the worst ratios are rms 0.95, max 1.12 (v_outlier at (1, 257, 1)), 1.10 x torch for bf16 x 6 and 1.53 x torch for the fp32
    kernel (q_2m100 at (3, 300, 43))."""
    qkv, ref, (_, max_torch) = X.attn_class(name, Fr, N, heads)
    o6, o32 = attn_pair(lib, cuda, qkv, Fr, N, heads)
    assert torch.isfinite(o6).all() and torch.isfinite(o32).all()
    rms6, max6 = X.column_error(o6, ref)
    rms32, max32 = X.column_error(o32, ref)
    print(f"\n[attn {name} ({Fr}, {N}, {heads})] x6 rms {rms6:.3e} max {max6:.3e} | f32 rms {rms32:.3e} max {max32:.3e} | torch fp32 max {max_torch:.3e}"
          f" | rms6/rms32 {rms6 / rms32:.3f} max6/max32 {max6 / max32:.3f} max6/torch {max6 / max_torch:.3f} max32/torch {max32 / max_torch:.3f}")
    bad = X.attn_gate_failures(rms6, max6, rms32, max32, max_torch)
    assert not bad, f"{name} ({Fr}, {N}, {heads}): " + "; ".join(bad)


@pytest.mark.parametrize("Fr,N,heads", ATTN_CASES)
def test_attn_edges_power_of_two_scaling_is_exact(lib, cuda, Fr, N, heads):
    """Both kernels: o(q, k, v 2^s) is ldexp(o(q, k, v), s) bit for bit at s = +-40, and o(q 2^40, k 2^-40, v) is o(q, k, v)."""
    qkv = X.bounded((Fr * N, 3 * heads * 64), 31)
    base = attn_pair(lib, cuda, qkv, Fr, N, heads)
    for s in X.BITWISE_SCALES:
        scaled = qkv.clone()
        X.attn_views(scaled, heads)[2].mul_(2.0 ** s)
        for which, g, b in zip(("x6", "f32"), attn_pair(lib, cuda, scaled, Fr, N, heads), base):
            assert torch.equal(bits(g), bits(b * 2.0 ** s)), f"{which}: v 2^{s} is not an exact scaling"
    scaled = qkv.clone()
    q, k, _ = X.attn_views(scaled, heads)
    q.mul_(2.0 ** 40)
    k.mul_(2.0 ** -40)
    for which, g, b in zip(("x6", "f32"), attn_pair(lib, cuda, scaled, Fr, N, heads), base):
        assert torch.equal(bits(g), bits(b)), f"{which}: q 2^40, k 2^-40 changes the result"


@pytest.mark.parametrize("Fr,N,heads", ATTN_CASES)
@pytest.mark.parametrize("part,value,last", [("q", float("nan"), False), ("k", float("nan"), True), ("k", float("inf"), False), ("v", float("inf"), True),
                                             ("v", float("nan"), False)], ids=["q-nan", "k-nan-last", "k-inf", "v-inf-last", "v-nan"])
def test_attn_edges_non_finite_stays_in_its_block(lib, cuda, part, value, last, Fr, N, heads):
    """Both kernels.  A NaN in one q row of head h makes that output row of head h non-finite and nothing else; a NaN or +Inf in one k or v row of
    (frame f, head h) -- the sequence's last token, which the clamped loads of a ragged key tile duplicate, or an interior one -- may make that
    (f, h) block non-finite, and every other block keeps the bits of the run with 1.0 in its place.  (Inside the q row's own wave the other rows
    keep their bits because no score here exceeds the running maximum by the lazy-rescale threshold: that decision is taken per wave.)"""
    qkv = X.uniform((Fr * N, 3 * heads * 64), 9, 2.0)
    f, h, tok, d = Fr - 1, heads // 2, (N - 1 if last else 70), 7
    cell = X.attn_views(qkv, heads)["qkv".index(part)][f * N + tok, h]
    cell[d] = 1.0
    clean = attn_pair(lib, cuda, qkv, Fr, N, heads)
    cell[d] = value
    got = attn_pair(lib, cuda, qkv, Fr, N, heads)
    touched = torch.zeros(Fr * N, heads, 64, dtype=torch.bool)
    if part == "q":
        touched[f * N + tok, h] = True
    else:
        touched[f * N:(f + 1) * N, h] = True
    touched = touched.reshape(Fr * N, heads * 64)
    for which, g, c in zip(("x6", "f32"), got, clean):
        assert torch.isfinite(c).all()
        assert torch.equal(bits(g)[~touched], bits(c)[~touched]), f"{which}: a non-finite {part} entry changed output outside its {'row' if part == 'q' else '(frame, head) block'}"
        if part == "q":
            assert not torch.isfinite(g[touched]).any(), f"{which}: a finite output in the row of a NaN query"
        else:
            assert not torch.isfinite(g[touched]).all(), f"{which}: a non-finite {part} entry left no trace in its block"
