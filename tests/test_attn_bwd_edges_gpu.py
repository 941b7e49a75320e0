"""Spatial attention backward (attn_spatial_bwd.hip) at the numeric edges the forward was held to in tests/test_x6_edges_gpu.py: peaked rows
from q / k outliers, a score offset of about 500, a v outlier channel, all-zero scores, an outlier channel in dO, exact power-of-two scaling and
NaN containment -- on shapes whose tasks are all split into workspace pieces, and on one with a whole round plus a split tail.  The backward
takes P = exp2(S log2e - L) from the forward's stored fp32 log-sum-exp L with no running maximum, and dS = P (dP - delta) cancels on peaked rows.

Yardstick: X.column_error on the dq, dk and dv thirds separately, next to torch's own fp32 autograd of the same attention on the CPU; the stored
lse by its absolute error next to torch's fp32 logsumexp of the same scores.  Inputs and references: tests/edge_inputs.py."""
import pytest
import torch

from endodav_amd import _lib

from . import edge_inputs as E
from .edge_inputs import bits
from .test_kernels_gpu import st

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = [pytest.param(*s, id="F{}xN{}xh{}".format(*s)) for s in E.ATTN_BWD_SHAPES]


def attn_fwd_bwd(lib, cuda, qkv, dO, Fr, N, heads):
    """edv_attn_spatial (planner's workspace, stores lse) then edv_attn_spatial_bwd; every workspace and output poisoned with NaN -> (dqkv, lse) on the CPU."""
    D = heads * 64
    qd, gd = qkv.to(cuda), dO.to(cuda)
    o = torch.full((Fr * N, D), NAN, device=cuda)
    lse = torch.full((Fr * heads * N,), NAN, device=cuda)
    nb = lib.edv_attn_spatial_workspace(Fr, N, heads)
    ws = torch.full((max(nb // 4, 4),), NAN, device=cuda)
    _lib.check(lib.edv_attn_spatial(qd.data_ptr(), o.data_ptr(), Fr, N, heads, ws.data_ptr(), nb, lse.data_ptr(), st()), "edv_attn_spatial")
    delta = torch.full((Fr * heads * N,), NAN, device=cuda)
    dqkv = torch.full((Fr * N, 3 * D), NAN, device=cuda)
    nbb = lib.edv_attn_spatial_bwd_workspace(Fr, N, heads)
    assert nbb > 0  # every shape here has split tasks
    wsb = torch.full((nbb // 4,), NAN, device=cuda)
    _lib.check(lib.edv_attn_spatial_bwd(qd.data_ptr(), o.data_ptr(), gd.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), Fr, N, heads,
                                        wsb.data_ptr(), nbb, st()), "edv_attn_spatial_bwd")
    torch.cuda.synchronize()
    return dqkv.cpu(), lse.cpu().reshape(Fr, heads, N)


@pytest.mark.parametrize("Fr,N,heads", CASES)
def test_attn_bwd_edges_device_plans_are_the_ones_the_cpu_test_checks(lib, cuda, Fr, N, heads):
    """The workspace the device asks for is the one of the 512-slot plan (two resident workgroups of either backward instantiation per CU) that
    tests/test_edge_inputs_cpu.py checks: pieces x 128 rows x 128 columns (dK | dV) floats."""
    from .test_edge_inputs_cpu import attn_bwd_plan

    p = attn_bwd_plan(lib, Fr, N, heads)
    assert lib.edv_attn_spatial_bwd_workspace(Fr, N, heads) == p["ws"] * E.ATTN_BWD_ROWS * 128 * 4


@pytest.mark.parametrize("Fr,N,heads", CASES)
@pytest.mark.parametrize("name", E.ATTN_BWD_CLASSES)
def test_attn_bwd_edges_accuracy(lib, cuda, name, Fr, N, heads):
    """dq, dk, dv per column against fp64 autograd, and the forward's lse, each next to torch fp32 on the same inputs.

    Measured on an MI355X, worst over the three shapes: kernel / torch rms and max, largest per-column error kernel | torch:
    class         dq                             dk                             dv                             lse (absolute, base 2)
    qk_outlier    3.02 12.1  7.0e-5 | 1.6e-5     1.94 2.94  2.2e-5 | 1.3e-5     2.86 5.26  2.9e-5 | 8.7e-6     1.02 1.18  3.7e-5 | 3.2e-5
    v_outlier     2.69 2.57  4.2e-6 | 1.9e-6     2.62 2.47  3.7e-6 | 1.5e-6     2.61 2.19  3.4e-6 | 1.9e-6     1.08 0.96  1.5e-6 | 1.6e-6
    shifted       88.1 84.9  1.4e-2 | 1.7e-4     1.38 2.00  3.7e-4 | 1.9e-4     1.25 1.70  3.7e-4 | 2.3e-4     0.82 1.38  3.5e-4 | 2.5e-4
    q_2m100       2.28 2.21  1.6e-6 | 7.3e-7     2.28 2.31  1.7e-6 | 7.5e-7     1.97 1.42  4.8e-6 | 3.4e-6     3.70 3.70  7.5e-7 | 2.2e-7
    dO_outlier    2.69 2.58  4.4e-6 | 1.8e-6     2.64 2.56  3.7e-6 | 1.6e-6     2.61 2.19  3.4e-6 | 1.9e-6     1.08 0.96  1.5e-6 | 1.6e-6
    qk_outlier (dq at two shapes, dv at one) and shifted (dq) exceed 4 x torch.  That is not a defect but what the algorithm costs (the derivation is the
    docstring of E.attn_bwd_rounding_sigma): P is recomputed from the fp32 lse in an accumulator that starts at -L, so every probability carries
    sqrt(32) ulp(L) ln2 / sqrt(12) of relative error the forward's did not have, delta = dO . O comes from the forward's, and a row of dS sums to zero
    only to that accuracy -- a component common to all keys (62 x the rest in `shifted`) then enters dq.  Those two classes are gated by that model
    instead: rms <= max(the ordinary gate, 2 x the model's), every element <= the ordinary gate + 8 sigma.  The model's rms / the kernel's, dq:
    qk_outlier 1.56e-6 / 1.30e-6, 2.06e-6 / 1.89e-6, 1.41e-6 / 8.2e-7; shifted 1.22e-3 / 1.04e-3, 1.63e-3 / 1.30e-3, 1.16e-3 / 4.9e-4 (the three
    shapes in order: the kernel's is 0.4 .. 0.9 of the model's, which gives the forward's scores the backward's variance, an upper estimate), and
    tests/test_edge_inputs_cpu.py reproduces the model by simulation."""
    qkv, dO, ref, lse_ref, torch_err, lse_torch = E.attn_bwd_class(name, Fr, N, heads)
    dqkv, lse = attn_fwd_bwd(lib, cuda, qkv, dO, Fr, N, heads)
    assert torch.isfinite(dqkv).all() and torch.isfinite(lse).all()
    errs = E.thirds_error(dqkv, ref)
    lse_err = E.rms_max((lse.double() - lse_ref).abs())
    what = f"attn_spatial_bwd {name} ({Fr}, {N}, {heads})"
    for n in E.THIRDS:
        print(f"\n[{what} {n}] {E.ratios(*errs[n], torch_err[n])}")
    print(f"\n[{what} lse] {E.ratios(*lse_err, lse_torch)}")
    if name in E.ATTN_BWD_DERIVED:
        sigma = E.attn_bwd_rounding_sigma(qkv, dO, Fr, N, heads)
        model = E.thirds_error(ref + sigma, ref)
        print(f"\n[{what} model] " + ", ".join(f"{n} rms {model[n][0]:.2e} largest sigma {model[n][1]:.2e}" for n in E.THIRDS))
        bad = E.attn_bwd_derived_failures(dqkv, ref, sigma, torch_err, E.FLOOR["attn_bwd"])
    else:
        bad = [f"{n}: {b}" for n in E.THIRDS for b in E.gate_failures(*errs[n], torch_err[n], E.FLOOR["attn_bwd"])]
    if not lse_err[1] <= max(E.MARGIN * lse_torch[1], E.FLOOR["lse"]):
        bad.append(f"lse: max {lse_err[1]:.3e} > max(4 x torch fp32 {lse_torch[1]:.3e}, 2e-5)")
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.parametrize("Fr,N,heads", CASES)
def test_attn_bwd_edges_power_of_two_scaling_is_exact(lib, cuda, Fr, N, heads):
    """dqkv(dO 2^s) is ldexp(dqkv(dO), s) bit for bit at s = +-40: delta, dP, dS, the three products and the sum of the workspace pieces are all
    linear in dO (operands bounded away from zero, scores within +-2: tests/test_edge_inputs_cpu.py)."""
    qkv, dO = E.attn_bounded(Fr, N, heads)
    base, _ = attn_fwd_bwd(lib, cuda, qkv, dO, Fr, N, heads)
    assert torch.isfinite(base).all()
    for s in E.BITWISE_SCALES:
        got, _ = attn_fwd_bwd(lib, cuda, qkv, dO * 2.0 ** s, Fr, N, heads)
        assert torch.equal(bits(got), bits(base * 2.0 ** s)), f"dO 2^{s} is not an exact scaling"


@pytest.mark.parametrize("Fr,N,heads", CASES)
@pytest.mark.parametrize("where", ["dO", "k"])
def test_attn_bwd_edges_non_finite_stays_in_its_block(lib, cuda, where, Fr, N, heads):
    """A NaN in one dO row, or in one k row (then the forward's out and lse of that block carry it too), of (frame f, head h) may make the (f, h)
    block of dq, dk and dv non-finite and leaves every other (frame, head) block -- pieces that met in the workspace included -- bit for bit what
    it is with 1.0 in its place."""
    qkv, dO = E.uniform((Fr * N, 3 * heads * 64), 9, 2.0), E.attn_dO(Fr, N, heads).clone()
    f, h, tok, d = Fr - 1, heads // 2, 70, 7
    cell = dO.view(Fr * N, heads, 64)[f * N + tok, h] if where == "dO" else E.attn_views(qkv, heads)[1][f * N + tok, h]
    cell[d] = 1.0
    clean, _ = attn_fwd_bwd(lib, cuda, qkv, dO, Fr, N, heads)
    cell[d] = NAN
    got, _ = attn_fwd_bwd(lib, cuda, qkv, dO, Fr, N, heads)
    touched = torch.zeros(Fr * N, 3, heads, 64, dtype=torch.bool)
    touched[f * N:(f + 1) * N, :, h] = True
    touched = touched.reshape(Fr * N, 3 * heads * 64)
    assert torch.isfinite(clean).all()
    assert torch.equal(bits(got)[~touched], bits(clean)[~touched]), f"a NaN in {where} changed gradients outside its (frame, head) block"
    assert not torch.isfinite(got[touched]).all(), f"a NaN in {where} left no trace in its block"
