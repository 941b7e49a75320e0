"""What tests/test_grad_edges_gpu.py takes for granted about the operands of tests/grad_inputs.py, checked without a GPU: the integer operands are
exact in any summation order, the cancelling operands cancel, the scaled operands stay normal, torch's own fp32 passes every accuracy gate the
kernels are held to (a gate the reference arithmetic cannot pass is a wrong gate), the integer operands see each mistake a reduction can make, and
the shapes reach the splits, tails and workgroup counts the tables claim."""
import pytest
import torch

from tests import grad_inputs as V

U = V.U
sid = lambda shape: "x".join(str(int(v)) for v in shape)
LORA_IDS = lambda cases: [f"{c}-{sid(s)}" for c, s in cases]


def absolute(o):
    return V.SimpleNamespace(**{k: (v.abs() if torch.is_tensor(v) else v) for k, v in vars(o).items()})


# ---- exact_int ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", V.LORA_SHAPES, ids=sid)
def test_lora_exact_int_is_exact_in_any_order(shape):
    o = V.lora_operands("exact_int", shape)
    M = shape[0]
    for t in (o.x, o.G, o.A, o.B, o.U, o.V, o.gamma):
        assert t is None or torch.equal(t, t.round())
    assert o.s == 2.0
    assert (o.x[V.split_edge_rows(M)] != 0).all() and (o.G[V.split_edge_rows(M)] != 0).all()
    for F, n in ((o.A, shape[1]), (o.B.T, shape[2])):
        assert (F[:, V.edge_columns(n)].abs() == 1).all() and F.abs().sum().item() == F.shape[0] * len(V.edge_columns(n))
    # the sum of the absolute values of all contributing terms, nested through t and u, in int64: the formula on the absolute operands
    terms = V.lora_formula(absolute(o), torch.int64)
    worst = max(int(v.max()) for v in terms.values() if v is not None)
    assert worst < V.EXACT_LIMIT, f"{worst} >= 2^24"
    assert worst == V.lora_exact_terms(o)
    want = V.lora_formula(o, torch.int64)
    c = V.lora_class("exact_int", shape)
    for n in V.lora_outputs(o):
        assert want[n].abs().max() > 0, n
        assert torch.equal(c.ref[n], want[n].double()), f"{n}: autograd in fp64 and the written-out formula differ"
        assert torch.equal(c.t32[n].double(), want[n].double()), f"{n}: torch fp32 does not reproduce the int64 answer"
        assert torch.equal(V.lora_formula(o, torch.float64)[n], want[n].double())


@pytest.mark.parametrize("shape", V.COLSUM_SHAPES, ids=sid)
def test_colsum_exact_int_is_exact_in_any_order(shape):
    c = V.colsum_class("exact_int", shape)
    assert c.mag.max().item() < V.EXACT_LIMIT
    assert torch.equal(c.ref, c.ref.round()) and c.ref.abs().max() > 0
    rs = None if c.rs is None else c.rs.long()
    want = V._colsum_apply(c.P.long(), rs, None if c.base is None else c.base.long(), shape[1] == 1, torch.int64)
    t32 = V._colsum_apply(c.P, c.rs, c.base, shape[1] == 1, torch.float32)
    assert torch.equal(want.double(), c.ref) and torch.equal(t32.double(), c.ref)


@pytest.mark.parametrize("shape", V.COLDOT_SHAPES, ids=sid)
def test_coldot_and_batch_exact_int_are_exact_in_any_order(shape):
    for use_q, use_s in V.COLDOT_VARIANTS:
        c = V.coldot_class("exact_int", shape, use_q, use_s)
        assert c.mag.max().item() < V.EXACT_LIMIT and torch.equal(c.ref, c.ref.round())
        lg = lambda t: None if t is None else t.long()
        assert torch.equal(V._coldot_apply(lg(c.P), lg(c.Q), lg(c.scale), torch.int64).double(), c.ref)
        assert torch.equal(V._coldot_apply(c.P, c.Q, c.scale, torch.float32).double(), c.ref)
    for k in range(len(V.BATCH_JOBS)):
        b = V.batch_class("exact_int", k)
        assert b.mag.max().item() < V.EXACT_LIMIT and torch.equal(b.ref, b.ref.round()) and torch.equal(b.t32.double(), b.ref)


# ---- cancelling and scaled ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in V.LORA_SHAPES if V.lora_has_class("cancelling", s)], ids=sid)
def test_lora_cancelling_cancels(shape):
    """Median |ref| / mag_outer <= 1e-5 for dA and dB."""
    c = V.lora_class("cancelling", shape)
    for n in ("dA", "dB"):
        med = (c.ref[n].abs() / c.mags[n][0]).median().item()
        print(f"\n[cancelling {sid(shape)} {n}] delta 2^{int(torch.log2(torch.tensor(V.delta_for(shape[0]))))} median |ref| / mag_outer {med:.2e}")
        assert med <= 1e-5, f"{n}: median {med:.2e}"


def test_column_sums_cancelling_cancel():
    cs = [V.colsum_class("cancelling", s) for s in V.COLSUM_SHAPES if V.colsum_has_class("cancelling", s)]
    cs += [V.coldot_class("cancelling", s, q, False) for s in V.COLDOT_SHAPES if V.colsum_has_class("cancelling", s) for q in (False, True)]
    cs += [V.batch_class("cancelling", k) for k in range(len(V.BATCH_JOBS))]
    assert len(cs) == 3 + 4 + len(V.BATCH_JOBS)
    for c in cs:
        assert (c.ref.abs() / c.mag).median().item() <= 1e-4  # one sum per column: delta / sqrt(M / 2) at its worst (M = 322)


@pytest.mark.parametrize("shape", V.LORA_SHAPES, ids=sid)
def test_scaled_operands_stay_normal(shape):
    """At 2^+-40 every operand and every output is a normal number: scaling by a power of two then commutes with every rounding.  (A partial sum
    that is not exactly zero is a multiple of its smallest term's ulp, at least 2^-8 2^-24 2^-40: it cannot fall below 2^-126 either.)"""
    c = V.lora_class("scaled", shape)
    normal = lambda t, p: ((t.double().abs() * 2.0 ** p > V.FP32_MIN_NORMAL * 2.0 ** 24) & (t.double().abs() * 2.0 ** p < 2.0 ** 100))[t != 0].all()
    for p in V.BITWISE_SCALES:
        assert normal(c.ops.x, p) and normal(c.ops.G, p)
        for n in V.lora_outputs(c.ops):
            assert normal(c.ref[n], p), n
    for t in (c.ops.x, c.ops.G, c.ops.A, c.ops.B):
        assert t.abs().min() >= 2.0 ** -4
    for s2 in V.COLSUM_SHAPES:
        cc = V.colsum_class("scaled", s2)
        assert all(normal(t, p) for p in V.BITWISE_SCALES for t in (cc.P, cc.ref))


# ---- torch fp32 under the kernels' gates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,shape", V.lora_cases(V.ACCURACY_CLASSES), ids=LORA_IDS(V.lora_cases(V.ACCURACY_CLASSES)))
def test_torch_fp32_passes_the_lora_gate(cls, shape):
    c = V.lora_class(cls, shape)
    for n in V.lora_outputs(c.ops):
        (mo, mi), (do, di) = c.mags[n], c.depths[n]
        assert (mi >= mo * (1 - 1e-12)).all() and (mo > 0).all()
        worst = V.bound_ratio(c.t32[n], c.ref[n], mo, do, mi, di)
        assert worst <= 1, f"{n}: torch fp32 is {worst:.2f} x the bound u ({do} mag_outer + {di} mag_inner)"
        assert not V.gate_failures(*c.torch_err[n], c.torch_err[n], U)


def test_torch_fp32_passes_the_column_sum_gates():
    for cls, shape in V.colsum_cases(V.ACCURACY_CLASSES):
        c = V.colsum_class(cls, shape)
        assert c.torch_err[1] <= c.depth * U, (cls, shape, c.torch_err, c.depth)
    for cls, shape in V.coldot_cases(V.ACCURACY_CLASSES):
        for use_q, use_s in V.COLDOT_VARIANTS:
            c = V.coldot_class(cls, shape, use_q, use_s)
            assert c.torch_err[1] <= c.depth * U, (cls, shape, use_q, use_s, c.torch_err, c.depth)
    for cls in V.ACCURACY_CLASSES:
        for k in range(len(V.BATCH_JOBS)):
            c = V.batch_class(cls, k)
            assert c.torch_err[1] <= c.depth * U, (cls, k, c.torch_err, c.depth)


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", V.LORA_SHAPES, ids=sid)
def test_integer_operands_see_each_mistake(shape):
    o = V.lora_operands("exact_int", shape)
    right = V.lora_formula(o, torch.float64)
    applied = 0
    for m in V.MISTAKES:
        if not V.mistake_applies(m, shape, o):
            continue
        wrong = V.lora_formula(o, torch.float64, m)
        assert any(not torch.equal(wrong[n], right[n]) for n in V.lora_outputs(o)), f"{m} changes nothing at {shape}"
        applied += 1
    assert applied >= 1


def test_every_mistake_applies_somewhere():
    for m in V.MISTAKES:
        assert any(V.mistake_applies(m, s, V.lora_operands("exact_int", s)) for s in V.LORA_SHAPES), m
    assert {V.lora_form(s, "exact_int") for s in V.LORA_SHAPES} == set(V.LORA_FORMS)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
def test_split_geometry_of_the_shapes():
    want = {1: (1, 1, 1), 3: (1, 3, 1), 63: (1, 63, 1), 64: (1, 64, 1), 65: (2, 33, 1), 130: (3, 44, 1), 1370: (22, 63, 6), 1000: (16, 63, 8),
            10960: (172, 64, 124)}
    for M, g in want.items():
        assert V.split_geometry(M) == g, M
    assert {s[0] for s in V.LORA_SHAPES} | {s[0] for s in V.COLDOT_SHAPES} == set(want)
    assert {s[3] for s in V.LORA_SHAPES} == {1, 2, 4, 8}
    M, nin, nout, r = zip(*V.LORA_SHAPES)
    assert any(m % 2 and rr == 1 for m, rr in zip(M, r))                              # the layout whose regions need padding
    assert any(n % V.TALL_COLS for n in nin) and any(n % V.TALL_COLS for n in nout)   # a cut 64-column block in both tall_tn calls
    assert any(n > V.SKINNY_STEP and n % V.SKINNY_STEP for n in nin + nout) and 588 % 256 == 76
    assert any(n * rr % V.REDUCE_COLS for n, rr in zip(nout, r))
    assert min(V.split_geometry(m)[1] for m in M) < V.REDUCE_SLICES
    assert all(s in V.LORA_SHAPES for s in V.ADJOINT_SHAPES) and any(s[1] * s[2] % 256 for s in V.ADJOINT_SHAPES)  # fold_lora's last block is cut


def test_colsum_geometry_of_the_shapes():
    g = {s: V.colsum_geometry(*s) for s in V.COLSUM_SHAPES}
    assert g[(3, 4)][2] < 256 and g[(2049, 4)][:3] == (2, 5, 2049) and g[(300000, 8)][0] == 293
    assert V.colsum_wanted(1100000, 4) == 538 and g[(1100000, 4)][:2] == (512, 9) and 1100000 % (512 * 256) != 0
    assert g[(4100, 1)] == (1, 5, 1025, 1) and g[(1, 1024)] == (1, 1, 256, 256)
    assert V.COLSUM_SHAPES[(777, 64)] == (True, True) and not V.COLSUM_SHAPES[(4100, 1)][0]
    parts = [V.batch_plan(m, n)[0] for n, m in V.BATCH_JOBS]
    assert min(parts) == 1 and max(parts) > 8 and all(m % 2 == 0 for _, m in V.BATCH_JOBS)
