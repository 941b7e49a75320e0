"""What the *_edges_gpu.py tests rely on, checked without a GPU: every input class of tests/edge_inputs.py has a finite fp64 reference, non-zero
yardstick denominators and a finite, positive torch-fp32 error; constant rows and slabs come back bit for bit from the project's two-pass
arithmetic emulated in torch fp32; the operands of the bit-for-bit scaling tests keep every intermediate a normal number at the asserted exponents;
the shapes dispatch the kernels and get the stream-K plans their comments name."""
import ctypes as C

import pytest
import torch

from . import edge_inputs as E
from . import x6_inputs as X

ATTN = 3  # edv_split_plan kind
LO, HI = X.FP32_MIN_NORMAL, 2.0 ** 127
pos_finite = lambda e: all(0 < v < float("inf") for v in e)


@pytest.mark.parametrize("rows,dim", E.LN_SHAPES)
@pytest.mark.parametrize("name", E.LN_CLASSES)
def test_layernorm_classes(name, rows, dim):
    for form in E.LN_FORMS:
        ref, err = E.ln_forward(name, rows, dim, form)   # row_error asserts the denominators
        assert torch.isfinite(ref).all()
        assert pos_finite(err) or (name == "const" and all(0 <= v < float("inf") for v in err)), (form, err)
    for dy_kind in ("uniform", "outlier"):
        for acc in (False, True):
            _, _, ref, err = E.ln_backward(name, rows, dim, dy_kind, acc)
            assert torch.isfinite(ref).all() and pos_finite(err), (dy_kind, acc, err)
    x = E.ln_operands(name, rows, dim)[0]
    if name in ("offset_1e3", "offset_1e4"):
        mean, sigma = (1e3, 0.03 / 3 ** 0.5) if name == "offset_1e3" else (1e4, 0.01 / 3 ** 0.5)
        assert (x.double().mean(1) - mean).abs().max() < 0.01 and (x.double().std(1) / sigma - 1).abs().max() < 0.3
    if name == "scaled_2m40":
        assert x.double().var(1).max() < 1e-6 * 2.0 ** -40


@pytest.mark.parametrize("dim", [32, 384, 1024])
def test_constant_rows_come_back_exactly_from_two_pass_arithmetic(dim):
    """sum of dim copies of a 12-bit value is exact in fp32 in any order (23 bits at most), the division by dim returns the value, the centred
    second moment is 0: x-hat is exactly 0 and y = 0 * w + b = b bit for bit."""
    x, w, b = E.ln_operands("const", 129, dim)[:3]
    assert len(set(x[:, 0].tolist())) == 129 and x[0, 0] == 1024.5 and x[1, 0] == -3 and x[2, 0] == 0
    assert ((x[:, 0] * 2 ** 12) % 1 == 0).all() and (x[:, 0].abs() < 2 ** 11).all()
    xh = E.ln_two_pass(x, 1e-6)
    assert torch.equal(xh, torch.zeros_like(xh))
    assert torch.equal(E.bits(xh * w + b), E.bits(b.expand_as(xh)))


@pytest.mark.parametrize("Fr,P,C", E.GN_SHAPES)
def test_constant_slabs_come_back_exactly_from_two_pass_arithmetic(Fr, P, C):
    """The same for a slab of P C / 32 values, and for the two-stage path: chunk means (sum x the reciprocal of the chunk's rows, a power of two)
    are the value itself, the weighted merge n_i mean_i sums exactly and divides back to the value."""
    x, w, b = E.gn_operands("const", Fr, P, C)
    cg = C // E.GROUPS
    s = E.slabs(x).permute(0, 2, 1, 3).reshape(Fr * E.GROUPS, P * cg)
    xh = E.ln_two_pass(s, E.GN_EPS)
    assert torch.equal(xh, torch.zeros_like(xh)) and (s != 0).all()
    last = P % 32 or 32
    assert last & (last - 1) == 0, "the last chunk must hold a power-of-two number of rows"
    n = torch.tensor([32.0] * (P // 32) + ([float(last)] if P % 32 else []))
    rows = [E.slabs(x)[:, p0:p0 + 32] for p0 in range(0, P, 32)]                                   # [F, n_i, 32, cg] per chunk
    means = torch.stack([r.sum(1) * (1.0 / torch.tensor(float(r.shape[1]))) for r in rows], 1)       # [F, chunks, 32, cg]
    merged = (means * n[None, :, None, None]).sum((1, 3)) / (torch.tensor(float(P)) * torch.tensor(float(cg)))
    assert torch.equal(E.bits(merged), E.bits(E.gn_const_values(Fr)))


@pytest.mark.parametrize("Fr,P,C", E.GN_SHAPES)
@pytest.mark.parametrize("name", E.GN_CLASSES)
def test_groupnorm_classes(name, Fr, P, C):
    ref, m, r, errs = E.gn_forward(name, Fr, P, C)
    assert torch.isfinite(ref).all() and torch.isfinite(m).all() and torch.isfinite(r).all()
    for e in errs:
        assert pos_finite(e) or (name == "const" and all(0 <= v < float("inf") for v in e)), errs
    for acc in (False, True):
        _, _, gref, gerr = E.gn_backward(name, Fr, P, C, acc)
        assert torch.isfinite(gref).all() and pos_finite(gerr)


@pytest.mark.parametrize("Fr,N,heads", E.ATTN_BWD_SHAPES[:2])
@pytest.mark.parametrize("name", E.ATTN_BWD_CLASSES)
def test_attention_backward_classes(name, Fr, N, heads):
    """(The 58-head shape is the same generator; its references are computed by the GPU test only.)"""
    qkv, dO, ref, lse, errs, lse_err = E.attn_bwd_class(name, Fr, N, heads)
    assert torch.isfinite(ref).all() and torch.isfinite(lse).all() and (ref.abs().amax(0) > 0).all()
    assert all(pos_finite(e) for e in errs.values()) and pos_finite(lse_err), (errs, lse_err)
    if name == "shifted":
        assert lse.abs().min() > 300  # |L| in the hundreds (base 2)


@pytest.mark.parametrize("name", E.ATTN_BWD_DERIVED)
def test_attention_backward_rounding_model_matches_a_simulation(name):
    """The first-order variances of E.attn_bwd_rounding_sigma against the flash-style backward run in fp64 with the modelled roundings injected:
    independent uniform errors of variance 32 ulp(L)^2 / 12 on the forward's and on the backward's base-2 scores, ulp^2 / 12 on the stored L,
    delta taken from the forward's output.  Per third, the simulated rms is within a factor 1.5 of the model's (first order; it ignores that the
    forward's error in L and in delta are correlated, and on peaked rows a few entries carry the sum) -- inside the factor 2 the GPU gate grants the
    model -- and no element exceeds 6 sigma."""
    import math

    Fr, N, heads = 1, 257, 1
    qkv, dO, ref, _, _, _ = E.attn_bwd_class(name, Fr, N, heads)
    sigma = E.attn_bwd_rounding_sigma(qkv, dO, Fr, N, heads)
    assert torch.isfinite(sigma).all() and (sigma > 0).all()
    q, k, v = (t.double()[:, 0] for t in E.attn_views(qkv, heads))
    g, ln2 = dO.double(), math.log(2.0)
    X2 = (q * 0.125) @ k.T / ln2
    L = torch.logsumexp(X2 * ln2, -1, keepdim=True) / ln2
    ulp = torch.exp2(torch.floor(torch.log2(L.abs().clamp(min=1.0))) - 23)
    gen = torch.Generator().manual_seed(5)
    noise = lambda shape, terms: (torch.rand(shape, generator=gen, dtype=torch.float64) - 0.5) * ulp * math.sqrt(terms)  # variance terms ulp^2 / 12
    Xf = X2 + noise((N, N), E.ATTN_BWD_STEPS)
    Lf = torch.logsumexp(Xf * ln2, -1, keepdim=True) / ln2
    delta = (g * (torch.exp2(Xf - Lf) @ v)).sum(-1, keepdim=True)
    P = torch.exp2(X2 + noise((N, N), E.ATTN_BWD_STEPS) - (Lf + noise((N, 1), 1)))
    dS = P * (g @ v.T - delta)
    sim = torch.cat([0.125 * dS @ k, 0.125 * dS.T @ q, P.T @ g], 1)
    for n in E.THIRDS:
        e, s = (E.thirds(sim)[n] - E.thirds(ref)[n]).abs(), E.thirds(sigma)[n]
        ratio = (e.pow(2).mean() / s.pow(2).mean()).sqrt().item()
        print(f"\n[{name} {n}] simulated / modelled rms {ratio:.3f}, largest |error| / sigma {(e / s).max().item():.2f}")
        assert 2 / 3 <= ratio <= 1.5 and (e / s).max().item() <= 6


@pytest.mark.parametrize("shape", list(E.TATTN_FWD_SHAPES.values()), ids=list(E.TATTN_FWD_SHAPES))
@pytest.mark.parametrize("name", E.TATTN_CLASSES)
def test_temporal_attention_classes(name, shape):
    qkv, ref, err = E.tattn_class(name, *shape)
    assert torch.isfinite(ref).all() and (ref.abs().amax(0) > 0).all() and pos_finite(err), err
    B, T, P, Cc = shape
    if T <= 32:
        _, _, gref, gerr, dq_scale = E.tattn_bwd_class(name, *shape)
        assert torch.isfinite(gref).all() and (gref.abs().amax(0) > 0).all() and all(pos_finite(e) for e in gerr.values()), gerr
        if name == "same_frames":  # dq is zero but for fp64 noise: judged against the terms that cancel
            assert E.thirds(gref)["dq"].abs().max() <= 1e-12 * dq_scale.max() and (dq_scale.amax(0) > 0).all() and gerr["dq"][1] < 1e-5
    q, k, v = (t.double() for t in E.tattn_views(qkv, *shape))
    s = torch.einsum("btphd,bsphd->bphts", q, k) * (Cc // E.HEADS) ** -0.5
    if name == "shifted":
        assert 250 < s.mean() < 1000
    if name == "same_frames":
        assert torch.allclose(s.softmax(-1), torch.full_like(s, 1.0 / T), rtol=1e-12, atol=0)


def test_temporal_shapes_dispatch_the_kernels_they_are_named_after():
    for kernel, (B, T, P, Cc) in E.TATTN_FWD_SHAPES.items():
        assert E.tattn_forward_kernel(T, Cc) == kernel and T not in (4, 8, 16, 32, 64)
    for kernel, (B, T, P, Cc) in E.TATTN_BWD_SHAPES.items():
        assert E.tattn_backward_kernel(T, Cc) == kernel.split(" ")[0]
    assert [E.tattn_forward_kernel(T, Cc) for _, T, _, Cc in E.TATTN_T1_SHAPES] == ["small<4>", "pixel<8>"]
    assert {B for B, _, _, _ in E.TATTN_FWD_SHAPES.values()} == {1, 2}


def nz_min(t):
    t = t.abs()
    return t[t > 0].min().item() if (t > 0).any() else float("inf")


@pytest.mark.parametrize("shape", list(E.TATTN_FWD_SHAPES.values()), ids=list(E.TATTN_FWD_SHAPES))
def test_temporal_bitwise_scaling_operands_stay_normal(shape):
    """Every product and sum of the forward and backward in torch fp32 -- q k, the probabilities, P v, dP = dO v, dS = P (dP - P . dP), dS k, dS q,
    P dO -- keeps 2^24 of headroom (another summation order may cancel deeper) above 2^-126 when v or dO is scaled by 2^-40 and stays below 2^127
    at 2^40; q 2^40 and k 2^-40 stay normal themselves, their products do not change."""
    B, T, P, Cc = shape
    qkv, dO = E.tattn_bounded(*shape)
    q, k, v = E.tattn_views(qkv, *shape)
    d = Cc // E.HEADS
    g = dO.view(B, T, P, E.HEADS, d)
    qk = torch.einsum("btphd,bsphd->bphtsd", q, k)
    s = qk.sum(-1) * d ** -0.5
    p = s.softmax(-1)
    dp = torch.einsum("btphd,bsphd->bphts", g, v)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * d ** -0.5
    unscaled = (qk, p)
    scaled = (torch.einsum("bphts,bsphd->bphtsd", p, v), torch.einsum("btphd,bsphd->bphtsd", g, v), dp, ds, torch.einsum("bphts,bsphd->bphtsd", ds, k),
              torch.einsum("bphts,btphd->bphtsd", ds, q), torch.einsum("bphts,btphd->bphtsd", p, g))
    assert min(nz_min(t) for t in unscaled) >= LO
    for sexp in E.BITWISE_SCALES:
        assert min(nz_min(t) for t in scaled) * 2.0 ** sexp >= LO * 2.0 ** 24 and max(t.abs().max().item() for t in scaled) * 2.0 ** sexp < HI
    assert nz_min(k) * 2.0 ** -40 >= LO and q.abs().max() * 2.0 ** 40 < HI


@pytest.mark.parametrize("Fr,N,heads", E.ATTN_BWD_SHAPES)
def test_attention_backward_bitwise_scaling_operands_stay_normal(Fr, N, heads):
    """dO 2^s: delta = dO . O, dP = dO V^T, dS = P (dP - delta) and the terms of dS K, dS^T Q, P^T dO (bounded below by the product of the factors'
    smallest non-zero magnitudes) keep 2^24 of headroom above 2^-126 at s = -40 and stay below 2^127 at s = 40."""
    qkv, dO = E.attn_bounded(Fr, N, heads)
    t = qkv.reshape(Fr, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    g = dO.reshape(Fr, N, heads, 64).permute(0, 2, 1, 3)
    p = ((t[0] * 0.125) @ t[1].transpose(-2, -1)).softmax(-1)
    dp = g @ t[2].transpose(-2, -1)
    ds = p * (dp - (g * (p @ t[2])).sum(-1, keepdim=True))
    lowest = min(nz_min(dO) * nz_min(t[2]), nz_min(dp), nz_min(ds), nz_min(ds) * nz_min(t[1]) * 0.125, nz_min(ds) * nz_min(t[0]) * 0.125, nz_min(p) * nz_min(dO))
    highest = max(dp.abs().max().item(), ds.abs().max().item() * N, float(N))
    assert nz_min(p) >= 2.0 ** -20
    for sexp in E.BITWISE_SCALES:
        assert lowest * 2.0 ** sexp >= LO * 2.0 ** 24 and highest * 2.0 ** sexp < HI


@pytest.mark.parametrize("kind", ["rows", "slabs"])
def test_norm_backward_bitwise_scaling_operands_stay_normal(kind):
    """dy 2^s through the norm backwards: dy w, its two row sums and dx keep their headroom."""
    for shape in (E.LN_SHAPES if kind == "rows" else E.GN_SHAPES):
        if kind == "rows":
            x, w = E.ln_operands("base", *shape)[:2]
            dy = E.bounded(shape, 51)
            dx = E._ln_grad(x, w, dy, torch.float32)
        else:
            x, w, b = E.gn_operands("base", *shape)
            dy = E.bounded(shape, 51)
            dx = E._gn_grad(x, w, b, dy, torch.float32)
        lowest, highest = min(nz_min(dy * w), nz_min(dx)), max((dy * w).abs().max().item() * dy[0].numel(), dx.abs().max().item())
        for sexp in E.BITWISE_SCALES:
            assert lowest * 2.0 ** sexp >= LO * 2.0 ** 24 and highest * 2.0 ** sexp < HI


def plan(lib, n, slots, k_tiles):
    out = (C.c_int64 * 8)()
    assert lib.edv_split_plan(ATTN, n, slots, k_tiles, out) == 0
    return dict(zip(("split", "grid", "whole_rounds", "chunk", "nsplit", "stride", "units", "ws"), out))


def attn_bwd_plan(lib, Fr, N, heads):
    return plan(lib, E.attn_bwd_tasks(Fr, N, heads), E.ATTN_BWD_SLOTS, -(-N // E.ATTN_BWD_TILE))


def test_attention_backward_shapes_get_the_plans_the_gpu_test_names(lib):
    """attn_spatial_bwd_kernel: 128 resident rows per task, 32 streamed rows per tile, two resident workgroups per CU = 512 slots (what the
    comments of test_attn_spatial_bwd assume; tests/test_attn_bwd_edges_gpu.py compares the device's own workspace size with this plan's)."""
    p = attn_bwd_plan(lib, 2, 321, 2)
    assert E.attn_bwd_tasks(2, 321, 2) == 12 and p["whole_rounds"] == 0 and p["stride"] == 12 and p["nsplit"] > 12  # every task split
    assert 321 % 128 == 65 and 321 % 32 == 1                                                                       # ragged resident block, last tile of one row
    p = attn_bwd_plan(lib, 1, 257, 1)
    assert E.attn_bwd_tasks(1, 257, 1) == 3 and p["whole_rounds"] == 0 and p["stride"] == 3 and p["nsplit"] > 3 and 257 % 128 == 1 and 257 % 32 == 1
    p = attn_bwd_plan(lib, 3, 300, 58)
    assert E.attn_bwd_tasks(3, 300, 58) == 522 and p["whole_rounds"] == 1 and p["stride"] == 10 and p["nsplit"] > 10  # one whole round + 10 split tasks
