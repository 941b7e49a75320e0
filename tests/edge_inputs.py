"""Edge-case operands, fp64 references and gates for the norm, temporal-attention and backward kernels (norms.hip, temporal.hip, bwd.hip,
attn_spatial_bwd.hip), shared by tests/test_edge_inputs_cpu.py and the three *_edges_gpu.py files.  The generators, the attention reference and
the per-column yardstick are those of tests/x6_inputs.py.

Every class function is seeded, works on CPU tensors only and returns, computed once per process (functools.lru_cache: do not write to what
they return): the inputs, the reference in fp64 (torch ops / autograd), and the error of torch's OWN fp32 op or autograd on the CPU against that
reference under the yardstick the kernel is judged by.  No yardstick is the global close(): one large row, slab or column must not hide the rest."""
import functools
import math

import torch
import torch.nn.functional as F

from . import x6_inputs as X
from .x6_inputs import BITWISE_SCALES, U, attn_reference, attn_views, bounded, column_error, lognormal, outlier_channels, uniform  # noqa: F401

MARGIN = 4.0  # against torch fp32 on the same inputs: the margin of x6_inputs.attn_gate_failures
# the uniform-input tolerances of tests/test_kernels_gpu.py, test_bwd_kernels_gpu.py and test_mapped_kernels_gpu.py
FLOOR = {"ln_fwd": 2e-6, "ln_bwd": 3e-6, "gn": 5e-6, "attn_bwd": 1e-5, "tattn_fwd": 3e-6, "tattn_bwd": 5e-6, "lse": 2e-5}
GELU_GATE = 1.5e-6  # test_gelu_accuracy: absolute error of the erf-form GELU


def rms_max(e):
    return e.pow(2).mean().sqrt().item(), e.max().item()


def gate_failures(rms, mx, torch_err, floor):
    """max <= max(4 x torch fp32's max, the kernel's uniform-input tolerance) and rms <= 4 x max(torch fp32's rms, u), over every element.  The 4
    covers what differs from torch: exp2 pre-scaling, hardware rsqrt / exp, another summation tree -- a few roundings per element each."""
    rms_t, max_t = torch_err
    bad = []
    if not mx <= max(MARGIN * max_t, floor):
        bad.append(f"max {mx:.3e} > max(4 x torch fp32 {max_t:.3e}, {floor:.0e})")
    if not rms <= MARGIN * max(rms_t, U):
        bad.append(f"rms {rms:.3e} > 4 x max(torch fp32 {rms_t:.3e}, u)")
    return bad


def ratios(rms, mx, torch_err):
    """'kernel / torch' as the tests print it (torch's error may be exactly zero on the exact classes)."""
    r = lambda a, b: f"{a / b:.2f}" if b > 0 else "-"
    return f"rms {rms:.2e} max {mx:.2e} | torch fp32 rms {torch_err[0]:.2e} max {torch_err[1]:.2e} | kernel/torch rms {r(rms, torch_err[0])} max {r(mx, torch_err[1])}"


def const_values(n):
    """n values k / 2 with |k| <= 4095 (at most 12 significant bits), the first three 1024.5, -3 and 0, the rest non-zero."""
    v = [1024.5, -3.0, 0.0] + [(((i * 61) % 8191) - 4095) / 2.0 for i in range(3, n)]
    return torch.tensor(v[:n], dtype=torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- rows: LayerNorm ---------------------------------------------------------------------------------------------------------------------
# (129, 32): 8 active lanes; (131, 384): two float4 per lane; (67, 1024): four.  rows % 4 != 0: the last workgroup of four waves is partial.
LN_SHAPES = ((129, 32), (131, 384), (67, 1024))
LN_CLASSES = ("offset_1e3", "offset_1e4", "outlier_ch", "lognormal", "scaled_2p40", "scaled_2m40", "const")
# form -> (eps, position embedding, activation, accumulate): edv_layernorm plain / with pe, edv_layernorm_mapped with GELU / accumulating
LN_FORMS = {"plain": (1e-6, False, 0, False), "pe": (1e-5, True, 0, False), "gelu": (1e-6, False, 1, False), "acc": (1e-5, True, 0, True)}
LN_RPF, LN_T = 7, 5  # rows per frame and frames of the position embedding
LN_BWD_EPS = 1e-6


def ln_outliers(dim):
    return (5, dim // 2 + 3, dim - 4)


def ln_base(rows, dim):
    """The input of test_layernorm."""
    return uniform((rows, dim), 1, 3.0) + 0.5


@functools.lru_cache(maxsize=None)
def ln_operands(name, rows, dim):
    """(x, w, b, pe, y_prev)"""
    if name == "offset_1e3":      # mean 1000, sigma 0.03 / sqrt 3 = 0.017
        x = 1000.0 + uniform((rows, dim), 1, 0.03)
    elif name == "offset_1e4":    # mean 1e4, sigma 0.006: six ulps of the values themselves
        x = 1e4 + uniform((rows, dim), 1, 0.01)
    elif name == "outlier_ch":
        x = outlier_channels(ln_base(rows, dim), ln_outliers(dim), 300.0)
    elif name == "lognormal":
        x = lognormal((rows, dim), 13)
    elif name == "scaled_2p40":
        x = ln_base(rows, dim) * 2.0 ** 40
    elif name == "scaled_2m40":   # variance 3 x 2^-80, far below eps
        x = ln_base(rows, dim) * 2.0 ** -40
    elif name == "const":
        x = const_values(rows)[:, None].expand(rows, dim).contiguous()
    elif name == "base":
        x = ln_base(rows, dim)
    else:
        raise KeyError(name)
    return x, uniform((dim,), 2) + 1.0, uniform((dim,), 3, 0.1), uniform((32, dim), 4), uniform((rows, dim), 5)


def ln_pe_rows(pe, rows):
    return pe[(torch.arange(rows) // LN_RPF) % LN_T]


def ln_apply(x, w, b, pe, y_prev, form, dtype):
    """The kernel's order: normalise, + pe, GELU, + what y held."""
    eps, use_pe, act, acc = LN_FORMS[form]
    c = lambda t: t.to(dtype)
    y = F.layer_norm(c(x), (x.shape[1],), c(w), c(b), eps)
    if use_pe:
        y = y + ln_pe_rows(c(pe), x.shape[0])
    if act:
        y = F.gelu(y)
    if acc:
        y = y + c(y_prev)
    return y


def row_error(y, ref):
    """Per element |y - ref| / max_c |ref[row, :]| -> (rms, max)."""
    den = ref.abs().amax(-1, keepdim=True)
    assert (den > 0).all()
    return rms_max((y.double().cpu() - ref).abs() / den)


@functools.lru_cache(maxsize=None)
def ln_forward(name, rows, dim, form):
    """(fp64 reference, row error of torch fp32)"""
    ops = ln_operands(name, rows, dim)
    ref = ln_apply(*ops, form, torch.float64)
    return ref, row_error(ln_apply(*ops, form, torch.float32), ref)


def ln_dy(rows, dim, kind):
    dy = uniform((rows, dim), 3)
    return outlier_channels(dy, ln_outliers(dim), 300.0) if kind == "outlier" else dy


def _ln_grad(x, w, dy, dtype):
    xs = x.detach().to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(F.layer_norm(xs, (x.shape[1],), w.to(dtype), None, LN_BWD_EPS), [xs], dy.to(dtype))
    return g


@functools.lru_cache(maxsize=None)
def ln_backward(name, rows, dim, dy_kind, acc):
    """(dy, dx_prev, fp64 reference of dx (+ dx_prev), row error of torch's fp32 autograd)"""
    x, w = ln_operands(name, rows, dim)[:2]
    dy, prev = ln_dy(rows, dim, dy_kind), uniform((rows, dim), 6)
    ref = _ln_grad(x, w, dy, torch.float64) + (prev.double() if acc else 0)
    t32 = _ln_grad(x, w, dy, torch.float32) + (prev if acc else 0)
    return dy, prev, ref, row_error(t32, ref)


def ln_two_pass(x, eps):
    """The kernels' arithmetic in torch fp32: sum, exact division by dim, centred second moment, rsqrt(var + eps) -> (x - mean) rstd."""
    dim = torch.tensor(float(x.shape[-1]))
    mean = x.sum(-1, keepdim=True) / dim
    d = x - mean
    return d * torch.rsqrt((d * d).sum(-1, keepdim=True) / dim + torch.tensor(eps))


# ---- slabs: GroupNorm --------------------------------------------------------------------------------------------------------------------
# channels per group 2 / 32 / 3.  (2, 100, 64): last 32-row chunk of 4 rows; (1, 33, 1024): 256 channel quads, one row per pass, last chunk of 1 row;
# (2, 65, 96): 24 channel quads (idle threads), last chunk of 1 row.  Every last chunk holds a power-of-two number of rows: the two-stage path's
# chunk mean multiplies by a reciprocal, which is exact only then.
GN_SHAPES = ((2, 100, 64), (1, 33, 1024), (2, 65, 96))
GN_CLASSES = ("offset_1e3", "chan_offsets", "outlier_pixel", "scaled_2p40", "const")
GROUPS, GN_EPS = 32, 1e-6


def gn_base(Fr, P, C):
    """The input of test_groupnorm."""
    return uniform((Fr, P, C), 1, 2.0) + 3.0


def gn_const_values(Fr):
    return const_values(Fr * GROUPS + 3)[3:].reshape(Fr, GROUPS)  # non-zero: the mean's yardstick divides by the slab's mean |x|


@functools.lru_cache(maxsize=None)
def gn_operands(name, Fr, P, C):
    """(x, w, b)"""
    cg = C // GROUPS
    if name == "offset_1e3":
        x = 1000.0 + uniform((Fr, P, C), 1, 0.03)
    elif name == "chan_offsets":  # the channels of one group at levels 0, 100, 200, ...
        assert cg >= 2
        x = uniform((Fr, P, C), 1) + 100.0 * (torch.arange(C) % cg).float()
    elif name == "outlier_pixel":
        x = gn_base(Fr, P, C)
        x[:, P // 2] *= 1e3
    elif name == "scaled_2p40":
        x = gn_base(Fr, P, C) * 2.0 ** 40
    elif name == "const":
        x = gn_const_values(Fr).repeat_interleave(cg, 1)[:, None, :].expand(Fr, P, C).contiguous()
    elif name == "base":
        x = gn_base(Fr, P, C)
    else:
        raise KeyError(name)
    return x, uniform((C,), 2) + 1.0, uniform((C,), 3, 0.1)


def slabs(t):
    """[F, P, C] -> [F, P, 32, C / 32]: slab (f, g) is [f, :, g, :]."""
    return t.reshape(t.shape[0], t.shape[1], GROUPS, t.shape[2] // GROUPS)


def slab_error(y, ref):
    """Per element |y - ref| / max over the (frame, group) slab of |ref| -> (rms, max)."""
    den = slabs(ref).abs().amax((1, 3), keepdim=True)
    assert (den > 0).all()
    return rms_max((slabs(y.double().cpu()) - slabs(ref)).abs() / den)


def gn_stats(x, dtype):
    """(mean, rstd) [F, 32], two passes in `dtype`."""
    s = slabs(x.to(dtype))
    return s.mean((1, 3)), (s.var((1, 3), unbiased=False) + GN_EPS).rsqrt()


def gn_stats_error(mean, rstd, ref_mean, ref_rstd, x):
    """mean: |mean - ref| / the slab's mean |x|; rstd: relative -> ((rms, max), (rms, max))"""
    den = slabs(x.double()).abs().mean((1, 3))
    assert (den > 0).all() and (ref_rstd > 0).all()
    return rms_max((mean.double().cpu() - ref_mean).abs() / den), rms_max((rstd.double().cpu() - ref_rstd).abs() / ref_rstd)


def _gn(x, w, b, dtype):
    return F.group_norm(x.to(dtype).permute(0, 2, 1), GROUPS, w.to(dtype), b.to(dtype), GN_EPS).permute(0, 2, 1)


@functools.lru_cache(maxsize=None)
def gn_forward(name, Fr, P, C):
    """(y, mean, rstd) in fp64 and torch fp32's (slab error of y, error of mean, error of rstd)"""
    x, w, b = gn_operands(name, Fr, P, C)
    ref, (m, r) = _gn(x, w, b, torch.float64), gn_stats(x, torch.float64)
    return ref, m, r, (slab_error(_gn(x, w, b, torch.float32), ref),) + gn_stats_error(*gn_stats(x, torch.float32), m, r, x)


def _gn_grad(x, w, b, dy, dtype):
    xs = x.detach().to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(_gn(xs, w, b, dtype), [xs], dy.to(dtype))
    return g


@functools.lru_cache(maxsize=None)
def gn_backward(name, Fr, P, C, acc):
    """(dy, dx_prev, fp64 reference of dx (+ dx_prev), slab error of torch's fp32 autograd)"""
    x, w, b = gn_operands(name, Fr, P, C)
    dy, prev = uniform((Fr, P, C), 4), uniform((Fr, P, C), 5)
    ref = _gn_grad(x, w, b, dy, torch.float64) + (prev.double() if acc else 0)
    return dy, prev, ref, slab_error(_gn_grad(x, w, b, dy, torch.float32) + (prev if acc else 0), ref)


# ---- spatial attention backward ----------------------------------------------------------------------------------------------------------
# (frames, tokens, heads).  attn_spatial_bwd_kernel keeps 128 rows resident per task and streams 32-row tiles; an MI355X keeps 512 of its
# workgroups resident (two per CU).  (2, 321, 2): 12 tasks, a resident block of 65 rows, a last streamed tile of one row, every task split;
# (1, 257, 1): 3 tasks, one resident row in the third block, all split; (3, 300, 58): 522 tasks = one whole round + 10 split tasks.
# tests/test_edge_inputs_cpu.py confirms the plans.
ATTN_BWD_SHAPES = ((2, 321, 2), (1, 257, 1), (3, 300, 58))
ATTN_BWD_SLOTS, ATTN_BWD_ROWS, ATTN_BWD_TILE = 512, 128, 32
ATTN_BWD_CLASSES = ("qk_outlier", "v_outlier", "shifted", "q_2m100", "dO_outlier")
THIRDS = ("dq", "dk", "dv")


def attn_bwd_tasks(Fr, N, heads):
    return Fr * heads * -(-N // ATTN_BWD_ROWS)


def thirds(t):
    D = t.shape[1] // 3
    return {n: t[:, j * D:(j + 1) * D] for j, n in enumerate(THIRDS)}


def thirds_error(got, ref, dq_scale=None):
    """X.column_error on the dq, dk and dv thirds separately -> {name: (rms, max)}.  Where dq is exactly zero in exact arithmetic (dq_scale given) its
    columns are divided by the largest dq_scale[:, c] instead of the largest |ref[:, c]|, which is fp64 noise there."""
    g, r = thirds(got), thirds(ref)
    out = {n: column_error(g[n], r[n]) for n in THIRDS}
    if dq_scale is not None:
        out["dq"] = rms_max((g["dq"].double().cpu() - r["dq"]).abs() / dq_scale.amax(0, keepdim=True))
    return out


def attn_dO(Fr, N, heads, outlier=False):
    dO = uniform((Fr * N, heads * X.HD), 2)
    if outlier:
        dO.view(Fr * N, heads, X.HD)[:, :, 5] *= 1e3
    return dO


def attn_bounded(Fr, N, heads):
    """q | k | v and dO of the bit-for-bit scaling test: |q|, |k|, |v| in (2^-5, 0.5), scores within +-2, so that no probability is below e^-4 / N."""
    return bounded((Fr * N, 3 * heads * X.HD), 31, 0.5), bounded((Fr * N, heads * X.HD), 32)


def _attn_grad(qkv, dO, Fr, N, heads, dtype):
    xs = qkv.detach().to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(attn_reference(xs, Fr, N, heads, dtype), [xs], dO.to(dtype))
    return g


def attn_lse2(qkv, Fr, N, heads, dtype):
    """Base-2 log-sum-exp of the scaled scores [F, heads, N] in `dtype` (fp32: torch's own fp32 scores and logsumexp)."""
    t = qkv.to(dtype).reshape(Fr, N, 3, heads, X.HD).permute(2, 0, 3, 1, 4)
    return torch.logsumexp((t[0] * X.HD ** -0.5) @ t[1].transpose(-2, -1), -1) * torch.tensor(1.0 / math.log(2.0), dtype=dtype)


ATTN_BWD_STEPS = 32  # v_mfma_f32_32x32x2_f32 steps that accumulate one score over the 64 head dimensions


def attn_bwd_rounding_sigma(qkv, dO, Fr, N, heads):
    """What the flash-style backward ALGORITHM owes to fp32, as a standard deviation per element of dq | dk | dv (fp64, shaped like dqkv).

    The kernel recomputes P_ij = exp2(X_ij), X_ij = S_ij log2e - L_i, in an accumulator that starts at -L_i and takes 32 MFMA steps: each step
    rounds at ulp(|L_i|), so X_ij carries 32 independent errors uniform in +-ulp(L_i) / 2 (variance ulp^2 / 12 each) and P_ij a relative error
    eps_ij of variance var_b = 32 ulp(L_i)^2 / 12 ln(2)^2.  The forward's scores, from which L_i and O (hence delta_i = dO_i . O_i) come, went
    through their own 32 steps; the model gives them the same variance (an upper estimate: their accumulators start at 0).  To first order
        dS'_ij = P_ij (1 + eps_i + eps_ij) (dP_ij - delta_i - ddelta_i),   ddelta_i = sum_l dS_il eps^f_il,
    with eps_i the row-common part (L_i's own rounding and the forward's error in it, sum_l P_il eps^f_il: var_c = var_b sum_l P_il^2 + ulp^2 / 12 ln(2)^2), so
        var dq_ic = d^-1 [var_b sum_j dS_ij^2 k_jc^2 + var(ddelta_i) (sum_j P_ij k_jc)^2] + var_c dq_ic^2
        var dk_jc = d^-1 sum_i [(var_b + var_c) dS_ij^2 + var(ddelta_i) P_ij^2] q_ic^2
        var dv_jc = sum_i (var_b + var_c) P_ij^2 dO_ic^2,                        var(ddelta_i) = var_b sum_l dS_il^2.
    torch's softmax backward has the same eps_ij in its fp32 scores but takes delta from the SAME probabilities, so its rows of dS sum to zero
    whatever eps is; here sum_j dS'_ij = O(eps), and a component common to all keys (k_j = k0_j + kbar) enters dq as kbar sum_j dS'_ij.  That is
    the price of not keeping the N x N probabilities, and it grows with |L| u: with scores offset by 500 and |kbar| = 62 |k0| it is 1e-3 of dq."""
    ln2 = math.log(2.0)
    t = qkv.double().reshape(Fr, N, 3, heads, X.HD).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    g = dO.double().reshape(Fr, N, heads, X.HD).permute(0, 2, 1, 3)
    S = (q * X.HD ** -0.5) @ k.transpose(-2, -1)
    L = torch.logsumexp(S, -1, keepdim=True)
    P = (S - L).exp()
    dP = g @ v.transpose(-2, -1)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    ulp = torch.exp2(torch.floor(torch.log2((L / ln2).abs().clamp(min=1.0))) - 23)  # of the base-2 accumulator, [F, h, N, 1]
    var_b = ATTN_BWD_STEPS * ulp ** 2 / 12 * ln2 ** 2
    var_c = var_b * (P ** 2).sum(-1, keepdim=True) + ulp ** 2 / 12 * ln2 ** 2
    var_delta = var_b * (dS ** 2).sum(-1, keepdim=True)
    dq = X.HD ** -0.5 * dS @ k
    var_dq = (var_b * (dS ** 2 @ k ** 2) + var_delta * (P @ k) ** 2) / X.HD + var_c * dq ** 2
    var_dk = ((dS ** 2 * (var_b + var_c) + P ** 2 * var_delta).transpose(-2, -1) @ q ** 2) / X.HD
    var_dv = (P ** 2 * (var_b + var_c)).transpose(-2, -1) @ g ** 2
    back = lambda x: x.permute(0, 2, 1, 3).reshape(Fr * N, heads * X.HD)
    return torch.cat([back(var_dq), back(var_dk), back(var_dv)], 1).sqrt()


# Classes on which the kernel exceeds 4 x torch fp32 for the reason above (|L| in the tens and hundreds): gated by the model instead --
# rms <= max(ordinary gate, 2 x the model's rms) and every element <= ordinary gate + 8 sigma.  2: the model does not know whether an MFMA step
# rounds once or twice (sqrt 2), nor the q log2e d^-1/2 pre-scaling and product roundings (a few per cent); 8 sigma: the largest of 3e6
# Gaussian samples is 5.2 sigma, the rest covers the tails of a sum of uniforms and the model's factor.
ATTN_BWD_DERIVED = ("qk_outlier", "shifted")


def attn_bwd_derived_failures(got, ref, sigma, torch_err, floor):
    bad = []
    for n in THIRDS:
        g, r, s = thirds(got)[n].double(), thirds(ref)[n], thirds(sigma)[n]
        den = r.abs().amax(0, keepdim=True)
        e = (g - r).abs()
        rms, (rms_t, max_t), rms_m = (e / den).pow(2).mean().sqrt().item(), torch_err[n], (s / den).pow(2).mean().sqrt().item()
        if not rms <= max(MARGIN * max(rms_t, U), 2 * rms_m):
            bad.append(f"{n}: rms {rms:.3e} > max(4 x max(torch fp32 {rms_t:.3e}, u), 2 x model {rms_m:.3e})")
        worst = (e / (max(MARGIN * max_t, floor) * den + 8 * s)).max().item()
        if not worst <= 1:
            bad.append(f"{n}: an element is {worst:.2f} x (ordinary gate + 8 sigma)")
    return bad


@functools.lru_cache(maxsize=4)
def attn_bwd_class(name, Fr, N, heads):
    """(qkv, dO, dqkv in fp64, lse in fp64, {dq, dk, dv: column error of torch's fp32 autograd}, (rms, max) absolute error of torch's fp32 lse)"""
    qkv = uniform((Fr * N, 3 * heads * X.HD), 3, 2.0) if name == "dO_outlier" else X.attn_class(name, Fr, N, heads)[0]
    dO = attn_dO(Fr, N, heads, name == "dO_outlier")
    ref, lse = _attn_grad(qkv, dO, Fr, N, heads, torch.float64), attn_lse2(qkv, Fr, N, heads, torch.float64)
    return (qkv, dO, ref, lse, thirds_error(_attn_grad(qkv, dO, Fr, N, heads, torch.float32), ref),
            rms_max((attn_lse2(qkv, Fr, N, heads, torch.float32).double() - lse).abs()))


# ---- temporal attention ------------------------------------------------------------------------------------------------------------------
# (B, T, P, C), 8 heads, d = C / 8: one shape per instantiation attn_temporal / attn_temporal_bwd dispatch without an environment variable; no T
# equals its template bound, so every kernel runs with padded frames.
HEADS = 8
TATTN_FWD_SHAPES = {"small<4>": (2, 3, 37, 64), "small<8>": (1, 5, 41, 128), "pixel<8>": (2, 5, 23, 192), "pixel<16>": (1, 12, 19, 64),
                    "pixel<32>": (1, 27, 13, 256), "pixel<64>": (1, 48, 11, 64)}
TATTN_BWD_SHAPES = {"pixel<8> d=8": (2, 3, 37, 64), "pixel<8> d=24": (2, 5, 23, 192), "pixel<16>": (1, 12, 19, 64), "pixel<32>": (1, 27, 13, 256)}
TATTN_T1_SHAPES = ((2, 1, 37, 64), (1, 1, 23, 192))  # forward small<4> and pixel<8>, backward pixel<8>
TATTN_CLASSES = ("qk_outlier", "shifted", "v_outlier", "q_2m100", "same_frames")


def tattn_forward_kernel(T, C):
    """The dispatch of attn_temporal (temporal.hip) for 8 heads with no environment variable set, restated."""
    d, HG = C // HEADS, HEADS
    while HG > 1 and (T * HG > 256 or T * 3 * HG * d * 4 > 64 * 1024 or HEADS % HG):
        HG -= 1
    cap = 160 * 1024 if (T > 32 and HG == 1) else 64 * 1024
    if T * HG <= 256 and T * 3 * HG * d * 4 <= cap and (T > 8 or d >= 24):
        return f"pixel<{8 if T <= 8 else 16 if T <= 16 else 32 if T <= 32 else 64}>"
    assert T <= 8
    return "small<4>" if T <= 4 else "small<8>"


def tattn_backward_kernel(T, C):
    """The dispatch of attn_temporal_bwd (bwd.hip), restated."""
    d, HG, TM = C // HEADS, HEADS, (8 if T <= 8 else 16 if T <= 16 else 32)
    lds = lambda hg: (T * 4 * hg * d + 2 * hg * T * TM) * 4
    while HG > 1 and (T * HG > 256 or lds(HG) > 64 * 1024 or HEADS % HG):
        HG -= 1
    assert T * HG <= 256 and lds(HG) <= (160 * 1024 if HG == 1 else 64 * 1024)
    return f"pixel<{TM}>"


def tattn_views(qkv, B, T, P, C):
    """q, k, v as views [B, T, P, 8, d] of the fused rows [(b T + t) P + p, 3 C]."""
    t = qkv.view(B, T, P, 3, HEADS, C // HEADS)
    return t[:, :, :, 0], t[:, :, :, 1], t[:, :, :, 2]


def tattn_reference(qkv, B, T, P, C, dtype=torch.float64):
    """The reference of test_attn_temporal, in `dtype`."""
    d = C // HEADS
    t = qkv.to(dtype).reshape(B, T, P, 3, HEADS, d).permute(3, 0, 2, 4, 1, 5)  # [3, B, P, h, T, d]
    a = ((t[0] @ t[1].transpose(-1, -2)) * d ** -0.5).softmax(-1)
    return (a @ t[2]).permute(0, 3, 1, 2, 4).reshape(B * T * P, C)


def tattn_base(B, T, P, C):
    return uniform((B * T * P, 3 * C), 1, 1.5)


def tattn_dO(B, T, P, C):
    return uniform((B * T * P, C), 2)


def tattn_bounded(B, T, P, C):
    return bounded((B * T * P, 3 * C), 41), bounded((B * T * P, C), 42)


@functools.lru_cache(maxsize=None)
def tattn_operands(name, B, T, P, C):
    qkv = tattn_base(B, T, P, C)
    q, k, v = tattn_views(qkv, B, T, P, C)
    d = C // HEADS
    if name == "qk_outlier":       # two head dimensions x 8 in q and k: scores reach +-70 d^-1/2 ..., the rows are peaked
        for c in (1, d - 2):
            q[..., c] *= 8
            k[..., c] *= 8
    elif name == "shifted":
        # q += 1 and k += c qbar, qbar the mean query of the (clip, pixel, head) over its frames: the scores of query t all carry the offset
        # c q_t . qbar d^-1/2, about c sqrt(d) = 500 -- softmax does not see it, fp32 scores lose 2^-15 to it
        q += 1.0
        k += (500.0 / math.sqrt(d)) * q.mean(1, keepdim=True)
    elif name == "v_outlier":
        v[..., 1] *= 1e3
    elif name == "q_2m100":        # every score is 0 to fp32
        q *= 2.0 ** -100
    elif name == "same_frames":    # k_t equal for all t: every probability is 1 / T
        k[:] = k[:, :1].clone()
    elif name != "base":
        raise KeyError(name)
    return qkv


@functools.lru_cache(maxsize=None)
def tattn_class(name, B, T, P, C):
    """(qkv, fp64 reference, column error of torch fp32)"""
    qkv = tattn_operands(name, B, T, P, C)
    ref = tattn_reference(qkv, B, T, P, C)
    return qkv, ref, column_error(tattn_reference(qkv, B, T, P, C, torch.float32), ref)


def _tattn_grad(qkv, dO, B, T, P, C, dtype):
    xs = qkv.detach().to(dtype).requires_grad_(True)
    (g,) = torch.autograd.grad(tattn_reference(xs, B, T, P, C, dtype), [xs], dO.to(dtype))
    return g


def tattn_dq_scale(qkv, dO, B, T, P, C):
    """d^-1/2 sum_j |dS_ij| |k_jc|, shaped like dq: the size of the terms of dq.  With the same key in every frame dq = k d^-1/2 sum_j dS_ij is exactly
    zero, so its error can only be measured against the terms that cancel."""
    d = C // HEADS
    t = qkv.double().reshape(B, T, P, 3, HEADS, d).permute(3, 0, 2, 4, 1, 5)  # [3, B, P, h, T, d]
    g = dO.double().reshape(B, T, P, HEADS, d).permute(0, 2, 3, 1, 4)
    p = ((t[0] @ t[1].transpose(-1, -2)) * d ** -0.5).softmax(-1)
    dp = g @ t[2].transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return ((ds.abs() @ t[1].abs()) * d ** -0.5).permute(0, 3, 1, 2, 4).reshape(B * T * P, C)


@functools.lru_cache(maxsize=None)
def tattn_bwd_class(name, B, T, P, C):
    """(qkv, dO, dqkv in fp64, {dq, dk, dv: column error of torch's fp32 autograd}, the dq yardstick of same_frames or None)"""
    qkv, dO = tattn_operands(name, B, T, P, C), tattn_dO(B, T, P, C)
    ref = _tattn_grad(qkv, dO, B, T, P, C, torch.float64)
    scale = tattn_dq_scale(qkv, dO, B, T, P, C) if name == "same_frames" else None
    return qkv, dO, ref, thirds_error(_tattn_grad(qkv, dO, B, T, P, C, torch.float32), ref, scale), scale
