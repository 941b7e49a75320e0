"""Exact-integer and numeric-edge operands, fp64 references, per-element magnitudes and rounding counts for the parameter-gradient reductions:
edv_lora_grads (bwd.hip), edv_colsum_rows (wgrad.hip), edv_col_dot (bwd.hip), edv_colsum_batch (bias_colsum.hip) and the forward twin
edv_fold_lora (prep.hip).  Shared by tests/test_grad_inputs_cpu.py and tests/test_grad_edges_gpu.py.  The generators are those of
tests/x6_inputs.py, the gate against torch's fp32 that of tests/edge_inputs.py.

Everything is seeded, works on CPU tensors only and is computed once per process (functools.lru_cache: do not write to what these functions
return).  Every class function returns the inputs, the fp64 reference (torch autograd for lora_grads), the magnitudes below and the error of
torch's OWN fp32 op or autograd on the CPU under the same yardstick.

The yardstick is per element, never global.  A gradient such as dB'[n, j] = s gamma_n sum_m G_mn t_mj, t_mj = sum_k x_mk a'_jk, has two
magnitudes, both in fp64:
    mag_outer = |s gamma_n| sum_m |G_mn| |t_mj|                  what a rounding error of the sum over the rows is proportional to
    mag_inner = |s gamma_n| sum_m |G_mn| sum_k |x_mk a'_jk|      what a rounding error made inside skinny_xwt is proportional to
(mag_inner >= mag_outer; it is the sum of the absolute values of ALL contributing terms, and the yardstick the comparison with torch uses).
The hard gate is err <= u (d_outer mag_outer + d_inner mag_inner) with the d counted from the kernels' code, see lora_depths."""
import functools
from types import SimpleNamespace

import torch

from .conv_inputs import integers
from .edge_inputs import MARGIN, bits, gate_failures, ratios, rms_max  # noqa: F401
from .x6_inputs import BITWISE_SCALES, U, bounded, lognormal, outlier_channels, uniform  # noqa: F401
from . import x6_inputs as X6

EXACT_LIMIT = 2 ** 24
FP32_MIN_NORMAL = X6.FP32_MIN_NORMAL
LOGNORMAL_SIGMA = 2.0  # the sigma of x6_inputs.lognormal

# restated from ops.hpp, bwd.hip, wgrad.hip and bias_colsum.hip; tests/test_grad_inputs_cpu.py checks what the shape tables claim against them
TALL_SPLITS = 64       # row splits of tall_tn / col_dot
TALL_COLS = 64         # columns per workgroup of tall_tn_partial_kernel / col_dot_partial_kernel
REDUCE_COLS = 32       # elements per workgroup of tall_tn_reduce_kernel
REDUCE_SLICES = 8      # slices of the split range in tall_tn_reduce_kernel / colsum_reduce_kernel
SKINNY_STEP = 256      # columns a wave of skinny_xwt_kernel takes per step
COLSUM_BLOCKS = 512    # cap of colsum_partial_kernel's grid
COLSUM_F4_PER_WG = 2048  # float4s a workgroup of colsum_partial_kernel is sized for
CS_MAX_PARTS, CS_ELEMS = 64, 65536  # colsum_job: at most 64 row chunks of about 64 K elements

CLASSES = ("exact_int", "scaled", "outlier_ch", "lognormal", "offset", "cancelling", "last_split_only")
ACCURACY_CLASSES = CLASSES[2:]
DELTA, DELTA_SMALL = 2.0 ** -12, 2.0 ** -14


def cdiv(a, b):
    return -(-a // b)


def split_geometry(M):
    """(rows_per_split, splits, rows of the last split) of tall_tn / col_dot."""
    rps = cdiv(M, TALL_SPLITS)
    splits = cdiv(M, rps)
    return rps, splits, M - (splits - 1) * rps


def tall_depth(M):
    """Roundings on the longest path of one tall_tn / col_dot sum, without products and scales: a wave adds ceil(rows_per_split / 4) terms in
    sequence, 2 additions join the four waves, stage 2 adds ceil(splits / 8) partials in sequence and 7 more join its slices."""
    rps, splits, _ = split_geometry(M)
    return cdiv(rps, 4) + 2 + cdiv(splits, REDUCE_SLICES) + 7


def skinny_depth(K):
    """skinny_xwt_kernel: a product, the four-term tree (2), one addition to the accumulator per 256-column step, the wave butterfly (6)."""
    return 1 + 2 + cdiv(K, SKINNY_STEP) + 6


def outlier_indices(n):
    """5, n / 2 + 3 and n - 4, clipped to the shape."""
    return sorted({min(5, n - 1), min(n // 2 + 3, n - 1), max(n - 4, 0)})


def row_factors(M, seed):
    """exp(sigma z_m): a few rows dominate."""
    g = torch.Generator().manual_seed(seed)
    return torch.exp(LOGNORMAL_SIGMA * torch.randn(M, 1, generator=g))


def choice(values, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def nonzero(t):
    return torch.where(t == 0, torch.ones_like(t), t)


def class_error(cls, y, ref, mag):
    """elem_error, or None for exact_int: that class is compared bit for bit, and its sparse operands leave elements without any term."""
    return None if cls == "exact_int" else elem_error(y, ref, mag)


def elem_error(y, ref, mag):
    """Per element |y - ref| / mag -> (rms, max); mag must be positive everywhere."""
    assert (mag > 0).all()
    return rms_max((y.double().cpu() - ref.double()).abs() / mag)


def bound_ratio(y, ref, mag_outer, d_outer, mag_inner=None, d_inner=0):
    """max over the elements of err / (u (d_outer mag_outer + d_inner mag_inner)): <= 1 passes the hard gate."""
    bound = U * (d_outer * mag_outer + (d_inner * mag_inner if mag_inner is not None else 0))
    assert (bound > 0).all()
    return ((y.double().cpu() - ref.double()).abs() / bound).max().item()


def delta_for(M):
    """The perturbation of `cancelling`.  What is left of a sum over M / 2 mirrored pairs is delta sum_m r_m g_m t_m, a random walk: about
    0.31 delta / sqrt(M / 2) of mag_outer in the median (0.31 from two CPU probes: 2.7e-6 at M = 1370, 9.3e-6 at M = 130).  At 2^-12 that is
    too close to the class's 1e-5 at M = 130 -- the test shape (130, 100, 588, 2) gave 1.07e-5 for dA -- so delta is 2^-12 from M = 256 on
    (6.7e-6 there) and 2^-14 below (2.3e-6 at M = 130, 3.3e-6 at M = 64)."""
    return DELTA if M >= 256 else DELTA_SMALL


# ---- edv_lora_grads ----------------------------------------------------------------------------------------------------------------------
# (M, nin, nout, r), the smallest shapes that reach each edge:
#   (1, 4, 4, 1)          one row, one split, one active lane; odd M with r = 1: the workspace layout whose regions need padding
#   (3, 68, 4, 2)         fewer than 8 splits; N = 68 = one full 64-column block + 4
#   (63, 64, 260, 8), (64, 256, 60, 4)   one row per split; K at and just past a 256 step; N r = 240 no multiple of the reduce kernel's 32
#   (65, 260, 64, 1)      33 splits of two rows, the last of one; r = 1 with odd M
#   (130, 100, 588, 2)    44 splits of three rows, the last of one; K = 588 (the patch-embed width) with a 76-column tail
#   (1370, 384, 1536, 4)  ViT-S fc1 on one frame: 22 rows per split, the last of 6
LORA_SHAPES = ((1, 4, 4, 1), (3, 68, 4, 2), (63, 64, 260, 8), (64, 256, 60, 4), (65, 260, 64, 1), (130, 100, 588, 2), (1370, 384, 1536, 4))
LORA_FORMS = ((False, False), (True, True), (False, True), (True, False))  # (DV-LoRA, gamma), cycled over the cases
LORA_OUTPUTS = ("dA", "dB", "dU", "dV")
ADJOINT_SHAPES = ((65, 260, 64, 1), (130, 100, 588, 2), (63, 64, 260, 8))
MISTAKES = ("drop_last_split", "drop_ragged_columns", "drop_k_tail", "dApT_untransposed", "gamma_off_dB", "swap_UV", "dV_wrong_axis")


def lora_form(shape, cls):
    """(dv, use_gamma) of a (shape, class) pair: the shapes cycle through the four forms, every class starts the cycle one further."""
    return LORA_FORMS[(LORA_SHAPES.index(shape) + CLASSES.index(cls)) % len(LORA_FORMS)]


def lora_has_class(cls, shape):
    return cls != "cancelling" or shape[0] % 2 == 0


def lora_cases(classes):
    return [(cls, shape) for cls in classes for shape in LORA_SHAPES if lora_has_class(cls, shape)]


def edge_columns(n):
    """The first and last column and both sides of every 256-column and every 64-column step."""
    c = {0, n - 1}
    for step in (SKINNY_STEP, TALL_COLS):
        for b in range(step, n, step):
            c |= {b - 1, b}
    return sorted(c)


def sparse_signs(rows, n, seed):
    """[rows, n], +-1 on edge_columns(n), zero elsewhere."""
    cols = edge_columns(n)
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(rows, n)
    out[:, cols] = torch.randint(0, 2, (rows, len(cols)), generator=g).float() * 2 - 1
    return out


def split_edge_rows(M):
    """First and last row of every split."""
    rps, splits, _ = split_geometry(M)
    return sorted({i * rps for i in range(splits)} | {min((i + 1) * rps, M) - 1 for i in range(splits)})


def last_split_rows(M):
    rps, splits, _ = split_geometry(M)
    return slice((splits - 1) * rps, M)


def mirror_rows(P, G, seed=77):
    """The second half of the rows mirrors the first: P equal, G = -G (1 + delta r), r uniform in (-1, 1)."""
    P, G = P.clone(), G.clone()
    h = P.shape[0] // 2
    assert 2 * h == P.shape[0]
    P[h:] = P[:h]
    G[h:] = -G[:h] * (1 + delta_for(P.shape[0]) * uniform(G[:h].shape, seed))
    return P, G


def _class_pair(cls, M, nx, ng, seeds=(1, 2)):
    """(X [M, nx], G [M, ng]) of an accuracy class or of `scaled`."""
    sx, sg = seeds
    if cls == "scaled":
        return bounded((M, nx), 20 + sx), bounded((M, ng), 20 + sg)
    x, G = uniform((M, nx), sx), uniform((M, ng), sg)
    if cls == "outlier_ch":
        return outlier_channels(x, outlier_indices(nx)), outlier_channels(G, outlier_indices(ng))
    if cls == "lognormal":
        return x, G * row_factors(M, 13)
    if cls == "offset":
        return 5.0 + x, 5.0 + G
    if cls == "cancelling":
        return mirror_rows(x, G)
    if cls == "last_split_only":
        keep = torch.zeros(M, 1)
        keep[last_split_rows(M)] = 1
        return x, G * keep
    raise KeyError(cls)


@functools.lru_cache(maxsize=None)
def lora_operands(cls, shape):
    """SimpleNamespace(x [M, nin], G [M, nout], A [r, nin], B [nout, r], U [r, 1] or None, V [nout, 1] or None, gamma [nout] or None, s)"""
    M, nin, nout, r = shape
    dv, use_gamma = lora_form(shape, cls)
    if cls == "exact_int":
        x, G = integers((M, nin), 1, 2), integers((M, nout), 2, 2)
        e = split_edge_rows(M)
        x[e], G[e] = nonzero(x[e]), nonzero(G[e])
        A, B = sparse_signs(r, nin, 3), sparse_signs(r, nout, 4).T.contiguous()
        Uv, Vv = choice((1, -1, 2), r, 5)[:, None], choice((1, 2, -1, -2), nout, 6)[:, None]
        gamma, s = choice((1, 2, -1), nout, 8), 2.0
    else:
        x, G = _class_pair(cls, M, nin, nout)
        mk = bounded if cls == "scaled" else uniform
        A, B = mk((r, nin), 3), mk((nout, r), 4)
        Uv, Vv, gamma, s = uniform((r, 1), 5) + 1.2, uniform((nout, 1), 6) + 1.2, uniform((nout,), 8) + 1.5, 0.75
    return SimpleNamespace(x=x, G=G, A=A, B=B, U=Uv if dv else None, V=Vv if dv else None, gamma=gamma if use_gamma else None, s=s, dv=dv)


def lora_scaled(shape, pg, px):
    """The `scaled` operands with G 2^pg and x 2^px."""
    o = lora_operands("scaled", shape)
    return SimpleNamespace(**{**vars(o), "x": o.x * 2.0 ** px, "G": o.G * 2.0 ** pg})


def lora_formula(o, dtype=torch.float64, mistake=None):
    """The gradients written out as the kernels compute them (t, u, dBp, dApT, finalize), in `dtype` (torch.int64 for the exact answer) ->
    {dA, dB, dU, dV} (dU, dV None for plain LoRA).  `mistake` applies one of MISTAKES."""
    c = lambda t: None if t is None else t.to(dtype)
    x, G, A, B, Uv, Vv, gam = c(o.x), c(o.G), c(o.A), c(o.B), c(o.U), c(o.V), c(o.gamma)
    s = int(o.s) if dtype == torch.int64 else o.s
    M, nin = x.shape
    nout, r = B.shape
    g = gam if gam is not None else torch.ones(nout, dtype=dtype)
    Ae = A * Uv if o.dv else A
    Bg = (B * Vv if o.dv else B) * g[:, None]
    kin, kout = (nin // SKINNY_STEP * SKINNY_STEP, nout // SKINNY_STEP * SKINNY_STEP) if mistake == "drop_k_tail" else (nin, nout)
    t, u = x[:, :kin] @ Ae[:, :kin].T, G[:, :kout] @ Bg[:kout]
    rps, splits, _ = split_geometry(M)
    mt = (splits - 1) * rps if mistake == "drop_last_split" else M
    dBp = s * (torch.ones_like(g) if mistake == "gamma_off_dB" else g)[:, None] * (G[:mt].T @ t[:mt])
    dApT = s * (x[:mt].T @ u[:mt])
    if mistake == "drop_ragged_columns":
        dBp[nout // TALL_COLS * TALL_COLS:] = 0
        dApT[nin // TALL_COLS * TALL_COLS:] = 0
    dAp = dApT.reshape(r, nin) if mistake == "dApT_untransposed" else dApT.T
    if not o.dv:
        return {"dA": dAp.contiguous(), "dB": dBp, "dU": None, "dV": None}
    dA, dB = (dAp * Vv[:r], dBp * Uv[:, 0][None, :]) if mistake == "swap_UV" else (dAp * Uv, dBp * Vv)
    dV = (dBp * B).sum(0)[torch.arange(nout) % r][:, None] if mistake == "dV_wrong_axis" else (dBp * B).sum(1, keepdim=True)
    return {"dA": dA, "dB": dB, "dU": (dApT.T * A).sum(1, keepdim=True), "dV": dV}


def mistake_applies(mistake, shape, o):
    M, nin, nout, r = shape
    return {"drop_last_split": M > 1, "drop_ragged_columns": nin % TALL_COLS != 0 or nout % TALL_COLS != 0,
            "drop_k_tail": nin % SKINNY_STEP != 0 or nout % SKINNY_STEP != 0, "dApT_untransposed": r > 1 and nin > 1,
            "gamma_off_dB": o.gamma is not None, "swap_UV": o.dv, "dV_wrong_axis": o.dv}[mistake]


def lora_autograd(o, dtype):
    """torch autograd through the reference's side product y = gamma (x A'^T B'^T s) in `dtype` -> {dA, dB, dU, dV}"""
    c = lambda t: None if t is None else t.to(dtype)
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in ((o.A, o.B, o.U, o.V) if o.dv else (o.A, o.B))]
    Ae, Be = (leaves[0] * leaves[2], leaves[1] * leaves[3]) if o.dv else leaves
    y = (c(o.x) @ Ae.T) @ Be.T * o.s
    if o.gamma is not None:
        y = y * c(o.gamma)
    grads = torch.autograd.grad(y, leaves, c(o.G))
    return dict(zip(LORA_OUTPUTS, tuple(grads) + (None, None)))


def lora_mags(o):
    """{output: (mag_outer, mag_inner)} in fp64, shaped like the outputs."""
    a = lambda t: t.double().abs()
    x, G, A, B = a(o.x), a(o.G), a(o.A), a(o.B)
    nout = B.shape[0]
    g = a(o.gamma) if o.gamma is not None else torch.ones(nout, dtype=torch.float64)
    Uv, Vv = (a(o.U), a(o.V)) if o.dv else (1.0, 1.0)
    gs = o.gamma.double() if o.gamma is not None else torch.ones(nout, dtype=torch.float64)
    Ae = o.A.double() * (o.U.double() if o.dv else 1.0)
    Bg = o.B.double() * (o.V.double() if o.dv else 1.0) * gs[:, None]
    t, u = (o.x.double() @ Ae.T).abs(), (o.G.double() @ Bg).abs()  # the exact t and u
    ti, ui = x @ Ae.abs().T, G @ Bg.abs()
    s = abs(o.s)
    dBp = [s * g[:, None] * (G.T @ q) for q in (t, ti)]
    dAp = [s * (x.T @ q).T for q in (u, ui)]                       # [r, nin]
    out = {"dA": tuple(q * Uv for q in dAp), "dB": tuple(q * Vv for q in dBp)}
    if o.dv:
        out["dU"] = tuple((q * A).sum(1, keepdim=True) for q in dAp)
        out["dV"] = tuple((q * B).sum(1, keepdim=True) for q in dBp)
    return out


def lora_depths(shape, o):
    """{output: (d_outer, d_inner)}: the roundings on the longest path through the kernels.
    inner  lora_factors_kernel (A U: 1; B V gamma: 2; a null factor multiplies by 1.f and is exact, it is counted all the same for gamma and V),
           then skinny_depth over nin (t) or nout (u)
    outer  the product y T (1), tall_depth(M), scale and rowscale (2), then the finalize: x V or x U (1 for DV-LoRA); dV adds a product and r
           additions; dU adds a product, ceil(nin / 256) additions per thread, the wave butterfly (6) and 2 to join the waves"""
    M, nin, nout, r = shape
    dv = 1 if o.dv else 0
    tall = 1 + tall_depth(M) + 2
    in_t, in_u = dv + skinny_depth(nin), 2 + skinny_depth(nout)
    d = {"dB": (tall + dv, in_t), "dA": (tall + dv, in_u)}
    if o.dv:
        d["dV"] = (tall + 1 + r, in_t)
        d["dU"] = (tall + 1 + cdiv(nin, 256) + 6 + 2, in_u)
    return d


def lora_outputs(o):
    return LORA_OUTPUTS if o.dv else LORA_OUTPUTS[:2]


@functools.lru_cache(maxsize=None)
def lora_class(cls, shape):
    """SimpleNamespace(ops, ref {fp64}, mags {(outer, inner)}, depths {(d_outer, d_inner)}, t32 {torch fp32 autograd},
    torch_err {(rms, max) of t32 over mag_inner})"""
    o = lora_operands(cls, shape)
    ref, mags, t32 = lora_autograd(o, torch.float64), lora_mags(o), lora_autograd(o, torch.float32)
    # exact_int is compared bit for bit, and dV has no terms in the rows where the sparse B is zero
    err = None if cls == "exact_int" else {n: elem_error(t32[n], ref[n], mags[n][1]) for n in lora_outputs(o)}
    return SimpleNamespace(ops=o, ref=ref, mags=mags, depths=lora_depths(shape, o), t32=t32, torch_err=err)


def lora_exact_terms(o):
    """The largest sum of absolute values of all contributing terms, nested through t and u, over every output element (int64)."""
    return max(int(m[1].max().item()) for m in lora_mags(o).values())


def fold_reference(o, dtype=torch.int64, W=None):
    """W + s (B V)(A U) in `dtype`."""
    c = lambda t: t.to(dtype)
    Ae, Be = (c(o.A) * c(o.U), c(o.B) * c(o.V)) if o.dv else (c(o.A), c(o.B))
    f = (int(o.s) if dtype == torch.int64 else o.s) * (Be @ Ae)
    return f if W is None else f + c(W)


def adjoint_directions(o, seed=90):
    """Integer directions {A, B, U, V: D shaped like the factor} with entries in -1 .. 1."""
    shapes = {"A": o.A.shape, "B": o.B.shape}
    if o.dv:
        shapes.update(U=o.U.shape, V=o.V.shape)
    d = {n: integers(sh, seed + i, 1) for i, (n, sh) in enumerate(shapes.items())}
    return {n: (nonzero(t) if t.numel() <= 8 else t) for n, t in d.items()}  # the two entries of a rank-2 U must not both be zero


# ---- edv_colsum_rows ---------------------------------------------------------------------------------------------------------------------
# (M, N) -> (rowscale, accumulate):
#   (1, 1024)      a single row at the widest N
#   (3, 4)         fewer float4s than threads
#   (2049, 4)      one float4 past a workgroup's 2048: two workgroups
#   (777, 64)      rowscale and accumulate together
#   (4100, 1)      the fold of a column vector viewed as [M / 4, 4]
#   (300000, 8)    293 workgroups
#   (1100000, 4)   538 workgroups wanted, capped at 512: a ragged ninth lap
COLSUM_SHAPES = {(1, 1024): (False, False), (3, 4): (True, False), (2049, 4): (False, True), (777, 64): (True, True), (4100, 1): (False, True),
                 (300000, 8): (True, False), (1100000, 4): (False, False)}


def colsum_geometry(M, N):
    """(workgroups, laps of the grid-stride loop, float4s, float4s per row) of colsum_rows."""
    if N == 1:
        M, N = M // 4, 4
    n4 = N // 4
    total4 = M * n4
    blocks = min(max(cdiv(total4, COLSUM_F4_PER_WG), 1), COLSUM_BLOCKS)
    return blocks, cdiv(total4, blocks * 256), total4, n4


def colsum_wanted(M, N):
    return cdiv((M // 4 if N == 1 else M) * (1 if N == 1 else N // 4), COLSUM_F4_PER_WG)


def colsum_depth(M, N):
    """A product with the row scale, one addition per lap, 256 / n4 additions of the threads that share a column group, ceil(blocks / 8)
    partials in sequence and 7 to join the slices, 2 for the fold, 1 to accumulate."""
    rs, acc = COLSUM_SHAPES[(M, N)]
    blocks, laps, _, n4 = colsum_geometry(M, N)
    return int(rs) + laps + 256 // n4 + cdiv(blocks, REDUCE_SLICES) + 7 + (2 if N == 1 else 0) + int(acc)


def colsum_has_class(cls, shape):
    return cls != "cancelling" or shape[0] % 2 == 0


def colsum_cases(classes):
    return [(cls, shape) for cls in classes for shape in COLSUM_SHAPES if colsum_has_class(cls, shape)]


def colsum_tail_rows(M, N):
    """The rows the ragged last lap of the grid-stride loop reads (all rows where there is one lap only)."""
    blocks, laps, total4, n4 = colsum_geometry(M, N)
    first4 = (laps - 1) * blocks * 256
    return slice((first4 // n4) * (4 if N == 1 else 1), M)


def _class_matrix(cls, M, N, Mq, seed, tail):
    """P [M, N] and Q [M, Mq] (a row scale: Mq = 1) of a class; the class sits on P, and on Q where the issue puts it on both operands."""
    if cls == "exact_int":
        return integers((M, N), seed, 4), integers((M, Mq), seed + 1, 3)
    if cls == "scaled":
        return bounded((M, N), 20 + seed), bounded((M, Mq), 21 + seed)
    P, Q = uniform((M, N), seed), uniform((M, Mq), seed + 1) + (1.5 if Mq == 1 else 0.0)
    if cls == "outlier_ch":
        P = outlier_channels(P, outlier_indices(N))
        Q = outlier_channels(Q, outlier_indices(N)) if Mq == N else Q
    elif cls == "lognormal":
        P = P * row_factors(M, 13)
    elif cls == "offset":
        P, Q = 5.0 + P, (5.0 + Q if Mq == N else Q)
    elif cls == "cancelling":
        Q, P = mirror_rows(Q, P)
    elif cls == "last_split_only":
        keep = torch.zeros(M, 1)
        keep[tail] = 1
        P = P * keep
    else:
        raise KeyError(cls)
    return P, Q


def _colsum_apply(P, rs, base, fold, dtype):
    v = P.to(dtype) * rs.to(dtype) if rs is not None else P.to(dtype)
    v = v.sum().reshape(1) if fold else v.sum(0)
    return v if base is None else v + base.to(dtype)


@functools.lru_cache(maxsize=None)
def colsum_class(cls, shape):
    """SimpleNamespace(P [M, N], rs [M, 1] or None, base [N] or None, ref, mag, depth, torch_err)"""
    M, N = shape
    use_rs, acc = COLSUM_SHAPES[shape]
    P, rs = _class_matrix(cls, M, N, 1, 1, colsum_tail_rows(M, N))
    base = {"exact_int": integers((N,), 3, 16), "scaled": bounded((N,), 23)}.get(cls, uniform((N,), 3))
    if cls == "cancelling":
        base = base * 2.0 ** -20  # small enough that the output stays the difference of the two halves
    rs, base = (rs if use_rs else None), (base if acc else None)
    ref, t32 = _colsum_apply(P, rs, base, N == 1, torch.float64), _colsum_apply(P, rs, base, N == 1, torch.float32)
    mag = _colsum_apply(P.abs(), None if rs is None else rs.abs(), None if base is None else base.abs(), N == 1, torch.float64)
    return SimpleNamespace(P=P, rs=rs, base=base, ref=ref, mag=mag, depth=colsum_depth(M, N), t32=t32, torch_err=class_error(cls, t32, ref, mag))


def colsum_scaled(shape, p):
    c = colsum_class("scaled", shape)
    return c.P * 2.0 ** p, c.rs, (None if c.base is None else c.base * 2.0 ** p)


# ---- edv_col_dot -------------------------------------------------------------------------------------------------------------------------
COLDOT_SHAPES = ((1, 1), (65, 65), (1000, 384), (10960, 8))
COLDOT_VARIANTS = ((False, False), (True, False), (False, True), (True, True))  # (Q, scale)


def coldot_depth(M, use_q, use_s):
    """test_col_dot's count: tall_depth, one rounding for the product, one for the scale."""
    return tall_depth(M) + int(use_q) + int(use_s)


def coldot_cases(classes):
    return [(cls, shape) for cls in classes for shape in COLDOT_SHAPES if colsum_has_class(cls, shape)]


@functools.lru_cache(maxsize=None)
def coldot_operands(cls, shape):
    """(P [M, N], Q [M, N], scale [N])"""
    M, N = shape
    P, Q = _class_matrix(cls, M, N, N, 1, last_split_rows(M))
    scale = choice((1, 2, -1, 4), N, 3) if cls == "exact_int" else uniform((N,), 3) + 1.5
    return P, Q, scale


def _coldot_apply(P, Q, scale, dtype):
    v = (P.to(dtype) * Q.to(dtype) if Q is not None else P.to(dtype)).sum(0)
    return v if scale is None else v * scale.to(dtype)


@functools.lru_cache(maxsize=None)
def coldot_class(cls, shape, use_q, use_s):
    """SimpleNamespace(P, Q or None, scale or None, ref, mag, depth, torch_err)"""
    P, Q, scale = coldot_operands(cls, shape)
    Q, scale = (Q if use_q else None), (scale if use_s else None)
    ref, t32 = _coldot_apply(P, Q, scale, torch.float64), _coldot_apply(P, Q, scale, torch.float32)
    mag = _coldot_apply(P.abs(), None if Q is None else Q.abs(), None if scale is None else scale.abs(), torch.float64)
    return SimpleNamespace(P=P, Q=Q, scale=scale, ref=ref, mag=mag, depth=coldot_depth(shape[0], use_q, use_s), t32=t32,
                           torch_err=class_error(cls, t32, ref, mag))


# ---- edv_colsum_batch --------------------------------------------------------------------------------------------------------------------
# One batch built like test_batched_colsum_kernel's: ragged row counts, ld > N, job 4 on the patch RowMap (20 patch rows after one cls row of
# 21-row frames), scale on jobs 1 and 4, accumulate on the even jobs.  (N, rows); rows even, so that every job has every class.
BATCH_JOBS = ((1, 10960), (3, 1530), (48, 3652), (384, 778), (1152, 2180), (1536, 322), (2048, 1564))
PATCH_ROWS, PATCH_NTOK = 20, 21


def batch_job(k):
    """dict(N, M, ld, map (period, stride, offset), phys (physical rows), rows (index of the logical rows), scale, acc)"""
    N, M = BATCH_JOBS[k]
    j = dict(N=N, M=M, ld=N + (k % 3), scale=(k % 3 == 1), acc=(k % 2 == 0), map=(0, 0, 0), phys=M, rows=torch.arange(M))
    if k == 4:
        frames = M // PATCH_ROWS
        assert frames * PATCH_ROWS == M
        j.update(map=(PATCH_ROWS, PATCH_NTOK, 1), phys=frames * PATCH_NTOK,
                 rows=torch.cat([torch.arange(f * PATCH_NTOK + 1, f * PATCH_NTOK + 1 + PATCH_ROWS) for f in range(frames)]))
    return j


def batch_plan(M, N):
    """(parts, chunk, row lanes) of colsum_job."""
    parts = min(max(cdiv(M * N, CS_ELEMS), 1), CS_MAX_PARTS, M)
    chunk = cdiv(M, parts)
    return cdiv(M, chunk), chunk, 256 >> min(max(N - 1, 0).bit_length(), 8)


def batch_depth(k):
    """Stage 1: a row lane walks ceil(chunk / lanes) rows on four accumulators (a quarter each, up to 3 leftovers on the first), fp64 additions join
    them and the row lanes in fp64, rounded once (1); stage 2 adds the parts in sequence; one rounding for the scale, one to accumulate."""
    j = batch_job(k)
    parts, chunk, lanes = batch_plan(j["M"], j["N"])
    return cdiv(cdiv(chunk, lanes), 4) + 3 + 1 + parts + int(j["scale"]) + int(j["acc"])


def batch_tail_rows(k):
    j = batch_job(k)
    parts, chunk, _ = batch_plan(j["M"], j["N"])
    return slice((parts - 1) * chunk, j["M"])


@functools.lru_cache(maxsize=None)
def batch_class(cls, k):
    """SimpleNamespace(job, src [phys, ld] (NaN wherever the job must not read), sc [N] or None, init [N] or None, ref, mag, depth, torch_err)"""
    j = batch_job(k)
    N, M = j["N"], j["M"]
    P, _ = _class_matrix(cls, M, N, 1, 30 + k, batch_tail_rows(k))
    sc = (choice((1, 2, -1, 4), N, 40 + k) if cls == "exact_int" else uniform((N,), 40 + k) + 1.25) if j["scale"] else None
    init = {"exact_int": integers((N,), 50 + k, 16), "scaled": bounded((N,), 50 + k)}.get(cls, uniform((N,), 50 + k)) if j["acc"] else None
    if cls == "cancelling" and init is not None:
        init = init * 2.0 ** -20
    src = torch.full((j["phys"], j["ld"]), float("nan"))
    src[j["rows"], :N] = P

    def apply(P, sc, init, dtype):
        v = P.to(dtype).sum(0)
        v = v if sc is None else v * sc.to(dtype)
        return v if init is None else v + init.to(dtype)

    ref, t32 = apply(P, sc, init, torch.float64), apply(P, sc, init, torch.float32)
    mag = apply(P.abs(), None if sc is None else sc.abs(), None if init is None else init.abs(), torch.float64)
    return SimpleNamespace(job=j, P=P, src=src, sc=sc, init=init, ref=ref, mag=mag, depth=batch_depth(k), t32=t32,
                           torch_err=class_error(cls, t32, ref, mag))
