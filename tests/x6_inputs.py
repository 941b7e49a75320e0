"""Edge-case operands for the bf16 x 6 kernels (gemm_x6.hip, attn_x6_kernel), shared by tests/test_x6_inputs_cpu.py and tests/test_x6_edges_gpu.py,
and a CPU emulation of the two GEMM constructions.

The emulations have the kernels' arithmetic -- the three-term bf16 split, exact bf16 x bf16 products, fp32 accumulation -- but NOT their summation
order: `emulate_x6` rounds to fp32 once per 16-k block and plane pair (the MFMA's internal order over its 16 k is not modelled, a tile's k range is
never cut into stream-K pieces), `emulate_f32` once per 2 k.  They say whether an input class is inside the construction's domain; they do not predict
the kernels' bits.

Everything here is seeded and returns fp32 CPU tensors."""
import functools

import torch

U = 2.0 ** -24            # fp32 unit roundoff
FP32_MIN_NORMAL = 2.0 ** -126


def uniform(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def bounded(shape, seed, scale=1.0):
    """sign x uniform(2^-4, 1) x scale: bounded away from zero, so that scaling by a power of two moves every split term and every product by
    exactly that power (none of them drops under 2^-126 unless all do)."""
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** -4 + torch.rand(*shape, generator=g) * (1 - 2.0 ** -4)
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    return sign * mag * scale


def outlier_channels(A, cols, factor=1e3):
    """A copy of A with the k-columns `cols` scaled by `factor` (outlier channels of a residual stream)."""
    A = A.clone()
    A[:, list(cols)] *= factor
    return A


def lognormal(shape, seed, sigma=2.0):
    """normal x exp(sigma normal): heavy-tailed, a few entries carry most of every dot product."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * torch.exp(sigma * torch.randn(*shape, generator=g))


def cancelling(A, W, seed=77):
    """The second half of k mirrors the first: A[:, h:] = -A[:, :h], W[:, h:] = W[:, :h] (1 + 2^-12 r), r uniform in (-1, 1).  A W^T is then
    about 2^-12 / sqrt(K) of sum |a w|: every output is the small difference of two large sums."""
    A, W = A.clone(), W.clone()
    h = A.shape[1] // 2
    A[:, h:2 * h] = -A[:, :h]
    W[:, h:2 * h] = W[:, :h] * (1 + 2.0 ** -12 * uniform((W.shape[0], h), seed))
    return A, W


def split3(x):
    """The kernels' split: p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), as fp32 tensors (torch's conversion keeps bf16 subnormals)."""
    p0 = x.to(torch.bfloat16).float()
    r1 = x - p0
    p1 = r1.to(torch.bfloat16).float()
    p2 = (r1 - p1).to(torch.bfloat16).float()
    return p0, p1, p2


KEPT = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))  # (A plane, W plane) of the six kept products, smallest terms first


def emulate_x6(A, W, kb=16):
    a, w = [p.double() for p in split3(A)], [p.double() for p in split3(W)]
    acc = torch.zeros(A.shape[0], W.shape[0])
    for k0 in range(0, A.shape[1], kb):
        for pa, pb in KEPT:
            acc = acc + (a[pa][:, k0:k0 + kb] @ w[pb][:, k0:k0 + kb].T).float()
    return acc


def emulate_f32(A, W, kb=2):
    Ad, Wd = A.double(), W.double()
    acc = torch.zeros(A.shape[0], W.shape[0])
    for k0 in range(0, A.shape[1], kb):
        acc = acc + (Ad[:, k0:k0 + kb] @ Wd[:, k0:k0 + kb].T).float()
    return acc


def gemm_reference(A, W):
    """(A W^T, |A| |W|^T) in fp64: the reference and the yardstick a dot product's rounding is judged by."""
    return A.double() @ W.double().T, A.double().abs() @ W.double().abs().T


def rel_error(C, ref, mag):
    """Per element |C - ref| / sum_k |a_k w_k| -> (rms, max)."""
    assert (mag > 0).all()
    e = (C.double().cpu() - ref).abs() / mag
    return e.pow(2).mean().sqrt().item(), e.max().item()


def gemm_gate_failures(rms6, max6, rms32, max32, K):
    """The gates of the edge-operand accuracy tests, as a list of what failed: the project's own margins against the fp32 path on the same
    operands, and the classical bound K u on any length-K fp32 dot product for both."""
    bad = []
    if not rms6 <= 1.05 * rms32:
        bad.append(f"rms6 {rms6 / U:.3f}u > 1.05 x rms32 {rms32 / U:.3f}u")
    if not max6 <= max(1.25 * max32, 4 * U):
        bad.append(f"max6 {max6 / U:.3f}u > max(1.25 x max32 {max32 / U:.3f}u, 4u)")
    if not max6 <= K * U:
        bad.append(f"max6 {max6 / U:.3f}u > K u")
    if not max32 <= K * U:
        bad.append(f"max32 {max32 / U:.3f}u > K u")
    return bad


# ---- the GEMM cases ---------------------------------------------------------------------------------------------------------------------
# (600, 512, 768): 5 x 4 = 20 tiles of 48 k-steps -- with a workspace gemm_x6_split_policy (min_kt 48, min_tiles 16) cuts every tile along k, without
# one the plain grid runs; (257, 200, 64): ragged M and N, 4 k-steps, plain grid only.  test_x6_inputs_cpu.py confirms both with edv_split_plan.
GEMM_SHAPES = ((600, 512, 768), (257, 200, 64))
GEMM_CLASSES = ("outlier_A", "outlier_AW", "lognormal_A", "cancelling", "A_2p100", "A_2m100", "W_2m100")
BITWISE_SCALES = (40, -40)  # exponents the GPU tests assert bit for bit


def gemm_base(M, N, K):
    """The operands of test_gemm_x6_is_as_accurate_as_the_fp32_pipe: |a| < 2, |w| < 0.05."""
    return uniform((M, K), 11, 2.0), uniform((N, K), 12, 0.05)


def gemm_bounded(M, N, K):
    return bounded((M, K), 21, 2.0), bounded((N, K), 22, 0.05)


@functools.lru_cache(maxsize=None)
def gemm_class(name, M, N, K):
    """(A, W, ref, mag) of one input class; computed once per process and shared: do not write to them."""
    A, W = gemm_base(M, N, K)
    if name == "outlier_A":
        A = outlier_channels(A, (5, K // 2 + 3, K - 4))
    elif name == "outlier_AW":
        A = outlier_channels(A, (5, K // 2 + 3, K - 4))
        W = outlier_channels(W, (7, K // 3))
    elif name == "lognormal_A":
        A = lognormal((M, K), 13)
    elif name == "cancelling":
        A, W = cancelling(A, W)
    elif name == "A_2p100":
        A = A * 2.0 ** 100
    elif name == "A_2m100":
        A = A * 2.0 ** -100
    elif name == "W_2m100":
        W = W * 2.0 ** -100
    else:
        raise KeyError(name)
    return (A, W) + gemm_reference(A, W)


# ---- the attention cases ----------------------------------------------------------------------------------------------------------------
# (frames, tokens, heads).  The bf16 x 6 kernel takes 256 queries and 64 keys per step: (2, 321, 2) has a ragged second query block and a ragged
# last key tile, 8 tasks, all split by keys; (1, 257, 1) one query in its second block; (3, 300, 43) 258 tasks on the 256 workgroups an MI355X keeps
# resident (one per CU), one whole round plus two tasks split by keys.  test_x6_inputs_cpu.py confirms the plans.
ATTN_SHAPES = ((2, 321, 2), (1, 257, 1), (3, 300, 43))
ATTN_CLASSES = ("qk_outlier", "v_outlier", "shifted", "v_2p100", "v_2m100", "q_2m100")
HD = 64


def attn_views(qkv, heads):
    """q, k, v as views [rows, heads, 64] of a q | k | v matrix [rows, 3 heads 64] (columns ordered [3][heads][64])."""
    t = qkv.view(qkv.shape[0], 3, heads, HD)
    return t[:, 0], t[:, 1], t[:, 2]


def attn_reference(qkv, Fr, N, heads, dtype=torch.float64):
    """reference() of tests/test_attn_x6_gpu.py, in `dtype`."""
    t = qkv.to(dtype).reshape(Fr, N, 3, heads, HD).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * HD ** -0.5, t[1], t[2]
    return ((q @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(Fr * N, heads * HD)


def column_error(o, ref):
    """Per element |o - ref| / max over rows of |ref[:, c]| -> (rms, max).  Per COLUMN: with one v channel scaled by 1e3 a normalisation by the global
    maximum would hide a thousandfold error in the head's other 63 columns."""
    e = (o.double().cpu() - ref).abs() / ref.abs().amax(0, keepdim=True)
    return e.pow(2).mean().sqrt().item(), e.max().item()


@functools.lru_cache(maxsize=None)
def attn_class(name, Fr, N, heads):
    """(qkv, fp64 reference, (rms, max) column error of torch's fp32 attention on the CPU against it); computed once and shared."""
    qkv = uniform((Fr * N, 3 * heads * HD), 3, 2.0)
    q, k, v = attn_views(qkv, heads)
    if name == "qk_outlier":      # scores reach +-60, the rows are peaked
        for d in (3, 40):
            q[:, :, d] *= 8
            k[:, :, d] *= 8
    elif name == "v_outlier":
        v[:, :, 5] *= 1e3
    elif name == "shifted":
        # every query gets a common component (q += 1), and k = k0 + c qbar with qbar the mean query of the (frame, head): the scores of query i
        # all carry the offset c q_i . qbar / 8 = c (64 +- 9) / 8, about 500 for c = 62.5 -- softmax does not see it, fp32 scores lose 2^-15 to it
        q += 1.0
        qbar = q.reshape(Fr, N, heads, HD).mean(1, keepdim=True)
        k += (62.5 * qbar).expand(Fr, N, heads, HD).reshape(Fr * N, heads, HD)
    elif name == "v_2p100":
        v *= 2.0 ** 100
    elif name == "v_2m100":
        v *= 2.0 ** -100
    elif name == "q_2m100":       # every score is 0 to fp32: uniform softmax
        q *= 2.0 ** -100
    else:
        raise KeyError(name)
    ref = attn_reference(qkv, Fr, N, heads)
    return qkv, ref, column_error(attn_reference(qkv, Fr, N, heads, torch.float32), ref)


def attn_gate_failures(rms6, max6, rms32, max32, max_torch):
    """The project's margins against the fp32 kernel on the same q | k | v, and for both kernels at most 4 x the error of the same attention
    evaluated by torch in fp32 (the exp2 pre-scaling and the tile-wise online rescale each add a few roundings per element)."""
    bad = []
    if not rms6 <= 1.10 * rms32:
        bad.append(f"rms6 {rms6:.3e} > 1.10 x rms32 {rms32:.3e}")
    if not max6 <= max(1.5 * max32, 1e-6):
        bad.append(f"max6 {max6:.3e} > max(1.5 x max32 {max32:.3e}, 1e-6)")
    if not max6 <= 4 * max_torch:
        bad.append(f"max6 {max6:.3e} > 4 x torch fp32 {max_torch:.3e}")
    if not max32 <= 4 * max_torch:
        bad.append(f"max32 {max32:.3e} > 4 x torch fp32 {max_torch:.3e}")
    return bad
