"""Exact-integer and numeric-edge operands, fp64 references and the per-element yardstick for the convolution family (conv_dma.hip, conv_halo.hip,
the LOAD_CONV3 loader of gemm.hip, wgrad.hip and the convolution kernels of bwd.hip), shared by tests/test_conv_inputs_cpu.py and
tests/test_conv_edges_gpu.py.  The generators are those of tests/x6_inputs.py, the gates those of tests/edge_inputs.py.

Everything is seeded, works on CPU tensors in torch's own layout (NCHW activations, [Cout, Cin, 3, 3] weights) and is computed once per process
(functools.lru_cache: do not write to what these functions return).  References and yardsticks come back channels-last, as the kernels store.

The yardstick is per element, never global: |y - ref| / mag with mag = sum |x| |w| + |bias| + |R1| + |R2| over THAT element's own taps (the same
torch op in fp64 on the absolute values), so a border pixel with four live taps is judged by four taps' worth of products."""
import functools

import torch
import torch.nn.functional as F

from .edge_inputs import MARGIN, bits, gate_failures, ratios, rms_max  # noqa: F401
from .x6_inputs import BITWISE_SCALES, U, bounded, lognormal, uniform  # noqa: F401

FLOOR = 4 * U  # the bias add, the two residual adds and the final rounding
EXACT_LIMIT = 2 ** 24

# ---- routes ------------------------------------------------------------------------------------------------------------------------------
# An entry point, a dispatch setting and the smallest shape that still reaches the kernel variant with ragged tiles.
# Forward shapes: (F, H, W, Cin, Cout, stride).
FWD_ROUTES = {
    "dma64": ((2, 9, 11, 64, 48, 1),),           # conv3_dma_kernel<2> plain: 198 pixels = 4 row tiles, the last of 6 rows; 48 of 64 columns
    "dma64_s2": ((2, 13, 10, 96, 80, 2),),       # stride 2, even W: 7 x 5 outputs, two column tiles
    "dma64_split": ((3, 19, 19, 64, 64, 1), (3, 19, 19, 192, 64, 1)),  # stream-K: 17 tiles x 18 / 54 k-tiles
    "dma128": ((2, 9, 17, 32, 32, 1), (1, 13, 11, 64, 8, 1)),          # conv3_dma_kernel<4>; Cout 8: 24 of a wave's 32 column lanes idle
    "dma128_split": ((6, 19, 19, 64, 32, 1),),   # 2166 pixels = 17 tiles of 128 rows x 18 k-tiles
    "halo": ((3, 9, 17, 32, 32, 1), (1, 40, 33, 64, 8, 1)),            # conv3_halo_kernel<1> / <2>: one pixel past an 8 x 16 patch both ways
    "reg": ((2, 19, 23, 48, 64, 1), (2, 9, 11, 48, 48, 2), (2, 5, 7, 16, 32, 1), (2, 11, 7, 4, 8, 1)),  # LOAD_CONV3 of gemm.hip: Cin % 32 != 0
}
DOT_SHAPES = FWD_ROUTES["halo"]                  # edv_conv3x3_dot on the halo kernel and, with EDV_CONV_HALO=0, on conv3_dma_kernel<4, 8 + act>
DOT_KERNELS = ("halo", "dma")
BWD_DATA_SHAPES = ((1, 9, 11, 48, 64), (1, 5, 6, 32, 4))  # (F, H, W, Cin, Cout): contracts over Cout = 64 (DMA loader) / 4 (register loader)
S2_BWD_SHAPES = ((2, 19, 19, 64), (1, 16, 20, 32), (1, 7, 10, 32), (1, 4, 5, 8))  # (F, H, W, C)
WGRAD_SHAPES = ((2, 9, 12, 32, 32, False), (3, 20, 26, 32, 32, False), (1, 6, 8, 48, 20, True), (2, 11, 7, 4, 8, False))  # (..., accumulate)
CONVT_SHAPES = ((1, 3, 4, 32, 4), (2, 5, 6, 96, 2))  # (F, h, w, C, s)

# name -> (pre_relu, post_relu, residuals): v = conv(relu?(x)) + bias; v = relu?(v); v += R1 + R2
EPILOGUES = {"bias": (0, 0, 0), "post": (0, 1, 0), "rcu": (1, 0, 2), "pre_post_r1": (1, 1, 1)}
DOT_EPILOGUES = ("bias", "post")                 # conv_dot_supported: no residual; conv_halo_supported admits all four
DOT_ACT2 = {"none": 0, "relu": 2}

ACCURACY_CLASSES = ("outlier_ch", "lognormal", "cancelling", "offset_1e3")
CLASSES = ("exact_int",) + ACCURACY_CLASSES + ("scaled",)


# The dispatch these shapes rely on, restated from gemm.hip (gemm), conv_dma.hip (conv_dma, launch_conv_ep, conv_dma_split_policy) and
# conv_halo.hip (conv_halo_supported, conv_halo_pays); tests/test_conv_inputs_cpu.py checks the table above against it.
CBK = 32                       # channels per k-tile of conv3_dma_kernel
CONV_SLOTS = 1024              # resident workgroups: 4 per CU on 256 CUs (conv_slots)
HALO_TH, HALO_TW = 8, 16       # output patch of conv3_halo_kernel
HALO_PAYS_TILES = 4096         # automatic mode sends fewer patches to conv3_dma_kernel


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def takes_dma_loader(Cin):
    return Cin % CBK == 0


def dma_tile(Cout):
    """(rows, columns) of a tile: conv3_dma_kernel<4> for Cout <= 32, <2> otherwise."""
    return (128, 32) if Cout <= 32 else (64, 64)


def dma_tiles(shape):
    """(tiles, k-tiles) of a shape on conv3_dma_kernel."""
    Fr, H, W, Cin, Cout, stride = shape
    OH, OW = out_hw(H, W, stride)
    bm, bn = dma_tile(Cout)
    return -(-(Fr * OH * OW) // bm) * -(-Cout // bn), 9 * Cin // CBK


def halo_supported(shape):
    Fr, H, W, Cin, Cout, stride = shape
    return stride == 1 and Cin in (32, 64) and Cout <= 32


def halo_patches(shape):
    Fr, H, W = shape[:3]
    return Fr * -(-H // HALO_TH) * -(-W // HALO_TW)


def halo_in_automatic_mode(shape):
    return halo_supported(shape) and halo_patches(shape) >= HALO_PAYS_TILES


def wgrad_pieces(Fr, H, Cin, Cout):
    """n_rc of wgrad_plan (wgrad.hip): the workspace pieces conv3_wgrad_reduce_kernel adds per element."""
    cdiv = lambda a, b: -(-a // b)
    n_cg, n_cb = cdiv(cdiv(9 * Cin, 32), 3), cdiv(Cout, 32)
    rpt = max(cdiv(Fr * H, max(4096 // (n_cg * n_cb), 1)), 1)
    return cdiv(Fr * H, rpt)


def fwd_cases():
    """[(route, shape, admitted epilogues)] in table order."""
    return [(route, shape, tuple(EPILOGUES)) for route, shapes in FWD_ROUTES.items() for shape in shapes]


def cycled_epilogue(case_index, cls, admitted=tuple(EPILOGUES)):
    """The epilogue a (case, class) pair runs: the cases cycle through the admitted ones, every class starts the cycle one further."""
    return admitted[(case_index + CLASSES.index(cls)) % len(admitted)]


# ---- generators --------------------------------------------------------------------------------------------------------------------------
def integers(shape, seed, bound):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, tuple(shape), generator=g).float()


def outlier_indices(C):
    """5, C / 2 + 3 and C - 4, folded into range for C = 4 and 16."""
    return sorted({5 % C, (C // 2 + 3) % C, C - 4})


def nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous()


def _mirror(x, w, pre, seed=77):
    """The second half of the input channels mirrors the first: x[:, h:2h] = -x[:, :h], w[:, h:2h] = w[:, :h] (1 + 2^-12 r).  Under pre_relu the
    sign moves to the weight (x[:, h:2h] = x[:, :h], w[:, h:2h] = -w[:, :h] (1 + 2^-12 r)): relu(-x) would not mirror relu(x).

    What is left of an output is a sum of n = 9 h products t r 2^-12 against mag = 2 sum |t|: for uniform operands its median is
    0.67 x 0.58 x 2^-12 x (rms t / mean |t| = 4 / 3) / (2 sqrt n) = 6.3e-5 / sqrt n of mag, and a pre_relu halves n.  That is 5e-6 at 32 channels
    but 1.5e-5 at 16 channels under pre_relu and at 4 channels: below 32 channels the perturbation is 2^-14, so that every shape stays under the
    1e-5 that tests/test_conv_inputs_cpu.py requires of the class."""
    x, w = x.clone(), w.clone()
    h = x.shape[1] // 2
    r = 1 + (2.0 ** -12 if x.shape[1] >= 32 else 2.0 ** -14) * uniform((w.shape[0], h, 3, 3), seed)
    x[:, h:2 * h] = x[:, :h] if pre else -x[:, :h]
    w[:, h:2 * h] = (-w[:, :h] if pre else w[:, :h]) * r
    return x, w


def _class_x(cls, shape_nchw, seed=1):
    """The activation operand of an accuracy class (before any mirroring)."""
    C = shape_nchw[1]
    if cls == "outlier_ch":
        x = uniform(shape_nchw, seed)
        x[:, outlier_indices(C)] *= 1e3
        return x
    if cls == "lognormal":
        return lognormal(shape_nchw, 13)
    if cls == "offset_1e3":
        return 1000.0 + uniform(shape_nchw, seed, 0.03)
    if cls == "cancelling":
        return uniform(shape_nchw, seed)
    raise KeyError(cls)


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_operands(cls, shape, ep):
    """(x [F, Cin, H, W], w [Cout, Cin, 3, 3], bias or None, R1 or None, R2 or None), residuals shaped like the output [F, Cout, OH, OW]."""
    Fr, H, W, Cin, Cout, stride = shape
    pre, post, res = EPILOGUES[ep]
    OH, OW = out_hw(H, W, stride)
    xs, ws, rs = (Fr, Cin, H, W), (Cout, Cin, 3, 3), (Fr, Cout, OH, OW)
    if cls == "exact_int":
        x, w, b = integers(xs, 1, 8), integers(ws, 2, 4), integers((Cout,), 3, 16)
        R = [integers(rs, 4 + i, 16) for i in range(res)]
    elif cls == "scaled":
        x, w, b = bounded(xs, 21, 2.0), bounded(ws, 22, 0.05), None
        R = [bounded(rs, 24 + i) for i in range(res)]
    else:
        x, w, b = _class_x(cls, xs), uniform(ws, 2, (9 * Cin) ** -0.5), uniform((Cout,), 3, 0.1)
        R = [uniform(rs, 4 + i) for i in range(res)]
        if cls == "cancelling":  # bias 0, and residuals small enough that the output stays the difference of the two sums
            x, w = _mirror(x, w, pre)
            b, R = None, [r * 2.0 ** -20 for r in R]
    return (x, w, b) + tuple(R + [None, None])[:2]


def fwd_apply(x, w, b, R1, R2, ep, stride, dtype):
    """The convolution and its epilogue in `dtype`, channels-last."""
    pre, post, _ = EPILOGUES[ep]
    c = lambda t: None if t is None else t.to(dtype)
    y = F.conv2d(F.relu(c(x)) if pre else c(x), c(w), c(b), stride=stride, padding=1)
    if post:
        y = F.relu(y)
    for r in (R1, R2):
        if r is not None:
            y = y + c(r)
    return nhwc(y)


def fwd_mag(x, w, b, R1, R2, ep, stride):
    pre = EPILOGUES[ep][0]
    a = lambda t: None if t is None else t.double().abs()
    m = F.conv2d(F.relu(x).double() if pre else a(x), a(w), a(b), stride=stride, padding=1)
    for r in (R1, R2):
        if r is not None:
            m = m + a(r)
    return nhwc(m)


def elem_error(y, ref, mag):
    """Per element |y - ref| / mag -> (rms, max); mag must be positive everywhere."""
    assert (mag > 0).all()
    return rms_max((y.double().cpu() - ref).abs() / mag)


@functools.lru_cache(maxsize=None)
def fwd_reference(cls, shape, ep):
    """(fp64 reference [F, OH, OW, Cout], mag, (rms, max) of torch's fp32 convolution on the CPU under the yardstick)"""
    ops, stride = fwd_operands(cls, shape, ep), shape[5]
    ref, mag = fwd_apply(*ops, ep, stride, torch.float64), fwd_mag(*ops, ep, stride)
    return ref, mag, elem_error(fwd_apply(*ops, ep, stride, torch.float32), ref, mag)


def fwd_exact_bound(shape, ep):
    """The largest |partial sum| any summation order can meet on the exact_int operands: 9 Cin x 8 x 4 + 16 (bias) + 16 per residual."""
    return 9 * shape[3] * 32 + 16 * (1 + EPILOGUES[ep][2])


def fwd_scaled(shape, ep, px, pw):
    """The `scaled` operands with x 2^px and w 2^pw; the residuals follow the product (2^(px + pw))."""
    x, w, b, R1, R2 = fwd_operands("scaled", shape, ep)
    s = lambda t, p: None if t is None else t * 2.0 ** p
    return s(x, px), s(w, pw), b, s(R1, px + pw), s(R2, px + pw)


# ---- the fused 1x1 to one channel --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dot_operands(cls, shape, ep):
    """fwd_operands plus (w2 [Cout], b2 [1])."""
    Cout = shape[4]
    if cls == "exact_int":
        w2, b2 = integers((Cout,), 6, 2), integers((1,), 7, 16)
    elif cls == "scaled":
        w2, b2 = bounded((Cout,), 26, 1.5), None
    else:
        w2, b2 = uniform((Cout,), 6, 1.5), (None if cls == "cancelling" else uniform((1,), 7, 0.3))
    return fwd_operands(cls, shape, ep) + (w2, b2)


def dot_apply(ops, ep, act2, dtype):
    x, w, b, R1, R2, w2, b2 = ops
    z = (fwd_apply(x, w, b, None, None, ep, 1, dtype) * w2.to(dtype)).sum(-1)
    if b2 is not None:
        z = z + b2.to(dtype)
    return F.relu(z) if act2 == "relu" else z


def dot_mag(ops, ep):
    """sum_c |w2[c]| (sum |x| |w| + |bias|)[c] + |b2|: the products of the whole chain, per pixel."""
    x, w, b, R1, R2, w2, b2 = ops
    m = (fwd_mag(x, w, b, None, None, ep, 1) * w2.double().abs()).sum(-1)
    return m if b2 is None else m + b2.double().abs()


@functools.lru_cache(maxsize=None)
def dot_reference(cls, shape, ep, act2):
    """(fp64 reference [F, H, W], mag, torch fp32's (rms, max))"""
    ops = dot_operands(cls, shape, ep)
    ref, mag = dot_apply(ops, ep, act2, torch.float64), dot_mag(ops, ep)
    return ref, mag, elem_error(dot_apply(ops, ep, act2, torch.float32), ref, mag)


def dot_exact_bound(shape):
    """|conv + bias| <= 9 Cin 32 + 16, times |w2| <= 2, over Cout channels, plus |b2| <= 16: about 1.2e6 at 64 -> 8 and 5.9e5 at 32 -> 32."""
    return (9 * shape[3] * 32 + 16) * 2 * shape[4] + 16


def dot_terms(shape):
    """Hard bound of the chain in u: (9 Cin + 4) for every convolution output, then test_conv_halo_gpu.dot_bound's 33 for a 32-term sum plus b2."""
    return 9 * shape[3] + 4 + 33


# ---- input gradients ---------------------------------------------------------------------------------------------------------------------
def _grad_x(dy, w, stride, H, W, dtype):
    """d conv2d(x, w, stride, padding 1) / dx for x [F, Cin, H, W]: the transposed convolution of dy."""
    OH, OW = out_hw(H, W, stride)
    op = (H - ((OH - 1) * stride + 1), W - ((OW - 1) * stride + 1))
    return F.conv_transpose2d(dy.to(dtype), w.to(dtype), None, stride=stride, padding=1, output_padding=op)


@functools.lru_cache(maxsize=None)
def bwd_data_class(cls, shape, stride=1):
    """(dy [F, Cout, OH, OW], w [Cout, Cin, 3, 3], fp64 dx [F, H, W, Cin], mag, torch fp32's (rms, max)).  The class sits on dy, the operand the
    kernel contracts over (Cout channels)."""
    Fr, H, W, Cin, Cout = shape
    OH, OW = out_hw(H, W, stride)
    ds, ws = (Fr, Cout, OH, OW), (Cout, Cin, 3, 3)
    if cls == "exact_int":
        dy, w = integers(ds, 3, 4), integers(ws, 2, 4)
    else:
        dy, w = _class_x(cls, ds, 3), uniform(ws, 2, 0.1)
        if cls == "cancelling":  # the contraction runs over Cout: mirror dy's channels and the weight's OUTPUT channels
            dy, wt = _mirror(dy, w.transpose(0, 1), False)
            w = wt.transpose(0, 1).contiguous()
    ref = nhwc(_grad_x(dy, w, stride, H, W, torch.float64))
    mag = nhwc(_grad_x(dy.abs(), w.abs(), stride, H, W, torch.float64))
    return dy, w, ref, mag, elem_error(nhwc(_grad_x(dy, w, stride, H, W, torch.float32)), ref, mag)


def s2_bwd_class(shape):
    """exact_int operands of the stride-2 input gradient, (F, H, W, C) with Cin = Cout = C."""
    Fr, H, W, Cc = shape
    return bwd_data_class("exact_int", (Fr, H, W, Cc, Cc), 2)


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------
WGRAD_CLASSES = ACCURACY_CLASSES


def wgrad_has_class(cls, shape):
    """`cancelling` needs two frames to mirror (the contraction runs over the pixels): x[1] = -x[0], dy[1] = dy[0] (1 + 2^-12 r)."""
    return cls != "cancelling" or shape[0] >= 2


def _wgrad(x, dy, dtype):
    Cout, Cin = dy.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(x.to(dtype), (Cout, Cin, 3, 3), dy.to(dtype), padding=1)


def wgrad_operands(cls, shape):
    """(x [F, Cin, H, W], dy [F, Cout, H, W], what dw holds before an accumulating call or None)"""
    Fr, H, W, Cin, Cout, acc = shape
    xs, ds, ws = (Fr, Cin, H, W), (Fr, Cout, H, W), (Cout, Cin, 3, 3)
    if cls == "exact_int":
        return integers(xs, 1, 8), integers(ds, 3, 4), (integers(ws, 4, 16) if acc else None)
    if cls == "scaled":
        return bounded(xs, 21, 2.0), bounded(ds, 23), (bounded(ws, 24) if acc else None)
    x, dy, base = _class_x(cls, xs), uniform(ds, 3), (uniform(ws, 4) if acc else None)
    if cls == "cancelling":
        assert Fr >= 2 and base is None
        x[1], dy[1] = -x[0], dy[0] * (1 + 2.0 ** -12 * uniform(ds[1:], 77))
        x[2:] *= 2.0 ** -12  # a third frame stays far below the two that cancel
    return x, dy, base


@functools.lru_cache(maxsize=None)
def wgrad_class(cls, shape):
    """(x, dy, base, fp64 dW [Cout, Cin, 3, 3] (+ base), mag = sum over pixels |dY| |X| (+ |base|), torch fp32's (rms, max))"""
    x, dy, base = wgrad_operands(cls, shape)
    add = lambda g, b: g if b is None else g + b.to(g.dtype)
    ref = add(_wgrad(x, dy, torch.float64), base)
    mag = add(_wgrad(x.abs(), dy.abs(), torch.float64), None if base is None else base.abs())
    return x, dy, base, ref, mag, elem_error(add(_wgrad(x, dy, torch.float32), base), ref, mag)


def wgrad_terms(shape):
    """Contraction length of the hard bound: F H W products plus one addition per workspace piece (plus the accumulate)."""
    Fr, H, W, Cin, Cout, acc = shape
    return Fr * H * W + wgrad_pieces(Fr, H, Cin, Cout) + int(acc)


def wgrad_scaled(shape, px, pdy):
    x, dy, base = wgrad_operands("scaled", shape)
    return x * 2.0 ** px, dy * 2.0 ** pdy, (None if base is None else base * 2.0 ** (px + pdy))


# ---- transposed convolution --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def convT_class(shape):
    """exact_int: (x [F, C, h, w], w [C, C, s, s], b [C], dy [F, C, h s, w s], y in fp64 channels-last, dx in fp64 channels-last)"""
    Fr, h, w_, Cc, s = shape
    x, wt, b = integers((Fr, Cc, h, w_), 1, 8), integers((Cc, Cc, s, s), 2, 4), integers((Cc,), 3, 16)
    dy = integers((Fr, Cc, h * s, w_ * s), 4, 4)
    y = F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=s)
    dx = F.conv2d(dy.double(), wt.double(), None, stride=s)  # the adjoint of a transposed convolution is the convolution with the same weight
    return x, wt, b, dy, nhwc(y), nhwc(dx)


# ---- where a mismatch lies ---------------------------------------------------------------------------------------------------------------
def describe_mismatch(y, ref, tile_rows=None):
    """For an exact comparison of channels-last tensors [F, H, W, C]: the first mismatching (frame, y, x, channel), how many there are and whether
    all of them lie on the image border, on a seam of `tile_rows`-pixel row tiles, or in one 32-channel block."""
    bad = (y.double().cpu() != ref.double()).nonzero()
    if len(bad) == 0:
        return "no mismatch"
    Fr, H, W, Cc = ref.shape
    f, yy, xx, c = bad.T
    on_border = ((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)).all().item()
    msg = f"{len(bad)} of {ref.numel()} differ, first at (frame, y, x, channel) = {tuple(bad[0].tolist())}: got {y[tuple(bad[0])].item()}, want {ref[tuple(bad[0])].item()}"
    msg += f"; all on the image border: {on_border}"
    if tile_rows:
        p = (f * H + yy) * W + xx
        r = p % tile_rows
        msg += f"; all on a {tile_rows}-row tile seam: {((r == 0) | (r == tile_rows - 1)).all().item()}; row tiles hit: {sorted(set((p // tile_rows).tolist()))[:8]}"
    blocks = sorted(set((c // 32).tolist()))
    msg += f"; 32-channel blocks hit: {blocks}"
    return msg
