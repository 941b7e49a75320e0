"""Inputs that reach the edges of the two fused losses (csrc/loss.hip, csrc/loss_trainer.hip), the float64 reference of both, the per-element
gate, and closed forms that do not go through the PyTorch definition.  Importable without a GPU: tests/test_loss_inputs_cpu.py checks that every
case reaches what its table row claims and that the definition's own float32 evaluation passes every gate; tests/test_loss_edges_gpu.py holds the
kernels to the same gates.

Classes (cameras are built in float64 and rounded to float32 once; the reference widens those float32 values):
  cameras      benign | out_of_view (tx = +-50: every projection clipped, far from the clip points) | half_out_x / half_out_y (about a third of the
               samples clipped in one direction) | behind (tz = -a depth near the median: near pixels get Z < 0 in the neighbour, far ones do not;
               tz sits in the middle of the widest gap of the depths, no pixel within 1e-3 of Z = 0) | rotated (0.5 rad about y) | rotated_wide (the same
               with four times the baseline: at disparity 0 the depth is 150 and d u / d depth keeps |t| / (depth |ray|) of its terms, so with
               |t| = 0.1 float32 torch itself comes within 3 % of the gate on a zero-disparity frame; with 0.4 it has a fourfold margin)
  disparities  smooth | ramp (affine in x, dyadic values: exact in float32) | with_0_and_1 (exact 0.0 and 1.0 on a lattice) | zero_frame (frame 1
               all 0.0)
  images       tissue | constant (frame value a_c, neighbour value b_c) | affine (p + q x + r y per channel and frame, inside [0, 1])
  masks        all_ones | random_90 | one_frame_only | single_pixel | border_band                                                   (trainer)
  flow         small | outward (about half the samples leave the map) | collide (a whole frame samples one cell) | empty_next (the next-frame
               neighbour's selection is empty)                                                                                       (trainer)

The gate (the one of tests/test_trainer_loss_gpu.py, with each frame's own maximum as the scale): an element may differ from the float64 gradient by
max(2e-4 of the frame's scale, 3 x how far the float64 gradient itself moves when every input is multiplied by 1 + eps, |eps| <= 8 fp32 ulps, six
draws, dilated 5 x 5 on tensors at the frame's resolution or finer), and never by more than half the scale.  Multiplicative noise keeps planted
zeros exact.  Values are held to 5e-6 relative."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from endodav_amd import losses, synth

FLAT = 2e-4          # of the frame's scale, every element
VALUE_RTOL = 5e-6
ULPS, DRAWS = 8.0, (1, 2, 3, 4, 5, 6)
BAND_CAP = 0.2       # share of a tensor's elements the band may decide (the existing trainer test's cap)
# constant images: frame value a_c, neighbour value b_c, registration r_c.  Dyadic with few bits: x^2, the sum of nine and its ninth are exact in
# float32 in any order, so every SSIM variance on the frame side is exactly 0; channel 1 has a = b: raw = 0, on the clamp's boundary
A_CONST, B_CONST, R_CONST = (0.25, 0.5, 0.75), (0.5, 0.5, 0.25), (0.375, 0.25, 0.5)
B2_CONST = (0.5, 0.75, 0.25)  # the trainer's neighbour: no channel equal to the frame's, so that d L1 / d refined = sign(a - b) is no kink
MASK_KEYS = [("occu_mask_backward", 0, -1), ("occu_mask_backward", 0, 1)]


# ---- case tables ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PhotoCase:
    name: str
    B: int
    T: int
    H: int
    W: int
    sizes: Tuple[Tuple[int, int], ...]
    camera: str
    disparity: str
    image: str
    smooth: float
    reaches: str


P20, P33, P64 = ((20, 28), (10, 14), (5, 7), (2, 3)), ((33, 65), (16, 32), (8, 16), (4, 8)), ((64, 32), (32, 16), (16, 8), (8, 4))
PHOTO_CASES = [
    PhotoCase("tiny_3x3", 1, 2, 3, 3, ((3, 3), (2, 2), (1, 2), (1, 1)), "benign", "smooth", "tissue", 1e-2,
              "the smallest frame; one-pixel and one-row maps through the resize (lin_ratio with a single input pixel)"),
    PhotoCase("benign_20x28", 1, 3, 20, 28, P20, "benign", "smooth", "tissue", 1e-3, "one tile hanging over both edges; reflection rows 1 and H - 2"),
    PhotoCase("behind_20x28", 1, 3, 20, 28, P20, "behind", "ramp", "tissue", 0.0, "Z < 0 in the neighbour for the near columns only"),
    PhotoCase("zero01_20x28", 1, 3, 20, 28, P20, "rotated", "with_0_and_1", "tissue", 1e-3, "disparity exactly 0.0 and 1.0"),
    PhotoCase("zero_frame_20x28", 1, 3, 20, 28, P20, "rotated_wide", "zero_frame", "tissue", 1e-2, "mean = 0, norm = D / 1e-7 on one frame"),
    PhotoCase("out_of_view_20x28", 1, 3, 20, 28, P20, "out_of_view", "smooth", "tissue", 0.0, "every sample clipped: zero gradient"),
    PhotoCase("benign_33x65", 2, 3, 33, 65, P33, "benign", "smooth", "tissue", 1e-3, "one-row and one-column tiles; two clips"),
    PhotoCase("half_out_x_33x65", 2, 3, 33, 65, P33, "half_out_x", "smooth", "tissue", 1e-3, "a third of the samples clipped in x, samples on W - 1"),
    PhotoCase("half_out_y_33x65", 2, 3, 33, 65, P33, "half_out_y", "smooth", "tissue", 1e-3, "a third of the samples clipped in y, samples on H - 1"),
    PhotoCase("rotated_33x65", 2, 3, 33, 65, P33, "rotated", "smooth", "tissue", 1e-3, "0.5 rad about y"),
    PhotoCase("behind_33x65", 2, 3, 33, 65, P33, "behind", "ramp", "affine", 0.0, "Z < 0 on one side of a column; affine images: no bilinear kink"),
    PhotoCase("constant_33x65", 2, 3, 33, 65, ((33, 65),) * 4, "rotated", "ramp", "constant", 1e-2,
              "closed form; SSIM variances exactly 0; maps at the frame size (a resize in float32 leaves d_y = +-1 ulp on a ramp: a kink at every pixel)"),
    PhotoCase("two_frames_64x32", 1, 2, 64, 32, P64, "benign", "smooth", "tissue", 1e-3, "T = 2: every frame has one neighbour; two tiles in y, exact in x"),
    PhotoCase("larger_maps_20x28", 1, 3, 20, 28, ((30, 42), (24, 30), (20, 29), (21, 28)), "half_out_x", "smooth", "tissue", 1e-3,
              "maps larger than the frame: resized down"),
]


@dataclass(frozen=True)
class TrainerCase:
    name: str
    n: int
    H: int
    W: int
    sizes: Tuple[Tuple[int, int], ...]
    camera: str
    disparity: str
    image: str
    mask: str
    flow: str
    weights: Tuple[Tuple[str, object], ...]
    reaches: str

    def wts(self, **over):
        kw = dict(self.weights)
        kw.update(over)
        return losses.TrainerLossWeights(**kw)


_DEPTH = (("depth_reproj", 1e-2), ("depth_flow", 1e-2), ("tune_temporal", True))
T16, T17, T33, T32, T3264 = ((16, 16), (8, 8), (4, 4), (2, 2)), ((17, 33), (9, 17), (5, 9), (3, 5)), ((30, 60), (17, 31), (9, 15), (5, 7)), \
    ((32, 32), (16, 16), (8, 8), (4, 4)), ((32, 64),) * 4
TRAINER_CASES = [
    TrainerCase("benign_16x16", 2, 16, 16, T16, "benign", "smooth", "tissue", "random_90", "small", (), "the smallest frame: a 2 x 2 colour map, 60 idle sum chunks, one tile"),
    TrainerCase("depth_16x16", 2, 16, 16, T16, "benign", "smooth", "tissue", "all_ones", "outward", _DEPTH, "zeros padding with 2, 3 and 4 corners outside; small counts"),
    TrainerCase("border_17x33", 3, 17, 33, T17, "rotated", "with_0_and_1", "tissue", "border_band", "small", (), "mask only where the reflection counts live; a one-column tile"),
    TrainerCase("one_frame_17x33", 3, 17, 33, T17, "rotated_wide", "zero_frame", "tissue", "one_frame_only", "small", (("disparity_smoothness", 1e-2),), "two frames masked out; the live one has zero disparity"),
    TrainerCase("behind_33x65", 2, 33, 65, T33, "behind", "ramp", "affine", "random_90", "outward", _DEPTH + (("disparity_smoothness", 0.0),), "both resize paths; Z < 0; depth terms with points behind the camera"),
    TrainerCase("rotated_33x65", 2, 33, 65, T33, "rotated", "smooth", "tissue", "random_90", "collide", _DEPTH, "every atomic of a frame on four addresses"),
    TrainerCase("single_pixel_32x32", 2, 32, 32, T32, "benign", "smooth", "tissue", "single_pixel", "small", (), "same_c at every scale; exactly one tile; sum m = 1"),
    TrainerCase("out_of_view_32x32", 2, 32, 32, T32, "out_of_view", "smooth", "tissue", "random_90", "small", (("disparity_smoothness", 0.0),), "every colour sample clipped"),
    TrainerCase("half_out_y_32x64", 3, 32, 64, T3264, "half_out_y", "smooth", "tissue", "all_ones", "small", (("depth_reproj", 1e-2), ("tune_temporal", True)), "all four maps at the frame size; samples on H - 1"),
    TrainerCase("constant_32x32", 3, 32, 32, T32, "rotated", "ramp", "constant", "random_90", "small", (), "closed form with sum m normalisation; no resize before the smoothness term"),
]
PHOTO = {c.name: c for c in PHOTO_CASES}
TRAINER = {c.name: c for c in TRAINER_CASES}


# ---- builders ----------------------------------------------------------------------------------------------------------------------------------
def _u(key, shape, lo, hi):
    return torch.from_numpy(synth.uniform(f"loss_edges:{key}", shape, lo, hi)).double()


def disparities(kind: str, n: int, sizes, seed: int = 0) -> Dict:
    out = losses.synthetic_disps(n, list(sizes), seed=seed)
    for s, (h, w) in enumerate(sizes):
        d = out[("disp", s)]
        if kind == "ramp":  # 1/8 + x step, step = the largest power of two with (w - 1) step <= 1/2: every value and every difference exact in float32
            d = (0.125 + torch.arange(w, dtype=torch.float32) * ramp_span_mean(w)[0]).view(1, 1, 1, w).expand(n, 1, h, w).contiguous()
        elif kind == "with_0_and_1":
            d = d.clone()
            d[:, :, 0::7, 1::9] = 0.0
            d[:, :, 3::7, 5::9] = 1.0
        elif kind == "zero_frame":
            d = d.clone()
            d[1 % n] = 0.0
        elif kind != "smooth":
            raise KeyError(kind)
        out[("disp", s)] = d
    return out


def ramp_span_mean(w: int) -> Tuple[float, float]:
    """(value step between neighbouring columns, mean) of the ramp at width w."""
    step = 2.0 ** -int(np.ceil(np.log2(2 * (w - 1)))) if w > 1 else 0.0
    return step, 0.125 + (w - 1) * step / 2


def depths64(disps, H, W):
    """float64 depth at the frame size of every scale: [4][n, 1, H, W]."""
    out = []
    for s in range(4):
        d = disps[("disp", s)].double()
        if d.shape[-2:] != (H, W):
            d = F.interpolate(d, [H, W], mode="bilinear", align_corners=True)
        out.append(losses.disp_to_depth(d)[1])
    return out


def _behind_tz(disps, H, W) -> float:
    """-(the middle of the widest gap between consecutive depths inside the 10th..40th percentile (the nearest tenth to two fifths of the pixels end up behind)): Z' = depth + tz changes sign there."""
    z = torch.cat([d.reshape(-1) for d in depths64(disps, H, W)]).sort().values
    lo, hi = int(0.1 * z.numel()), int(0.4 * z.numel())
    gaps = z[lo + 1:hi] - z[lo:hi - 1]
    i = int(gaps.argmax())
    return -float((z[lo + i] + z[lo + i + 1]) / 2)


def _pose(kind: str, sign: float, disps, H, W) -> torch.Tensor:
    """float64 4x4 pose towards the next (sign = +1) / previous (-1) frame."""
    T = torch.eye(4, dtype=torch.float64)
    if kind == "benign":
        T[0, 3], T[2, 3] = 0.05 * sign, -0.02 * sign
    elif kind == "out_of_view":
        T[0, 3], T[1, 3] = 50.0 * sign, 50.0 * sign  # clipped in x AND y: a sample clipped in x alone still moves along the last column
    elif kind == "half_out_x":
        T[0, 3] = 0.08 * sign
    elif kind == "half_out_y":
        T[1, 3] = 0.065 * sign
    elif kind == "behind":
        T[2, 3] = _behind_tz(disps, H, W)
        T[0, 3] = 0.01 * sign
    elif kind in ("rotated", "rotated_wide"):
        a = 0.5 * sign
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        T[0, 3] = (-0.1 if kind == "rotated" else -0.4) * sign
    else:
        raise KeyError(kind)
    return T


def cameras(kind: str, n: int, H: int, W: int, disps):
    """K, inv_K, T_prev, T_next [n, 4, 4] float32 (built in float64, rounded once)."""
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 0.82 * W, 1.02 * H, 0.5 * W, 0.5 * H
    rep = lambda m: m.unsqueeze(0).repeat(n, 1, 1).float().contiguous()
    return rep(K), rep(torch.linalg.inv(K)), rep(_pose(kind, -1.0, disps, H, W)), rep(_pose(kind, 1.0, disps, H, W))


def images(kind: str, n: int, H: int, W: int, role: str = "frame", seed: int = 0) -> torch.Tensor:
    """[n, 3, H, W] float32.  role: "frame" (photometric: even frames a_c, odd frames b_c when constant), "a" / "b" / "r" (a constant everywhere)."""
    if kind == "tissue":
        x = synth.synth_clip(1, n, H, W, seed=seed, kind="tissue")[0] + synth.uniform(f"loss_edges:noise:{role}:{seed}", (n, 3, H, W), -0.05, 0.05)
        return torch.from_numpy(np.clip(x, 0.0, 1.0).astype(np.float32))
    if kind == "constant":
        vals = {"a": A_CONST, "b": B_CONST, "b2": B2_CONST, "r": R_CONST}
        x = torch.empty(n, 3, H, W)
        for f in range(n):
            v = vals[role] if role in vals else (A_CONST if f % 2 == 0 else B_CONST)
            x[f] = torch.tensor(v).view(3, 1, 1)
        return x
    if kind == "affine":
        p, q, r = _u(f"aff_p:{role}", (n, 3, 1, 1), 0.3, 0.5), _u(f"aff_q:{role}", (n, 3, 1, 1), -0.14, 0.14), _u(f"aff_r:{role}", (n, 3, 1, 1), -0.14, 0.14)
        xs, ys = torch.linspace(0, 1, W, dtype=torch.float64).view(1, 1, 1, W), torch.linspace(0, 1, H, dtype=torch.float64).view(1, 1, H, 1)
        return (p + q * xs + r * ys).float()
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def photo_inputs(name: str) -> Dict:
    c = PHOTO[name]
    n = c.B * c.T
    disps = disparities(c.disparity, n, c.sizes)
    cams = [cameras(c.camera, c.T, c.H, c.W, {k: v[b * c.T:(b + 1) * c.T] for k, v in disps.items()}) for b in range(c.B)]
    K, inv_K, Tp, Tn = [torch.cat([cm[i] for cm in cams]) for i in range(4)]
    return {"frames": images(c.image, n, c.H, c.W), "disps": disps, "K": K, "inv_K": inv_K, "T_prev": Tp, "T_next": Tn}


def masks(kind: str, n: int, H: int, W: int, fid: int, base: torch.Tensor) -> torch.Tensor:
    m = torch.zeros(n, 1, H, W)
    if kind == "all_ones":
        m[:] = 1.0
    elif kind == "random_90":
        m = base.clone()
    elif kind == "one_frame_only":
        m[1 % n] = base[1 % n]  # the zero_frame class's frame: the only live frame is the one of zero disparity
    elif kind == "single_pixel":
        y, x = SINGLE_PIXEL(H, W, fid)
        m[0, 0, y, x] = 1.0
    elif kind == "border_band":
        m[:] = 1.0
        m[:, :, 2:-2, 2:-2] = 0.0
    else:
        raise KeyError(kind)
    return m


def SINGLE_PIXEL(H, W, fid):
    return (H // 2, W // 3) if fid == -1 else (H // 3, W // 2)


COLLIDE_TARGET = (0.4, 0.6)  # of (H - 1, W - 1), plus a fraction of a pixel


def flows(kind: str, n: int, H: int, W: int, s: int, fid: int, base: torch.Tensor) -> torch.Tensor:
    """("position", "high", s, fid) [n, 2, H, W]; channel 0 is the row displacement."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    if kind == "small":
        return base.clone()
    if kind == "outward":  # p + 0.45 (p - centre) + noise: about half the samples leave, a band lands in (-1, 0) and (size - 1, size)
        jit = _u(f"flow_out:{s}:{fid}", (n, 2, H, W), -0.45, 0.45)
        f = torch.stack([0.45 * (ys - 0.5 * (H - 1)), 0.45 * (xs - 0.5 * (W - 1))]).unsqueeze(0) + jit
        return f.float()
    if kind in ("collide", "empty_next"):
        ty = torch.floor(torch.tensor(COLLIDE_TARGET[0] * (H - 1))) + 0.25 + 0.125 * s
        tx = torch.floor(torch.tensor(COLLIDE_TARGET[1] * (W - 1))) + 0.625 - 0.125 * s
        f = torch.stack([ty - ys, tx - xs]).unsqueeze(0).repeat(n, 1, 1, 1)
        if kind == "empty_next" and fid == 1:
            f = f + 4.0 * max(H, W)  # every sample far outside: warp = 0 everywhere, the selection is empty
        return f.float()
    raise KeyError(kind)


def _trainer_build(c: TrainerCase, flow: str):
    inp = dict(losses.synthetic_trainer_inputs(c.n, c.H, c.W, seed=21))
    disps = disparities(c.disparity, c.n, c.sizes, seed=21)
    K64 = inp["K"].double()
    if c.camera != "benign":
        for fid in losses.FIDS:
            inp[("cam_T_cam", 0, fid)] = _pose(c.camera, float(fid), disps, c.H, c.W).unsqueeze(0).repeat(c.n, 1, 1).float().contiguous()
    inp["inv_K"] = torch.linalg.inv(K64).float()
    if c.image != "tissue":
        for s in range(4):
            inp[("color", 0, s)] = images(c.image, c.n, c.H >> s, c.W >> s, "a")
        for fid in losses.FIDS:
            inp[("color", fid, 0)] = images(c.image, c.n, c.H, c.W, "b2" if c.image == "constant" else f"nb{fid}")
            for s in range(4):
                inp[("registration", s, fid)] = images(c.image, c.n, c.H, c.W, "r" if c.image == "constant" else f"reg{s}{fid}")
                if c.image == "constant":
                    inp[("refined", s, fid)] = images(c.image, c.n, c.H, c.W, "a")
                    # transform_high: affine per channel, dyadic steps (exact): t_c = (c + 1) x / 64 - (c + 2) y / 128
                    ys, xs = torch.meshgrid(torch.arange(c.H, dtype=torch.float32), torch.arange(c.W, dtype=torch.float32), indexing="ij")
                    inp[("transform", "high", s, fid)] = torch.stack([(ch + 1) * xs / 64.0 - (ch + 2) * ys / 128.0 for ch in range(3)]).unsqueeze(0).repeat(c.n, 1, 1, 1).contiguous()
    for fid in losses.FIDS:
        inp[("occu_mask_backward", 0, fid)] = masks(c.mask, c.n, c.H, c.W, fid, inp[("occu_mask_backward", 0, fid)])
        for s in range(4):
            inp[("position", "high", s, fid)] = flows(flow, c.n, c.H, c.W, s, fid, inp[("position", "high", s, fid)])
    return inp, disps


@functools.lru_cache(maxsize=None)
def trainer_inputs(name: str, flow: str = ""):
    c = TRAINER[name]
    return _trainer_build(c, flow or c.flow)


def trainer_leaves(inp, disps):
    """The tensors the reference's autograd reaches (tests/test_losses_cpu.py::kat_leaves)."""
    leaves = {("disp", s): disps[("disp", s)] for s in range(4)}
    leaves["K"], leaves["inv_K"] = inp["K"], inp["inv_K"]
    for fid in losses.FIDS:
        leaves[("cam_T_cam", 0, fid)] = inp[("cam_T_cam", 0, fid)]
        for s in range(4):
            leaves[("refined", s, fid)] = inp[("refined", s, fid)]
            leaves[("transform", "high", s, fid)] = inp[("transform", "high", s, fid)]
    return leaves


# ---- the definition in a chosen precision, optionally at inputs moved by a few fp32 ulps -----------------------------------------------------------
def _mover(eps_ulps: float, seed: int, dtype):
    g = torch.Generator().manual_seed(seed)

    def move(v):
        v = v.to(dtype)
        if eps_ulps:  # multiplicative only: an exact zero stays an exact zero
            v = v * (1.0 + (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * eps_ulps * 1.2e-7)
        return v
    return move


def photo_eval(name: str, dtype=torch.float64, eps_ulps: float = 0.0, seed: int = 0, smooth=None):
    """(value, {("disp", s): gradient}) of losses.photometric_loss (mean over the clips)."""
    c, inp = PHOTO[name], photo_inputs(name)
    mv = _mover(eps_ulps, seed, dtype)
    leaves = {k: mv(v).clone().requires_grad_(True) for k, v in inp["disps"].items()}
    fr, K, iK, Tp, Tn = (mv(inp[k]) for k in ("frames", "K", "inv_K", "T_prev", "T_next"))
    total = 0.0
    for b in range(c.B):
        sl = slice(b * c.T, (b + 1) * c.T)
        total = total + losses.photometric_loss({k: v[sl] for k, v in leaves.items()}, fr[sl], K[sl], iK[sl], Tp[sl], Tn[sl],
                                                disparity_smoothness=c.smooth if smooth is None else smooth)
    total = total / c.B
    total.backward()
    return float(total.detach()), {k: v.grad for k, v in leaves.items()}


def trainer_eval(name: str, dtype=torch.float64, eps_ulps: float = 0.0, seed: int = 0, flow: str = "", wts=None):
    """({entry: value}, {leaf: gradient}) of losses.trainer_losses."""
    c = TRAINER[name]
    inp, disps = trainer_inputs(name, flow)
    mv = _mover(eps_ulps, seed, dtype)
    x = {k: (v.to(dtype) if k in MASK_KEYS else mv(v)) for k, v in inp.items()}
    leaves = {k: (x[k] if not (isinstance(k, tuple) and k[0] == "disp") else mv(disps[k])).clone().requires_grad_(True) for k in trainer_leaves(inp, disps)}
    x.update({k: v for k, v in leaves.items() if not (isinstance(k, tuple) and k[0] == "disp")})
    out = losses.trainer_losses({k: v for k, v in leaves.items() if isinstance(k, tuple) and k[0] == "disp"}, x, wts or c.wts())
    if bool(torch.isfinite(out["loss"])):
        out["loss"].backward()
    return {k: float(v.detach()) for k, v in out.items()}, {k: v.grad for k, v in leaves.items()}


@functools.lru_cache(maxsize=None)
def photo_reference(name: str):
    """float64 value and gradients, and the six moved gradients of the band: computed once per case."""
    val, g = photo_eval(name)
    return val, g, [photo_eval(name, eps_ulps=ULPS, seed=sd)[1] for sd in DRAWS]


@functools.lru_cache(maxsize=None)
def trainer_reference(name: str, flow: str = ""):
    val, g = trainer_eval(name, flow=flow)
    return val, g, [trainer_eval(name, eps_ulps=ULPS, seed=sd, flow=flow)[1] for sd in DRAWS]


# ---- the gate --------------------------------------------------------------------------------------------------------------------------------------
CEILING = 0.5  # of the frame's scale: what an element may be off by wherever the band decides (the existing trainer test's backstop)


def gate(got: torch.Tensor, ref: torch.Tensor, moved, frame_hw=None) -> Dict:
    """Every element of `got` against the float64 `ref` [n, ...]: scale = each frame's own max |ref|; a frame whose reference is all zero must be
    exactly zero.  Allowance = max(FLAT, 3 x spread), never more than CEILING.  The spread is dilated 5 x 5 on per-pixel tensors at the frame's
    resolution or finer (a kink at one frame pixel reaches the 5 x 5 frame pixels around it through the SSIM windows); an element of a coarser
    disparity map already sums the block of frame pixels under it, neighbourhood included, in the very draw that moves it: no dilation there.
    Returns the violation count, the worst error of scale, the share of elements the band decides and the worst error / allowance."""
    n = ref.shape[0]
    shape = (n,) + (1,) * (ref.dim() - 1)
    scale = ref.abs().reshape(n, -1).amax(1).view(shape)
    live = (scale > 0).expand_as(ref)
    safe = scale.clamp_min(1e-300)
    err = (got.double() - ref).abs() / safe
    spread = torch.stack([(m - ref).abs() for m in moved]).max(0).values / safe
    if spread.dim() == 4 and (frame_hw is None or (spread.shape[-2] >= frame_hw[0] and spread.shape[-1] >= frame_hw[1])):
        spread = F.max_pool2d(spread, 5, 1, 2)
    allow = torch.clamp(3 * spread, min=FLAT, max=CEILING)
    viol = torch.where(live, err > allow, got.double() != 0)
    return {"viol": int(viol.sum()), "n": ref.numel(), "worst": float(err[live].max()) if bool(live.any()) else 0.0,
            "band": float((3 * spread > FLAT)[live].double().mean()) if bool(live.any()) else 0.0,
            "ratio": float((err / allow)[live].max()) if bool(live.any()) else 0.0, "dead_frames": int((scale == 0).sum())}


def value_ok(got: float, ref: float) -> bool:
    return abs(got - ref) <= VALUE_RTOL * abs(ref) + 1e-12


def band_capped(case, key) -> bool:
    """Is this tensor's band share held under BAND_CAP?  Every disparity map, refined and transform_high are, with two exceptions: scale 3's map under
    a `behind` or `rotated` camera (a 2 x 3 to 5 x 7 map whose every element sums an eighth of the frame's clipped and behind-the-camera samples), and
    the disparity maps of the constant-image rows (a ramp has d_y = 0 at every pixel: sign(0) is a kink everywhere; the closed forms hold those maps
    to 1e-6) together with their refined gradients (ill-conditioned, see below).  The per-frame sums K / inv_K / T are not capped, as in tests/test_trainer_loss_gpu.py.  Uncapped elements still meet CEILING."""
    if isinstance(key, tuple) and key[0] == "disp":
        if case.image == "constant":
            return False
        return not (key[1] == 3 and (case.camera == "behind" or case.camera.startswith("rotated")))
    if isinstance(key, tuple) and key[0] == "refined" and case.image == "constant":
        return False  # d SSIM / d refined of constant images is a cancelled sum of terms of size 1 / C2: 8 ulps of input move it by 4e-4 of its scale
    return isinstance(key, tuple) and key[0] in ("refined", "transform")


def check_gate(case, got_val, got_grads, ref_val, ref_grads, moved, what):
    """Values to VALUE_RTOL, every gradient element through L.gate, the band cap.  Returns the failures."""
    bad = []
    vals = ref_val.items() if isinstance(ref_val, dict) else [("loss", ref_val)]
    for k, v in vals:
        g = got_val[k] if isinstance(got_val, dict) else got_val
        if not value_ok(float(g), v):
            bad.append(f"{k}: {float(g)!r} against {v!r} ({abs(float(g) - v) / abs(v):.2e} relative)")
    for k, r in ref_grads.items():
        res = gate(got_grads[k], r, [m[k] for m in moved], (case.H, case.W))
        print(f"  [{case.name}] {what} {k}: worst {res['worst']:.2e} of the frame's scale, {res['ratio']:.3f} of the allowance, band decides {res['band']:.1%}, "
              f"{res['viol']} of {res['n']} beyond the gate" + (f", {res['dead_frames']} frames exactly zero" if res["dead_frames"] else ""))
        if res["viol"]:
            bad.append(f"{k}: {res['viol']} of {res['n']} elements beyond the gate, worst {res['ratio']:.2f} x its allowance")
        if band_capped(case, k) and not res["band"] < BAND_CAP:
            bad.append(f"{k}: the band decides {res['band']:.1%} of the elements")
    return bad


# ---- what a case reaches, from the float64 definition --------------------------------------------------------------------------------------------------
def sample_coords(depth, K, inv_K, T, H, W):
    """Un-clipped source coordinates (ix, iy) and Z of every pixel: [n, H, W] each, float64."""
    n = depth.shape[0]
    pix = losses.pixel_grid(n, H, W, "cpu", torch.float64)
    cam = losses.backproject(depth, inv_K.double(), pix)
    camp = torch.matmul(torch.matmul(K.double(), T.double())[:, :3, :], cam)
    z = camp[:, 2].view(n, H, W)
    return (camp[:, 0].view(n, H, W) / (z + 1e-7)), (camp[:, 1].view(n, H, W) / (z + 1e-7)), z


def corners_outside(ix, iy, H, W):
    """Per sample, how many of the four bilinear corners lie outside the map (zeros padding)."""
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = torch.zeros_like(ix, dtype=torch.long)
    for dx in (0, 1):
        for dy in (0, 1):
            out += (~((x0 + dx >= 0) & (x0 + dx < W) & (y0 + dy >= 0) & (y0 + dy < H))).long()
    return out


def photo_reach(name: str) -> Dict:
    """Shares over the KEPT (frame, neighbour) pairs of every scale: clipped in x / y, Z < 0, the smallest |Z|, samples exactly on the last row / column."""
    c, inp = PHOTO[name], photo_inputs(name)
    n = c.B * c.T
    t = torch.arange(n) % c.T
    st = {"clip_x": [], "clip_y": [], "neg_z": [], "min_abs_z": [], "on_last": []}
    for depth in depths64(inp["disps"], c.H, c.W):
        for T, keep in ((inp["T_prev"], t > 0), (inp["T_next"], t < c.T - 1)):
            ix, iy, z = sample_coords(depth, inp["K"], inp["inv_K"], T, c.H, c.W)
            ix, iy, z = ix[keep], iy[keep], z[keep]
            st["clip_x"].append(((ix <= 0) | (ix >= c.W - 1)).double().mean())
            st["clip_y"].append(((iy <= 0) | (iy >= c.H - 1)).double().mean())
            st["neg_z"].append((z < 0).double().mean())
            st["min_abs_z"].append(z.abs().min())
            st["on_last"].append(((ix >= c.W - 1) | (iy >= c.H - 1)).double().mean())
    return {k: (float(min(v)) if k == "min_abs_z" else float(sum(v) / len(v))) for k, v in st.items()}


def trainer_reach(name: str, flow: str = "") -> Dict:
    c = TRAINER[name]
    inp, disps = trainer_inputs(name, flow)
    w = c.wts()
    st = {"clip": [], "neg_z": [], "min_abs_z": [], "drp_count": [], "dfl_count": [], "flow_corners": torch.zeros(5, dtype=torch.long), "drp_corners": torch.zeros(5, dtype=torch.long)}
    for s, depth in enumerate(depths64(disps, c.H, c.W)):
        for fid in losses.FIDS:
            ix, iy, z = sample_coords(depth, inp["K"], inp["inv_K"], inp[("cam_T_cam", 0, fid)], c.H, c.W)
            st["clip"].append(((ix <= 0) | (ix >= c.W - 1) | (iy <= 0) | (iy >= c.H - 1)).double().mean())
            st["neg_z"].append((z < 0).double().mean())
            st["min_abs_z"].append(z.abs().min())
            src = slice(None, -1) if fid == 1 else slice(1, None)
            tgt = slice(1, None) if fid == 1 else slice(None, -1)
            if w.tune_temporal and w.depth_reproj:
                grid = torch.stack([ix[src] / (c.W - 1) * 2 - 1, iy[src] / (c.H - 1) * 2 - 1], -1)
                sampled = F.grid_sample(depth[tgt], grid, padding_mode="zeros", align_corners=True)
                st["drp_count"].append(int((sampled > 1e-3).sum()))
                st["drp_corners"] += torch.bincount(corners_outside(ix[src], iy[src], c.H, c.W).reshape(-1), minlength=5)
            if w.tune_temporal and w.depth_flow:
                fl = inp[("position", "high", s, fid)].double()[src]
                warp = losses.flow_sample(depth[src], fl, "zeros")
                st["dfl_count"].append(int((warp > 1e-3).sum()))
                ys, xs = torch.meshgrid(torch.arange(c.H, dtype=torch.float64), torch.arange(c.W, dtype=torch.float64), indexing="ij")
                st["flow_corners"] += torch.bincount(corners_outside(xs + fl[:, 1], ys + fl[:, 0], c.H, c.W).reshape(-1), minlength=5)
    return {"clip": float(sum(st["clip"]) / len(st["clip"])), "neg_z": float(sum(st["neg_z"]) / len(st["neg_z"])), "min_abs_z": float(min(st["min_abs_z"])),
            "drp_count": st["drp_count"], "dfl_count": st["dfl_count"], "flow_corners": st["flow_corners"].tolist(), "drp_corners": st["drp_corners"].tolist()}


def tiles(H, W):
    return -(-H // 32), -(-W // 32)


# ---- closed forms (constant images, ramp disparity): no warp, no pooling, no autograd -----------------------------------------------------------------
def rep_constant(a=A_CONST, b=B_CONST) -> float:
    """0.85 mean_c clamp((1 - (2 a b + C1) / (a^2 + b^2 + C1)) / 2, 0, 1) + 0.15 mean_c |a - b|: every window is constant, every variance exactly 0."""
    c1 = 0.01 ** 2
    a, b = np.float32(a).astype(np.float64), np.float32(b).astype(np.float64)
    ss = np.clip((1 - (2 * a * b + c1) / (a * a + b * b + c1)) / 2, 0, 1)
    return float(0.85 * ss.mean() + 0.15 * np.abs(a - b).mean())


def photo_closed_form(name: str) -> float:
    """Frames alternate a, b, so every kept pair compares a with b; the ramp's |d_x norm| is step / (mean + 1e-7) on every pair, |d_y norm| = 0; the
    maps are resized to the frame width W, where an affine map stays affine: step_W = step_w (w - 1) / (W - 1)."""
    c = PHOTO[name]
    assert c.image == "constant" and c.disparity == "ramp"
    total = 0.0
    for s, (h, w) in enumerate(c.sizes):
        step, mean = ramp_span_mean(w)
        total += 2 * rep_constant() / 2.0 + c.smooth * (step * (w - 1) / (c.W - 1) / (mean + 1e-7)) / 2 ** s
    return total / 4


def trainer_closed_form(name: str) -> Dict[str, float]:
    """Per scale: rep = rep_constant(a, b) per neighbour whatever the mask (a weighted mean of one number), tr = mean_c |a_c - r_c|, cvt = mean_c |step_x|
    + mean_c |step_y| of the affine transform_high (the residue colour - registration is constant: every edge weight is 1), smooth at the colour
    scale's width."""
    c = TRAINER[name]
    assert c.image == "constant" and c.disparity == "ramp"
    w = c.wts()
    a, r = np.float32(A_CONST).astype(np.float64), np.float32(R_CONST).astype(np.float64)
    tr = float(np.abs(a - r).mean())
    cvt = float(np.mean([(ch + 1) / 64.0 for ch in range(3)]) + np.mean([(ch + 2) / 128.0 for ch in range(3)]))
    out, total = {}, 0.0
    for s, (h, wd) in enumerate(c.sizes):
        step, mean = ramp_span_mean(wd)
        wc = c.W >> s
        sm = step * (wd - 1) / (wc - 1) / (mean + 1e-7)
        terms = {"loss_reprojection": 2 * rep_constant(A_CONST, B2_CONST) / 2.0, "loss_transform": w.transform_constraint * 2 * tr / 2.0, "loss_cvt": w.transform_smoothness * 2 * cvt / 2.0,
                 "loss_smooth": w.disparity_smoothness * sm / 2 ** s}
        for k, v in terms.items():
            out[f"loss/{k}/{s}"] = v
        out[f"loss/{s}"] = sum(terms.values())
        total += out[f"loss/{s}"]
    out["loss"] = total / 4
    return out
