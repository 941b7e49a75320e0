"""LayerNorm and GroupNorm, forward and backward (norms.hip, bwd.hip), at the numeric edges: a mean far above the spread, constant rows and slabs,
outlier channels and pixels, heavy tails, variance far below eps, operands scaled by 2^+-40, exact power-of-two scaling of the backward, and where
a NaN may and may not show.  The input classes, fp64 references and gates come from tests/edge_inputs.py (checked by tests/test_edge_inputs_cpu.py).

No gate here is close(): LayerNorm is judged per row (|y - ref| / max_c |ref[row, :]|), GroupNorm per (frame, group) slab, next to the error of
torch's own fp32 op on the same inputs: max <= max(4 x torch's, the kernel's uniform-input tolerance), rms <= 4 x max(torch's, u)."""
import math

import pytest
import torch

from endodav_amd import _lib

from . import edge_inputs as E
from .edge_inputs import bits
from .test_kernels_gpu import st

pytestmark = pytest.mark.gpu

NAN = float("nan")
LN_CASES = [pytest.param(*s, id="{}x{}".format(*s)) for s in E.LN_SHAPES]
GN_CASES = [pytest.param(*s, id="F{}xP{}xC{}".format(*s)) for s in E.GN_SHAPES]
PATHS = pytest.mark.parametrize("two_stage", [False, True], ids=["strided", "two_stage"])


def report(what, rms, mx, torch_err, floor):
    print(f"\n[{what}] {E.ratios(rms, mx, torch_err)}")
    bad = E.gate_failures(rms, mx, torch_err, floor)
    assert not bad, f"{what}: " + "; ".join(bad)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
def layernorm(lib, cuda, x, w, b, pe, y_prev, form):
    """edv_layernorm for the plain and pe forms, edv_layernorm_mapped (identity maps) for GELU and accumulate -> CPU tensor."""
    eps, use_pe, act, acc = E.LN_FORMS[form]
    rows, dim = x.shape
    xd, wd, bd, ped = x.to(cuda), w.to(cuda), b.to(cuda), pe.to(cuda)
    y = y_prev.to(cuda) if acc else torch.full((rows, dim), NAN, device=cuda)
    pe_args = (ped.data_ptr(), E.LN_RPF, E.LN_T) if use_pe else (None, 0, 0)
    if act or acc:
        _lib.check(lib.edv_layernorm_mapped(xd.data_ptr(), None, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), None, rows, dim, eps, *pe_args, act, int(acc), st()),
                   "edv_layernorm_mapped")
    else:
        _lib.check(lib.edv_layernorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), rows, dim, eps, *pe_args, st()), "edv_layernorm")
    torch.cuda.synchronize()
    return y.cpu()


def layernorm_bwd(lib, cuda, x, w, dy, prev, acc):
    rows, dim = x.shape
    xd, wd, gd = x.to(cuda), w.to(cuda), dy.to(cuda)
    dx = prev.to(cuda) if acc else torch.full((rows, dim), NAN, device=cuda)
    _lib.check(lib.edv_layernorm_bwd(xd.data_ptr(), wd.data_ptr(), gd.data_ptr(), dx.data_ptr(), rows, dim, E.LN_BWD_EPS, int(acc), st()), "edv_layernorm_bwd")
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize("rows,dim", LN_CASES)
@pytest.mark.parametrize("form", list(E.LN_FORMS))
@pytest.mark.parametrize("name", E.LN_CLASSES)
def test_layernorm_edges_accuracy(lib, cuda, name, form, rows, dim):
    """Per-row error against fp64 next to torch's fp32 layer_norm (+ pe, GELU, + y) on the same inputs.

    Measured on an MI355X, worst over the three shapes and the four forms (plain, pe, gelu, acc): kernel / torch rms, kernel / torch max, and the
    largest per-row error, kernel | torch:
    class          rms    max    largest error
    offset_1e3     1.24   1.39   5.2e-3 | 7.9e-3    (the fp32 mean of 1000 +- 0.017 is 3e-5 off: 2e-3 of sigma, for torch alike)
    offset_1e4     0.93   0.87   1.7e-1 | 2.3e-1    (sigma is six ulps of the values)
    outlier_ch     0.91   0.88   2.8e-7 | 1.2e-6
    lognormal      1.03   1.23   2.6e-7 | 6.9e-7
    scaled_2p40    1.02   1.26   2.4e-7 | 3.3e-7
    scaled_2m40    1.02   1.00   1.1e-7 | 1.1e-7    (x-hat is x 1e3 of 2^-40: y = b to fp32, kernel and torch give the same bits)
    const          1.03   1.00   8.7e-8 | 8.7e-8    (plain: 0 | 0; test_layernorm_constant_rows_are_exact)
    No class needs more than the uniform-input tolerance or 1.4 x torch."""
    ref, torch_err = E.ln_forward(name, rows, dim, form)
    y = layernorm(lib, cuda, *E.ln_operands(name, rows, dim), form)
    assert torch.isfinite(y).all()
    report(f"layernorm {name} {form} {rows}x{dim}", *E.row_error(y, ref), torch_err, E.FLOOR["ln_fwd"])


@pytest.mark.parametrize("rows,dim", LN_CASES)
def test_layernorm_constant_rows_are_exact(lib, cuda, rows, dim):
    """Every row one 12-bit value: the row sum is exact in any order, sum / dim is the value, x-hat is exactly 0 (tests/test_edge_inputs_cpu.py runs the
    same arithmetic in torch fp32).  So y == b bit for bit, y == b + pe with pe, y == (b + pe) + y_prev when accumulating, in fp32 and in that
    order; with GELU y is within the GELU gate (1.5e-6 absolute) of gelu(b) in fp64."""
    x, w, b, pe, y_prev = E.ln_operands("const", rows, dim)
    per = E.ln_pe_rows(pe, rows)
    assert torch.equal(bits(layernorm(lib, cuda, x, w, b, pe, y_prev, "plain")), bits(b.expand(rows, dim)))
    assert torch.equal(bits(layernorm(lib, cuda, x, w, b, pe, y_prev, "pe")), bits(b + per))
    assert torch.equal(bits(layernorm(lib, cuda, x, w, b, pe, y_prev, "acc")), bits((b + per) + y_prev))
    err = (layernorm(lib, cuda, x, w, b, pe, y_prev, "gelu").double() - torch.nn.functional.gelu(b.double())).abs().max().item()
    assert err <= E.GELU_GATE, err


@pytest.mark.parametrize("rows,dim", LN_CASES)
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("dy_kind", ["uniform", "outlier"])
@pytest.mark.parametrize("name", E.LN_CLASSES)
def test_layernorm_bwd_edges_accuracy(lib, cuda, name, dy_kind, acc, rows, dim):
    """Per-row error of dx against fp64 autograd next to torch's fp32 autograd; dy uniform, or with the three outlier channels x 300.  On constant
    rows x-hat is 0 and dx = (g w - mean(g w)) rsqrt(eps), about 1e3.

    Measured on an MI355X, worst over the three shapes, store and accumulate: kernel / torch rms and max, largest per-row error kernel | torch:
    class          dy uniform                      dy with outlier channels
    offset_1e3     0.38  0.58   1.6e-3 | 2.8e-3    0.43  0.71   1.4e-3 | 2.0e-3
    offset_1e4     0.49  0.44   6.0e-2 | 1.4e-1    0.55  0.83   6.3e-2 | 7.6e-2
    outlier_ch     1.00  1.69   4.0e-7 | 2.7e-7    0.93  1.30   1.3e-6 | 1.5e-6
    lognormal      1.00  0.99   2.4e-7 | 3.4e-7    1.07  0.87   2.1e-7 | 3.0e-7
    scaled_2p40    1.01  1.00   1.7e-7 | 2.3e-7    1.09  1.00   1.9e-7 | 2.0e-7
    scaled_2m40    0.67  0.78   1.6e-7 | 2.1e-7    0.68  0.87   1.6e-7 | 2.0e-7
    const          1.6e-7 against torch's 2.6e-3   1.6e-7 against 1.3e-3   (torch's fp32 mean of a constant row is an ulp off, times rsqrt(eps))"""
    dy, prev, ref, torch_err = E.ln_backward(name, rows, dim, dy_kind, acc)
    x, w = E.ln_operands(name, rows, dim)[:2]
    dx = layernorm_bwd(lib, cuda, x, w, dy, prev, acc)
    assert torch.isfinite(dx).all()
    report(f"layernorm_bwd {name} dy {dy_kind} {'acc' if acc else 'store'} {rows}x{dim}", *E.row_error(dx, ref), torch_err, E.FLOOR["ln_bwd"])


@pytest.mark.parametrize("rows,dim", LN_CASES)
def test_layernorm_bwd_power_of_two_scaling_is_exact(lib, cuda, rows, dim):
    """dx(dy 2^s) is ldexp(dx(dy), s) bit for bit at s = +-40 (dy bounded away from zero: tests/test_edge_inputs_cpu.py)."""
    x, w = E.ln_operands("base", rows, dim)[:2]
    dy = E.bounded((rows, dim), 51)
    base = layernorm_bwd(lib, cuda, x, w, dy, None, False)
    for s in E.BITWISE_SCALES:
        assert torch.equal(bits(layernorm_bwd(lib, cuda, x, w, dy * 2.0 ** s, None, False)), bits(base * 2.0 ** s)), f"dy 2^{s} is not an exact scaling"


def _rows_contained(got, clean, rows):
    keep = torch.ones(got.shape[0], dtype=torch.bool)
    keep[list(rows)] = False
    assert torch.isfinite(clean).all()
    assert torch.equal(bits(got[keep]), bits(clean[keep])), "a NaN changed other rows"
    for r in rows:
        assert not torch.isfinite(got[r]).all(), f"row {r} holds a NaN operand and is wholly finite"


@pytest.mark.parametrize("rows,dim", LN_CASES)
def test_layernorm_non_finite_stays_in_its_row(lib, cuda, rows, dim):
    """A NaN in an interior row and in the last row of x (forward; backward: of x, and of dy) leaves every other row bit for bit what it is with 1.0
    in its place."""
    x, w, b, pe, y_prev = (t.clone() for t in E.ln_operands("base", rows, dim))
    dy = E.ln_dy(rows, dim, "uniform").clone()
    spots = ((rows // 2, 7), (rows - 1, dim - 2))
    where = [r for r, _ in spots]
    for r, c in spots:
        x[r, c] = dy[r, c] = 1.0
    clean_f = {f: layernorm(lib, cuda, x, w, b, pe, y_prev, f) for f in ("plain", "acc")}
    clean_b = layernorm_bwd(lib, cuda, x, w, dy, None, False)
    xn, dyn = x.clone(), dy.clone()
    for r, c in spots:
        xn[r, c] = dyn[r, c] = NAN
    for f in ("plain", "acc"):
        _rows_contained(layernorm(lib, cuda, xn, w, b, pe, y_prev, f), clean_f[f], where)
    _rows_contained(layernorm_bwd(lib, cuda, xn, w, dy, None, False), clean_b, where)
    _rows_contained(layernorm_bwd(lib, cuda, x, w, dyn, None, False), clean_b, where)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------
def groupnorm(lib, cuda, x, w, b, two_stage):
    """-> (y, mean [F, 32], rstd [F, 32]) on the CPU; the two-stage workspace is poisoned with NaN as in test_groupnorm."""
    Fr, P, Cc = x.shape
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    y, stats = torch.full_like(xd, NAN), torch.full((Fr * E.GROUPS * 2,), NAN, device=cuda)
    nb = lib.edv_groupnorm_workspace(Fr, P, Cc) if two_stage else 0
    ws = torch.full((max(nb // 4, 4),), NAN, device=cuda)
    _lib.check(lib.edv_groupnorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), stats.data_ptr(), Fr, P, Cc, E.GROUPS, E.GN_EPS,
                                 ws.data_ptr() if two_stage else None, nb, st()), "edv_groupnorm")
    torch.cuda.synchronize()
    s = stats.cpu().reshape(Fr, E.GROUPS, 2)
    return y.cpu(), s[..., 0], s[..., 1]


def groupnorm_bwd(lib, cuda, x, w, b, dy, prev, acc, two_stage):
    """The forward (for the stats the backward consumes), then edv_groupnorm_bwd -> dx on the CPU."""
    Fr, P, Cc = x.shape
    xd, wd, bd, gd = x.to(cuda), w.to(cuda), b.to(cuda), dy.to(cuda)
    y, stats, sums = torch.empty_like(xd), torch.full((Fr * E.GROUPS * 2,), NAN, device=cuda), torch.full((Fr * E.GROUPS * 2,), NAN, device=cuda)
    nb = lib.edv_groupnorm_workspace(Fr, P, Cc) if two_stage else 0
    ws = torch.full((max(nb // 4, 4),), NAN, device=cuda)
    _lib.check(lib.edv_groupnorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), stats.data_ptr(), Fr, P, Cc, E.GROUPS, E.GN_EPS,
                                 ws.data_ptr() if two_stage else None, nb, st()), "edv_groupnorm")
    dx = prev.to(cuda) if acc else torch.full((Fr, P, Cc), NAN, device=cuda)
    _lib.check(lib.edv_groupnorm_bwd(xd.data_ptr(), stats.data_ptr(), wd.data_ptr(), gd.data_ptr(), sums.data_ptr(), dx.data_ptr(), Fr, P, Cc, E.GROUPS, int(acc),
                                     st()), "edv_groupnorm_bwd")
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize("Fr,P,Cc", GN_CASES)
@pytest.mark.parametrize("name", E.GN_CLASSES)
def test_groupnorm_edges_accuracy(lib, cuda, name, Fr, P, Cc):
    """Both statistics paths.  y per (frame, group) slab, the stats buffer the backward consumes (mean relative to the slab's mean |x|, rstd relative)
    against fp64, next to torch fp32 (group_norm; mean and var(unbiased=False) of the slab); and the two paths against each other under the same gates.

    Measured on an MI355X, worst over the three shapes: kernel / torch rms and max (largest error kernel | torch), strided path ; two-stage path:
    class           y                                                   mean                       rstd
    offset_1e3      0.51 0.27 (1.0e-3 | 3.9e-3) ; the same              0.24 0.22 ; 0.24 0.22      0.95 0.79 (7.9e-8 | 1.0e-7) ; the same
    chan_offsets    0.87 1.04 (2.1e-7 | 3.5e-7) ; 0.87 1.23             0.27 0.22 ; 0.28 0.25      1.04 1.27 ; 1.04 1.04
    outlier_pixel   1.13 1.24 (1.9e-7 | 1.6e-7) ; 1.27 1.24             0.36 0.34 ; 0.36 0.35      1.27 1.88 ; 1.37 1.92 (1.5e-7 | 7.8e-8)
    scaled_2p40     0.59 0.71 (1.8e-7 | 2.6e-7) ; 0.64 0.73             0.23 0.21 ; 0.23 0.21      0.95 1.20 ; 1.08 1.20
    const           exact (test_groupnorm_constant_slabs_are_exact); torch's fp32 group_norm is 1.8 of the slab's |b| off there
    Two-stage against strided: y within 1.94 x torch's error against fp64 (outlier_pixel), mean 0.49, rstd 2.86 (2.2e-7).
    This class found a defect.  Before the corrected two-pass form (norms.hip) offset_1e3 gave an rstd error of 2.1e-5 / 2.4e-5 / 1.5e-5 on the strided
    path (143 .. 264 x torch's 1e-7) and 1.7e-4 / 5.3e-5 / 2.2e-4 on the two-stage path: the fp32 mean of thousands of values near 1000 is a few
    ulps off (delta), the second pass returned var + delta^2, and a chunk mean rounded to fp32 entered the merge as spread between the chunks."""
    x, w, b = E.gn_operands(name, Fr, P, Cc)
    ref, ref_mean, ref_rstd, (t_y, t_mean, t_rstd) = E.gn_forward(name, Fr, P, Cc)
    outs = {}
    for two_stage in (False, True):
        y, mean, rstd = outs[two_stage] = groupnorm(lib, cuda, x, w, b, two_stage)
        assert torch.isfinite(y).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
        what = f"groupnorm {name} {'two_stage' if two_stage else 'strided'} ({Fr}, {P}, {Cc})"
        e_mean, e_rstd = E.gn_stats_error(mean, rstd, ref_mean, ref_rstd, x)
        report(what + " y", *E.slab_error(y, ref), t_y, E.FLOOR["gn"])
        report(what + " mean", *e_mean, t_mean, E.FLOOR["gn"])
        report(what + " rstd", *e_rstd, t_rstd, E.FLOOR["gn"])
    (ya, ma, ra), (yb, mb, rb) = outs[False], outs[True]
    what = f"groupnorm {name} two_stage against strided ({Fr}, {P}, {Cc})"
    e_mean, e_rstd = E.gn_stats_error(mb, rb, ma.double(), ra.double(), x)
    report(what + " y", *E.slab_error(yb, ya.double()), t_y, E.FLOOR["gn"])
    report(what + " mean", *e_mean, t_mean, E.FLOOR["gn"])
    report(what + " rstd", *e_rstd, t_rstd, E.FLOOR["gn"])


@pytest.mark.parametrize("Fr,P,Cc", GN_CASES)
@PATHS
def test_groupnorm_constant_slabs_are_exact(lib, cuda, Fr, P, Cc, two_stage):
    """One 12-bit value per (frame, group): y == b[c] bit for bit, the stored mean is the value, rstd is rsqrt(eps) to 1 ulp.  On the two-stage path
    the chunk mean multiplies by the reciprocal of the chunk's rows: exact because every chunk here holds a power-of-two number of rows."""
    x, w, b = E.gn_operands("const", Fr, P, Cc)
    y, mean, rstd = groupnorm(lib, cuda, x, w, b, two_stage)
    assert torch.equal(bits(y), bits(b.expand(Fr, P, Cc)))
    assert torch.equal(bits(mean), bits(E.gn_const_values(Fr)))
    want = torch.tensor(1.0 / math.sqrt(float(torch.tensor(E.GN_EPS, dtype=torch.float32))), dtype=torch.float32)  # correctly rounded: 1000.0
    assert (bits(rstd) - bits(want)).abs().max().item() <= 1, rstd


@pytest.mark.parametrize("Fr,P,Cc", GN_CASES)
@PATHS
@pytest.mark.parametrize("name", E.GN_CLASSES)
def test_groupnorm_bwd_edges_accuracy(lib, cuda, name, two_stage, Fr, P, Cc):
    """dx per slab against fp64 autograd next to torch's fp32 autograd, from the stats of either forward path (accumulating onto dx on the two-stage one).

    Measured on an MI355X, worst over the three shapes: kernel / torch rms and max, largest per-slab error kernel | torch:
    class           strided stats, store            two-stage stats, accumulate
    offset_1e3      0.19  0.19   2.4e-4 | 1.6e-3    0.19  0.18   2.4e-4 | 1.6e-3
    chan_offsets    1.11  1.21   2.3e-7 | 2.5e-7    1.00  1.00   5.8e-8 | 5.8e-8
    outlier_pixel   1.14  1.36   2.1e-7 | 2.6e-7    1.00  1.00   5.8e-8 | 5.8e-8
    scaled_2p40     1.02  0.99   1.7e-7 | 2.0e-7    1.00  1.00   (dx is 2^-40 of what it is added to)
    const           1.3e-7 against torch's 2.3e-3   1.6e-7 against 2.3e-3"""
    acc = two_stage
    x, w, b = E.gn_operands(name, Fr, P, Cc)
    dy, prev, ref, torch_err = E.gn_backward(name, Fr, P, Cc, acc)
    dx = groupnorm_bwd(lib, cuda, x, w, b, dy, prev, acc, two_stage)
    assert torch.isfinite(dx).all()
    report(f"groupnorm_bwd {name} {'two_stage acc' if two_stage else 'strided store'} ({Fr}, {P}, {Cc})", *E.slab_error(dx, ref), torch_err, E.FLOOR["gn"])


@pytest.mark.parametrize("Fr,P,Cc", GN_CASES)
def test_groupnorm_bwd_power_of_two_scaling_is_exact(lib, cuda, Fr, P, Cc):
    x, w, b = E.gn_operands("base", Fr, P, Cc)
    dy = E.bounded((Fr, P, Cc), 51)
    base = groupnorm_bwd(lib, cuda, x, w, b, dy, None, False, False)
    for s in E.BITWISE_SCALES:
        assert torch.equal(bits(groupnorm_bwd(lib, cuda, x, w, b, dy * 2.0 ** s, None, False, False)), bits(base * 2.0 ** s)), f"dy 2^{s} is not an exact scaling"


def _slab_contained(got, clean, f, g):
    touched = torch.zeros(E.slabs(clean).shape, dtype=torch.bool)
    touched[f, :, g] = True
    assert torch.isfinite(clean).all()
    assert torch.equal(bits(E.slabs(got))[~touched], bits(E.slabs(clean))[~touched]), "a NaN changed other (frame, group) slabs"
    assert not torch.isfinite(E.slabs(got)[touched]).all(), "the slab that holds the NaN is wholly finite"


@pytest.mark.parametrize("Fr,P,Cc", GN_CASES)
@PATHS
def test_groupnorm_non_finite_stays_in_its_slab(lib, cuda, Fr, P, Cc, two_stage):
    """A NaN at one element of slab (f, g) -- of x in the forward, of x and of dy in the backward -- leaves every other slab bit for bit what it
    is with 1.0 in its place.  (With 2 or 3 channels per group one thread's channel quad spans two or three groups.)"""
    x, w, b = (t.clone() for t in E.gn_operands("base", Fr, P, Cc))
    dy = E.uniform((Fr, P, Cc), 4)
    cg = Cc // E.GROUPS
    f, g, p = Fr - 1, 13, P - 1
    c = g * cg + cg - 1
    x[f, p, c] = dy[f, p, c] = 1.0
    clean_y = groupnorm(lib, cuda, x, w, b, two_stage)[0]
    clean_dx = groupnorm_bwd(lib, cuda, x, w, b, dy, None, False, two_stage)
    xn, dyn = x.clone(), dy.clone()
    xn[f, p, c] = dyn[f, p, c] = NAN
    _slab_contained(groupnorm(lib, cuda, xn, w, b, two_stage)[0], clean_y, f, g)
    _slab_contained(groupnorm_bwd(lib, cuda, xn, w, b, dy, None, False, two_stage), clean_dx, f, g)
    _slab_contained(groupnorm_bwd(lib, cuda, x, w, b, dyn, None, False, two_stage), clean_dx, f, g)
