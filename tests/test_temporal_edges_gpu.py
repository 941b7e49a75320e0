"""Temporal attention forward and backward (temporal.hip, bwd.hip) at numeric edges, one shape per kernel instantiation the dispatch reaches without
an environment variable (forward small<4>, small<8>, pixel<8>, <16>, <32>, <64>; backward pixel<8>, <16>, <32>), every T below its template
bound so that padded frames are in play: q / k outlier dimensions, a score offset of about 500, a v outlier channel, all-zero scores, identical
keys in every frame, T = 1, exact power-of-two scaling, and where a NaN / Inf may and may not show.

Yardstick: X.column_error (per output column; on the dq, dk and dv thirds separately for the backward) next to torch's own fp32 attention / autograd
on the CPU.  Inputs, references and the restated dispatch: tests/edge_inputs.py, checked by tests/test_edge_inputs_cpu.py."""
import pytest
import torch

from endodav_amd import _lib

from . import edge_inputs as E
from .edge_inputs import HEADS, bits
from .test_kernels_gpu import st

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
FWD = [pytest.param(*s, id=k) for k, s in E.TATTN_FWD_SHAPES.items()]
BWD = [pytest.param(*s, id=k) for k, s in E.TATTN_BWD_SHAPES.items()]
T1 = [pytest.param(*s, id="d{}".format(s[3] // HEADS)) for s in E.TATTN_T1_SHAPES]


def tattn(lib, cuda, qkv, B, T, P, Cc):
    qd = qkv.to(cuda)
    o = torch.full((B * T * P, Cc), NAN, device=cuda)
    _lib.check(lib.edv_attn_temporal(qd.data_ptr(), o.data_ptr(), B, T, P, Cc, HEADS, st()), "edv_attn_temporal")
    torch.cuda.synchronize()
    return o.cpu()


def tattn_bwd(lib, cuda, qkv, dO, B, T, P, Cc):
    qd, gd = qkv.to(cuda), dO.to(cuda)
    dq = torch.full((B * T * P, 3 * Cc), NAN, device=cuda)
    _lib.check(lib.edv_attn_temporal_bwd(qd.data_ptr(), gd.data_ptr(), dq.data_ptr(), B, T, P, Cc, HEADS, st()), "edv_attn_temporal_bwd")
    torch.cuda.synchronize()
    return dq.cpu()


@pytest.mark.parametrize("B,T,P,Cc", FWD)
@pytest.mark.parametrize("name", E.TATTN_CLASSES)
def test_tattn_edges_accuracy(lib, cuda, name, B, T, P, Cc):
    """Per-column error against the fp64 attention next to torch's fp32 attention.

    Measured on an MI355X, worst over the six instantiations: kernel / torch rms and max, largest per-column error kernel | torch:
    qk_outlier    1.01  1.50   3.9e-6 | 5.6e-6
    shifted       0.91  1.06   8.9e-5 | 1.3e-4    (fp32 scores near 500 lose 2^-15: torch alike; no stored log-sum-exp here, the maximum is subtracted)
    v_outlier     1.14  1.30   4.3e-7 | 4.8e-7
    q_2m100       1.19  1.46   4.1e-7 | 4.5e-7
    same_frames   1.40  1.38   4.1e-7 | 4.5e-7"""
    qkv, ref, torch_err = E.tattn_class(name, B, T, P, Cc)
    o = tattn(lib, cuda, qkv, B, T, P, Cc)
    assert torch.isfinite(o).all()
    rms, mx = E.column_error(o, ref)
    what = f"attn_temporal {name} ({B}, {T}, {P}, {Cc})"
    print(f"\n[{what}] {E.ratios(rms, mx, torch_err)}")
    bad = E.gate_failures(rms, mx, torch_err, E.FLOOR["tattn_fwd"])
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.parametrize("B,T,P,Cc", BWD)
@pytest.mark.parametrize("name", E.TATTN_CLASSES)
def test_tattn_bwd_edges_accuracy(lib, cuda, name, B, T, P, Cc):
    """dq, dk, dv per column against fp64 autograd next to torch's fp32 autograd.

    With the same key in every frame dq is exactly zero; its error is then divided by the size of the terms that cancel (E.tattn_dq_scale).

    Measured on an MI355X, worst over the four shapes: kernel / torch rms and max (largest per-column error kernel | torch):
    class         dq                             dk                             dv
    qk_outlier    1.02 0.97  4.3e-6 | 4.5e-6     1.01 1.04  5.0e-6 | 4.8e-6     1.04 1.17  8.8e-7 | 1.4e-6
    shifted       0.94 1.14  1.1e-4 | 1.3e-4     0.89 0.91  5.3e-5 | 1.0e-4     0.91 0.92  6.7e-5 | 1.2e-4
    v_outlier     0.98 1.19  4.9e-7 | 6.5e-7     0.99 1.75  6.4e-7 | 5.7e-7     0.99 1.16  4.0e-7 | 4.1e-7
    q_2m100       1.10 1.00  3.5e-7 | 3.5e-7     1.02 1.04  3.5e-7 | 4.0e-7     1.22 1.26  2.7e-7 | 2.4e-7
    same_frames   1.36 1.45  1.5e-7 | 1.5e-7     1.02 1.04  3.5e-7 | 4.0e-7     1.12 1.12  2.7e-7 | 2.4e-7"""
    qkv, dO, ref, torch_err, dq_scale = E.tattn_bwd_class(name, B, T, P, Cc)
    dqkv = tattn_bwd(lib, cuda, qkv, dO, B, T, P, Cc)
    assert torch.isfinite(dqkv).all()
    errs = E.thirds_error(dqkv, ref, dq_scale)
    what = f"attn_temporal_bwd {name} ({B}, {T}, {P}, {Cc})"
    for n in E.THIRDS:
        print(f"\n[{what} {n}] {E.ratios(*errs[n], torch_err[n])}")
    bad = [f"{n}: {b}" for n in E.THIRDS for b in E.gate_failures(*errs[n], torch_err[n], E.FLOOR["tattn_bwd"])]
    assert not bad, f"{what}: " + "; ".join(bad)


@pytest.mark.parametrize("B,T,P,Cc", T1)
def test_tattn_single_frame_is_the_identity(lib, cuda, B, T, P, Cc):
    """T = 1: the one probability is exp(0) / 1 = 1, so out == v bit for bit; dS = 1 (dP - 1 dP) = 0, so dq == 0, dk == 0 and dv == dO bit for bit."""
    qkv, dO = E.tattn_base(B, T, P, Cc), E.tattn_dO(B, T, P, Cc)
    assert torch.equal(bits(tattn(lib, cuda, qkv, B, T, P, Cc)), bits(qkv[:, 2 * Cc:]))
    g = E.thirds(tattn_bwd(lib, cuda, qkv, dO, B, T, P, Cc))
    assert torch.count_nonzero(g["dq"]) == 0 and torch.count_nonzero(g["dk"]) == 0
    assert torch.equal(bits(g["dv"]), bits(dO))


@pytest.mark.parametrize("B,T,P,Cc", FWD)
def test_tattn_edges_power_of_two_scaling_is_exact(lib, cuda, B, T, P, Cc):
    """out(q, k, v 2^s) is ldexp(out, s) bit for bit at s = +-40, and out(q 2^40, k 2^-40, v) is out(q, k, v)."""
    qkv, _ = E.tattn_bounded(B, T, P, Cc)
    base = tattn(lib, cuda, qkv, B, T, P, Cc)
    assert torch.isfinite(base).all()
    for s in E.BITWISE_SCALES:
        scaled = qkv.clone()
        scaled[:, 2 * Cc:] *= 2.0 ** s
        assert torch.equal(bits(tattn(lib, cuda, scaled, B, T, P, Cc)), bits(base * 2.0 ** s)), f"v 2^{s} is not an exact scaling"
    scaled = qkv.clone()
    scaled[:, :Cc] *= 2.0 ** 40
    scaled[:, Cc:2 * Cc] *= 2.0 ** -40
    assert torch.equal(bits(tattn(lib, cuda, scaled, B, T, P, Cc)), bits(base)), "q 2^40, k 2^-40 changes the result"


@pytest.mark.parametrize("B,T,P,Cc", BWD)
def test_tattn_bwd_edges_power_of_two_scaling_is_exact(lib, cuda, B, T, P, Cc):
    """dqkv(dO 2^s) is ldexp(dqkv(dO), s) bit for bit at s = +-40."""
    qkv, dO = E.tattn_bounded(B, T, P, Cc)
    base = tattn_bwd(lib, cuda, qkv, dO, B, T, P, Cc)
    assert torch.isfinite(base).all()
    for s in E.BITWISE_SCALES:
        assert torch.equal(bits(tattn_bwd(lib, cuda, qkv, dO * 2.0 ** s, B, T, P, Cc)), bits(base * 2.0 ** s)), f"dO 2^{s} is not an exact scaling"


SPOTS = [("q", NAN, False), ("k", NAN, False), ("v", NAN, False), ("v", INF, True)]


def _contained(got, clean, B, T, P, Cc, b, p, head, parts, what):
    """Everything outside (b, every t, p, head) keeps the clean run's bits; inside, not everything is finite."""
    touched = torch.zeros(B, T, P, parts, HEADS, Cc // HEADS, dtype=torch.bool)
    touched[b, :, p, :, head] = True
    touched = touched.reshape(B * T * P, parts * Cc)
    assert torch.isfinite(clean).all()
    assert torch.equal(bits(got)[~touched], bits(clean)[~touched]), f"{what} changed values outside its (clip, pixel, head)"
    assert not torch.isfinite(got[touched]).all(), f"{what} left no trace in its (clip, pixel, head)"


@pytest.mark.parametrize("B,T,P,Cc", FWD)
def test_tattn_edges_non_finite_stays_in_its_pixel_and_head(lib, cuda, B, T, P, Cc):
    """A NaN in q, k or v of (b, t, p, head), and an Inf in v of the LAST frame (the row the clamped loads of the padded frames j >= T duplicate,
    times a zero probability), stay in (b, every t, p, head); forward, and backward where T <= 32 (there also a NaN in dO)."""
    qkv, dO = E.tattn_base(B, T, P, Cc), E.tattn_dO(B, T, P, Cc)
    b, p, head, c = B - 1, P // 2, 5, 3
    backward = T <= 32
    for part, value, last in SPOTS + ([("dO", NAN, False)] if backward else []):
        t = T - 1 if last else T // 2
        row = (b * T + t) * P + p
        src = dO if part == "dO" else qkv
        col = head * (Cc // HEADS) + c + (0 if part == "dO" else "qkv".index(part) * Cc)
        keep = src[row, col].item()
        src[row, col] = 1.0
        clean_f = tattn(lib, cuda, qkv, B, T, P, Cc)
        clean_b = tattn_bwd(lib, cuda, qkv, dO, B, T, P, Cc) if backward else None
        src[row, col] = value
        what = f"a {value} in {part} of frame {t}"
        if part != "dO":
            _contained(tattn(lib, cuda, qkv, B, T, P, Cc), clean_f, B, T, P, Cc, b, p, head, 1, what + " (forward)")
        if backward:
            _contained(tattn_bwd(lib, cuda, qkv, dO, B, T, P, Cc), clean_b, B, T, P, Cc, b, p, head, 3, what + " (backward)")
        src[row, col] = keep
