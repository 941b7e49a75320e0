"""The parameter-gradient reductions on the operands of tests/grad_inputs.py: edv_lora_grads, edv_colsum_rows, edv_col_dot, edv_colsum_batch and,
through the adjoint identity, edv_fold_lora.

  exact        integer operands whose answer is the int64 one in any summation order, bit for bit: a dropped split, a cut 64-column block, a lost
               K tail or a swapped index cannot hide inside a tolerance (tests/test_grad_inputs_cpu.py shows the operands see each of them)
  scaling      operands times 2^+-40 give ldexp of the base result bit for bit
  accuracy     outlier, heavy-tailed, offset, cancelling and last-split-only operands against fp64, per element, under two gates:
               (a) err <= u (d_outer mag_outer + d_inner mag_inner) with the roundings counted from the kernels (grad_inputs.lora_depths, colsum_depth,
               coldot_depth, batch_depth), (b) rms and max within 4 x torch fp32's on the same operands (edge_inputs.gate_failures, floor u)
  containment  a NaN in one column stays in the outputs that column feeds
  bounds       every output between NaN guard bands, every workspace exactly its advertised size inside a NaN-filled buffer, pre-filled with NaN
  determinism  two runs, identical bits

No yardstick is the global close(): a column wrong by a thousand times its own rounding error must not pass because another column is large."""
import ctypes as C

import pytest
import torch

from endodav_amd import _lib
from tests import grad_inputs as V

pytestmark = pytest.mark.gpu

U = V.U
NAN = float("nan")
GUARD = 64  # floats on either side of every output and workspace (a multiple of 4: what lies between stays 16-byte aligned)
sid = lambda shape: "x".join(str(int(v)) for v in shape)
ids = lambda cases: [f"{c}-{sid(s)}" for c, s in cases]


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n, cuda, init=None):
    """(buffer, view of n floats between two NaN guard bands); the view starts as NaN or as `init`."""
    big = torch.full((n + 2 * GUARD,), NAN, device=cuda)
    if init is not None:
        big[GUARD:GUARD + n] = init.reshape(-1).to(cuda)
    return big, big[GUARD:GUARD + n]


def guards_intact(big, n):
    return bool(torch.isnan(big[:GUARD]).all() and torch.isnan(big[GUARD + n:]).all())


def dev(t, cuda):
    return None if t is None else t.contiguous().to(cuda)


def same_bits(a, b):
    return torch.equal(V.bits(a), V.bits(b))


def check_accuracy(what, got, ref, mag_outer, d_outer, torch_err, mag_inner=None, d_inner=0):
    """Both gates on one output; prints the kernel-to-torch ratios and the worst error in u next to the derived bound."""
    yard = mag_outer if mag_inner is None else mag_inner
    rms, mx = V.elem_error(got, ref, yard)
    worst = V.bound_ratio(got, ref, mag_outer, d_outer, mag_inner, d_inner)
    print(f"\n[{what}] {V.ratios(rms, mx, torch_err)} | max {mx / U:.2f}u | {worst:.3f} of the bound u ({d_outer} mag_outer + {d_inner} mag_inner)")
    bad = V.gate_failures(rms, mx, torch_err, U)
    if not worst <= 1:
        bad.append(f"an element is {worst:.2f} x u ({d_outer} mag_outer + {d_inner} mag_inner)")
    return [f"{what}: {b}" for b in bad]


# ---- edv_lora_grads ----------------------------------------------------------------------------------------------------------------------
def lora_run(lib, cuda, o, runs=2):
    """edv_lora_grads on CPU operands -> {dA, dB, dU, dV} on the CPU.  Outputs and workspace sit between NaN guard bands, the workspace has exactly
    edv_lora_grads_workspace bytes and starts as NaN, and `runs` launches must agree bit for bit."""
    M, nin = o.x.shape
    nout, r = o.B.shape
    xd, Gd, Ad, Bd, Ud, Vd, gd = (dev(t, cuda) for t in (o.x, o.G, o.A, o.B, o.U, o.V, o.gamma))
    nb = lib.edv_lora_grads_workspace(M, nin, nout, r)
    sizes = {"dA": r * nin, "dB": nout * r, "dU": r, "dV": nout}
    names = V.lora_outputs(o)
    results = []
    for _ in range(runs):
        ws_big, ws = guarded(nb // 4, cuda)
        outs = {n: guarded(sizes[n], cuda) for n in names}
        p = lambda n: outs[n][1].data_ptr() if n in outs else None
        _lib.check(lib.edv_lora_grads(xd.data_ptr(), Gd.data_ptr(), M, nin, nout, r, Ad.data_ptr(), Bd.data_ptr(), _lib.ptr(Ud) or None, _lib.ptr(Vd) or None,
                                      o.s, _lib.ptr(gd) or None, ws.data_ptr(), nb, p("dA"), p("dB"), p("dU"), p("dV"), st()), "edv_lora_grads")
        torch.cuda.synchronize()
        assert guards_intact(ws_big, nb // 4), "a write outside the workspace"
        for n in names:
            assert guards_intact(outs[n][0], sizes[n]), f"a write outside {n}"
        results.append({n: outs[n][1].cpu() for n in names})
    for n in names:
        assert all(same_bits(results[0][n], q[n]) for q in results[1:]), f"{n} is not bit-reproducible"
    shapes = {"dA": (r, nin), "dB": (nout, r), "dU": (r, 1), "dV": (nout, 1)}
    return {n: results[0][n].view(shapes[n]) for n in names}


@pytest.mark.parametrize("shape", V.LORA_SHAPES, ids=sid)
def test_lora_grads_exact(lib, cuda, shape):
    o = V.lora_operands("exact_int", shape)
    got, want = lora_run(lib, cuda, o), V.lora_formula(o, torch.int64)
    for n in V.lora_outputs(o):
        bad = (got[n].double() != want[n].double()).nonzero()
        assert len(bad) == 0, f"{n}: {len(bad)} of {want[n].numel()} differ from the int64 answer, first at {tuple(bad[0].tolist())}: " \
                              f"got {got[n][tuple(bad[0])].item()}, want {want[n][tuple(bad[0])].item()}"


@pytest.mark.parametrize("shape", V.LORA_SHAPES, ids=sid)
def test_lora_grads_scale_bit_for_bit(lib, cuda, shape):
    """G 2^s and x 2^s give ldexp of the base result, G 2^40 with x 2^-40 the base bits."""
    base = lora_run(lib, cuda, V.lora_scaled(shape, 0, 0), runs=1)
    for pg, px in [(p, 0) for p in V.BITWISE_SCALES] + [(0, p) for p in V.BITWISE_SCALES] + [(40, -40)]:
        got = lora_run(lib, cuda, V.lora_scaled(shape, pg, px), runs=1)
        for n, b in base.items():
            assert torch.isfinite(got[n]).all() and same_bits(got[n], b * 2.0 ** (pg + px)), f"{n}: G 2^{pg}, x 2^{px} is not ldexp(base, {pg + px})"


LORA_ACC = V.lora_cases(V.ACCURACY_CLASSES)


@pytest.mark.parametrize("cls,shape", LORA_ACC, ids=ids(LORA_ACC))
def test_lora_grads_accuracy(lib, cuda, cls, shape):
    """Every element within u (d_outer mag_outer + d_inner mag_inner), the roundings on the longest path through the kernels:
      d_inner  lora_factors_kernel (A U: 1 for DV-LoRA; B V gamma: 2), then skinny_xwt_kernel: a product, the four-term tree (2), one addition per
               256-column step (ceil(K / 256)), the wave butterfly (6)
      d_outer  tall_tn: the product y T (1), ceil(rows_per_split / 4) additions in a wave, 2 to join the waves, ceil(splits / 8) in a slice of
               the reduce kernel, 7 to join its slices, scale and rowscale (2); then lora_grad_finalize_kernel: x V or x U (1 for DV-LoRA); dV adds
               a product and r additions; dU (lora_grad_u_kernel) a product, ceil(nin / 256) additions, the wave butterfly (6) and 2 to join the waves
    and rms and max of err / mag_inner within 4 x torch's fp32 autograd on the same operands."""
    c = V.lora_class(cls, shape)
    got, bad = lora_run(lib, cuda, c.ops), []
    for n in V.lora_outputs(c.ops):
        (mo, mi), (do, di) = c.mags[n], c.depths[n]
        bad += check_accuracy(f"lora {cls} {sid(shape)} {n}", got[n], c.ref[n], mo, do, c.torch_err[n], mi, di)
    assert not bad, "; ".join(bad)


def _nan_rows(M):
    """The first row and a row of the last, short split."""
    return sorted({0, M - 1})


@pytest.mark.parametrize("shape", V.LORA_SHAPES, ids=sid)
def test_lora_grads_contain_a_nan(lib, cuda, shape):
    """A NaN in G[m0, n0] reaches u[m0, :], hence all of dA and dU, but of dB and dV only row n0; a NaN in x[m0, k0] reaches t[m0, :], hence all of
    dB and dV, but of dA only column k0."""
    M, nin, nout, r = shape
    o = V.lora_class("offset", shape).ops
    clean = lora_run(lib, cuda, o, runs=1)
    n0, k0 = nout // 2 + 1, nin // 2 + 1  # inside a float4, next to clean neighbours
    others = lambda n, i: torch.arange(n) != i
    for m0 in _nan_rows(M):
        G = o.G.clone()
        G[m0, n0] = NAN
        got = lora_run(lib, cuda, V.SimpleNamespace(**{**vars(o), "G": G}), runs=1)
        assert torch.isnan(got["dB"][n0]).all() and same_bits(got["dB"][others(nout, n0)], clean["dB"][others(nout, n0)]), f"G[{m0}, {n0}]: dB"
        if o.dv:
            assert torch.isnan(got["dV"][n0]).all() and same_bits(got["dV"][others(nout, n0)], clean["dV"][others(nout, n0)]), f"G[{m0}, {n0}]: dV"
        x = o.x.clone()
        x[m0, k0] = NAN
        got = lora_run(lib, cuda, V.SimpleNamespace(**{**vars(o), "x": x}), runs=1)
        assert torch.isnan(got["dA"][:, k0]).all() and same_bits(got["dA"][:, others(nin, k0)], clean["dA"][:, others(nin, k0)]), f"x[{m0}, {k0}]: dA"


# ---- fold <-> gradient -------------------------------------------------------------------------------------------------------------------
def fold(lib, cuda, o, W):
    nout, r = o.B.shape
    nin = o.A.shape[1]
    Wd, Ad, Bd, Ud, Vd = (dev(t, cuda) for t in (W, o.A, o.B, o.U, o.V))
    big, out = guarded(nout * nin, cuda)
    _lib.check(lib.edv_fold_lora(Wd.data_ptr(), Ad.data_ptr(), Bd.data_ptr(), _lib.ptr(Ud) or None, _lib.ptr(Vd) or None, o.s, out.data_ptr(), nout, nin, r, st()),
               "edv_fold_lora")
    torch.cuda.synchronize()
    assert guards_intact(big, nout * nin), "edv_fold_lora wrote outside its output"
    return out.view(nout, nin)


@pytest.mark.parametrize("shape", V.ADJOINT_SHAPES, ids=sid)
def test_fold_is_the_adjoint_of_the_gradient(lib, cuda, shape):
    """y = x fold(A, B, U, V)^T gamma is linear in each factor, so <G, x (fold(F + D) - fold(F))^T gamma> = <dF, D> exactly on integer operands
    with an integer direction D: the left side from edv_fold_lora and edv_gemm, the right side from edv_lora_grads, both summed in int64."""
    M, nin, nout, r = shape
    o = V.lora_operands("exact_int", shape)
    W = V.integers((nout, nin), 9, 8)
    grads = lora_run(lib, cuda, o, runs=1)
    f0 = fold(lib, cuda, o, W)
    assert torch.equal(f0.cpu().long(), V.fold_reference(o, torch.int64, W)), "edv_fold_lora differs from the int64 fold"
    xd, gd = dev(o.x, cuda), dev(o.gamma, cuda)
    for name, D in V.adjoint_directions(o).items():
        moved = V.SimpleNamespace(**{**vars(o), name: getattr(o, name) + D})
        dW = (fold(lib, cuda, moved, W) - f0).contiguous()
        y = torch.full((M, nout), NAN, device=cuda)
        _lib.check(lib.edv_gemm(xd.data_ptr(), dW.data_ptr(), y.data_ptr(), M, nout, nin, None, 0, _lib.ptr(gd) or None, None, None, 0, st()), "edv_gemm")
        torch.cuda.synchronize()
        lhs = int((o.G.long() * y.cpu().long()).sum())
        rhs = int((grads["d" + name].long() * D.long()).sum())
        want = int((V.lora_formula(o, torch.int64)["d" + name] * D.long()).sum())
        assert lhs == rhs == want and want != 0, f"direction in {name}: <G, dy> = {lhs}, <d{name}, D> = {rhs}, int64 {want}"


# ---- edv_colsum_rows ---------------------------------------------------------------------------------------------------------------------
def colsum_run(lib, cuda, shape, P, rs, base, runs=2):
    M, N = shape
    Pd, rd = dev(P, cuda), dev(rs, cuda)
    nb = lib.edv_colsum_workspace(N)
    results = []
    for _ in range(runs):
        ws_big, ws = guarded(nb // 4, cuda)
        big, out = guarded(N, cuda, base)
        _lib.check(lib.edv_colsum_rows(Pd.data_ptr(), _lib.ptr(rd) or None, M, N, ws.data_ptr(), nb, out.data_ptr(), int(base is not None), st()), "edv_colsum_rows")
        torch.cuda.synchronize()
        assert guards_intact(ws_big, nb // 4) and guards_intact(big, N), "a write outside the workspace or the output"
        results.append(out.cpu())
    assert all(same_bits(results[0], q) for q in results[1:]), "colsum_rows is not bit-reproducible"
    return results[0]


@pytest.mark.parametrize("shape", V.COLSUM_SHAPES, ids=sid)
def test_colsum_rows_exact_and_scaled(lib, cuda, shape):
    c = V.colsum_class("exact_int", shape)
    got = colsum_run(lib, cuda, shape, c.P, c.rs, c.base)
    assert torch.equal(got.double(), c.ref), f"differs from the int64 answer in columns {(got.double() != c.ref).nonzero().flatten().tolist()[:8]}"
    base = colsum_run(lib, cuda, shape, *V.colsum_scaled(shape, 0), runs=1)
    for p in V.BITWISE_SCALES:
        got = colsum_run(lib, cuda, shape, *V.colsum_scaled(shape, p), runs=1)
        assert torch.isfinite(got).all() and same_bits(got, base * 2.0 ** p), f"P 2^{p} is not ldexp(base, {p})"


COLSUM_ACC = V.colsum_cases(V.ACCURACY_CLASSES)


@pytest.mark.parametrize("cls,shape", COLSUM_ACC, ids=ids(COLSUM_ACC))
def test_colsum_rows_accuracy(lib, cuda, cls, shape):
    """Every column within depth x u of sum_m |rowscale_m P_mn| (+ |what out held|): a product with the row scale (1), one addition per lap of the
    grid-stride loop, 256 / n4 additions of the threads that share a column group, ceil(blocks / 8) partials in sequence and 7 to join the slices,
    2 for the fold, 1 to accumulate; and within 4 x torch fp32's sum."""
    c = V.colsum_class(cls, shape)
    got = colsum_run(lib, cuda, shape, c.P, c.rs, c.base)
    bad = check_accuracy(f"colsum_rows {cls} {sid(shape)}", got, c.ref, c.mag, c.depth, c.torch_err)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("shape", [s for s in V.COLSUM_SHAPES if s[1] > 1], ids=sid)
def test_colsum_rows_contain_a_nan(lib, cuda, shape):
    """A NaN in column n0 shows in out[n0] alone, its float4 neighbours included; once in the first row, once in the ragged last lap."""
    M, N = shape
    c = V.colsum_class("offset", shape)
    clean = colsum_run(lib, cuda, shape, c.P, c.rs, c.base, runs=1)
    n0 = N // 2 + 1
    rest = torch.arange(N) != n0
    for m0 in _nan_rows(M):
        P = c.P.clone()
        P[m0, n0] = NAN
        got = colsum_run(lib, cuda, shape, P, c.rs, c.base, runs=1)
        assert torch.isnan(got[n0]) and same_bits(got[rest], clean[rest]), f"P[{m0}, {n0}]"


# ---- edv_col_dot -------------------------------------------------------------------------------------------------------------------------
def coldot_run(lib, cuda, shape, P, Q, scale, runs=2):
    M, N = shape
    Pd, Qd, sd = dev(P, cuda), dev(Q, cuda), dev(scale, cuda)
    results = []
    for _ in range(runs):
        ws_big, part = guarded(V.TALL_SPLITS * N, cuda)
        big, out = guarded(N, cuda)
        _lib.check(lib.edv_col_dot(Pd.data_ptr(), _lib.ptr(Qd) or None, M, N, _lib.ptr(sd) or None, part.data_ptr(), out.data_ptr(), st()), "edv_col_dot")
        torch.cuda.synchronize()
        assert guards_intact(ws_big, V.TALL_SPLITS * N) and guards_intact(big, N), "a write outside the partials or the output"
        results.append(out.cpu())
    assert all(same_bits(results[0], q) for q in results[1:]), "col_dot is not bit-reproducible"
    return results[0]


@pytest.mark.parametrize("shape", V.COLDOT_SHAPES, ids=sid)
def test_col_dot_exact_and_scaled(lib, cuda, shape):
    for use_q, use_s in V.COLDOT_VARIANTS:
        c = V.coldot_class("exact_int", shape, use_q, use_s)
        got = coldot_run(lib, cuda, shape, c.P, c.Q, c.scale)
        assert torch.equal(got.double(), c.ref), f"Q={use_q} scale={use_s}: columns {(got.double() != c.ref).nonzero().flatten().tolist()[:8]} differ from the int64 answer"
        c = V.coldot_class("scaled", shape, use_q, use_s)
        base = coldot_run(lib, cuda, shape, c.P, c.Q, c.scale, runs=1)
        for p in V.BITWISE_SCALES:
            got = coldot_run(lib, cuda, shape, c.P * 2.0 ** p, c.Q, c.scale, runs=1)
            assert torch.isfinite(got).all() and same_bits(got, base * 2.0 ** p), f"Q={use_q} scale={use_s}: P 2^{p} is not ldexp(base, {p})"


COLDOT_ACC = V.coldot_cases(V.ACCURACY_CLASSES)


@pytest.mark.parametrize("cls,shape", COLDOT_ACC, ids=ids(COLDOT_ACC))
def test_col_dot_accuracy(lib, cuda, cls, shape):
    """test_col_dot's count -- ceil(rows_per_split / 4) + 2 + ceil(splits / 8) + 7, one rounding for the product, one for the scale -- on every
    column, relative to |scale_n| sum_m |P Q|; and within 4 x torch fp32's."""
    bad = []
    for use_q, use_s in V.COLDOT_VARIANTS:
        c = V.coldot_class(cls, shape, use_q, use_s)
        got = coldot_run(lib, cuda, shape, c.P, c.Q, c.scale)
        bad += check_accuracy(f"col_dot {cls} {sid(shape)} Q={int(use_q)} scale={int(use_s)}", got, c.ref, c.mag, c.depth, c.torch_err)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("shape", [s for s in V.COLDOT_SHAPES if s[1] > 1], ids=sid)
def test_col_dot_contains_a_nan(lib, cuda, shape):
    M, N = shape
    c = V.coldot_class("offset", shape, True, True)
    clean = coldot_run(lib, cuda, shape, c.P, c.Q, c.scale, runs=1)
    n0 = N // 2 + 1
    rest = torch.arange(N) != n0
    for m0 in _nan_rows(M):
        P = c.P.clone()
        P[m0, n0] = NAN
        got = coldot_run(lib, cuda, shape, P, c.Q, c.scale, runs=1)
        assert torch.isnan(got[n0]) and same_bits(got[rest], clean[rest]), f"P[{m0}, {n0}]"


# ---- edv_colsum_batch --------------------------------------------------------------------------------------------------------------------
def batch_run(lib, cuda, cases, srcs=None, runs=2):
    """One edv_colsum_batch call for all jobs of `cases` (a list of grad_inputs.batch_class results) -> list of outputs on the CPU."""
    n = len(cases)
    jobs = [c.job for c in cases]
    src = [dev(s, cuda) for s in (srcs or [c.src for c in cases])]
    sc = [dev(c.sc, cuda) for c in cases]
    rows_ = (C.c_int64 * n)(*[j["M"] for j in jobs])
    cols = (C.c_int32 * n)(*[j["N"] for j in jobs])
    nbytes = lib.edv_colsum_batch_workspace(n, rows_, cols)
    results = []
    for _ in range(runs):
        ws_big, ws = guarded(nbytes // 4, cuda)
        dsts = [guarded(j["N"], cuda, c.init) for j, c in zip(jobs, cases)]
        _lib.check(lib.edv_colsum_batch(n, (C.c_void_p * n)(*[s.data_ptr() for s in src]), (C.c_int64 * n)(*[j["ld"] for j in jobs]), rows_,
                                        (C.c_int32 * (3 * n))(*[v for j in jobs for v in j["map"]]), cols,
                                        (C.c_void_p * n)(*[(s.data_ptr() if s is not None else None) for s in sc]),
                                        (C.c_void_p * n)(*[d[1].data_ptr() for d in dsts]), (C.c_int32 * n)(*[int(j["acc"]) for j in jobs]),
                                        ws.data_ptr(), nbytes, _lib.stream_ptr(cuda)), "edv_colsum_batch")
        torch.cuda.synchronize()
        assert guards_intact(ws_big, nbytes // 4), "a write outside the workspace"
        for k, (j, d) in enumerate(zip(jobs, dsts)):
            assert guards_intact(d[0], j["N"]), f"job {k}: a write outside its output"
        results.append([d[1].cpu() for d in dsts])
    for k in range(n):
        assert all(same_bits(results[0][k], q[k]) for q in results[1:]), f"job {k} is not bit-reproducible"
    return results[0]


def batch_cases(cls):
    return [V.batch_class(cls, k) for k in range(len(V.BATCH_JOBS))]


def test_colsum_batch_exact_and_scaled(lib, cuda):
    """The padding columns (ld > N) and the cls rows the patch RowMap skips hold NaN: a read that strays poisons the exact answer."""
    cases = batch_cases("exact_int")
    for k, (got, c) in enumerate(zip(batch_run(lib, cuda, cases), cases)):
        assert torch.equal(got.double(), c.ref), f"job {k}: columns {(got.double() != c.ref).nonzero().flatten().tolist()[:8]} differ from the int64 answer"
    cases = batch_cases("scaled")
    base = batch_run(lib, cuda, cases, runs=1)
    for p in V.BITWISE_SCALES:
        moved = [V.SimpleNamespace(**{**vars(c), "init": None if c.init is None else c.init * 2.0 ** p}) for c in cases]
        got = batch_run(lib, cuda, moved, [c.src * 2.0 ** p for c in cases], runs=1)
        for k in range(len(cases)):
            assert torch.isfinite(got[k]).all() and same_bits(got[k], base[k] * 2.0 ** p), f"job {k}: P 2^{p} is not ldexp(base, {p})"


@pytest.mark.parametrize("cls", V.ACCURACY_CLASSES)
def test_colsum_batch_accuracy(lib, cuda, cls):
    """Every column within depth x u of |scale_n| sum_m |P_mn| (+ |what dst held|).  Stage 1: a row lane walks ceil(chunk / lanes) rows on four
    accumulators (a quarter each, up to 3 leftovers on the first), the accumulators and the row lanes are joined in fp64 and rounded once (1); stage 2
    adds the parts in sequence; one rounding for the scale, one to accumulate.  And within 4 x torch fp32's sum."""
    cases, bad = batch_cases(cls), []
    for k, (got, c) in enumerate(zip(batch_run(lib, cuda, cases), cases)):
        bad += check_accuracy(f"colsum_batch {cls} job {k} N={c.job['N']} M={c.job['M']}", got, c.ref, c.mag, c.depth, c.torch_err)
    assert not bad, "; ".join(bad)


def test_colsum_batch_contains_a_nan(lib, cuda):
    """A NaN in column n0 of job k0 shows in that output element alone: not in its neighbours, not in the jobs next to it in the slab."""
    cases = batch_cases("offset")
    clean = batch_run(lib, cuda, cases, runs=1)
    for k0 in (2, 4):  # an identity job and the patch-map job
        j = cases[k0].job
        n0 = j["N"] // 2 + 1
        for m0 in _nan_rows(j["M"]):
            srcs = [c.src for c in cases]
            srcs[k0] = srcs[k0].clone()
            srcs[k0][j["rows"][m0], n0] = NAN
            got = batch_run(lib, cuda, cases, srcs, runs=1)
            for k in range(len(cases)):
                rest = torch.ones(cases[k].job["N"], dtype=torch.bool)
                if k == k0:
                    rest[n0] = False
                    assert torch.isnan(got[k][n0]), f"job {k0}: the NaN in row {m0} did not arrive"
                assert same_bits(got[k][rest], clean[k][rest]), f"NaN in job {k0} row {m0} column {n0} reached job {k}"
