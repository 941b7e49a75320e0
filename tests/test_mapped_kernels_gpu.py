"""Per-kernel parity on MI355X for the operator forms only the engine reaches: GEMM descriptors with row maps, a broadcast residual, a
pre-activation addend, two residuals, leading dimensions and bf16 planes (edv_gemm_desc -> gemm(), so the dispatcher is under test), LayerNorm
forward / backward with row maps, activation and accumulation, the weight folds, col_dot, ssb_prep, sigmoid_bwd and the fused bilinear add.

Every reference is an fp64 restatement on the CPU; the RowMap formula of csrc/common.hpp is applied as an index tensor.  Outputs start from a
finite sentinel, and everything outside the image of the output map (the cls row of each frame, rows before `offset`, columns >= N of a wider
matrix) must come back bit-identical.  Every GEMM / LayerNorm case also carries "wrong" references -- the feature under test shifted or removed --
that must sit >= 1e-3 (scale-relative) away from the true one: the inputs can see the error the case exists for (SENSITIVITY, a CPU condition)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from endodav_amd import _lib

pytestmark = pytest.mark.gpu

ID = (0, 0, 0, 1)
SENT = -3.25          # finite sentinel of the outputs (exact in fp32)
GUARD_SENT = 12345.0  # guard bands round every device operand
GUARD = 64 * 1024     # floats on either side: more than 64 rows x ld of every case below
SENSITIVITY = 1e-3    # > 300 x the tolerances
COUNTER_FLOATS = 4096  # MAX_COUNTERS of gemm_dma.hip
FR = 3                # frames


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def close(a, b, rtol, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    assert err <= rtol, f"{what}: scale-relative error {err:.3e} > {rtol:.1e}"
    return err


def rows_of(m, n):
    """RowMap::operator() of csrc/common.hpp for logical rows 0..n-1."""
    period, stride, offset, inner = m
    idx = torch.arange(n)
    if period == 0:
        return idx
    return (idx // period) * stride + offset + inner * (idx % period)


def cmap(m):
    return (C.c_int32 * 4)(*m)


def sensitive(true, wrong, scale, what):
    d = (true - wrong).abs().max().item() / scale
    assert d >= SENSITIVITY, f"{what}: the shifted reference is only {d:.2e} away -- these inputs could not see that error"


def guarded(t, cuda, fill=float("nan")):
    """t on the device between two guard bands (inputs: NaN, so a read that strays poisons the output)."""
    big = torch.full((t.numel() + 2 * GUARD,), fill, device=cuda)
    big[GUARD:GUARD + t.numel()] = t.reshape(-1).to(cuda)
    return big, big[GUARD:GUARD + t.numel()].view(t.shape)


def guards_intact(big, n, fill):
    return bool((big[:GUARD] == fill).all()) and bool((big[GUARD + n:] == fill).all())


_WS = {}


def gemm_ws(lib, cuda):
    """Stream-K workspace as test_kernels_gpu.gemm_ws: arrival counters zero, piece slots NaN (a piece nobody wrote would show)."""
    if "ws" not in _WS:
        nbytes = lib.edv_gemm_workspace()
        assert nbytes > 0 and nbytes % 16 == 0
        w = torch.full((nbytes // 4,), float("nan"), device=cuda)
        w[:COUNTER_FLOATS] = 0
        _WS["ws"] = (w, nbytes)
    return _WS["ws"]


# ==============================================================================================================================
# GEMM descriptors
# ==============================================================================================================================
class GemmCase:
    """One descriptor, on the CPU.  A [a_rows, lda]; W = columns w_col0 .. w_col0 + K of Wfull [N, ldw]; C = columns col0 .. col0 + N of a
    [c_rows, ldc] buffer; R1 likewise (or C itself: inplace); R2 [c_rows, N]; P1 [p1_rows, N]."""

    def __init__(self, M, N, K, *, a_map=ID, a_rows=None, c_map=ID, c_rows=None, bias=True, act=0, gamma=False, r1_rows=0, r1_map=ID, inplace=False,
                 r2=False, p1_rows=0, p1_map=ID, lda=None, ldc=None, col0=0, w_halves=0, w_right=False):
        self.M, self.N, self.K, self.act, self.col0, self.inplace = M, N, K, act, col0, inplace
        self.a_map, self.c_map, self.r1_map, self.p1_map = a_map, c_map, r1_map, p1_map
        self.lda, self.ldc = lda or K, ldc or N
        self.A = rnd(a_rows or M, self.lda, seed=1)
        self.ldw = 2 * K if w_halves else K
        self.w_col0 = K if w_right else 0
        self.Wfull = rnd(N, self.ldw, seed=2, scale=1 / math.sqrt(K))
        self.bias = rnd(N, seed=3, scale=0.1) if bias else None
        self.gamma = rnd(N, seed=4) + 1.2 if gamma else None
        c_rows = c_rows or M
        self.Cinit = rnd(c_rows, self.ldc, seed=5) if inplace else torch.full((c_rows, self.ldc), SENT)
        self.R1 = rnd(r1_rows, self.ldc, seed=6) if r1_rows else None  # same leading dimension and column offset as C
        self.R2 = rnd(c_rows, N, seed=7) if r2 else None
        self.P1 = rnd(p1_rows, N, seed=8) if p1_rows else None

    def reference(self, **wrong):
        """The [c_rows, ldc] buffer after the call, in fp64, and the mask of the elements the call owns.  `wrong`: a map replaced
        (a_map= / c_map= / r1_map= / p1_map=), an operand dropped (drop="R2"), or a leading dimension ignored (dense="lda" / "ldc" / "ldr1": the
        operand addressed from the same pointer as if its rows were K / N floats long)."""
        g = lambda k: wrong.get(k, getattr(self, k))
        M, N, K, c0 = self.M, self.N, self.K, self.col0
        W = self.Wfull[:, self.w_col0:self.w_col0 + K].double()
        dense = wrong.get("dense")
        A = self.A.reshape(-1)[:self.A.shape[0] * K].view(-1, K) if dense == "lda" else self.A
        v = A[rows_of(g("a_map"), M)][:, :K].double() @ W.T
        if self.bias is not None:
            v = v + self.bias.double()
        if self.P1 is not None:
            v = v + self.P1[rows_of(g("p1_map"), M)].double()
        v = F.gelu(v) if self.act == 1 else F.relu(v) if self.act == 2 else v
        if self.gamma is not None:
            v = v * self.gamma.double()
        crow = rows_of(g("c_map"), M)
        r1 = self.Cinit if self.inplace else self.R1
        if r1 is not None and dense == "ldr1":
            v = v + r1.reshape(-1)[c0:c0 + r1.shape[0] * N].view(-1, N)[rows_of(g("r1_map"), M)].double()
        elif r1 is not None:
            v = v + r1[rows_of(g("r1_map"), M)][:, c0:c0 + N].double()
        if self.R2 is not None and wrong.get("drop") != "R2":
            v = v + self.R2[crow].double()
        out = self.Cinit.double().clone()
        if dense == "ldc":
            out.view(-1)[c0:c0 + out.shape[0] * N].view(-1, N)[crow] = v
        else:
            out[crow, c0:c0 + N] = v
        mask = torch.zeros_like(out, dtype=torch.bool)
        mask[crow, c0:c0 + N] = True
        return out, mask

    def check_sensitivity(self, wrongs, what):
        ref, mask = self.reference()
        scale = ref[mask].abs().max().item()
        for name, kw in wrongs.items():
            sensitive(ref, self.reference(**kw)[0], scale, f"{what}: {name}")

    def run(self, lib, cuda, split=False, planes=None):
        """edv_gemm_desc on the device; returns the whole C buffer."""
        keep = []

        def dev(t, fill=float("nan")):
            if t is None:
                return None
            big, view = guarded(t, cuda, fill)
            keep.append(big)
            return view

        A, W, bias, gamma, R2, P1 = dev(self.A), dev(self.Wfull), dev(self.bias), dev(self.gamma), dev(self.R2), dev(self.P1)
        bigC, Cd = guarded(self.Cinit, cuda, GUARD_SENT)
        R1 = Cd if self.inplace else dev(self.R1)
        d = _lib.GemmDescC()
        d.A, d.lda, d.a_map = A.data_ptr(), self.lda, cmap(self.a_map)
        d.W, d.ldw = W.data_ptr() + 4 * self.w_col0, self.ldw
        d.C, d.ldc, d.c_map = Cd.data_ptr() + 4 * self.col0, self.ldc, cmap(self.c_map)
        d.M, d.N, d.K = self.M, self.N, self.K
        d.bias, d.act, d.gamma = _lib.ptr(bias) or None, self.act, _lib.ptr(gamma) or None
        if R1 is not None:
            d.R1, d.ldr1, d.r1_map = R1.data_ptr() + 4 * self.col0, self.ldc, cmap(self.r1_map)
        if R2 is not None:
            d.R2, d.ldr2 = R2.data_ptr(), self.N
        if P1 is not None:
            d.P1, d.ldp1, d.p1_map = P1.data_ptr(), self.N, cmap(self.p1_map)
        ws = None
        if split:
            ws, nbytes = gemm_ws(lib, cuda)
            d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
        if planes is not None:
            d.x6_planes = planes.data_ptr()
        _lib.check(lib.edv_gemm_desc(C.byref(d), st()), "edv_gemm_desc")
        torch.cuda.synchronize()
        assert guards_intact(bigC, self.Cinit.numel(), GUARD_SENT), "a store escaped the C buffer"
        if split:
            assert int(ws[:COUNTER_FLOATS].view(torch.int32).abs().sum()) == 0, "arrival counters not left at zero"
        return Cd.cpu()

    def check(self, got, what):
        ref, mask = self.reference()
        assert torch.equal(got[~mask], self.Cinit[~mask]), f"{what}: an element outside the output map's image changed"
        err = close(got[mask], ref[mask], 3e-6, what)
        print(f"\n[{what}] scale-relative error {err:.2e} (tolerance 3e-6)")
        return err


def patch_embed_case(P0, N, K, gamma=False):
    """engine_forward.hip patch embed: rows of frame f go behind its cls row, the position table is a residual broadcast over frames
    (stride 0).  R1 holds FR * ntok rows so that the wrong stride of the sensitivity check stays inside it; the kernel reads ntok."""
    ntok = P0 + 1
    return GemmCase(FR * P0, N, K, c_map=(P0, ntok, 1, 1), c_rows=FR * ntok, r1_rows=FR * ntok, r1_map=(P0, 0, 1, 1), gamma=gamma)


PATCH_WRONG = lambda P0: {"c_map offset - 1": dict(c_map=(P0, P0 + 1, 0, 1)), "r1_map offset - 1": dict(r1_map=(P0, 0, 0, 1)),
                          "r1_map stride ntok": dict(r1_map=(P0, P0 + 1, 1, 1))}


# Instantiations (gemm.hip launch_rows has no EP 5: K % 32 != 0 or N <= 32 takes the general epilogue whatever epilogue_kind says):
#   K = 588          gemm_kernel<64, 64, 2, 2, LOAD_DENSE, STORE_ROWS, 0> (N > 32; K tail 588 = 18 * 32 + 12), <128, 32, 4, 1, ..., 0> (N = 32)
#   K = 64 / 608     N = 32: gemm_kernel<128, 32, 4, 1, LOAD_DENSE, STORE_ROWS, 0>;
#                    N > 32: gemm_dma_kernel<STORE_ROWS, 5, false, 2> (gemm_epilogue_mapped) for P0 >= 32, <STORE_ROWS, 0, false, 2> below
#   608 = PE_K, the padded im2col width the engine's patch embed runs with (19 k-tiles: an odd count through the two-stage loop)
# P0 = 32 is the boundary of epilogue_kind 5; with 33 and 37 a 64-row tile spans two periods (a 128-row one four), every 32-row block
# but the first crosses a period boundary, and the last block is partial (M = 99 / 111).
@pytest.mark.parametrize("N", [32, 48, 96])
@pytest.mark.parametrize("K", [588, 64, 608])
@pytest.mark.parametrize("P0", [12, 31, 32, 33, 37, 100])
def test_gemm_patch_embed_form(lib, cuda, P0, K, N):
    case, what = patch_embed_case(P0, N, K), f"gemm patch-embed P0={P0} K={K} N={N}"
    case.check_sensitivity(PATCH_WRONG(P0), what)
    case.check(case.run(lib, cuda), what)


@pytest.mark.parametrize("P0,K,N", [(37, 64, 96), (37, 588, 48), (12, 64, 96)])
def test_gemm_patch_embed_form_with_gamma(lib, cuda, P0, K, N):
    """gamma through gemm_epilogue_mapped (EP 5), the register-staged general epilogue and the DMA kernel's general epilogue."""
    case, what = patch_embed_case(P0, N, K, gamma=True), f"gemm patch-embed + gamma P0={P0} K={K} N={N}"
    case.check_sensitivity(PATCH_WRONG(P0), what)
    case.check(case.run(lib, cuda), what)


def tap_case(P0, N, K):
    """engine_forward.hip tap projection: A skips the cls row of every frame, C is dense."""
    return GemmCase(FR * P0, N, K, a_map=(P0, P0 + 1, 1, 1), a_rows=FR * (P0 + 1))


TAP_WRONG = lambda P0: {"a_map offset - 1": dict(a_map=(P0, P0 + 1, 0, 1)), "a_map dropped": dict(a_map=ID)}


# gemm_dma_kernel<STORE_ROWS, 1, false, 1> (BUF = 1: buffer descriptors with the row map's division compiled in; buffer epilogue)
@pytest.mark.parametrize("N", [48, 96])
@pytest.mark.parametrize("K", [64, 384])
def test_gemm_tap_projection_form(lib, cuda, K, N):
    case, what = tap_case(37, N, K), f"gemm tap-projection K={K} N={N}"
    case.check_sensitivity(TAP_WRONG(37), what)
    case.check(case.run(lib, cuda), what)


def test_gemm_tap_projection_form_streamk(lib, cuda):
    """gemm_dma_kernel<STORE_ROWS, 1, true, 1>.  M = 111, N = 640, K = 768: 2 x 10 = 20 tiles of 768 / 32 = 24 k-tiles.  launch_dma splits when
    tiles > 16 (20), tiles % slots != 0 and tiles < 8 * slots (slots = 3 workgroups x the CU count, hundreds), K / 32 >= 24 (24): all hold, so
    with a workspace the 480 k-tile units are cut into runs of chunk_min = 6 and every tile is merged from 4 pieces."""
    case, what = tap_case(37, 640, 768), "gemm tap-projection stream-K"
    case.check_sensitivity(TAP_WRONG(37), what)
    for _ in range(2):  # the second launch depends on the first leaving the counters at zero
        case.check(case.run(lib, cuda, split=True), what)


def readout_case(P0, N, K, right):
    """engine_forward.hip cls-token readout: W is one half of an [N, 2K] matrix, P1 one addend row per frame (inner 0), GELU."""
    return GemmCase(FR * P0, N, K, act=1, p1_rows=FR, p1_map=(P0, 1, 0, 0), w_halves=2, w_right=right, bias=False)


READOUT_WRONG = {"P1 of frame 0 for every frame": dict(p1_map=(37, 0, 0, 0))}


# gemm_dma_kernel<STORE_ROWS, 0, false, 2>: P1 forces the general epilogue (gemm_epilogue)
@pytest.mark.parametrize("right", [False, True], ids=["left-half", "right-half"])
@pytest.mark.parametrize("N,K", [(64, 64), (96, 384)])
def test_gemm_readout_form(lib, cuda, N, K, right):
    case, what = readout_case(37, N, K, right), f"gemm readout N={N} K={K} {'right' if right else 'left'} half"
    case.check_sensitivity(READOUT_WRONG, what)
    case.check(case.run(lib, cuda), what)


def test_gemm_readout_form_streamk(lib, cuda):
    """gemm_dma_kernel<STORE_ROWS, 0, true, 2>: 20 tiles of 24 k-tiles (see the tap-projection split case); the workgroup that merges a tile's
    pieces applies P1 + GELU in the general epilogue."""
    case, what = readout_case(37, 640, 768, True), "gemm readout stream-K"
    case.check_sensitivity(READOUT_WRONG, what)
    for _ in range(2):
        case.check(case.run(lib, cuda, split=True), what)


# engine_forward.hip motion-module out projection: R1 == C in place and R2.  gemm_dma_kernel<STORE_ROWS, 1 + act, false, 2>: the buffer epilogue
# (gemm_epilogue_buf) with both residual descriptors
@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("NK", [64, 256])
@pytest.mark.parametrize("M", [111, 300])
def test_gemm_two_residuals(lib, cuda, M, NK, act):
    case, what = GemmCase(M, NK, NK, act=act, inplace=True, r2=True), f"gemm R1 == C + R2 M={M} N=K={NK} act={act}"
    case.check_sensitivity({"R2 dropped": dict(drop="R2")}, what)
    case.check(case.run(lib, cuda), what)


def test_gemm_two_residuals_streamk(lib, cuda):
    """gemm_dma_kernel<STORE_ROWS, 1, true, 2>: M = 700, N = 128, K = 1024 is 11 x 2 = 22 tiles of 32 k-tiles (> 16 tiles, >= 24 k-tiles)."""
    case, what = GemmCase(700, 128, 1024, inplace=True, r2=True), "gemm R1 == C + R2 stream-K"
    case.check_sensitivity({"R2 dropped": dict(drop="R2")}, what)
    for _ in range(2):
        case.check(case.run(lib, cuda, split=True), what)


# Leading dimensions the engine does not use today.  "buffer": gemm_dma_kernel<STORE_ROWS, 1, false, 2> (gemm_epilogue_buf, EP 1..3);
# "general": the same kernel with EP 0 (an identity-mapped P1 forces gemm_epilogue); "fast": gemm_kernel<64, 64, ..., 1> (gemm_epilogue_fast, K = 588)
@pytest.mark.parametrize("path", ["buffer", "general", "fast"])
@pytest.mark.parametrize("which", ["lda", "ldc"])
def test_gemm_leading_dimensions(lib, cuda, path, which):
    M, N, K = 111, 96, 588 if path == "fast" else 64
    kw = dict(p1_rows=M) if path == "general" else {}
    if which == "lda":
        case = GemmCase(M, N, K, lda=K + 4, r1_rows=M, **kw)
    else:  # C and R1 are columns 4 .. N + 4 of [M, N + 8] matrices
        case = GemmCase(M, N, K, ldc=N + 8, col0=4, r1_rows=M, **kw)
    what = f"gemm {which} {path}"
    case.check_sensitivity({"lda ignored": dict(dense="lda")} if which == "lda" else {"ldc ignored": dict(dense="ldc"), "ldr1 ignored": dict(dense="ldr1")}, what)
    case.check(case.run(lib, cuda), what)


# bf16 planes supplied with descriptors the bf16x6 kernel does not implement (forms 1-3): gemm_x6_supported must say no and gemm() must run the
# fp32 kernel -- same tolerance, and the same bits as without planes.  NaN planes show which path ran: the supported descriptor of the control
# test turns them into NaN outputs, these must not.
X6_CASES = {"patch-embed": lambda: patch_embed_case(37, 96, 64), "tap-projection": lambda: tap_case(37, 96, 384),
            "readout": lambda: readout_case(37, 96, 384, False)}


def x6_planes(lib, cuda, case):
    W = case.Wfull[:, case.w_col0:case.w_col0 + case.K].contiguous().to(cuda)
    planes = torch.zeros(lib.edv_gemm_x6_planes_bytes(case.N, case.K) // 2, dtype=torch.bfloat16, device=cuda)
    _lib.check(lib.edv_gemm_x6_split(W.data_ptr(), planes.data_ptr(), case.N, case.K, st()), "edv_gemm_x6_split")
    torch.cuda.synchronize()
    return planes


@pytest.mark.parametrize("form", list(X6_CASES))
def test_gemm_x6_planes_fall_back_on_mapped_descriptors(lib, cuda, form):
    case, what = X6_CASES[form](), f"gemm bf16x6 fallback {form}"
    plain = case.run(lib, cuda)
    with_planes = case.run(lib, cuda, planes=x6_planes(lib, cuda, case))
    case.check(with_planes, what)
    assert torch.equal(with_planes, plain), f"{what}: planes changed the result of a descriptor the bf16x6 kernel does not support"
    poisoned = case.run(lib, cuda, planes=torch.full_like(x6_planes(lib, cuda, case), float("nan")))
    assert torch.equal(poisoned, plain), f"{what}: the planes were read"


def test_gemm_x6_planes_are_used_on_a_supported_descriptor(lib, cuda):
    """Control of the fallback test: identity maps, no P1, ldw = K -- gemm_x6_supported says yes, edv_gemm_desc passes the planes on."""
    case = GemmCase(515, 200, 48, gamma=True)  # a shape of test_gemm_x6: ragged rows and columns (no ReLU: it would turn the NaN into 0)
    case.check(case.run(lib, cuda, planes=x6_planes(lib, cuda, case)), "gemm bf16x6 on a supported descriptor")
    poisoned = case.run(lib, cuda, planes=torch.full_like(x6_planes(lib, cuda, case), float("nan")))
    assert torch.isnan(poisoned).all()


def test_gemm_desc_rejects_what_gemm_does_not_check(lib, cuda):
    z, out = torch.zeros(64 * 64, device=cuda), torch.zeros(64 * 64, device=cuda)

    def desc(**kw):
        d = _lib.GemmDescC()
        d.A = d.W = z.data_ptr()
        d.C = out.data_ptr()
        d.lda = d.ldw = d.ldc = d.N = d.K = 32
        d.M = 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad = [desc(ldc=31), desc(R1=z.data_ptr(), ldr1=31), desc(R2=z.data_ptr(), ldr2=0), desc(P1=z.data_ptr(), ldp1=31), desc(act=3), desc(act=-1),
           desc(c_map=cmap((4, 4, 0, 2))), desc(a_map=cmap((-1, 0, 0, 1))), desc(r1_map=cmap((4, 0, 0, -1)))]
    for d in bad:
        assert lib.edv_gemm_desc(C.byref(d), st()) != 0 and lib.edv_last_error()
    assert lib.edv_gemm_desc(None, st()) != 0
    _lib.check(lib.edv_gemm_desc(C.byref(desc()), st()), "edv_gemm_desc")
    torch.cuda.synchronize()


# ==============================================================================================================================
# LayerNorm with row maps, activation, accumulation
# ==============================================================================================================================
def ln_inputs(n_rows, dim):
    return rnd(n_rows, dim, seed=1, scale=3) + 0.5, rnd(dim, seed=2) + 1.0, rnd(dim, seed=3, scale=0.1)


def ln_reference(x, w, b, y0, rows, in_map, out_map, act, acc):
    dim = x.shape[1]
    v = F.layer_norm(x[rows_of(in_map, rows)].double(), (dim,), w.double(), b.double(), 1e-6)
    if act:
        v = F.gelu(v)
    out, orow = y0.double().clone(), rows_of(out_map, rows)
    out[orow] = v + (out[orow] if acc else 0)
    mask = torch.zeros(y0.shape[0], dtype=torch.bool)
    mask[orow] = True
    return out, mask


def ln_forms(P0):
    """name -> (rows, x rows, y rows, in_map, out_map, act, accumulate, {wrong name: overrides})"""
    ntok, MP = P0 + 1, FR * P0
    skip, cls = (P0, ntok, 1, 1), (1, ntok, 0, 1)
    return {
        "a": (MP, FR * ntok, MP + 2, skip, ID, 0, False, {"in_map offset - 1": dict(in_map=(P0, ntok, 0, 1))}),          # final-norm taps
        "b": (FR, FR * ntok, FR + 2, cls, ID, 0, False, {"in_map offset + 1": dict(in_map=(1, ntok, 1, 1))}),            # cls rows
        "c": (MP, MP, FR * ntok, ID, skip, 0, True, {"out_map offset - 1": dict(out_map=(P0, ntok, 0, 1)), "accumulate dropped": dict(acc=False)}),
        "d": (MP, MP, MP + 2, ID, ID, 1, False, {"GELU dropped": dict(act=0)}),                                          # res-bottleneck norm + GELU
        "e": (MP, MP, FR * ntok, ID, skip, 1, True, {"out_map offset - 1": dict(out_map=(P0, ntok, 0, 1)), "accumulate dropped": dict(acc=False),
                                                     "GELU dropped": dict(act=0)}),
    }


# layernorm_kernel<1, NV>, NV = 1 (dim 64), 2 (384), 4 (1024).  15 / 111 / 3 rows: the last workgroup of four waves is partial
@pytest.mark.parametrize("form", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("P0", [5, 37])
@pytest.mark.parametrize("dim", [64, 384, 1024])
def test_layernorm_mapped(lib, cuda, dim, P0, form):
    rows, xr, yr, in_map, out_map, act, acc, wrongs = ln_forms(P0)[form]
    x, w, b = ln_inputs(xr, dim)
    y0 = rnd(yr, dim, seed=4) if acc else torch.full((yr, dim), SENT)
    cfg = dict(in_map=in_map, out_map=out_map, act=act, acc=acc)
    ref, mask = ln_reference(x, w, b, y0, rows, **cfg)
    what = f"layernorm form {form} dim={dim} P0={P0}"
    for name, kw in wrongs.items():
        sensitive(ref, ln_reference(x, w, b, y0, rows, **{**cfg, **kw})[0], ref[mask].abs().max().item(), f"{what}: {name}")
    (bx, xd), (bw, wd), (bb, bd) = guarded(x, cuda), guarded(w, cuda), guarded(b, cuda)
    bigY, yd = guarded(y0, cuda, GUARD_SENT)
    _lib.check(lib.edv_layernorm_mapped(xd.data_ptr(), cmap(in_map), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(), cmap(out_map), rows, dim, 1e-6, None, 0, 0,
                                        act, int(acc), st()), "edv_layernorm_mapped")
    torch.cuda.synchronize()
    assert guards_intact(bigY, y0.numel(), GUARD_SENT), "a store escaped the y buffer"
    got = yd.cpu()
    assert torch.equal(got[~mask], y0[~mask]), f"{what}: a row outside the output map's image changed"
    err = close(got[mask], ref[mask], 2e-6, what)
    print(f"\n[{what}] scale-relative error {err:.2e} (tolerance 2e-6)")


def test_layernorm_mapped_rejects_bad_arguments(lib, cuda):
    z = torch.zeros(8, 64, device=cuda)
    args = lambda m, act: (z.data_ptr(), m, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 4, 64, 1e-6, None, 0, 0, act, 0, st())
    assert lib.edv_layernorm_mapped(*args(cmap((2, 2, 0, 3)), 0)) != 0
    assert lib.edv_layernorm_mapped(*args(None, 2)) != 0  # ReLU is not a LayerNorm activation


def ln_bwd_reference(x, w, g, dx0, rows, xmap, dxmap, acc):
    dim = x.shape[1]
    xs = x[rows_of(xmap, rows)].double().requires_grad_(True)
    (d,) = torch.autograd.grad(F.layer_norm(xs, (dim,), w.double(), None, 1e-6), [xs], g.double())
    out, orow = dx0.double().clone(), rows_of(dxmap, rows)
    out[orow] = d + (out[orow] if acc else 0)
    mask = torch.zeros(dx0.shape[0], dtype=torch.bool)
    mask[orow] = True
    return out, mask


# engine_backward.hip tap gradients: x and dx through the same map, dy dense, accumulate onto the running dx.  layernorm_bwd_kernel (one instantiation)
@pytest.mark.parametrize("form", ["patch-rows", "cls-rows"])
@pytest.mark.parametrize("P0", [5, 37])
@pytest.mark.parametrize("dim", [64, 384, 1024])
def test_layernorm_bwd_mapped(lib, cuda, dim, P0, form):
    ntok = P0 + 1
    rows, m, shifted = (FR * P0, (P0, ntok, 1, 1), (P0, ntok, 0, 1)) if form == "patch-rows" else (FR, (1, ntok, 0, 1), (1, ntok, 1, 1))
    x, w, _ = ln_inputs(FR * ntok, dim)
    g, dx0 = rnd(rows, dim, seed=5), rnd(FR * ntok, dim, seed=6)
    ref, mask = ln_bwd_reference(x, w, g, dx0, rows, m, m, True)
    what, scale = f"layernorm_bwd {form} dim={dim} P0={P0}", ref[mask].abs().max().item()
    sensitive(ref, ln_bwd_reference(x, w, g, dx0, rows, shifted, m, True)[0], scale, f"{what}: x map shifted")
    sensitive(ref, ln_bwd_reference(x, w, g, dx0, rows, m, shifted, True)[0], scale, f"{what}: dx map shifted")
    sensitive(ref, ln_bwd_reference(x, w, g, dx0, rows, m, m, False)[0], scale, f"{what}: accumulate dropped")
    (bx, xd), (bw, wd), (bg, gd) = guarded(x, cuda), guarded(w, cuda), guarded(g, cuda)
    bigD, dxd = guarded(dx0, cuda, GUARD_SENT)
    _lib.check(lib.edv_layernorm_bwd_mapped(xd.data_ptr(), cmap(m), wd.data_ptr(), gd.data_ptr(), None, dxd.data_ptr(), cmap(m), rows, dim, 1e-6, 1, st()),
               "edv_layernorm_bwd_mapped")
    torch.cuda.synchronize()
    assert guards_intact(bigD, dx0.numel(), GUARD_SENT), "a store escaped the dx buffer"
    got = dxd.cpu()
    assert torch.equal(got[~mask], dx0[~mask]), f"{what}: a row outside the dx map's image changed"
    err = close(got[mask], ref[mask], 3e-6, what)  # the tolerance of test_layernorm_bwd
    print(f"\n[{what}] scale-relative error {err:.2e} (tolerance 3e-6)")


# ==============================================================================================================================
# folds and reductions
# ==============================================================================================================================
def out_buf(n, cuda, extra=5):
    """n outputs + `extra` sentinel elements behind them that must stay."""
    return torch.full((n + extra,), SENT, device=cuda)


def tail_intact(buf, n):
    return bool((buf[n:] == SENT).all())


def report(what, err, tol=2e-6):
    print(f"\n[{what}] scale-relative error {err:.2e} (tolerance {tol:.0e})")


def test_fold_ssb(lib, cuda):
    nout, nin = 77, 52
    W, a, b = rnd(nout, nin, seed=1, scale=0.05), rnd(nin, seed=2) + 1.5, rnd(nout, seed=3) + 1.5
    ref = a.double()[None, :] * W.double() * b.double()[:, None]
    Wd, ad, bd, out = W.to(cuda), a.to(cuda), b.to(cuda), out_buf(nout * nin, cuda)
    _lib.check(lib.edv_fold_ssb(Wd.data_ptr(), ad.data_ptr(), bd.data_ptr(), out.data_ptr(), nout, nin, st()), "edv_fold_ssb")
    assert tail_intact(out, nout * nin)
    report("fold_ssb", close(out[:nout * nin].view(nout, nin), ref, 2e-6, "fold_ssb"))


def test_fold_bn(lib, cuda):
    """Eval-mode BatchNorm after a convolution in fp64: w' = s * w, b' = (b - mean) * s + beta, s = gamma / sqrt(var + eps); var = 0, eps / 100 and
    eps in three channels (s up to gamma / sqrt(eps) = 316 gamma).  The weight is compared row by row at the row's own scale (the large-s channels
    would otherwise hide the others), the bias at |b - mean| s + |beta| (its terms may cancel)."""
    nout, K = 70, 9 * 12
    eps = float(torch.tensor(1e-5, dtype=torch.float32))  # the value the kernel receives
    w, b = rnd(nout, K, seed=1, scale=0.1), rnd(nout, seed=2, scale=0.1)
    gamma, beta, mean, var = rnd(nout, seed=3) + 1.5, rnd(nout, seed=4, scale=0.2), rnd(nout, seed=5, scale=0.3), rnd(nout, seed=6, scale=0.4) + 0.5
    var[0], var[1], var[2] = 0.0, eps / 100, eps
    s = gamma.double() / torch.sqrt(var.double() + eps)
    ref_w, ref_b = w.double() * s[:, None], (b.double() - mean.double()) * s + beta.double()
    wd, bout = out_buf(nout * K, cuda), out_buf(nout, cuda)
    wd[:nout * K] = w.reshape(-1).to(cuda)
    dv = [t.to(cuda) for t in (b, gamma, beta, mean, var)]
    _lib.check(lib.edv_fold_bn(wd.data_ptr(), *(t.data_ptr() for t in dv), eps, bout.data_ptr(), nout, K, st()), "edv_fold_bn")
    assert tail_intact(wd, nout * K) and tail_intact(bout, nout)
    got_w, got_b = wd[:nout * K].view(nout, K).double().cpu(), bout[:nout].double().cpu()
    err_w = ((got_w - ref_w).abs().amax(1) / ref_w.abs().amax(1)).max().item()
    err_b = ((got_b - ref_b).abs() / ((b.double() - mean.double()).abs() * s + beta.double().abs())).max().item()
    report("fold_bn weight (per row)", err_w)
    report("fold_bn bias", err_b)
    assert err_w <= 2e-6 and err_b <= 2e-6


@pytest.mark.parametrize("r", [1, 4, 8])
def test_fold_dash(lib, cuda, r):
    nout, nin = 70, 52
    W, U, idx, V = rnd(nout, nin, seed=1, scale=0.05), rnd(nout, r, seed=2), rnd(r, seed=3) + 1.2, rnd(r, nin, seed=4, scale=0.1)
    ref = W.double() + (U.double() * idx.double()) @ V.double()
    io = out_buf(nout * nin, cuda)
    io[:nout * nin] = W.reshape(-1).to(cuda)
    Ud, id_, Vd = U.to(cuda), idx.to(cuda), V.to(cuda)
    _lib.check(lib.edv_fold_dash(Ud.data_ptr(), id_.data_ptr(), Vd.data_ptr(), io.data_ptr(), nout, nin, r, st()), "edv_fold_dash")
    assert tail_intact(io, nout * nin)
    report(f"fold_dash r={r}", close(io[:nout * nin].view(nout, nin), ref, 2e-6, "fold_dash"))


@pytest.mark.parametrize("use_gamma", [False, True])
def test_ssb_prep(lib, cuda, use_gamma):
    nout, nin = 77, 52  # nout > nin and nout * nin no multiple of 256
    W, a, b = rnd(nout, nin, seed=1, scale=0.05), rnd(nin, seed=2) + 1.5, rnd(nout, seed=3) + 1.5
    gamma = rnd(nout, seed=4) + 1.2 if use_gamma else None
    ref_wa, ref_gb = W.double() * a.double()[None, :], b.double() * (gamma.double() if use_gamma else 1.0)
    Wd, ad, bd, gd = W.to(cuda), a.to(cuda), b.to(cuda), (gamma.to(cuda) if use_gamma else None)
    Wa, gb = out_buf(nout * nin, cuda), out_buf(nout, cuda)
    _lib.check(lib.edv_ssb_prep(Wd.data_ptr(), ad.data_ptr(), bd.data_ptr(), _lib.ptr(gd) or None, Wa.data_ptr(), gb.data_ptr(), nout, nin, st()), "edv_ssb_prep")
    assert tail_intact(Wa, nout * nin) and tail_intact(gb, nout)
    report("ssb_prep Wa", close(Wa[:nout * nin].view(nout, nin), ref_wa, 2e-6, "ssb_prep Wa"))
    report("ssb_prep gb", close(gb[:nout], ref_gb, 2e-6, "ssb_prep gb"))


TALL_SPLITS = 64  # ops.hpp


# col_dot_partial_kernel + tall_tn_reduce_kernel.  M below / at / above TALL_SPLITS: 1, 3, 63, 64 rows -> one row per split; 65 -> 33 splits of two
# rows, the last short; 1000 -> 63 splits of 16 rows, the last of 8.  N around the 64-column block of stage 1 and the 32-column block of stage 2.
@pytest.mark.parametrize("N", [1, 8, 63, 64, 65, 384])
@pytest.mark.parametrize("M", [1, 3, 63, 64, 65, 1000])
def test_col_dot(lib, cuda, M, N):
    """Tolerance from the summation order, relative to scale[n] * sum_m |P Q| (what a rounding error of this sum is proportional to): a wave adds
    ceil(rows_per_split / 4) terms in sequence, 2 more additions join the four waves, stage 2 adds ceil(splits / 8) partials in sequence and 7 more
    join its slices; one rounding for the product, one for the scale: depth * 2^-24."""
    P, Q, scale = rnd(M, N, seed=1), rnd(M, N, seed=2), rnd(N, seed=3) + 1.5
    rps = -(-M // TALL_SPLITS)
    splits = -(-M // rps)
    tol = (-(-rps // 4) + 2 + -(-splits // 8) + 7 + 2) * 2.0 ** -24
    Pd, Qd, sd = P.to(cuda), Q.to(cuda), scale.to(cuda)
    worst = 0.0
    for use_q in (False, True):
        for use_s in (False, True):
            terms = P.double() * (Q.double() if use_q else 1.0)
            sc = scale.double() if use_s else torch.ones(N, dtype=torch.float64)
            ref, mag = terms.sum(0) * sc, terms.abs().sum(0) * sc.abs()
            outs = []
            for _ in range(2):
                part, out = torch.full((TALL_SPLITS * N,), float("nan"), device=cuda), out_buf(N, cuda)
                _lib.check(lib.edv_col_dot(Pd.data_ptr(), Qd.data_ptr() if use_q else None, M, N, sd.data_ptr() if use_s else None, part.data_ptr(),
                                           out.data_ptr(), st()), "edv_col_dot")
                assert tail_intact(out, N)
                outs.append(out[:N].cpu())
            assert torch.equal(outs[0], outs[1]), "col_dot is not bit-reproducible"
            err = ((outs[0].double() - ref).abs() / mag).max().item()
            worst = max(worst, err)
            assert err <= tol, f"col_dot M={M} N={N} Q={use_q} scale={use_s}: {err:.3e} of sum |P Q| > {tol:.2e}"
    print(f"\n[col_dot M={M} N={N}] error {worst:.2e} of scale * sum |P Q| (tolerance {tol:.2e})")


@pytest.mark.parametrize("n", [1003, 70001])  # no multiple of 4 or of the 256-thread block
def test_sigmoid_bwd(lib, cuda, n):
    g, s = rnd(n, seed=1), torch.sigmoid(rnd(n, seed=2, scale=6))
    ref = g.double() * s.double() * (1 - s.double())
    gd, sd, out = g.to(cuda), s.to(cuda), out_buf(n, cuda)
    _lib.check(lib.edv_sigmoid_bwd(gd.data_ptr(), sd.data_ptr(), out.data_ptr(), n, st()), "edv_sigmoid_bwd")
    assert tail_intact(out, n)
    report(f"sigmoid_bwd n={n}", close(out[:n], ref, 2e-6, "sigmoid_bwd"))


# bilinear_c4_kernel with its addend (the fused skip add of the fusion blocks)
@pytest.mark.parametrize("Fr,H,W,Cc,OH,OW", [(2, 1, 2, 32, 3, 4), (2, 19, 19, 64, 37, 37)])
def test_bilinear_add(lib, cuda, Fr, H, W, Cc, OH, OW):
    x, add = rnd(Fr, Cc, H, W, seed=1), rnd(Fr, OH, OW, Cc, seed=2)
    up = F.interpolate(x.double(), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    ref = up + add.double()
    sensitive(ref, up, ref.abs().max().item(), "bilinear_add: addend dropped")
    xd, ad = x.permute(0, 2, 3, 1).contiguous().to(cuda), add.to(cuda)
    n = Fr * OH * OW * Cc
    y = out_buf(n, cuda)
    _lib.check(lib.edv_bilinear_add(xd.data_ptr(), ad.data_ptr(), y.data_ptr(), Fr, H, W, Cc, OH, OW, st()), "edv_bilinear_add")
    assert tail_intact(y, n)
    report("bilinear_add", close(y[:n].view(Fr, OH, OW, Cc), ref, 2e-6, "bilinear_add"))
    assert lib.edv_bilinear_add(xd.data_ptr(), None, y.data_ptr(), Fr, H, W, Cc, OH, OW, st()) != 0
