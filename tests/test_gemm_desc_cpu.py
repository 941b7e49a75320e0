"""CPU: the descriptor of the test entry point edv_gemm_desc -- layout of the ctypes mirror and the argument checks that run before any launch."""
import ctypes as C

from endodav_amd import _lib


def test_gemm_desc_layout():
    D = _lib.GemmDescC  # edv_gemm_desc_t of include/endodav_hip.h on LP64: pointers and int64 8-byte aligned, four int32[4] maps
    assert C.sizeof(D) == 224
    assert (D.A.offset, D.a_map.offset, D.W.offset, D.C.offset, D.c_map.offset, D.M.offset, D.N.offset, D.K.offset) == (0, 12, 32, 48, 60, 80, 88, 92)
    assert (D.bias.offset, D.act.offset, D.gamma.offset, D.R1.offset, D.r1_map.offset, D.R2.offset, D.P1.offset, D.p1_map.offset) == (96, 104, 112, 120, 132, 152,
                                                                                                                                     168, 180)
    assert (D.workspace.offset, D.workspace_bytes.offset, D.x6_planes.offset) == (200, 208, 216)


def test_gemm_desc_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 1024)()  # never dereferenced: every descriptor below is refused by the entry point's own checks
    p = C.addressof(buf)

    def desc(**kw):
        d = _lib.GemmDescC()
        d.A = d.W = d.C = p
        d.lda = d.ldw = d.ldc = d.N = d.K = 32
        d.M = 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    m = lambda *v: (C.c_int32 * 4)(*v)
    for d, word in [(desc(ldc=31), b"ldc"), (desc(R1=p, ldr1=31), b"ldr1"), (desc(R2=p, ldr2=8), b"ldr2"), (desc(P1=p, ldp1=0), b"ldp1"),
                    (desc(act=3), b"act"), (desc(act=-1), b"act"), (desc(c_map=m(4, 4, 0, 2)), b"row map"), (desc(a_map=m(-1, 0, 0, 1)), b"row map"),
                    (desc(r1_map=m(4, -4, 0, 1)), b"row map"), (desc(p1_map=m(4, 1, -1, 0)), b"row map")]:
        assert lib.edv_gemm_desc(C.byref(d), None) != 0
        assert word in lib.edv_last_error(), lib.edv_last_error()
    assert lib.edv_gemm_desc(None, None) != 0 and b"null" in lib.edv_last_error()
    one = (C.c_int32 * 4)(2, 2, 0, 3)
    assert lib.edv_layernorm_mapped(p, one, p, p, p, None, 4, 64, 1e-6, None, 0, 0, 0, 0, None) != 0 and b"row map" in lib.edv_last_error()
    assert lib.edv_layernorm_bwd_mapped(p, None, p, p, None, p, one, 4, 64, 1e-6, 0, None) != 0 and b"row map" in lib.edv_last_error()
