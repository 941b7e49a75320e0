"""edv_ingest_u8 on MI355X through ctypes: uint8 HWC frames -> [0, 1] fp32 planar CHW, resized in the same kernel.  The expectation is the
two-step path it replaces -- torch's conversion on the device, then edv_resize_bicubic -- and the comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from endodav_amd import _lib

pytestmark = pytest.mark.gpu


def st():
    return C.c_void_p(_lib.stream_ptr())


def two_step(lib, frames: torch.Tensor, OH: int, OW: int) -> torch.Tensor:
    """frames uint8 [n, H, W, 3] on the device -> [n, 3, OH, OW]"""
    n, H, W, _ = frames.shape
    cur = frames.permute(0, 3, 1, 2).to(torch.float32).div_(255.0)
    if (OH, OW) == (H, W):
        return cur
    cur = cur.contiguous()  # .to() keeps the permuted strides (memory still HWC); edv_resize_bicubic takes planes, so make them: a pure copy
    out = torch.empty((n, 3, OH, OW), device=frames.device, dtype=torch.float32)
    _lib.check(lib.edv_resize_bicubic(cur.data_ptr(), out.data_ptr(), n * 3, H, W, OH, OW, st()), "edv_resize_bicubic")
    return out


def ingest(lib, src: torch.Tensor, slots, n: int, OH: int, OW: int, out=None) -> torch.Tensor:
    frames, H, W, _ = src.shape
    if out is None:
        out = torch.empty((n, 3, OH, OW), device=src.device, dtype=torch.float32)
    arr = None if slots is None else (C.c_int32 * len(slots))(*slots)
    _lib.check(lib.edv_ingest_u8(src.data_ptr(), frames, arr, n, out.data_ptr(), H, W, OH, OW, st()), "edv_ingest_u8")
    return out


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def random_frames(cuda, n, H, W, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)).to(cuda)


def test_all_256_byte_values_convert_as_torch_does(lib, cuda):
    t = torch.arange(768, dtype=torch.int32).remainder(256).to(torch.uint8).reshape(1, 16, 16, 3).to(cuda)
    want = t.permute(0, 3, 1, 2).to(torch.float32).div_(255.0)
    got = ingest(lib, t, None, 1, 16, 16)
    assert sorted(set(t.cpu().numpy().ravel().tolist())) == list(range(256))
    assert same(got, want)


@pytest.mark.parametrize("H,W,OH,OW", [(60, 80, 42, 56), (30, 40, 42, 56), (45, 57, 42, 56), (5, 7, 14, 14), (42, 56, 42, 56)],
                         ids=["down", "up", "row_stride_171", "border_clamped", "same_size"])
def test_resize_equals_the_two_step_path(lib, cuda, H, W, OH, OW):
    src = random_frames(cuda, 3, H, W, seed=H * W)
    want = two_step(lib, src, OH, OW)
    got = ingest(lib, src, None, 3, OH, OW)
    assert got.shape == (3, 3, OH, OW)
    assert same(got, want)


def test_slots_gather_repeat_and_default_to_the_identity(lib, cuda):
    src = random_frames(cuda, 5, 30, 40, seed=5)
    slots = [4, 0, 4, 2]
    want = two_step(lib, src[slots], 42, 56)
    assert same(ingest(lib, src, slots, 4, 42, 56), want)
    assert same(ingest(lib, src, None, 5, 42, 56), two_step(lib, src, 42, 56))
    assert same(ingest(lib, src, None, 3, 42, 56), two_step(lib, src[:3], 42, 56))  # NULL with n < src_frames: the first n


def test_64_slots(lib, cuda):
    src = random_frames(cuda, 7, 14, 14, seed=64)
    slots = [(5 * i + 3) % 7 for i in range(64)]
    assert same(ingest(lib, src, slots, 64, 14, 14), two_step(lib, src[slots], 14, 14))
    assert same(ingest(lib, src, slots, 64, 28, 21), two_step(lib, src[slots], 28, 21))


@pytest.mark.parametrize("H,W,OH,OW", [(45, 57, 42, 56), (42, 56, 42, 56)], ids=["resized", "same_size"])
def test_guard_bands_around_source_and_output(lib, cuda, H, W, OH, OW):
    """The output is carved out of a larger buffer holding a bit pattern; the source is the middle of a larger uint8 buffer whose neighbours hold
    255: a read outside the source would move the border pixels, a write outside the output would change the guards."""
    n, guard = 2, 4096
    frames = random_frames(cuda, n, H, W, seed=9)
    frames[:, 0, :, :] = 0      # dark borders: a neighbouring 255 read by mistake shows
    frames[:, -1, :, :] = 0
    nbytes = n * H * W * 3
    big_src = torch.full((guard + 1 + nbytes + guard,), 255, dtype=torch.uint8, device=cuda)  # + 1: the source starts at an odd address
    src = big_src[guard + 1:guard + 1 + nbytes].view(n, H, W, 3)
    src.copy_(frames)
    count = n * 3 * OH * OW
    pattern = np.uint32(0x7FC0BEEF).view(np.float32)  # a NaN with a payload
    big_out = torch.from_numpy(np.full(guard + count + guard, pattern, dtype=np.float32)).to(cuda)
    out = big_out[guard:guard + count].view(n, 3, OH, OW)
    ingest(lib, src, [1, 0], n, OH, OW, out=out)
    assert same(out, two_step(lib, frames[[1, 0]], OH, OW))
    host = big_out.cpu().numpy().view(np.uint32)
    assert (host[:guard] == 0x7FC0BEEF).all() and (host[guard + count:] == 0x7FC0BEEF).all()
    assert (big_src[:guard + 1] == 255).all() and (big_src[guard + 1 + nbytes:] == 255).all()


def test_bad_arguments_launch_nothing(lib, cuda):
    H, W, OH, OW = 12, 10, 14, 14
    src = random_frames(cuda, 3, H, W, seed=1)
    pattern = np.uint32(0x7FC0BEEF).view(np.float32)
    out = torch.from_numpy(np.full(64 * 3 * OH * OW, pattern, dtype=np.float32)).to(cuda)
    ok = (C.c_int32 * 3)(0, 1, 2)

    def call(src_p=src.data_ptr(), frames=3, slots=ok, n=3, out_p=out.data_ptr(), h=H, w=W, oh=OH, ow=OW):
        return lib.edv_ingest_u8(src_p, frames, slots, n, out_p, h, w, oh, ow, st())

    big = 1 << 15  # 2 * OH * H beyond 2^31: the bound edv_resize_bicubic checks
    bad = {
        "null source": dict(src_p=None),
        "null output": dict(out_p=None),
        "n = 0": dict(n=0),
        "n = 65": dict(n=65, slots=None, frames=65),
        "negative slot": dict(slots=(C.c_int32 * 3)(0, -1, 2)),
        "slot = src_frames": dict(slots=(C.c_int32 * 3)(0, 3, 2)),
        "identity beyond src_frames": dict(slots=None, n=4),
        "height overflow": dict(h=big, oh=big),
        "width overflow": dict(w=big, ow=big),
        "empty frame": dict(h=0),
    }
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        assert lib.edv_last_error(), what
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == 0x7FC0BEEF).all()
    assert call() == 0  # and the good call next to them goes through
    torch.cuda.synchronize()
    assert same(out[:3 * 3 * OH * OW].view(3, 3, OH, OW), two_step(lib, src, OH, OW))
