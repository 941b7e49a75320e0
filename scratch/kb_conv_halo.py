"""Per-shape A/B of the head's Cout <= 32 convolutions at the headline shapes (ViT-S, 518x518, T = 8): conv3_dma_kernel (mode 1) against
conv3_halo_kernel (mode 2), and the output tail conv + dot_channels against the fused launches.  HIP events around REPS back-to-back launches,
ROUNDS alternations per variant.  `vitb` as the only argument: the ViT-B T = 16 output convolution instead.  Run it under
rocprofv3 --kernel-trace --stats, or --pmc in a pass of its own, for the per-kernel figures of profiles/conv_halo_notes.txt."""
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from endodav_amd import _lib  # noqa: E402

lib = _lib.load()
cuda = torch.device("cuda:0")
REPS, ROUNDS = 30, 4


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(cuda)


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3  # us


def run(name, Fr, H, W, Cin, Cout, post, tail):
    x = rnd(Fr, H, W, Cin, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=1 / math.sqrt(9 * Cin))
    b = rnd(Cout, seed=3, scale=0.1)
    w2, b2 = rnd(Cout, seed=6), rnd(1, seed=7)
    wp = torch.empty(Cout * 9 * Cin, device=cuda)
    _lib.check(lib.edv_pack_conv3x3(w.data_ptr(), wp.data_ptr(), Cout, Cin, st()))
    y = torch.empty((Fr, H, W, Cout), device=cuda)
    d = torch.empty((Fr, H, W), device=cuda)

    def conv():
        _lib.check(lib.edv_conv3x3(x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), Fr, H, W, Cin, Cout, 1, 0, post, None, None, st()))

    def conv_then_dot():
        conv()
        _lib.check(lib.edv_dot_channels(y.data_ptr(), w2.data_ptr(), b2.data_ptr(), d.data_ptr(), Fr * H * W, Cout, 2, st()))

    def fused():
        _lib.check(lib.edv_conv3x3_dot(x.data_ptr(), wp.data_ptr(), b.data_ptr(), d.data_ptr(), Fr, H, W, Cin, Cout, 1, 0, post, w2.data_ptr(), b2.data_ptr(), 2, st()))

    variants = [("dma", 1, "1", conv), ("halo", 2, "1", conv)]
    if tail:
        variants += [("dma+dot_channels", 1, "1", conv_then_dot), ("dma_fused", 2, "0", fused), ("halo_fused", 2, "1", fused)]
    res = {v[0]: [] for v in variants}
    for _ in range(ROUNDS):
        for vname, mode, halo, fn in variants:
            os.environ["EDV_CONV_HALO"] = halo
            _lib.check(lib.edv_set_conv_impl(mode))
            res[vname].append(round(timed(fn), 1))
    _lib.check(lib.edv_set_conv_impl(0))
    os.environ.pop("EDV_CONV_HALO", None)
    for vname, ts in res.items():
        print(f"{name:28s} {vname:18s} mean {sum(ts) / len(ts):7.1f} us  min {min(ts):7.1f} max {max(ts):7.1f}  {ts}", flush=True)
    return res


out = {}
if len(sys.argv) > 1 and sys.argv[1] == "vitb":
    out["vitb16 conv2.0 64->32 518^2"] = run("vitb16 conv2.0 64->32 518^2", 16, 518, 518, 64, 32, 1, True)
    sys.exit(0)
out["output_conv2.0 32->32 518^2"] = run("output_conv2.0 32->32 518^2", 8, 518, 518, 32, 32, 1, True)
out["output_conv1 64->32 296^2"] = run("output_conv1 64->32 296^2", 8, 296, 296, 64, 32, 0, False)
