"""infer_video_depth end to end: a synthetic uint8 video on the host -> depth maps on the host; frames/s in both
products modes, host and device stitch alternating in one run.

    python scratch/video_rate.py [n_frames] [--size HxW] [--stitch host|device|both] [--modes f32,bf16x6] [--reps N]
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import endodav_amd
from endodav_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=232)
ap.add_argument("--size", default="256x320", help="frame size HxW (the network runs at 224x280)")
ap.add_argument("--stitch", default="both", choices=["host", "device", "both"])
ap.add_argument("--modes", default="f32,bf16x6")
ap.add_argument("--reps", type=int, default=2, help="host/device alternations per products mode")
args = ap.parse_args()
fh, fw = (int(v) for v in args.size.split("x"))
n = args.n

dev = torch.device("cuda:0")
model = endodav_amd.endodav(encoder="vits", features=64, out_channels=[48, 96, 192, 384], image_shape=(224, 280), lora_type="dvlora", disable_conv_head=True).eval()
synth.fill_module_(model)
model = model.to(dev)
rng = np.random.default_rng(0)
frames = rng.integers(0, 256, size=(n, fh, fw, 3), dtype=np.uint8)
paths = ["host", "device"] if args.stitch == "both" else [args.stitch]
for mode in args.modes.split(","):
    model.products = mode
    for path in paths:  # warm (contexts, planes, workspaces, pinned memory)
        out = model.infer_video_depth(frames, device="cuda", stitch=path)
        del out
    torch.cuda.synchronize()
    for rep in range(args.reps):
        for path in paths:
            t0 = time.perf_counter()
            out = model.infer_video_depth(frames, device="cuda", stitch=path)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"{mode:7s} stitch={path:6s} {n} frames {fh}x{fw} -> 224x280 windows of 32: {dt * 1e3:8.1f} ms  {n / dt:8.1f} frames/s  out {out.shape} mean {float(out.mean()):.6f}", flush=True)
            del out
