"""Colour-mapped depth on the GPU (opt-in): what the reference does in numpy on one core wherever a depth map becomes a picture.

``Render`` says how a depth map [h, w] becomes indices 0..255 and which table colours them; ``colorize`` applies it to a clip.  The four
``norm`` values and the reference code each mirrors:

  norm        range (lo, hi)                              eps            clip  mirrors
  "video"     min and max of the whole clip               float32(1e-6)  no    utils/eval_utils.py:284-295 ``save_video``, bit for bit
  "frame"     min and max of each frame                   0              no    evaluate_depth_video.py:32-36 ``render_depth``
  "fixed"     the caller's ``lo`` and ``hi``              0              yes   a clip to a given range
  "quantile"  per frame the order statistics of rank      0              yes   test_simple.py:156-167 (vmin = min, vmax = 95th percentile:
              floor(q * (h*w - 1)) for q_lo and q_hi                           the default q = (0.0, 0.95))

  den = (hi - lo) + eps;  t = (x - lo) / den;  clip: t = min(max(t, 0), 1);  idx = 0 if den == 0 else uint8(trunc(t * 255));  out = table[idx]

all in float32 (``edv_render_range`` / ``edv_render_colorize``, include/endodav_hip.h).  Two departures from the reference, both on purpose:
a constant frame gives index 0 under "frame", where ``render_depth`` divides 0 by 0; and "quantile" takes exact lower order statistics
(``np.percentile(..., method="lower")``) where test_simple interpolates linearly between two neighbouring order statistics, so the two
differ by less than the gap between those neighbours (and the interpolated value depends on the numpy version's arithmetic).

The tables are matplotlib's (``colormaps``), red-green-blue; ``order="bgr"`` reverses the columns, which is what a cv2 consumer expects.
Parity with ``cv2.applyColorMap`` (``render_depth``'s table) is unpinned: cv2 is absent where this project is built and tested.
Inputs are finite; NaN is unsupported."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, colormaps

NORMS = ("video", "frame", "fixed", "quantile")
CHUNK = 32  # frames coloured per call of the kernels


@dataclass(frozen=True, eq=False)
class Render:
    norm: str = "video"
    cmap: object = "inferno"                 # a name of colormaps.TABLES or a uint8 array [256, 3]
    lo: Optional[float] = None               # "fixed" only
    hi: Optional[float] = None
    q: Tuple[float, float] = (0.0, 0.95)     # "quantile" only
    order: str = "rgb"

    def __post_init__(self):
        if self.norm not in NORMS:
            raise ValueError(f"norm must be one of {NORMS}, got {self.norm!r}")
        if self.order not in ("rgb", "bgr"):
            raise ValueError(f"order must be 'rgb' or 'bgr', got {self.order!r}")
        if isinstance(self.cmap, str):
            if self.cmap not in colormaps.TABLES:
                raise ValueError(f"cmap must be one of {colormaps.NAMES} or a uint8 array [256, 3], got {self.cmap!r}")
        else:
            table = self.cmap
            if not isinstance(table, np.ndarray) or table.dtype != np.uint8 or table.shape != (256, 3):
                raise ValueError("a colour table must be a numpy uint8 array [256, 3]")
        if self.norm == "fixed":
            if self.lo is None or self.hi is None or not (math.isfinite(self.lo) and math.isfinite(self.hi)) or not float(np.float32(self.lo)) < float(np.float32(self.hi)):
                raise ValueError(f"norm='fixed' needs finite lo < hi (as float32), got lo={self.lo!r}, hi={self.hi!r}")
        try:
            q_lo, q_hi = (float(v) for v in self.q)
        except (TypeError, ValueError):
            raise ValueError(f"q must be a pair (q_lo, q_hi), got {self.q!r}") from None
        if not 0.0 <= q_lo <= q_hi <= 1.0:
            raise ValueError(f"q must satisfy 0 <= q_lo <= q_hi <= 1, got {self.q!r}")

    def table(self) -> np.ndarray:
        """The uint8 table [256, 3] in the output's channel order, contiguous."""
        t = colormaps.TABLES[self.cmap] if isinstance(self.cmap, str) else self.cmap
        return np.ascontiguousarray(t[:, ::-1] if self.order == "bgr" else t)

    def ranks(self, h: int, w: int) -> Tuple[int, int]:
        """The ranks of "quantile" on a frame of h * w pixels: floor(q * (h*w - 1)) in Python floats."""
        m = h * w
        return int(math.floor(float(self.q[0]) * (m - 1))), int(math.floor(float(self.q[1]) * (m - 1)))

    @property
    def eps(self) -> np.float32:
        return np.float32(1e-6) if self.norm == "video" else np.float32(0.0)

    @property
    def clip(self) -> int:
        return int(self.norm in ("fixed", "quantile"))


_tables: dict = {}  # (device index, the table's bytes) -> the table on that device


def _device_table(table: np.ndarray, dev: torch.device) -> torch.Tensor:
    """Uploaded once per (device, table) and complete when returned, so any stream may read it."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), table.tobytes())
    t = _tables.get(key)
    if t is None:
        with torch.cuda.device(dev):
            t = torch.from_numpy(table.copy()).to(dev)
            torch.cuda.current_stream(dev).synchronize()
        _tables[key] = t
    return t


class DeviceRenderer:
    """One ``Render`` on one device at one frame size: the table, the (lo, hi) pairs of a chunk and the workspace of the range kernels,
    allocated once.  ``staging=True`` adds a uint8 buffer [32, h, w, 3] for results that go to the host.  The buffers are reused by every
    call, so all calls of one renderer must be ordered on one stream (the stitch stream of the video paths, or the caller's)."""

    def __init__(self, render: Render, dev: torch.device, h: int, w: int, staging: bool = False):
        self.render, self.dev, self.h, self.w = render, dev, h, w
        self.lib = _lib.load()
        self.mode = {"frame": 0, "video": 1, "quantile": 2, "fixed": None}[render.norm]
        self.rank_lo, self.rank_hi = render.ranks(h, w) if render.norm == "quantile" else (0, 0)
        self.lut = _device_table(render.table(), dev)
        with torch.cuda.device(dev):
            if render.norm == "fixed":
                self.range = torch.tensor([float(render.lo), float(render.hi)], dtype=torch.float32).to(dev)
                torch.cuda.current_stream(dev).synchronize()  # complete before another stream reads it
                self.ws = None
            else:
                self.range = torch.empty((CHUNK, 2), dtype=torch.float32, device=dev)
                self.ws = torch.empty(int(self.lib.edv_render_workspace(CHUNK)), dtype=torch.uint8, device=dev)
            self.stage = torch.empty((CHUNK, h, w, 3), dtype=torch.uint8, device=dev) if staging else None
        self.stride = 0 if render.norm in ("fixed", "video") else 2

    def video_range(self, x: torch.Tensor, st) -> None:
        """norm="video": one range pass over the whole clip; every later ``color`` uses its pair."""
        n = x.shape[0]
        full = torch.empty((n, 2), dtype=torch.float32, device=self.dev)
        ws = torch.empty(int(self.lib.edv_render_workspace(n)), dtype=torch.uint8, device=self.dev)
        _lib.check(self.lib.edv_render_range(x.data_ptr(), n, self.h, self.w, 1, 0, 0, full.data_ptr(), ws.data_ptr(), ws.numel(), st), "edv_render_range")
        self.range = full

    def color(self, x: torch.Tensor, out: torch.Tensor, st, beside: Optional[torch.Tensor] = None) -> None:
        """x [m <= 32, h, w] float32 -> out [m, h, w (2w with ``beside``), 3] uint8, both contiguous on the device; enqueued on stream ``st``."""
        m = x.shape[0]
        assert 1 <= m <= CHUNK and x.is_contiguous() and out.is_contiguous() and x.dtype == torch.float32 and out.dtype == torch.uint8
        assert tuple(out.shape) == (m, self.h, self.w * (2 if beside is not None else 1), 3)
        lib, r = self.lib, self.render
        if self.mode in (0, 2):
            _lib.check(lib.edv_render_range(x.data_ptr(), m, self.h, self.w, self.mode, self.rank_lo, self.rank_hi, self.range.data_ptr(), self.ws.data_ptr(),
                                            self.ws.numel(), st), "edv_render_range")
        _lib.check(lib.edv_render_colorize(x.data_ptr(), m, self.h, self.w, self.range.data_ptr(), self.stride, float(r.eps), r.clip, self.lut.data_ptr(),
                                           _lib.ptr(beside), out.data_ptr(), st), "edv_render_colorize")

    def color_into(self, x: torch.Tensor, dst: torch.Tensor) -> None:
        """``color`` on the current stream for any number of frames, into ``dst`` [m, h, w, 3]: a device tensor is written in place, a pinned host
        tensor through the staging buffer (one copy per chunk, stream-ordered behind the kernel that filled it)."""
        st = C.c_void_p(_lib.stream_ptr(self.dev))
        for a in range(0, x.shape[0], CHUNK):
            b = min(a + CHUNK, x.shape[0])
            if dst.is_cuda:
                self.color(x[a:b], dst[a:b], st)
            else:
                self.color(x[a:b], self.stage[:b - a], st)
                dst[a:b].copy_(self.stage[:b - a], non_blocking=True)


def _on_device(a, dev: torch.device) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(dev).contiguous()
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)  # torch refuses to wrap a read-only array without a warning


def colorize(depth, render: Render, frames=None, output: str = "host"):
    """``depth``: float32 [n, h, w], a numpy array or a tensor on the GPU.  ``frames``: optional uint8 [n, h, w, 3] (array or tensor) put to the
    left of every coloured frame, as ``save_video`` does.  Returns uint8 [n, h, w, 3] (``[n, h, 2w, 3]`` with ``frames``): a numpy array, or
    with ``output="device"`` a tensor on the GPU.  Runs on the caller's current stream, 32 frames at a time; "video" takes one range pass
    over the whole clip first.  A host result is complete when returned; a device result is ordered on the caller's stream."""
    if not isinstance(render, Render):
        raise ValueError(f"render must be a render.Render, got {type(render).__name__}")
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if isinstance(depth, torch.Tensor):
        if not depth.is_cuda:
            raise ValueError("a depth tensor must live on the GPU (pass host data as a numpy array)")
        dev = depth.device
    else:
        depth = np.asarray(depth)
        dev = torch.device("cuda", torch.cuda.current_device())
    if depth.ndim != 3 or str(depth.dtype).replace("torch.", "") != "float32":
        raise ValueError(f"expected float32 depth [n, h, w], got {depth.dtype} {tuple(depth.shape)}")
    n, h, w = (int(v) for v in depth.shape)
    if frames is not None and (tuple(frames.shape) != (n, h, w, 3) or str(frames.dtype).replace("torch.", "") != "uint8"):
        raise ValueError(f"expected uint8 frames [{n}, {h}, {w}, 3], got {frames.dtype} {tuple(frames.shape)}")
    wide = w * (2 if frames is not None else 1)
    with torch.cuda.device(dev):
        if n == 0 or h == 0 or w == 0:
            return torch.empty((n, h, wide, 3), dtype=torch.uint8, device=dev) if output == "device" else np.empty((n, h, wide, 3), dtype=np.uint8)
        x = _on_device(depth, dev)
        side = None if frames is None else _on_device(frames, dev)
        r = DeviceRenderer(render, dev, h, w)
        st = C.c_void_p(_lib.stream_ptr(dev))
        if render.norm == "video":
            r.video_range(x, st)
        out = torch.empty((n, h, wide, 3), dtype=torch.uint8, device=dev)
        for a in range(0, n, CHUNK):
            b = min(a + CHUNK, n)
            r.color(x[a:b], out[a:b], st, None if side is None else side[a:b])
        if output == "device":
            return out
        host = torch.empty((n, h, wide, 3), dtype=torch.uint8, pin_memory=True)
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        return host.numpy()
