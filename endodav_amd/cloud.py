"""Point clouds on the GPU (opt-in): a depth video lifted to world-space points with the frames' colours, masked, subsampled and compacted
in order on the device.  What the reference does in float64 numpy on one core, one frame at a time, from depth first copied to the host:
``get_point_cloud(downsample_factor)`` of the loaders in tools/viser-rgbd/utils, and the cloud ``visualize_reconstruction.py`` writes as a ``.ply``.

``Cloud`` says how a clip [n, h, w] becomes points; ``lift`` applies it on the GPU (``edv_cloud_count`` / ``edv_cloud_scatter``,
include/endodav_hip.h) and ``lift_host`` is its numpy mirror, the same operations in the same order, so the two agree bit for bit:

  grid      oh, ow = ceil(h / step), ceil(w / step): the size of ``rgb[::step, ::step]``.  Output pixel (oy, ox) samples the source pixel
            sy = min(oy*step + step//2, h-1), sx = min(ox*step + step//2, w-1), the one that holds the reference's grid position
            ((ox + 0.5) * step, (oy + 0.5) * step)
  depth     float32, every operation rounded separately.  source="depth": z = x * gain.  source="disparity": scaled = lo + span * x,
            z = 1 / scaled, z = z * gain with lo = float32(1 / max_depth), span = float32(1 / min_depth - 1 / max_depth): ``disp_to_depth``,
            then a scale
  kept      (mask is None or mask != 0) and z > near and z < far.  NaN and +-Inf are dropped, so every point is finite
  geometry  float64, every multiply and add rounded separately, with Kinv = inv(K) and T_world_camera = [R | t]:
            u = (ox + 0.5) * step, v = (oy + 0.5) * step;  l_i = (Kinv[i,0]*u + Kinv[i,1]*v) + Kinv[i,2];
            r_i = (R[i,0]*l_0 + R[i,1]*l_1) + R[i,2]*l_2;  p_i = float32(t_i + r_i * float64(z))
            which is the reference's ``T[:, -1] + (R @ (inv(K) @ [u, v, 1])) * depth`` with the order of the sums fixed
  order     frame-major, then row-major over the kept output pixels of a frame: the order of ``rgb[mask]``

Two departures from the reference, both on purpose.  Depth, mask **and colour** of an output pixel all come from the one sampled pixel above,
where the reference's viewer takes the colour from the corner pixel of ``rgb[::step, ::step]`` and the depth from the centre; the two are
identical at ``step = 1``.  And ``K`` is inverted in float64 where the reference inverts the float32 matrix it loaded, which is more exact.

``write_ply`` / ``read_ply`` are the binary little-endian ``.ply`` that ``visualize_reconstruction.py`` writes through open3d, in numpy alone."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

SOURCES = ("depth", "disparity")
MAX_FRAMES = 65535  # frames of one call: the frame is a workgroup index of the kernels


def __getattr__(name):
    if name == "TILE_PIXELS":  # output pixels per workgroup of the kernels, from the library's own constant
        return int(_lib.load().edv_cloud_tile_pixels())
    raise AttributeError(name)


def _stack(a, rows, what):
    """``a`` as float64 [m, rows, cols]: one matrix for all frames (m = 1) or one per frame."""
    a = np.asarray(a, dtype=np.float64)
    ok = {3: ((3, 3),), 4: ((3, 4), (4, 4))}[rows]
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] < 1 or tuple(a.shape[1:]) not in ok or not np.isfinite(a).all():
        raise ValueError(f"{what} must be finite, {' or '.join(str(list(s)) for s in ok)}, or one of them per frame; got shape {tuple(np.shape(a))}")
    return a


@dataclass(frozen=True, eq=False)
class Cloud:
    K: object                                # intrinsics [3, 3] or [n, 3, 3]
    pose: object = None                      # T_world_camera [3, 4] / [4, 4] or one per frame; None = identity
    step: int = 1
    source: str = "disparity"
    min_depth: float = 0.1                   # "disparity" only
    max_depth: float = 150.0
    gain: float = 1.0
    near: float = 1e-3
    far: float = 150.0
    mask: object = None                      # [h, w] or [n, h, w], bool or uint8; non-zero = keep

    def __post_init__(self):
        object.__setattr__(self, "K", _stack(self.K, 3, "K"))
        object.__setattr__(self, "pose", _stack(np.eye(4)[:3] if self.pose is None else self.pose, 4, "pose")[:, :3, :])
        if isinstance(self.step, bool) or not isinstance(self.step, (int, np.integer)) or not 1 <= self.step < 2 ** 31:
            raise ValueError(f"step must be an integer >= 1, got {self.step!r}")
        if self.source not in SOURCES:
            raise ValueError(f"source must be one of {SOURCES}, got {self.source!r}")
        if not (math.isfinite(self.min_depth) and math.isfinite(self.max_depth) and 0.0 < self.min_depth < self.max_depth):
            raise ValueError(f"need finite 0 < min_depth < max_depth, got {self.min_depth!r}, {self.max_depth!r}")
        if not math.isfinite(self.gain):
            raise ValueError(f"gain must be finite, got {self.gain!r}")
        if not float(np.float32(self.near)) < float(np.float32(self.far)):  # NaN fails too
            raise ValueError(f"need near < far (as float32), got near={self.near!r}, far={self.far!r}")
        if (np.linalg.matrix_rank(self.K) < 3).any():
            raise ValueError("K must be invertible")
        if self.mask is not None:
            m = np.asarray(self.mask)
            if m.ndim not in (2, 3) or m.dtype not in (np.bool_, np.uint8):
                raise ValueError(f"mask must be bool or uint8, [h, w] or [n, h, w]; got {m.dtype} {m.shape}")
            object.__setattr__(self, "mask", np.ascontiguousarray(m != 0).view(np.uint8))

    @property
    def mode(self) -> int:
        return SOURCES.index(self.source)

    def scalars(self):
        """(lo, span, gain, near, far) as the float32 values both implementations compute with, formed from Python doubles."""
        lo, span = 1.0 / float(self.max_depth), 1.0 / float(self.min_depth) - 1.0 / float(self.max_depth)
        return tuple(np.float32(v) for v in (lo, span, self.gain, self.near, self.far))

    def cams(self, n: int) -> np.ndarray:
        """float64 [1 or n, 21]: per camera inv(K) [3, 3], R [3, 3] and t [3], the matrices row-major; one row when K and pose are shared by all
        frames.  K is inverted in float64 (``np.linalg.inv(K.astype(np.float64))``): the reference inverts in float32, this is more exact."""
        for a, what in ((self.K, "K"), (self.pose, "pose")):
            if a.shape[0] not in (1, n):
                raise ValueError(f"{what} holds {a.shape[0]} matrices for {n} frames")
        m = max(self.K.shape[0], self.pose.shape[0])
        kinv = np.broadcast_to(np.linalg.inv(self.K.astype(np.float64)), (m, 3, 3))
        pose = np.broadcast_to(self.pose, (m, 3, 4))
        return np.ascontiguousarray(np.concatenate([kinv.reshape(m, 9), pose[:, :, :3].reshape(m, 9), pose[:, :, 3]], axis=1))

    def frame_mask(self, n: int, h: int, w: int) -> Optional[np.ndarray]:
        """The mask as uint8 [h, w] or [n, h, w], checked against the clip."""
        if self.mask is not None and tuple(self.mask.shape) not in ((h, w), (n, h, w)):
            raise ValueError(f"mask {tuple(self.mask.shape)} fits neither [{h}, {w}] nor [{n}, {h}, {w}]")
        return self.mask


@dataclass(frozen=True, eq=False)
class PointCloud:
    """``points`` float32 [total, 3] and ``colors`` uint8 [total, 3] or None (numpy arrays, or tensors on the GPU), frame-major;
    ``offsets`` int64 [n + 1] on the host: frame i owns points offsets[i] .. offsets[i + 1]."""
    points: object
    colors: object
    offsets: np.ndarray

    def __len__(self) -> int:
        return int(self.offsets[-1])

    def frame(self, i: int):
        """(points, colors) of frame i: views, no copy."""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.points[a:b], None if self.colors is None else self.colors[a:b]


def _check_clip(depth, spec, frames):
    if not isinstance(spec, Cloud):
        raise ValueError(f"spec must be a cloud.Cloud, got {type(spec).__name__}")
    if depth.ndim != 3 or str(depth.dtype).replace("torch.", "") != "float32":
        raise ValueError(f"expected float32 depth [n, h, w], got {depth.dtype} {tuple(depth.shape)}")
    n, h, w = (int(v) for v in depth.shape)
    if frames is not None and (tuple(frames.shape) != (n, h, w, 3) or str(frames.dtype).replace("torch.", "") != "uint8"):
        raise ValueError(f"expected uint8 frames [{n}, {h}, {w}, 3], got {frames.dtype} {tuple(frames.shape)}")
    return n, h, w


def _empty(n: int, coloured: bool, dev=None) -> PointCloud:
    if dev is None:
        return PointCloud(np.empty((0, 3), np.float32), np.empty((0, 3), np.uint8) if coloured else None, np.zeros(n + 1, np.int64))
    return PointCloud(torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.uint8, device=dev) if coloured else None,
                      np.zeros(n + 1, np.int64))


def lift_host(depth, spec: Cloud, frames=None) -> PointCloud:
    """The numpy mirror of the kernels (module docstring): float32 depth [n, h, w] and optional uint8 frames [n, h, w, 3] -> ``PointCloud``."""
    depth = np.asarray(depth)
    n, h, w = _check_clip(depth, spec, frames)
    if n == 0 or h == 0 or w == 0:
        return _empty(n, frames is not None)
    step = int(spec.step)
    oh, ow = -(-h // step), -(-w // step)
    sy = np.minimum(np.arange(oh, dtype=np.int64) * step + step // 2, h - 1)
    sx = np.minimum(np.arange(ow, dtype=np.int64) * step + step // 2, w - 1)
    lo, span, gain, near, far = spec.scalars()
    x = depth[:, sy][:, :, sx]
    with np.errstate(all="ignore"):
        if spec.source == "depth":
            z = x * gain
        else:
            scaled = lo + span * x
            z = np.float32(1.0) / scaled
            z = z * gain
        keep = (z > near) & (z < far)
    mask = spec.frame_mask(n, h, w)
    if mask is not None:
        keep &= (mask[..., sy, :][..., sx] != 0)
    u = np.broadcast_to(((np.arange(ow, dtype=np.float64) + 0.5) * float(step))[None, :], (oh, ow))
    v = np.broadcast_to(((np.arange(oh, dtype=np.float64) + 0.5) * float(step))[:, None], (oh, ow))
    cams = spec.cams(n)
    points, colors, offsets = [], [], np.zeros(n + 1, np.int64)
    for f in range(n):
        cam = cams[f if cams.shape[0] > 1 else 0]
        kinv, rot, t = cam[:9].reshape(3, 3), cam[9:18].reshape(3, 3), cam[18:]
        k = keep[f]
        uu, vv, zz = u[k], v[k], z[f][k].astype(np.float64)
        l = [(kinv[i, 0] * uu + kinv[i, 1] * vv) + kinv[i, 2] for i in range(3)]
        p = np.empty((uu.shape[0], 3), np.float32)
        with np.errstate(all="ignore"):
            for i in range(3):
                r = (rot[i, 0] * l[0] + rot[i, 1] * l[1]) + rot[i, 2] * l[2]
                p[:, i] = (t[i] + r * zz).astype(np.float32)
        points.append(p)
        if frames is not None:
            colors.append(np.asarray(frames[f])[sy][:, sx][k])
        offsets[f + 1] = offsets[f] + uu.shape[0]
    return PointCloud(np.concatenate(points), np.concatenate(colors) if frames is not None else None, offsets)


def _on_device(a, dev: torch.device) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(dev).contiguous()
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)  # torch refuses to wrap a read-only array without a warning


def selection(x: torch.Tensor, spec: Cloud, mask: Optional[torch.Tensor]) -> _lib.CloudSelection:
    """The ``edv_cloud_selection`` of a contiguous float32 clip [n, h, w] on the GPU and an optional uint8 mask there."""
    n, h, w = (int(v) for v in x.shape)
    lo, span, gain, near, far = (float(v) for v in spec.scalars())
    return _lib.CloudSelection(x.data_ptr(), n, h, w, int(spec.step), spec.mode, lo, span, gain, near, far, _lib.ptr(mask),
                               h * w if mask is not None and mask.dim() == 3 else 0)


def lift(depth, spec: Cloud, frames=None, output: str = "host") -> PointCloud:
    """``depth``: float32 [n, h, w], a numpy array or a tensor on the GPU, which is used in place with no copy.  ``frames``: optional uint8
    [n, h, w, 3] (array or tensor), the points' colours.  Runs on the caller's current stream: the count, one read of the total (the one host
    synchronisation), an exact allocation, the scatter.  Returns a ``PointCloud`` of numpy arrays, or with ``output="device"`` of tensors on the
    GPU (``offsets`` is on the host either way).  A host result is complete when returned; a device result is ordered on the caller's stream."""
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if isinstance(depth, torch.Tensor):
        if not depth.is_cuda:
            raise ValueError("a depth tensor must live on the GPU (pass host data as a numpy array)")
        dev = depth.device
    else:
        depth = np.asarray(depth)
        dev = torch.device("cuda", torch.cuda.current_device()) if output == "device" or depth.size else None
    n, h, w = _check_clip(depth, spec, frames)
    if n > MAX_FRAMES:
        raise ValueError(f"at most {MAX_FRAMES} frames per call, got {n}")
    cams = spec.cams(n)
    mask = spec.frame_mask(n, h, w)
    if n == 0 or h == 0 or w == 0:  # nothing to lift: the library is not touched
        return _empty(n, frames is not None, dev if output == "device" else None)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        st = C.c_void_p(stream.cuda_stream)
        x = _on_device(depth, dev)
        rgb = None if frames is None else _on_device(frames, dev)
        mask_d = None if mask is None else _on_device(mask, dev)
        cams_d = _on_device(cams, dev)
        sel = selection(x, spec, mask_d)
        ws = torch.empty(max(int(lib.edv_cloud_workspace(n, h, w, int(spec.step))), 8), dtype=torch.uint8, device=dev)
        offsets_d = torch.empty(n + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.edv_cloud_count(C.byref(sel), offsets_d.data_ptr(), ws.data_ptr(), ws.numel(), st), "edv_cloud_count")
        offsets = torch.empty(n + 1, dtype=torch.int64, pin_memory=True)
        offsets.copy_(offsets_d, non_blocking=True)
        stream.synchronize()
        offsets = offsets.numpy().copy()
        total = int(offsets[n])
        points = torch.empty((total, 3), dtype=torch.float32, device=dev)
        colors = None if rgb is None else torch.empty((total, 3), dtype=torch.uint8, device=dev)
        if total:
            _lib.check(lib.edv_cloud_scatter(C.byref(sel), cams_d.data_ptr(), 21 if cams.shape[0] > 1 else 0, _lib.ptr(rgb), offsets_d.data_ptr(), ws.data_ptr(),
                                             ws.numel(), points.data_ptr(), _lib.ptr(colors), total, st), "edv_cloud_scatter")
        if output == "device":
            return PointCloud(points, colors, offsets)
        host_p = torch.empty((total, 3), dtype=torch.float32, pin_memory=True)
        host_p.copy_(points, non_blocking=True)
        host_c = None
        if colors is not None:
            host_c = torch.empty((total, 3), dtype=torch.uint8, pin_memory=True)
            host_c.copy_(colors, non_blocking=True)
        stream.synchronize()
        return PointCloud(host_p.numpy(), None if host_c is None else host_c.numpy(), offsets)


# ---- .ply ---------------------------------------------------------------------------------------------------------------------------------
def _vertex_dtype(coloured: bool) -> np.dtype:
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if coloured else [])
    return np.dtype(fields)  # packed: 12 or 15 bytes a vertex


def write_ply(path, cloud: PointCloud, frame: Optional[int] = None) -> None:
    """Binary little-endian ``.ply``: vertices ``x y z`` float and, if the cloud has colours, ``red green blue`` uchar.  ``frame``: that frame alone."""
    points, colors = (cloud.points, cloud.colors) if frame is None else cloud.frame(frame)
    if isinstance(points, torch.Tensor):
        points, colors = points.cpu().numpy(), None if colors is None else colors.cpu().numpy()
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    vertex = np.empty(points.shape[0], _vertex_dtype(colors is not None))
    for i, name in enumerate("xyz"):
        vertex[name] = points[:, i]
    if colors is not None:
        colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
        for i, name in enumerate(("red", "green", "blue")):
            vertex[name] = colors[:, i]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {points.shape[0]}", "property float x", "property float y", "property float z"]
    if colors is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vertex.tobytes())


def read_ply(path) -> PointCloud:
    """A ``.ply`` as ``write_ply`` writes it -> ``PointCloud`` of one frame (``offsets = [0, count]``)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a .ply file")
    lines = data[:end].decode("ascii").split("\n")[:-1]
    if lines[1] != "format binary_little_endian 1.0" or not lines[2].startswith("element vertex "):
        raise ValueError(f"{path}: expected a binary little-endian .ply that starts with its vertices")
    count, props = int(lines[2].split()[2]), lines[3:]
    xyz = ["property float x", "property float y", "property float z"]
    rgb = ["property uchar red", "property uchar green", "property uchar blue"]
    if props not in (xyz, xyz + rgb):
        raise ValueError(f"{path}: vertex properties other than x y z float (and red green blue uchar)")
    dt = _vertex_dtype(props != xyz)
    body = data[end + len(b"end_header\n"):]
    if len(body) != count * dt.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes of vertices, the header says {count} x {dt.itemsize}")
    vertex = np.frombuffer(body, dt)
    points = np.stack([vertex["x"], vertex["y"], vertex["z"]], axis=1).astype(np.float32) if count else np.empty((0, 3), np.float32)
    colors = None
    if props != xyz:
        colors = np.stack([vertex["red"], vertex["green"], vertex["blue"]], axis=1) if count else np.empty((0, 3), np.uint8)
    return PointCloud(points, colors, np.array([0, count], np.int64))
