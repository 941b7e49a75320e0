"""Surface fusion on the GPU (opt-in): a depth video with its poses integrated into one truncated signed distance (TSDF) volume, and the zero
crossings of that volume as one coloured point list.  Not in the reference, whose ``3d_reconstruction`` clouds concatenate every frame's points:
a thousand re-observations of the same tissue, each frame's depth noise a shell of its own.  Here every voxel averages what the frames saw.

``Volume`` says where the voxels are; ``Tsdf`` owns the arrays on the GPU (``edv_tsdf_integrate`` / ``edv_tsdf_count`` / ``edv_tsdf_extract``,
include/endodav_hip.h) and ``TsdfHost`` is its numpy mirror, the same operations in the same order, so the two agree bit for bit.  The clip,
its depth rule, mask and cameras are a ``cloud.Cloud`` with ``step = 1``:

  state     ``tsdf``, ``weight`` float32 [nz, ny, nx] and optionally ``color`` float32 [nz, ny, nx, 3]; fresh: tsdf = 1, weight = 0, color = 0
  cameras   formed once on the host in float64 and handed to both implementations: W = rows 0..2 of ``np.linalg.inv`` of the 4x4 pose
            T_world_camera, and rows 0 and 1 of K (whose last row must be [0, 0, 1])
  integrate one thread per voxel, the frames in order.  Per voxel (i_x, i_y, i_z) and frame, every operation rounded separately:
            float64  c_a = origin_a + (i_a + 0.5) * voxel;  q_i = ((W[i,0]*c_x + W[i,1]*c_y) + W[i,2]*c_z) + W[i,3];  skip unless q_2 > 0
            float64  u = ((K00*q_0 + K01*q_1) + K02*q_2) / q_2, v likewise from row 1 (pixel centres at (x + 0.5, y + 0.5), the cloud's
                     convention);  skip unless 0 <= u < w and 0 <= v < h;  px = int(u), py = int(v)
            float32  z and the keep predicate of pixel (py, px) are the cloud's (module docstring of ``cloud``);  skip if not kept
            float64  sdf = float64(z) - q_2;  skip if sdf < -trunc;  d = float32(min(1, sdf / trunc))
            float32  wn = weight + 1;  tsdf = (tsdf*weight + d) / wn;  color = (color*weight + float32(rgb)) / wn;  weight = min(wn, max_weight)
  surface   voxel a in linear order (x fastest), axis k in x, y, z, b the neighbour of a along +k inside the grid; the pair emits a point when
            both weights are >= min_weight and (tsdf_a < 0) != (tsdf_b < 0), with 0 and -0 non-negative:
            float32  t = tsdf_a / (tsdf_a - tsdf_b)
            float64  p_k = origin_k + ((i_k + 0.5) + float64(t)) * voxel, the other two coordinates the voxel centre's, stored as float32
            float32  c = c_a + t * (c_b - c_a);  colour = uint8(min(255, max(0, floor(c + 0.5))))
            ordered voxel-major, axis-minor

What is not built: meshes and normals (the points are the edge crossings marching cubes would start from), hashed or sparse volumes, and pose
estimation; poses are inputs, as for the cloud."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .cloud import MAX_FRAMES, Cloud, PointCloud, _check_clip, _on_device, selection


def __getattr__(name):
    if name == "TILE_VOXELS":  # voxels per workgroup of the extraction kernels, from the library's own constant
        return int(_lib.load().edv_tsdf_tile_voxels())
    raise AttributeError(name)


@dataclass(frozen=True, eq=False)
class Volume:
    origin: object                           # the corner of voxel (0, 0, 0), world units: three floats
    voxel: float                             # edge of a voxel
    dims: object                             # (nx, ny, nz)
    trunc: float = None                      # truncation distance; None = 4 * voxel
    max_weight: float = 64.0                 # the running average forgets beyond this many observations

    def __post_init__(self):
        origin = np.asarray(self.origin, dtype=np.float64)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError(f"origin must be three finite numbers, got {self.origin!r}")
        object.__setattr__(self, "origin", tuple(float(v) for v in origin))
        if not _positive(self.voxel):
            raise ValueError(f"voxel must be finite and positive, got {self.voxel!r}")
        object.__setattr__(self, "voxel", float(self.voxel))
        dims = tuple(self.dims) if np.ndim(self.dims) == 1 else ()
        if len(dims) != 3 or any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 1 for d in dims):
            raise ValueError(f"dims must be three integers >= 1, got {self.dims!r}")
        dims = tuple(int(d) for d in dims)
        if dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError(f"a volume holds fewer than 2^31 voxels, got {dims}")
        object.__setattr__(self, "dims", dims)
        trunc = 4.0 * self.voxel if self.trunc is None else self.trunc
        if not _positive(trunc):
            raise ValueError(f"trunc must be finite and positive, got {self.trunc!r}")
        object.__setattr__(self, "trunc", float(trunc))
        if not _positive(self.max_weight) or not _positive(float(np.float32(self.max_weight))):
            raise ValueError(f"max_weight must be finite and positive (as float32), got {self.max_weight!r}")
        object.__setattr__(self, "max_weight", float(self.max_weight))

    @property
    def voxels(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    @classmethod
    def bounding(cls, points, voxel, margin=None, trunc=None, max_weight=64.0) -> "Volume":
        """The volume of ``voxel``-sized voxels around host ``points`` [m, 3] with ``margin`` (default: the truncation distance) on every side."""
        p = np.asarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1 or not np.isfinite(p).all():
            raise ValueError(f"points must be finite, [m, 3] with m >= 1; got shape {tuple(p.shape)}")
        if not _positive(voxel):
            raise ValueError(f"voxel must be finite and positive, got {voxel!r}")
        if margin is None:
            margin = 4.0 * float(voxel) if trunc is None else float(trunc)
        if not (isinstance(margin, (int, float, np.floating, np.integer)) and math.isfinite(margin) and margin >= 0.0):
            raise ValueError(f"margin must be finite and >= 0, got {margin!r}")
        lo, hi = p.min(axis=0) - float(margin), p.max(axis=0) + float(margin)
        dims = np.maximum(np.ceil((hi - lo) / float(voxel)), 1.0).astype(np.int64)
        dims += (lo + dims * float(voxel) < hi)  # the division rounded down across an integer
        return cls(origin=lo, voxel=voxel, dims=tuple(int(d) for d in dims), trunc=trunc, max_weight=max_weight)


def _positive(x) -> bool:
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and math.isfinite(x) and x > 0.0


def cameras(spec: Cloud, n: int) -> np.ndarray:
    """float64 [1 or n, 18]: per camera rows 0..2 of ``np.linalg.inv`` of the 4x4 T_world_camera, row-major, then K00 K01 K02 K10 K11 K12; one row
    when K and pose are shared by all frames.  Formed once, in float64, and used by the kernels and the mirror alike."""
    for a, what in ((spec.K, "K"), (spec.pose, "pose")):
        if a.shape[0] not in (1, n):
            raise ValueError(f"{what} holds {a.shape[0]} matrices for {n} frames")
    if not (spec.K[:, 2, :] == np.array([0.0, 0.0, 1.0])).all():
        raise ValueError("the last row of K must be [0, 0, 1]")
    m = max(spec.K.shape[0], spec.pose.shape[0])
    T = np.zeros((spec.pose.shape[0], 4, 4))
    T[:, :3, :], T[:, 3, 3] = spec.pose, 1.0
    try:
        inv = np.linalg.inv(T)
    except np.linalg.LinAlgError:
        raise ValueError("pose must be invertible") from None
    W = np.broadcast_to(inv[:, :3, :], (m, 3, 4))
    K = np.broadcast_to(spec.K[:, :2, :], (m, 2, 3))
    return np.ascontiguousarray(np.concatenate([W.reshape(m, 12), K.reshape(m, 6)], axis=1))


def _check_integrate(depth, spec, frames, coloured):
    n, h, w = _check_clip(depth, spec, frames)
    if int(spec.step) != 1:
        raise ValueError(f"fusion samples the full-resolution clip: the Cloud must have step 1, got {spec.step}")
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError(f"1 to {MAX_FRAMES} frames per call, got {n}")
    if h < 1 or w < 1:
        raise ValueError(f"empty frames: {h} x {w}")
    if coloured != (frames is not None):
        raise ValueError("a coloured volume takes frames and an uncoloured one takes none")
    return n, h, w, cameras(spec, n), spec.frame_mask(n, h, w)


def _check_surface(min_weight, output):
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, float, np.floating, np.integer)) or not min_weight >= 0.0 or math.isinf(min_weight):
        raise ValueError(f"min_weight must be finite and >= 0, got {min_weight!r}")
    return np.float32(min_weight)


def _staged(a: np.ndarray, dev: torch.device) -> torch.Tensor:
    """A host array on the GPU through pinned memory, ordered on the current stream: the host does not wait for the stream's earlier work."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).pin_memory().to(dev, non_blocking=True)


class TsdfHost:
    """The numpy mirror of the kernels (module docstring): vectorised over the voxels, a loop over the frames."""

    def __init__(self, volume: Volume, coloured: bool = True):
        if not isinstance(volume, Volume):
            raise ValueError(f"volume must be a fusion.Volume, got {type(volume).__name__}")
        self.volume, self.coloured = volume, bool(coloured)
        self.reset()

    def reset(self) -> None:
        nx, ny, nz = self.volume.dims
        self.tsdf = np.ones((nz, ny, nx), np.float32)
        self.weight = np.zeros((nz, ny, nx), np.float32)
        self.color = np.zeros((nz, ny, nx, 3), np.float32) if self.coloured else None

    def arrays(self):
        """(tsdf, weight, color or None): copies."""
        return self.tsdf.copy(), self.weight.copy(), None if self.color is None else self.color.copy()

    def _index(self):
        nx, ny, nz = self.volume.dims
        a = np.arange(self.volume.voxels, dtype=np.int64)
        return a % nx, (a // nx) % ny, a // (nx * ny)

    def integrate(self, depth, spec: Cloud, frames=None) -> None:
        depth = np.asarray(depth)
        n, h, w, cams, mask = _check_integrate(depth, spec, frames, self.coloured)
        vol = self.volume
        origin, voxel, trunc = np.float64(vol.origin), np.float64(vol.voxel), np.float64(vol.trunc)
        cap, one = np.float32(vol.max_weight), np.float32(1.0)
        lo, span, gain, near, far = spec.scalars()
        cx, cy, cz = (origin[k] + (i.astype(np.float64) + 0.5) * voxel for k, i in enumerate(self._index()))
        t, wt = self.tsdf.reshape(-1), self.weight.reshape(-1)           # views: updated in place
        col = None if self.color is None else self.color.reshape(-1, 3)
        rgb = None if frames is None else np.asarray(frames)
        for f in range(n):
            cam = cams[f if cams.shape[0] > 1 else 0]
            W, K = cam[:12].reshape(3, 4), cam[12:].reshape(2, 3)
            with np.errstate(all="ignore"):
                q = [((W[i, 0] * cx + W[i, 1] * cy) + W[i, 2] * cz) + W[i, 3] for i in range(3)]
                ok = q[2] > 0.0
                u = ((K[0, 0] * q[0] + K[0, 1] * q[1]) + K[0, 2] * q[2]) / q[2]
                v = ((K[1, 0] * q[0] + K[1, 1] * q[1]) + K[1, 2] * q[2]) / q[2]
                ok &= (u >= 0.0) & (u < float(w)) & (v >= 0.0) & (v < float(h))
                px, py = np.where(ok, u, 0.0).astype(np.int64), np.where(ok, v, 0.0).astype(np.int64)
                x = depth[f][py, px]
                if spec.source == "depth":
                    z = x * gain
                else:
                    scaled = lo + span * x
                    z = one / scaled
                    z = z * gain
                ok &= (z > near) & (z < far)
                if mask is not None:
                    ok &= (mask[f] if mask.ndim == 3 else mask)[py, px] != 0
                sdf = z.astype(np.float64) - q[2]
                ok &= ~(sdf < -trunc)
                ratio = sdf / trunc
                d = np.where(ratio < 1.0, ratio, 1.0).astype(np.float32)
                wn = wt + one
                t[:] = np.where(ok, (t * wt + d) / wn, t)
                if col is not None:
                    c = rgb[f][py, px].astype(np.float32)
                    col[:] = np.where(ok[:, None], (col * wt[:, None] + c) / wn[:, None], col)
                wt[:] = np.where(ok, np.where(wn < cap, wn, cap), wt)

    def surface(self, min_weight: float = 1.0, output: str = "host") -> PointCloud:
        mw = _check_surface(min_weight, output)
        if output != "host":
            raise ValueError("the host mirror has no device output")
        vol = self.volume
        nx, ny, nz = vol.dims
        origin, voxel = np.float64(vol.origin), np.float64(vol.voxel)
        idx = self._index()
        t, wt = self.tsdf.reshape(-1), self.weight.reshape(-1)
        N = vol.voxels
        cross, tb = np.zeros((N, 3), bool), np.zeros((N, 3), np.float32)
        hop = (1, nx, nx * ny)
        for k in range(3):
            a = np.nonzero(idx[k] + 1 < vol.dims[k])[0]
            b = a + hop[k]
            cross[a, k] = (wt[a] >= mw) & (wt[b] >= mw) & ((t[a] < 0) != (t[b] < 0))
            tb[a, k] = t[b]
        a, k = np.nonzero(cross)                                     # row-major: voxel-major, axis-minor
        with np.errstate(all="ignore"):
            frac = t[a] / (t[a] - tb[a, k])
            points = np.empty((a.shape[0], 3), np.float32)
            for j in range(3):
                ctr = idx[j][a].astype(np.float64) + 0.5
                points[:, j] = (origin[j] + np.where(k == j, ctr + frac.astype(np.float64), ctr) * voxel).astype(np.float32)
            colors = None
            if self.color is not None:
                col = self.color.reshape(-1, 3)
                ca, cb = col[a], col[a + np.asarray(hop, np.int64)[k]]
                c = ca + frac[:, None] * (cb - ca)
                colors = np.minimum(np.float32(255.0), np.maximum(np.float32(0.0), np.floor(c + np.float32(0.5)))).astype(np.uint8)
        return PointCloud(points, colors, np.array([0, a.shape[0]], np.int64))


class Tsdf:
    """A TSDF volume on the GPU.  ``integrate`` folds clips into it, ``surface`` reads its zero crossings; both run on the caller's current
    stream.  ``arrays`` and the tensors ``tsdf``, ``weight`` and ``color`` show the state."""

    def __init__(self, volume: Volume, coloured: bool = True, device="cuda"):
        if not isinstance(volume, Volume):
            raise ValueError(f"volume must be a fusion.Volume, got {type(volume).__name__}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"a Tsdf lives on the GPU (fusion.TsdfHost is the numpy mirror), got device {device!r}")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self.volume, self.coloured = volume, bool(coloured)
        self._lib = _lib.load()
        nx, ny, nz = volume.dims
        with torch.cuda.device(self.device):
            self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
            self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
            self.color = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.device) if self.coloured else None
        self.reset()

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            self.tsdf.fill_(1.0)
            self.weight.zero_()
            if self.color is not None:
                self.color.zero_()

    def arrays(self):
        """(tsdf, weight, color or None) as numpy arrays: host copies."""
        with torch.cuda.device(self.device):
            return self.tsdf.cpu().numpy(), self.weight.cpu().numpy(), None if self.color is None else self.color.cpu().numpy()

    def struct(self) -> _lib.TsdfVolume:
        """The ``edv_tsdf_volume`` of this volume."""
        v = self.volume
        return _lib.TsdfVolume(self.tsdf.data_ptr(), self.weight.data_ptr(), _lib.ptr(self.color), v.dims[0], v.dims[1], v.dims[2],
                               (C.c_double * 3)(*v.origin), v.voxel, v.trunc, float(np.float32(v.max_weight)))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def integrate(self, depth, spec: Cloud, frames=None) -> None:
        """``depth``: float32 [n, h, w], a numpy array or a tensor on this volume's GPU, which is used in place with no copy.  ``frames``: uint8
        [n, h, w, 3] (array or tensor), required by a coloured volume.  One launch on the caller's current stream, ordered on that stream; the
        host does not wait for it."""
        if isinstance(depth, torch.Tensor):
            if not depth.is_cuda or depth.device != self.device:
                raise ValueError(f"a depth tensor must live on the volume's GPU {self.device} (pass host data as a numpy array)")
        else:
            depth = np.asarray(depth)
        n, h, w, cams, mask = _check_integrate(depth, spec, frames, self.coloured)
        with torch.cuda.device(self.device):
            x = _on_device(depth, self.device)
            rgb = None if frames is None else _on_device(frames, self.device)
            mask_d = None if mask is None else _staged(mask, self.device)
            cams_d = _staged(cams, self.device)
            sel = selection(x, spec, mask_d)
            vol = self.struct()
            _lib.check(self._lib.edv_tsdf_integrate(C.byref(vol), C.byref(sel), cams_d.data_ptr(), 18 if cams.shape[0] > 1 else 0, _lib.ptr(rgb),
                                                    self._stream()), "edv_tsdf_integrate")

    def surface(self, min_weight: float = 1.0, output: str = "host") -> PointCloud:
        """The zero crossings between voxels of weight >= ``min_weight``: the count, one read of the total (the one host synchronisation), an
        exact allocation, the extract.  Returns a ``cloud.PointCloud`` with ``offsets = [0, total]``: numpy arrays, or with ``output="device"``
        tensors on the GPU, ordered on the caller's stream.  ``colors`` is None for an uncoloured volume."""
        mw = float(_check_surface(min_weight, output))
        lib, dev, v = self._lib, self.device, self.volume
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            st = self._stream()
            vol = self.struct()
            ws = torch.empty(int(lib.edv_tsdf_workspace(*v.dims)), dtype=torch.uint8, device=dev)
            total_d = torch.empty(1, dtype=torch.int64, device=dev)
            _lib.check(lib.edv_tsdf_count(C.byref(vol), mw, total_d.data_ptr(), ws.data_ptr(), ws.numel(), st), "edv_tsdf_count")
            total_h = torch.empty(1, dtype=torch.int64, pin_memory=True)
            total_h.copy_(total_d, non_blocking=True)
            stream.synchronize()
            total = int(total_h[0])
            offsets = np.array([0, total], np.int64)
            points = torch.empty((total, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((total, 3), dtype=torch.uint8, device=dev) if self.coloured else None
            if total:  # an empty surface launches nothing
                _lib.check(lib.edv_tsdf_extract(C.byref(vol), mw, ws.data_ptr(), ws.numel(), points.data_ptr(), _lib.ptr(colors), total, st), "edv_tsdf_extract")
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
