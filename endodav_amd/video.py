"""Whole-video inference around the per-clip forward: windowing, key-frame reuse and stitching
(reference ``models/endodav/endodav.py:162-254`` with ``utils/util.py:16-74`` and the
``Resize`` size rule of ``models/endodav/util/transform.py:52-105``).

Differences in *where* work happens, not in what is computed:
  - each window's 32 frames are uploaded as uint8 while the previous window computes, converted to float and
    (if needed) bicubically resized on the GPU by ``edv_resize_bicubic`` instead of per-frame ``cv2.resize`` on the host;
  - each window's 32 disparity maps are resized to the native frame size on the GPU by
    ``edv_bilinear`` and come back in ONE device→host copy instead of 32, behind the next window's forward;
  - the windows of one video are independent given the input frames (``window_sources``) and can be sharded over ranks
    (``shard_windows=True``, opt-in);
  - the least-squares scale/shift and the cross-fade run in numpy float32 exactly as the reference's (``stitch="host"``, the default), or
    on the GPU with fp64 sums, fused with the resize back to the frame size (``stitch="device"``, opt-in: ``edv_stitch_fit`` /
    ``edv_stitch_apply``, tests/test_stitch_gpu.py).

The cv2.INTER_CUBIC pre-resize is "parity unpinned" (cv2 is absent from the build
container and the reference has no fixture for it); the kernel implements the published algorithm
(Keys cubic, a = -0.75, half-pixel centres, clamped borders) and is held to it in fp64 at the sizes a
video feeds it (``tests/test_kernels_gpu.py``).  When the frames already have the network's size the
resize is the identity (bit for bit) and the whole path is pinned by ``tests/test_video_gpu.py``
(windowing, key frames, stitching: reference goldens of 2 and 6 windows; the pipelined runner against
the window-by-window forward) and ``tests/test_host_cpu.py`` (the host logic alone).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

INFER_LEN = 32
OVERLAP = 10
KEYFRAMES = [6, 12, 24, 25, 26, 27, 28, 29, 30, 31]
INTERP_LEN = 8


# ---------------------------------------------------------------------------------------------
# host logic (pure numpy / python; shared with the tests)
# ---------------------------------------------------------------------------------------------
def lower_bound_size(width: int, height: int, target_w: int, target_h: int, multiple: int = 14) -> Tuple[int, int]:
    """transform.py:52-105 for keep_aspect_ratio=True, resize_method='lower_bound':
    scale both axes by the larger of the two ratios, round to a multiple of 14, never below target."""
    scale = max(target_w / width, target_h / height)

    def snap(x, lo):
        y = int(np.round(x / multiple) * multiple)
        if y < lo:
            y = int(np.ceil(x / multiple) * multiple)
        return y

    return snap(scale * width, target_w), snap(scale * height, target_h)


def window_plan(n_frames: int) -> Tuple[int, List[int]]:
    """endodav.py:185-193: pad with copies of the last frame to k*22+10 frames; windows start every 22."""
    step = INFER_LEN - OVERLAP
    pad = (step - (n_frames % step)) % step + (INFER_LEN - step)
    return n_frames + pad, list(range(0, n_frames, step))


def scale_and_shift(pred: np.ndarray, target: np.ndarray) -> Tuple[float, float]:
    """Least-squares (s, t) with s*pred + t ≈ target over all pixels (utils/util.py:40-63, mask = 1)."""
    pred = pred.astype(np.float32)
    target = target.astype(np.float32)
    a00 = np.sum(pred * pred)
    a01 = np.sum(pred)
    a11 = np.float32(pred.size)
    b0 = np.sum(pred * target)
    b1 = np.sum(target)
    det = a00 * a11 - a01 * a01
    if det == 0:
        return 1, 0
    return (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det


def stitch_windows(depths: List[np.ndarray], n_keep: int) -> np.ndarray:
    """endodav.py:213-254.  ``depths``: per-window arrays [32, H, W] in window order."""
    align_len = OVERLAP - INTERP_LEN
    out: List[np.ndarray] = []
    # cross-fade weights of get_interpolate_frames (utils/util.py:66-74): python floats 0, 1/7, ..., 1
    step = 1.0 / (INTERP_LEN - 1)
    fade = [0.0] + [i * step for i in range(1, INTERP_LEN - 1)] + [1.0]
    for wi, cur in enumerate(depths):
        if wi == 0:
            out.extend(cur[i] for i in range(INFER_LEN))
            continue
        pre = out[-INTERP_LEN:]
        post = [cur[i] for i in range(align_len, OVERLAP)]
        s, t = scale_and_shift(np.concatenate(post), np.concatenate(pre))
        for i in range(INTERP_LEN):
            p = post[i] * s + t
            p[p < 0] = 0
            out[len(out) - INTERP_LEN + i] = pre[i] * (1 - fade[i]) + p * fade[i]
        for i in range(OVERLAP, INFER_LEN):
            d = cur[i] * s + t
            d[d < 0] = 0
            out.append(d)
    return np.stack(out[:n_keep], axis=0)


def window_sources(n_frames: int) -> List[np.ndarray]:
    """For every window, the index of the ORIGINAL frame each of its 32 input slots shows (endodav.py:185-199).

    Slots of window k are frames s0 .. s0+31 of the padded list (padding = copies of the last frame), except that the first
    OVERLAP slots are refilled with the KEYFRAMES slots of window k-1's *input* -- itself refilled the same way, so slot 0 of
    window k is slot 6 of window k-1, which is slot 26 of window k-2.  Inputs never depend on outputs, so the whole chain
    resolves to indices up front and any window can be built (and run, on any GPU) independently of the others."""
    _, starts = window_plan(n_frames)
    out: List[np.ndarray] = []
    for k, s0 in enumerate(starts):
        idx = np.minimum(np.arange(s0, s0 + INFER_LEN), n_frames - 1)
        if k > 0:
            idx[:OVERLAP] = out[k - 1][KEYFRAMES]
        out.append(idx)
    return out


def _video_lanes(model, dev: torch.device):
    """(dash, depth, flight) of the video paths: the model's cached ``_video_flight`` (built once: a lane's engine context holds packed weights
    and a workspace), shared by ``HipWindowRunner`` and ``DepthStream``.
    A lora_type="dash" model counts its forwards (one DashLinear call counter per model, switched on after 100 calls) and so has one
    engine context only: its windows run one at a time on lane 0, on one stream, one _dash_step per window in window
    order -- the reference's sequence of forward calls.  The copies still overlap the forward."""
    from .pipeline import ClipsInFlight

    dash = getattr(model, "lora_type", None) == "dash"
    depth = 1 if dash else ClipsInFlight.auto_depth(model, INFER_LEN)
    flight = None if dash else getattr(model, "_video_flight", None)
    if not dash and (flight is None or flight.dev != dev or flight.depth != depth):
        flight = ClipsInFlight(model, dev, depth=depth)
        try:
            model._video_flight = flight
        except Exception:
            pass
    return dash, depth, flight


def _pre_resize(lib, cur: torch.Tensor, fh: int, fw: int, th: int, tw: int, st) -> torch.Tensor:
    """The pre-resize step of ``HipWindowRunner._run_windows``, shared with ``DepthStream`` so that both feed the forward the same bits:
    ``cur`` is the window's converted frames (``permute -> float32 -> div_(255.0)``, in the memory layout ``.to`` leaves it in)."""
    if (th, tw) == (fh, fw):
        return cur
    small = torch.empty((INFER_LEN, 3, th, tw), device=cur.device, dtype=torch.float32)
    _lib.check(lib.edv_resize_bicubic(cur.data_ptr(), small.data_ptr(), INFER_LEN * 3, fh, fw, th, tw, st), "edv_resize_bicubic")
    return small


class _DeviceStitch:
    """The state of the device stitch, shared by ``HipWindowRunner.run_stitched`` and ``DepthStream``: two frame-size buffers [32, fh, fw] that
    alternate between the windows (the 8-frame tail window k is fitted against is the end of window k-1's buffer), (s, t) and the workspace
    of edv_stitch_fit, and ``done``, the number of output frames handed out as final.  After window k the output has 32 + 22 k frames of
    which all but the last 8 are final; window 0 holds frames 0..31, window k >= 1 frames 22 k + 10 .. 22 k + 31."""

    def __init__(self, lib, dev: torch.device, fh: int, fw: int, nbuf: int = 2):
        self.lib, self.fh, self.fw = lib, fh, fw
        self.ring = [torch.empty((INFER_LEN, fh, fw), dtype=torch.float32, device=dev) for _ in range(nbuf)]
        self.st = torch.empty(2, dtype=torch.float32, device=dev)
        self.ws = torch.empty(int(lib.edv_stitch_workspace()), dtype=torch.uint8, device=dev)
        self.done = 0

    def window(self, k: int, disp: torch.Tensor, s_st: torch.cuda.Stream) -> None:
        """Fit and apply window k's network-size disparity [32, 1, ih, iw]; called under ``torch.cuda.stream(s_st)``, in window order, once
        ``s_st`` waits for the lane.  ``disp`` belongs to the lane's allocator pool: ``record_stream`` keeps it until ``s_st`` has read it."""
        lib, fh, fw, ring = self.lib, self.fh, self.fw, self.ring
        step = INFER_LEN - OVERLAP
        st = C.c_void_p(s_st.cuda_stream)
        disp = disp.contiguous()
        ih, iw = disp.shape[-2], disp.shape[-1]
        cur = ring[k % 2]
        if k == 0:
            _lib.check(lib.edv_stitch_apply(disp.data_ptr(), ih, iw, None, None, cur.data_ptr(), fh, fw, st), "edv_stitch_apply")
        else:
            tail = ring[(k - 1) % 2][(INFER_LEN if k == 1 else step) - INTERP_LEN:]
            _lib.check(lib.edv_stitch_fit(disp.data_ptr(), ih, iw, tail.data_ptr(), fh, fw, self.st.data_ptr(), self.ws.data_ptr(), self.ws.numel(), st),
                       "edv_stitch_fit")
            _lib.check(lib.edv_stitch_apply(disp.data_ptr(), ih, iw, self.st.data_ptr(), tail.data_ptr(), cur.data_ptr(), fh, fw, st), "edv_stitch_apply")
        disp.record_stream(s_st)

    def final_pieces(self, upto: int) -> List[Tuple[int, torch.Tensor]]:
        """[(g, frames g .. g + len - 1 as a view of a buffer)] covering output frames ``done`` .. ``upto`` - 1, in order, and ``done`` moves to
        ``upto``: at most two pieces per window, the faded tail in window k-1's buffer, then window k's own frames."""
        step = INFER_LEN - OVERLAP
        pieces = []
        g = self.done
        while g < upto:
            w, i = (0, g) if g < INFER_LEN else ((g - OVERLAP) // step, (g - OVERLAP) % step)
            cnt = min(upto - g, (INFER_LEN if w == 0 else step) - i)
            pieces.append((g, self.ring[w % 2][i:i + cnt]))
            g += cnt
        self.done = max(self.done, upto)
        return pieces


class HipWindowRunner:
    """Runs 32-frame windows of one video through the HIP forward, pipelined over copy streams and (round 3) up to three compute lanes:

      copy-in stream   window k+1: pinned uint8 frames [32, H, W, 3] -> HBM (2.5 MB .. 126 MB; the whole video is never resident,
                       and nothing is converted to fp32 on the host: the reference ships 4x the bytes, endodav.py:195-197)
      lane streams     window k (and, where a window does not fill the part, k-1, k-2 beside it): uint8 -> [0, 1] fp32 NCHW, bicubic pre-resize to the network's size (edv_resize_bicubic, replaces the
                       host's per-frame cv2.resize), edv_forward, bilinear back to the frame size (edv_bilinear)
      copy-out stream  window k-1: the 32 maps -> pinned host memory in ONE copy (the reference: 32 synchronous .cpu() calls, :205-206)

    so the PCIe transfers of the neighbouring windows hide behind the forward.  Two buffers per stage; the host blocks only
    when it is about to reuse one."""

    def __init__(self, model, frames: np.ndarray, dev: torch.device):
        self.model, self.frames, self.dev = model, frames, dev
        self.n, self.fh, self.fw = frames.shape[:3]
        ih, iw = model.image_shape
        self.tw, self.th = lower_bound_size(self.fw, self.fh, iw, ih)

    def _run_windows(self, sources: Sequence[np.ndarray], begin, before_forward, after_forward) -> None:
        """The part both stitch paths share: upload, conversion, pre-resize and forward of every window, on the copy-in stream and the lanes.
        ``begin(nbuf, entry)`` allocates the caller's buffers (``nbuf`` slots are in use at a time; ``entry``: see the stream contract below),
        ``before_forward(k, slot)`` runs on the host before window k is enqueued, ``after_forward(k, slot, stream, disp)`` under the lane's
        stream right after its forward: ``disp`` [32, 1, ih, iw] is the window's network-size disparity, valid in stream order."""
        lib = _lib.load()
        dev, fh, fw, th, tw = self.dev, self.fh, self.fw, self.th, self.tw
        with torch.cuda.device(dev), torch.no_grad():
            # Round 3: consecutive windows are independent (window_sources), so up to `depth` of them are in flight on the GPU, each on its own
            # engine context and stream (pipeline.ClipsInFlight; depth by auto_depth: 3 lanes at the reference's 224 x 280, one at 518 x 518 where a
            # 32-frame window fills the part alone -- ViT-S 224 x 280 T=32: 4140 -> 4380..4760 frames/s, profiles/r03_notes.txt).  A lane's stream
            # carries the whole per-window chain: uint8 -> float, pre-resize, forward, resize back.
            # A lora_type="dash" model runs its windows one at a time on lane 0, on one stream of this runner (_video_lanes).
            dash, depth, flight = _video_lanes(self.model, dev)
            nbuf = min(depth + 1, len(sources))
            s_in = torch.cuda.Stream(device=dev)
            s_dash = torch.cuda.Stream(device=dev) if dash else None
            # Stream contract: run() orders itself after everything the caller has enqueued on its current stream so far -- an optimizer.step() or
            # load_state_dict whose weights the first forward on a lane folds and packs, and earlier users of the memory the buffers below get
            # from that stream's allocator pool, which are first written on the streams of this runner.  The copy-in stream and every lane wait
            # for this event once; the copy-out stream (the stitch stream) follows the lanes.  All work is drained before run() returns host arrays.
            entry = torch.cuda.Event()
            entry.record(torch.cuda.current_stream(dev))
            s_in.wait_event(entry)
            h_in = [torch.empty((INFER_LEN, fh, fw, 3), dtype=torch.uint8).pin_memory() for _ in range(nbuf)]
            d_in = [torch.empty((INFER_LEN, fh, fw, 3), dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            begin(nbuf, entry)
            up_done: List[Optional[torch.cuda.Event]] = [None] * nbuf     # H2D of the slot finished (host buffer reusable, device buffer valid)
            used: List[Optional[torch.cuda.Event]] = [None] * nbuf        # the conversion that read d_in[slot] finished (device buffer reusable)

            def upload(k: int) -> None:
                slot = k % nbuf
                if up_done[slot] is not None:
                    up_done[slot].synchronize()       # the host buffer is about to be rewritten
                np.take(self.frames, sources[k], axis=0, out=h_in[slot].numpy())
                with torch.cuda.stream(s_in):
                    if used[slot] is not None:
                        s_in.wait_event(used[slot])   # the conversion of the window that used this slot before has read the device buffer
                    d_in[slot].copy_(h_in[slot], non_blocking=True)
                    up_done[slot] = torch.cuda.Event()
                    up_done[slot].record(s_in)

            upload(0)
            for k in range(len(sources)):
                slot = k % nbuf
                if k + 1 < len(sources):
                    upload(k + 1)                     # overlaps the windows in flight
                before_forward(k, slot)
                stream, lane = (s_dash, 0) if dash else flight.next_lane(INFER_LEN)
                if k < depth:
                    stream.wait_event(entry)          # the lanes come round-robin: the first `depth` windows reach each of them once
                with torch.cuda.stream(stream):
                    st = C.c_void_p(_lib.stream_ptr(dev))
                    stream.wait_event(up_done[slot])
                    cur = d_in[slot].permute(0, 3, 1, 2).to(torch.float32).div_(255.0)  # [32, 3, H, W] in [0, 1]
                    used[slot] = torch.cuda.Event()
                    used[slot].record(stream)
                    cur = _pre_resize(lib, cur, fh, fw, th, tw, st)
                    disp = self.model(cur.unsqueeze(0), lane=lane)[("disp", 0)]  # [32, 1, ih, iw]
                    after_forward(k, slot, stream, disp)

    def run(self, sources: Sequence[np.ndarray]) -> List[np.ndarray]:
        """The frame-size maps [32, fh, fw] of the given windows, in the order given (``stitch="host"``, and one rank's share of
        ``shard_windows=True``): edv_bilinear on the lane, one device->host copy per window on the copy-out stream."""
        lib = _lib.load()
        dev, fh, fw = self.dev, self.fh, self.fw
        if not sources:
            return []
        results: List[np.ndarray] = []
        h_out: List[torch.Tensor] = []
        d_out: List[torch.Tensor] = []
        out_done: List[Optional[torch.cuda.Event]] = []                   # D2H of the slot finished
        s_out = torch.cuda.Stream(device=dev)

        def begin(nbuf: int, entry: torch.cuda.Event) -> None:
            h_out.extend(torch.empty((INFER_LEN, fh, fw), dtype=torch.float32).pin_memory() for _ in range(nbuf))
            d_out.extend(torch.empty((INFER_LEN, fh, fw), dtype=torch.float32, device=dev) for _ in range(nbuf))
            out_done.extend([None] * nbuf)

        def drain(slot: int) -> None:
            if out_done[slot] is not None:
                out_done[slot].synchronize()
                results.append(h_out[slot].numpy().copy())
                out_done[slot] = None

        def before_forward(k: int, slot: int) -> None:
            drain(slot)                               # frees d_out[slot] / h_out[slot] (window k - nbuf's copy), in window order

        def after_forward(k: int, slot: int, stream: torch.cuda.Stream, disp: torch.Tensor) -> None:
            full = d_out[slot]
            st = C.c_void_p(_lib.stream_ptr(dev))
            _lib.check(lib.edv_bilinear(disp.data_ptr(), full.data_ptr(), INFER_LEN, disp.shape[-2], disp.shape[-1], 1, fh, fw, st), "edv_bilinear")
            ready = torch.cuda.Event()
            ready.record(stream)
            with torch.cuda.stream(s_out):
                s_out.wait_event(ready)
                h_out[slot].copy_(full, non_blocking=True)
                out_done[slot] = torch.cuda.Event()
                out_done[slot].record(s_out)

        self._run_windows(sources, begin, before_forward, after_forward)
        nbuf = len(h_out)
        for k in range(max(len(sources) - nbuf, 0), len(sources)):  # in window order: oldest slot first
            drain(k % nbuf)
        return results

    def run_stitched(self, sources: Sequence[np.ndarray], n_keep: int, output: str = "host", render=None):
        """``stitch="device"``: all windows of the video (``window_sources``) -> the stitched result [n_keep, fh, fw], float32, in pinned host memory
        (``output="host"``) or, by the same kernels and with the same bits, as a tensor on the device (``output="device"``: the final frames are
        copied device-to-device instead of to the pinned buffer).  Either way all work is drained before the call returns.

        The windows run as in ``run``.  One more stream, the stitch stream, takes the lanes' ``ready`` events in window order and, for window k,
        fits (s, t) against the 8-frame tail of the output so far (edv_stitch_fit; k >= 1), writes the window's new frames and cross-fades the
        tail in place (edv_stitch_apply), and copies the frames that became final straight into the result: after window k the output has
        32 + 22 k frames of which all but the last 8 are final.  Both kernels upsample the network-size disparity on the fly, so the 32
        frame-size maps of a window exist nowhere; two frame-size buffers [32, fh, fw] alternate between the windows (the tail is the end of the
        previous window's buffer), whatever the length of the video.  Padding frames beyond ``n_keep`` are computed and never copied.
        A window's disparity is a tensor of the lane's allocator pool: ``record_stream`` keeps its memory from being handed out again before
        the stitch stream has read it.

        ``render`` (a ``render.Render``): the result is the coloured video, uint8 [n_keep, fh, fw, 3].  For "frame", "fixed" and "quantile" the
        stitch stream colours every block of final frames where it would have copied it (``render.DeviceRenderer``) and copies the uint8 block
        into the result: no fp32 video exists anywhere and 3 bytes a pixel leave the device instead of 4.  "video" needs the range of the
        whole video first: the fp32 video is built on the device as for ``output="device"``, then one range pass, then the colouring."""
        lib = _lib.load()
        dev, fh, fw = self.dev, self.fh, self.fw
        step = INFER_LEN - OVERLAP
        last = len(sources) - 1
        on_device = output == "device"
        if render is not None and render.norm == "video":
            from . import render as render_mod

            with torch.cuda.device(dev):
                return render_mod.colorize(self.run_stitched(sources, n_keep, output="device"), render, output=output)
        shape, dtype = ((n_keep, fh, fw), torch.float32) if render is None else ((n_keep, fh, fw, 3), torch.uint8)
        if last < 0:
            return torch.empty((0,) + shape[1:], dtype=dtype, device=dev) if on_device else torch.empty((0,) + shape[1:], dtype=dtype).numpy()
        s_st = torch.cuda.Stream(device=dev)
        state: dict = {"done": 0}

        def begin(nbuf: int, entry: torch.cuda.Event) -> None:
            s_st.wait_event(entry)
            state["stitch"] = _DeviceStitch(lib, dev, fh, fw, min(2, len(sources)))
            # the device result comes from the caller's stream's pool and is first written on the stitch stream, which has waited for `entry`
            state["out"] = torch.empty(shape, dtype=dtype, device=dev) if on_device else torch.empty(shape, dtype=dtype, pin_memory=True)
            if render is not None:
                from .render import DeviceRenderer

                state["render"] = DeviceRenderer(render, dev, fh, fw, staging=not on_device)

        def after_forward(k: int, slot: int, stream: torch.cuda.Stream, disp: torch.Tensor) -> None:
            stitch, out = state["stitch"], state["out"]
            ready = torch.cuda.Event()
            ready.record(stream)
            with torch.cuda.stream(s_st):
                s_st.wait_event(ready)
                stitch.window(k, disp, s_st)
                upto = n_keep if k == last else min(n_keep, INFER_LEN + step * k - INTERP_LEN)
                for g, piece in stitch.final_pieces(upto):
                    if render is None:
                        out[g:g + piece.shape[0]].copy_(piece, non_blocking=True)
                    else:
                        state["render"].color_into(piece, out[g:g + piece.shape[0]])
                state["done"] = stitch.done

        self._run_windows(sources, begin, lambda k, slot: None, after_forward)
        s_st.synchronize()
        assert state["done"] == n_keep
        return state["out"] if on_device else state["out"].numpy()

    def resized_clip(self, source: np.ndarray) -> torch.Tensor:
        """The network input of one window, [1, 32, 3, th, tw] on the device (what ``run`` feeds the forward): for tests."""
        lib = _lib.load()
        with torch.cuda.device(self.dev), torch.no_grad():
            st = C.c_void_p(_lib.stream_ptr(self.dev))
            cur = torch.from_numpy(np.take(self.frames, source, axis=0)).to(self.dev).permute(0, 3, 1, 2).to(torch.float32).div_(255.0)
            if (self.th, self.tw) != (self.fh, self.fw):
                small = torch.empty((INFER_LEN, 3, self.th, self.tw), device=self.dev, dtype=torch.float32)
                _lib.check(lib.edv_resize_bicubic(cur.data_ptr(), small.data_ptr(), INFER_LEN * 3, self.fh, self.fw, self.th, self.tw, st), "edv_resize_bicubic")
                cur = small
            return cur.unsqueeze(0)


# ---------------------------------------------------------------------------------------------
def infer_video_depth(model, frames, input_size=518, device="cuda", runner=None, shard_windows=False, rank=None, world=None, stitch="host", output="host",
                      render=None):
    """endodav.infer_video_depth (endodav.py:162-254).  By default every window of the video runs on the calling rank, whatever process group
    exists: that is what ``evaluate.evaluate_video`` needs, where each rank already holds a DIFFERENT clip (sharding the windows of those clips
    over the same ranks would pair up collectives of different clips -- ADVICE round 2).

    ``shard_windows=True`` (opt-in, for ONE long video that every rank calls this function with): the windows are dealt round-robin over the
    ranks (they depend on each other through input key frames only, ``window_sources``), every rank runs its share on its own GPU, rank 0
    gathers the per-window maps, stitches them in window order and returns the result; the other ranks return None.  ``rank`` / ``world``
    default to the process group's.  No data-path collective besides that gather.

    ``stitch``: ``"host"`` (default) aligns and cross-fades the windows in numpy float32 exactly as the reference does (``stitch_windows``);
    ``"device"`` (opt-in) does both on the GPU, window by window behind the forwards, and copies every frame to the host once
    (``HipWindowRunner.run_stitched``).  The device path sums in fp64, so it is closer to exact arithmetic than the reference's float32 solve;
    the two agree to about 1e-6 of the output's scale on well-conditioned clips and are not bit-identical.  Its result lies in pinned host
    memory.  It does not combine with ``shard_windows=True``, which stitches on the host of rank 0.

    ``output``: ``"host"`` (default) returns a numpy array; ``"device"`` (needs ``stitch="device"``, so it does not combine with
    ``shard_windows=True`` either) returns the stitched video as a float32 ``torch.Tensor`` [n, fh, fw] on the GPU -- the same kernels and the
    same bits, the final frames copied device-to-device instead of to the host (what ``evaluate.evaluate_video(metrics="device")`` consumes).
    All work is drained before the call returns, as for the host result: the tensor can be used on any stream at once.

    ``render``: None (default) or a ``render.Render`` (needs ``stitch="device"``, does not combine with ``shard_windows=True``): the result is
    the colour-mapped video, uint8 [n, fh, fw, 3], in pinned host memory or (``output="device"``) on the GPU, coloured on the stitch stream
    (``HipWindowRunner.run_stitched``); it equals ``render.colorize`` of the fp32 result byte for byte.

    ``runner``: anything with ``run(sources) -> [np.ndarray [32, H, W]]`` (default ``HipWindowRunner``; the gloo tests pass a stub);
    ``stitch="device"`` needs its ``run_stitched(sources, n) -> np.ndarray [n, H, W]`` as well, ``output="device"`` that it takes
    ``output="device"``, and ``render`` that it takes ``render=``."""
    from . import parallel

    if stitch not in ("host", "device"):
        raise ValueError(f"stitch must be 'host' or 'device', got {stitch!r}")
    if output not in ("host", "device"):
        raise ValueError(f"output must be 'host' or 'device', got {output!r}")
    if output == "device" and (stitch != "device" or shard_windows):
        raise ValueError("output='device' needs stitch='device' and does not combine with shard_windows=True: only the device stitch leaves the video on the GPU")
    if stitch == "device" and shard_windows:
        raise ValueError("stitch='device' does not combine with shard_windows=True: sharded windows are gathered and stitched on the host of rank 0")
    if render is not None:
        from .render import Render

        if not isinstance(render, Render):
            raise ValueError(f"render must be None or a render.Render, got {type(render).__name__}")
        if stitch != "device" or shard_windows:
            raise ValueError("render needs stitch='device' and does not combine with shard_windows=True: the frames are coloured where the device stitch finishes them")
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError(f"expected frames [N, H, W, 3], got {frames.shape}")
    n = frames.shape[0]
    if runner is None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("infer_video_depth runs on MI355X only (device must be a CUDA/ROCm device)")
        runner = HipWindowRunner(model, np.ascontiguousarray(frames), dev)
    sources = window_sources(n)
    if stitch == "device":
        kw = {} if render is None else {"render": render}  # a keyword reaches the runner only when it is not the default
        return runner.run_stitched(sources, n, output="device", **kw) if output == "device" else runner.run_stitched(sources, n, **kw)
    if not shard_windows:
        return stitch_windows(runner.run(sources), n)
    if rank is None or world is None:
        rank, world = parallel.rank_world()
    mine = parallel.clip_shard(len(sources), rank, world)
    windows = runner.run([sources[k] for k in mine])
    shards = parallel.gather_to_rank0(windows)
    if shards is None:
        return None
    return stitch_windows(parallel.merge_shards(shards, len(sources)), n)


# ---------------------------------------------------------------------------------------------
# streaming: frames are pushed as they arrive, depth comes back as soon as it is final
# ---------------------------------------------------------------------------------------------
STREAM_RING = 64  # frames the device ring holds; tests/test_stream_cpu.py derives the bound it must meet from window_sources


def stream_trigger(k: int) -> int:
    """Frames that must have arrived before window k can run: its last input frame is 22 k + 31.  For every n >= stream_trigger(k),
    ``window_sources(n)[k]`` is the same (no padding reaches the window), so the window run then reproduces the offline one."""
    return (INFER_LEN - OVERLAP) * k + INFER_LEN


def stream_final(k: int) -> int:
    """Output frames that are final once window k is stitched and is not the last one: all 32 + 22 k but the 8 the next window fades."""
    return INFER_LEN + (INFER_LEN - OVERLAP) * k - INTERP_LEN


def stream_next_source(k: int, prev: Optional[np.ndarray]) -> np.ndarray:
    """``window_sources(n)[k]`` for any n >= stream_trigger(k), from window k-1's: one link of the key-frame chain."""
    idx = np.arange((INFER_LEN - OVERLAP) * k, (INFER_LEN - OVERLAP) * k + INFER_LEN)
    if k > 0:
        idx[:OVERLAP] = prev[KEYFRAMES]
    return idx


class DepthStream:
    """``model.stream_video_depth(...)``: whole-video inference, incrementally.  ``push`` takes the frames as they arrive and returns the depth
    of the frames that became final, ``close`` the rest; for any chunking the concatenation of all they return equals
    ``model.infer_video_depth(all_frames, stitch="device")`` bit for bit -- the same kernels in the same order.

    Schedule (host arithmetic only: ``stream_trigger``, ``stream_final``): window k runs at the first push that brings the count to
    22 k + 32; once it is stitched, frames < 24 + 22 k are final.  A chunk that crosses a trigger is taken in pieces, so the ring never holds
    a frame newer than the trigger of the window about to run.  ``close`` runs the windows that are left (at least one), with the sources of
    ``window_sources(n)`` -- the padding with the last frame --, and emits up to n.

    Ring: the raw uint8 frames live once in a device ring [STREAM_RING, fh, fw, 3], frame j in slot j % STREAM_RING, uploaded through pinned
    staging buffers on the copy-in stream.  A window's input is read from its 32 slots on the lane's stream (one edv_ingest_u8 when the frames
    have the network's size; a gather and the runner's conversion and pre-resize otherwise); key frames are not uploaded a second time.  Window k reads back to frame 22 k - 16 (slot 0: two hops of the key-frame chain), 48 frames in all.

    Stream contract: every push orders itself after what the caller has enqueued on its current stream so far (an event recorded there, for
    which the copy-in stream, the lanes it uses and the stitch stream wait), as ``HipWindowRunner._run_windows`` does once per run.  A lane
    waits for the upload of its window's last frame.  Hazard: frame j overwrites frame j - 64, so uploads of frames >= 22 k + 48 race window
    k's read of the ring: an event is recorded after every window's read, and the copy-in stream waits for it before it uploads any frame after that
    window's trigger.  The stitch stream takes the windows in window order, whichever lanes they ran on.  Lanes are the model's cached
    ``_video_flight`` (shared with ``infer_video_depth``); a lora_type="dash" model runs one window at a time on lane 0.  Stitch state, ring
    and counters belong to this object: two streams of one model may be pushed alternately.

    ``push(chunk, wait=True)`` returns every frame the windows enqueued so far make final and blocks until they are there; ``wait=False``
    never blocks and returns the finished prefix only.  ``output="host"``: numpy arrays the caller owns; ``"device"``: float32 tensors on the
    GPU, complete when returned.  Device memory does not grow with the length of the stream.

    ``render`` (a ``render.Render`` with norm "frame", "fixed" or "quantile"; "video" needs the whole video and raises): ``push`` and ``close``
    return the colour-mapped frames, uint8 [r, fh, fw, 3], coloured on the stitch stream where the fp32 frames would have been copied; the
    concatenation equals ``infer_video_depth(..., stitch="device", render=render)``.  The table, the range workspace and the staging buffer are
    allocated once with the ring.  Side by side with the input frames is ``render.colorize(frames=...)`` only: the ring may have dropped a
    frame by the time its depth is final.

    ``backend``: the object that touches the GPU (default ``_HipStreamBackend``); tests pass a stub with ``begin_push()``,
    ``upload(first, frames)``, ``window(k, source, upto)``, ``collect(wait) -> [r, fh, fw]`` and ``release()``."""

    def __init__(self, model, frame_shape: Tuple[int, int], device="cuda", output: str = "host", backend=None, render=None):
        if output not in ("host", "device"):
            raise ValueError(f"output must be 'host' or 'device', got {output!r}")
        if render is not None:
            from .render import Render

            if not isinstance(render, Render):
                raise ValueError(f"render must be None or a render.Render, got {type(render).__name__}")
            if render.norm == "video":
                raise ValueError("render.norm='video' needs the range of the whole video, which a stream never sees: use 'frame', 'fixed' or 'quantile'")
        self.render = render
        fh, fw = (int(v) for v in frame_shape)
        if fh <= 0 or fw <= 0:
            raise ValueError(f"frame_shape must be (height, width) > 0, got {frame_shape!r}")
        self.fh, self.fw, self.output = fh, fw, output
        if backend is None:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise RuntimeError("stream_video_depth runs on MI355X only (device must be a CUDA/ROCm device)")
            backend = _HipStreamBackend(model, fh, fw, dev, output, render)
        self._backend = backend
        self.pushed = 0          # frames taken
        self.emitted = 0         # frames returned
        self.windows = 0         # windows enqueued
        self.closed = False
        self._source: Optional[np.ndarray] = None

    def _window(self, source: np.ndarray, upto: int) -> None:
        self._backend.window(self.windows, source, upto)
        self._source = source
        self.windows += 1

    def _collect(self, wait: bool):
        got = self._backend.collect(wait)
        self.emitted += int(got.shape[0])
        return got

    def push(self, chunk, wait: bool = True):
        if self.closed:
            raise RuntimeError("push after close: the stream has emitted its last frames")
        chunk = np.asarray(chunk)
        if chunk.dtype != np.uint8:
            raise ValueError(f"expected uint8 frames, got {chunk.dtype}")
        if chunk.ndim == 3:
            chunk = chunk[None]
        if chunk.ndim != 4 or chunk.shape[0] < 1 or chunk.shape[1:] != (self.fh, self.fw, 3):
            raise ValueError(f"expected frames [m >= 1, {self.fh}, {self.fw}, 3] or one frame [{self.fh}, {self.fw}, 3], got {chunk.shape}")
        self._backend.begin_push()
        pos, m = 0, chunk.shape[0]
        while pos < m:
            trigger = stream_trigger(self.windows)       # pushed < trigger here: the window would have run
            take = min(m - pos, trigger - self.pushed)
            self._backend.upload(self.pushed, chunk[pos:pos + take])
            self.pushed += take
            pos += take
            if self.pushed == trigger:
                self._window(stream_next_source(self.windows, self._source), stream_final(self.windows))
        return self._collect(wait)

    def close(self):
        """The frames not returned yet (``wait`` or not); afterwards ``pushed == emitted``.  A second close returns an empty array."""
        if not self.closed and self.pushed:
            n = self.pushed
            sources = window_sources(n)
            assert self.windows < len(sources)           # 22 k + 32 <= n implies 22 (k + 1) < n: an eager window is never the last
            self._backend.begin_push()
            for k in range(self.windows, len(sources)):
                self._window(sources[k], n if k == len(sources) - 1 else min(n, stream_final(k)))
        self.closed = True
        got = self._collect(True)
        self._backend.release()
        return got


class _HipStreamBackend:
    """What ``DepthStream`` does on the GPU (its docstring states the stream contract).  Allocated once: the ring, two pinned staging buffers
    of 32 frames (a piece between two triggers is at most that long), the stitch state."""

    def __init__(self, model, fh: int, fw: int, dev: torch.device, output: str, render=None):
        self.model, self.fh, self.fw, self.dev, self.on_device = model, fh, fw, dev, output == "device"
        self.shape, self.dtype = ((fh, fw), torch.float32) if render is None else ((fh, fw, 3), torch.uint8)
        ih, iw = model.image_shape
        self.tw, self.th = lower_bound_size(fw, fh, iw, ih)
        self.lib = _lib.load()
        with torch.cuda.device(dev):
            self.s_in = torch.cuda.Stream(device=dev)
            self.s_st = torch.cuda.Stream(device=dev)
            # from the pool of the caller's stream, first written on the streams of this object, which wait for the first push's entry event
            self.ring = torch.empty((STREAM_RING, fh, fw, 3), dtype=torch.uint8, device=dev)
            self.stitch = _DeviceStitch(self.lib, dev, fh, fw)
            self.render = None
            if render is not None:
                from .render import DeviceRenderer

                self.render = DeviceRenderer(render, dev, fh, fw, staging=not self.on_device)
        self.h_in = [torch.empty((INFER_LEN, fh, fw, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.up_done: List[Optional[torch.cuda.Event]] = [None, None]  # H2D out of the staging buffer finished
        self.n_up = 0
        self.uploaded: Optional[torch.cuda.Event] = None               # the newest frame is in the ring
        self.ingested: List[torch.cuda.Event] = []                     # ingests the next upload must wait for
        self.entry: Optional[torch.cuda.Event] = None
        self.blocks: List[Tuple[torch.Tensor, torch.cuda.Event]] = []  # final frames on their way, in order

    def begin_push(self) -> None:
        self.entry = torch.cuda.Event()
        self.entry.record(torch.cuda.current_stream(self.dev))
        self.s_in.wait_event(self.entry)
        self.s_st.wait_event(self.entry)

    def upload(self, first: int, frames: np.ndarray) -> None:
        m = frames.shape[0]
        b = self.n_up % 2
        self.n_up += 1
        if self.up_done[b] is not None:
            self.up_done[b].synchronize()                # the staging buffer is about to be rewritten
        stage = self.h_in[b][:m]
        np.copyto(stage.numpy(), frames)
        with torch.cuda.device(self.dev), torch.cuda.stream(self.s_in):
            for ev in self.ingested:                     # the windows whose ring slots these frames may overwrite have read them
                self.s_in.wait_event(ev)
            self.ingested = []
            slot = first % STREAM_RING
            head = min(m, STREAM_RING - slot)
            self.ring[slot:slot + head].copy_(stage[:head], non_blocking=True)
            if head < m:                                 # the piece wraps round the ring
                self.ring[:m - head].copy_(stage[head:], non_blocking=True)
            self.up_done[b] = self.uploaded = torch.cuda.Event()
            self.uploaded.record(self.s_in)

    def window(self, k: int, source: np.ndarray, upto: int) -> None:
        lib, dev, fh, fw = self.lib, self.dev, self.fh, self.fw
        with torch.cuda.device(dev), torch.no_grad():
            dash, _, flight = _video_lanes(self.model, dev)
            if dash:
                # lane 0's engine context is single-user: every stream of this model queues its windows on one HIP stream kept with the model
                stream = getattr(self.model, "_video_dash_stream", None)
                if stream is None or stream.device != dev:
                    stream = self.model._video_dash_stream = torch.cuda.Stream(device=dev)
                lane = 0
            else:
                stream, lane = flight.next_lane(INFER_LEN)
            stream.wait_event(self.entry)                # the first forward on a lane folds and packs the weights on the lane's stream
            stream.wait_event(self.uploaded)
            slots = [int(j) % STREAM_RING for j in source]
            with torch.cuda.stream(stream):
                st = C.c_void_p(stream.cuda_stream)
                if (self.th, self.tw) == (fh, fw):
                    # one kernel over the 32 ring slots, bit-identical to the runner's conversion (tests/test_ingest_gpu.py: all 256 bytes)
                    cur = torch.empty((INFER_LEN, 3, fh, fw), device=dev, dtype=torch.float32)
                    _lib.check(lib.edv_ingest_u8(self.ring.data_ptr(), STREAM_RING, (C.c_int32 * INFER_LEN)(*slots), INFER_LEN, cur.data_ptr(), fh, fw, fh, fw, st),
                               "edv_ingest_u8")
                else:
                    # frames that need the pre-resize take the runner's own two steps on a per-window gather of the ring, so that the stream
                    # equals infer_video_depth bit for bit at every size (DESIGN.md "Streaming": why the fused resize is not used here yet)
                    clip = torch.empty((INFER_LEN, fh, fw, 3), dtype=torch.uint8, device=dev)
                    i = 0
                    while i < INFER_LEN:                 # runs of consecutive slots: the 10 key frames one by one, then 22 frames in one or two copies
                        r = 1
                        while i + r < INFER_LEN and slots[i + r] == slots[i] + r:
                            r += 1
                        clip[i:i + r].copy_(self.ring[slots[i]:slots[i] + r], non_blocking=True)
                        i += r
                    cur = _pre_resize(lib, clip.permute(0, 3, 1, 2).to(torch.float32).div_(255.0), fh, fw, self.th, self.tw, st)
                done = torch.cuda.Event()
                done.record(stream)
                self.ingested.append(done)
                disp = self.model(cur.unsqueeze(0), lane=lane)[("disp", 0)]  # [32, 1, ih, iw]
                ready = torch.cuda.Event()
                ready.record(stream)
            count = upto - self.stitch.done
            # a device block comes from the caller's stream's pool (as run_stitched's result does) and is first written on the stitch stream
            block = torch.empty((count,) + self.shape, dtype=self.dtype, device=dev) if self.on_device else torch.empty((count,) + self.shape, dtype=self.dtype, pin_memory=True)
            with torch.cuda.stream(self.s_st):
                self.s_st.wait_event(ready)
                g0 = self.stitch.done
                self.stitch.window(k, disp, self.s_st)
                for g, piece in self.stitch.final_pieces(upto):
                    if self.render is None:
                        block[g - g0:g - g0 + piece.shape[0]].copy_(piece, non_blocking=True)
                    else:
                        self.render.color_into(piece, block[g - g0:g - g0 + piece.shape[0]])
                copied = torch.cuda.Event()
                copied.record(self.s_st)
            self.blocks.append((block, copied))

    def collect(self, wait: bool):
        got = []
        while self.blocks:
            block, copied = self.blocks[0]
            if wait:
                copied.synchronize()
            elif not copied.query():
                break
            got.append(block)
            self.blocks.pop(0)
        if self.on_device:
            with torch.cuda.device(self.dev):
                if not got:
                    return torch.empty((0,) + self.shape, dtype=self.dtype, device=self.dev)
                if len(got) == 1:
                    return got[0]
                out = torch.cat(got)                     # on the caller's stream, from complete blocks
                torch.cuda.current_stream(self.dev).synchronize()
                return out
        if not got:
            return torch.empty((0,) + self.shape, dtype=self.dtype).numpy()
        return np.concatenate([b.numpy() for b in got])  # a copy out of the pinned blocks: the caller owns it

    def release(self) -> None:
        """After the last collect: nothing is in flight; drop the device buffers."""
        self.ring = self.stitch = self.render = None
        self.h_in = []
