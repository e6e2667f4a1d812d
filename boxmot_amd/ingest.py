"""Pinned-host frame ingest ring ("real frame ingest").

The reference hands every tracker a numpy frame per call (basetracker.py:120-147) and its native binding copies it again
(native/trackers/botsort.py:200-230).  On a PCIe-attached GPU the per-frame upload (6.2 MB at 1080p) from pageable memory is
the larger part of a host-API step, so the ring gives the decoder page-locked buffers to write into and moves them with
asynchronous DMAs on a copy stream of their own:

    ring = FrameRing(n_slots=3, n_streams=S, rows=1080, cols=1920)
    ring.host_view(0)[s] = first frame of stream s ; ring.submit(0)
    for t in range(T):
        k, k1 = t % 3, (t + 1) % 3
        ring.host_view(k1)[...] = frames of t + 1            # decode straight into pinned memory (host_done(k1) first if reused)
        ring.submit(k1)                                      # its upload overlaps the kernels of frame t
        rows = tracker.update_batch(dets[t], ring=ring, slot=k)   # MultiStreamBotSort: waits for slot k on the device, no host wait

Decoders hand out NV12 (a full-resolution Y plane followed by a half-resolution plane of interleaved U, V pairs: 1.5 bytes per
pixel), not packed BGR.  ``FrameRing(..., fmt="nv12")`` takes those bytes as they are -- half the PCIe traffic, no conversion on the
host -- and converts them into the same BGR device frames with one kernel behind the DMA on the copy stream; everything downstream
(``update_batch(ring=...)``, ``wait`` / ``release``, per-stream sizes) is unchanged:

    ring = FrameRing(3, S, rows=1080, cols=1920, fmt="nv12")
    ring.host_view(k, s)[...] = nv12 frame, (rows * 3 // 2, cols) uint8 ; ring.submit(k)
    ring.submit_device_nv12(k, y_ptrs, uv_ptrs, pitch_y, pitch_uv)      # surfaces a hardware decoder left in HBM (any ring)

Everything is a thin ctypes wrapper over boxmot_hip_ingest_* (include/boxmot_hip.h).
"""
from __future__ import annotations

import ctypes
import sys

import numpy as np

from boxmot_amd import _lib


class FrameRing:
    def __init__(self, n_slots: int, n_streams: int, rows: int | None = None, cols: int | None = None, sizes=None, fmt: str = "bgr"):
        """``rows, cols``: one frame size for every stream; or ``sizes``: a ``(rows, cols)`` per stream (cameras of different
        resolutions in one ring).  ``fmt``: what the host slots hold -- ``"bgr"`` (rows, cols, 3) frames, or ``"nv12"``
        (rows * 3 // 2, cols) frames that ``submit`` converts to BGR on the device; sizes are image sizes either way."""
        self.n_slots, self.n_streams = int(n_slots), int(n_streams)
        if fmt not in ("bgr", "nv12"):
            raise ValueError(f"FrameRing: unknown fmt {fmt!r} (\"bgr\" or \"nv12\")")
        self.fmt = fmt
        if sizes is not None:
            if rows is not None or cols is not None:
                raise ValueError("FrameRing takes rows / cols or sizes, not both")
            sizes = [tuple(int(v) for v in sz) for sz in sizes]
            if len(sizes) != self.n_streams:
                raise ValueError(f"FrameRing: sizes has {len(sizes)} entries for {self.n_streams} streams")
            for s, sz in enumerate(sizes):
                if len(sz) != 2 or sz[0] < 1 or sz[1] < 1:
                    raise ValueError(f"stream {s}: size must be a positive (rows, cols), got {sz}")
        else:
            if rows is None or cols is None:
                raise ValueError("FrameRing needs rows and cols, or sizes")
            sizes = [(int(rows), int(cols))] * self.n_streams
        if fmt == "nv12":
            for s, sz in enumerate(sizes):
                if sz[0] % 2 or sz[1] % 2:
                    raise ValueError(f"stream {s}: NV12 frames have even rows and cols, got {sz}")
        self.sizes = sizes
        self.mixed = len(set(sizes)) > 1
        self.rows, self.cols = sizes[0]             # (of stream 0; the size of every stream on a uniform ring)
        self._lib = _lib.load()
        if fmt == "nv12":
            r = np.array([sz[0] for sz in sizes], dtype=np.int32)
            c = np.array([sz[1] for sz in sizes], dtype=np.int32)
            self._handle = self._lib.boxmot_hip_ingest_create_nv12(self.n_slots, self.n_streams, r.ctypes.data, c.ctypes.data)
        elif self.mixed:
            r = np.array([sz[0] for sz in sizes], dtype=np.int32)
            c = np.array([sz[1] for sz in sizes], dtype=np.int32)
            self._handle = self._lib.boxmot_hip_ingest_create_sized(self.n_slots, self.n_streams, r.ctypes.data, c.ctypes.data)
        else:
            self._handle = self._lib.boxmot_hip_ingest_create(self.n_slots, self.n_streams, self.rows, self.cols)
        if not self._handle:
            raise RuntimeError(_lib.last_error())
        self._views = {}
        self._roots = {}

    def host_view(self, slot: int, stream: int | None = None) -> np.ndarray:
        """``host_view(slot)``: (n_streams, rows, cols, 3) uint8 view of the slot's page-locked host memory (uniform rings);
        ``host_view(slot, stream)``: that stream's (rows, cols, 3) frame (any ring).  On an NV12 ring a frame is
        (rows * 3 // 2, cols): the Y plane, then the rows // 2 lines of interleaved U, V pairs."""
        if self.fmt == "nv12":
            return self._host_view_nv12(slot, stream)
        if stream is not None:
            stream = int(stream)
            if not 0 <= stream < self.n_streams:
                raise ValueError(f"stream {stream} out of range")
            if not self.mixed:
                return self.host_view(slot)[stream]
            key = (slot, stream)
        else:
            if self.mixed:
                raise ValueError("host_view(slot) needs one frame size; this ring's streams differ: use host_view(slot, stream)")
            key = slot
        if key not in self._views:
            p = self._lib.boxmot_hip_ingest_host_ptr(self._handle, int(slot), stream or 0)
            if not p:
                raise RuntimeError(_lib.last_error())
            r, c = self.sizes[stream or 0]
            n = (1 if self.mixed else self.n_streams) * r * c * 3
            buf = (ctypes.c_uint8 * n).from_address(p)
            root = np.frombuffer(buf, dtype=np.uint8)        # numpy collapses view chains onto this array: every slice a caller
            self._roots[key] = root                          # keeps holds a reference to IT (close() counts them)
            self._views[key] = root.reshape((r, c, 3) if self.mixed else (self.n_streams, r, c, 3))
        return self._views[key]

    def _host_view_nv12(self, slot, stream):
        if stream is not None:
            stream = int(stream)
            if not 0 <= stream < self.n_streams:
                raise ValueError(f"stream {stream} out of range")
            if not self.mixed:
                return self.host_view(slot)[stream]
            key = (slot, stream)
        else:
            if self.mixed:
                raise ValueError("host_view(slot) needs one frame size; this ring's streams differ: use host_view(slot, stream)")
            key = slot
        if key not in self._views:
            p = self._lib.boxmot_hip_ingest_host_ptr(self._handle, int(slot), stream or 0)
            if not p:
                raise RuntimeError(_lib.last_error())
            r, c = self.sizes[stream or 0]
            n = r * c * 3 // 2
            pitch = (n + 255) // 256 * 256           # the frames of a slot lie at 256-byte aligned offsets
            total = n if self.mixed else pitch * (self.n_streams - 1) + n
            root = np.frombuffer((ctypes.c_uint8 * total).from_address(p), dtype=np.uint8)
            self._roots[key] = root
            if self.mixed:
                self._views[key] = root.reshape(r * 3 // 2, c)
            else:
                self._views[key] = np.ndarray((self.n_streams, r * 3 // 2, c), np.uint8, buffer=root, strides=(pitch, c, 1))
        return self._views[key]

    def submit(self, slot: int, n_streams: int | None = None) -> None:
        _lib.check(self._lib.boxmot_hip_ingest_submit(self._handle, int(slot), int(n_streams or self.n_streams)))

    def submit_device_nv12(self, slot: int, y_ptrs, uv_ptrs, pitch_y, pitch_uv) -> None:
        """Convert NV12 surfaces that already are in device memory (one Y and one UV device address and their byte pitches per
        stream, ``pitch >= cols``) into the slot's BGR frames: no DMA, same ``wait`` / ``release`` protocol as ``submit``.  Works
        on any ring whose sizes are even.  The surfaces must be complete when the call is made (synchronise with whatever
        produced them first) and stay untouched until the slot's consumer has waited for it."""
        lists = {"y_ptrs": y_ptrs, "uv_ptrs": uv_ptrs, "pitch_y": pitch_y, "pitch_uv": pitch_uv}
        for name, v in lists.items():
            if len(v) != self.n_streams:
                raise ValueError(f"submit_device_nv12: {name} has {len(v)} entries for {self.n_streams} streams")
        for s, (r, c) in enumerate(self.sizes):
            if r % 2 or c % 2:
                raise ValueError(f"stream {s}: NV12 frames have even rows and cols, this stream is {(r, c)}")
            if int(pitch_y[s]) < c or int(pitch_uv[s]) < c:
                raise ValueError(f"stream {s}: pitch ({int(pitch_y[s])}, {int(pitch_uv[s])}) below the {c} columns of the frame")
            if not int(y_ptrs[s]) or not int(uv_ptrs[s]):
                raise ValueError(f"stream {s}: null NV12 plane")
        n = self.n_streams
        yp = (ctypes.c_void_p * n)(*[int(v) for v in y_ptrs])
        up = (ctypes.c_void_p * n)(*[int(v) for v in uv_ptrs])
        py = np.array([int(v) for v in pitch_y], dtype=np.int32)
        pu = np.array([int(v) for v in pitch_uv], dtype=np.int32)
        _lib.check(self._lib.boxmot_hip_ingest_submit_device_nv12(self._handle, int(slot), n, ctypes.addressof(yp), ctypes.addressof(up),
                                                                  py.ctypes.data, pu.ctypes.data))

    def download(self, slot: int, stream: int) -> np.ndarray:
        """(rows, cols, 3) copy of the slot's BGR device frame of ``stream`` once its upload is done (test / utility: it blocks)."""
        stream = int(stream)
        if not 0 <= stream < self.n_streams:
            raise ValueError(f"stream {stream} out of range")
        r, c = self.sizes[stream]
        out = np.empty((r, c, 3), dtype=np.uint8)
        _lib.check(self._lib.boxmot_hip_ingest_download(self._handle, int(slot), stream, out.ctypes.data))
        return out

    def wait(self, slot: int, consumer_stream: int) -> None:
        _lib.check(self._lib.boxmot_hip_ingest_wait(self._handle, int(slot), ctypes.c_void_p(consumer_stream)))

    def release(self, slot: int, consumer_stream: int) -> None:
        _lib.check(self._lib.boxmot_hip_ingest_release(self._handle, int(slot), ctypes.c_void_p(consumer_stream)))

    def host_done(self, slot: int) -> None:
        _lib.check(self._lib.boxmot_hip_ingest_host_done(self._handle, int(slot)))

    def device_frames(self, slot: int) -> int:
        """Device address of the slot's table of per-stream frame pointers (the ``d_frames`` of ``step_device``)."""
        p = self._lib.boxmot_hip_ingest_device_frames(self._handle, int(slot))
        if not p:
            raise RuntimeError(_lib.last_error())
        return int(p)

    def close(self, force: bool = False) -> None:
        """Free the ring.  The arrays ``host_view`` handed out alias the page-locked memory this frees: while the caller still
        holds one (or a slice of one) ``close`` refuses, unless ``force`` (interpreter shutdown / ``__del__``)."""
        h = getattr(self, "_handle", None)
        if h:
            if not force:
                # a slot's root array is referenced by: _roots, the cached 4-D view's base, getrefcount's argument; and the 4-D
                # view by: _views, getrefcount's argument
                held = [s for s in self._views if sys.getrefcount(self._roots[s]) > 3 or sys.getrefcount(self._views[s]) > 2]
                if held:
                    raise RuntimeError(f"FrameRing.close(): host views of slot(s) {held} are still referenced; drop them first")
            self._views.clear()
            self._roots.clear()
            self._lib.boxmot_hip_ingest_destroy(h)
            self._handle = None

    def __del__(self):
        try:
            self.close(force=True)
        except Exception:
            pass


def nv12_to_bgr(frame_nv12, rows: int, cols: int) -> np.ndarray:
    """The device conversion of one host NV12 frame ((rows * 3 // 2, cols) uint8, or those bytes flat) -> (rows, cols, 3) BGR:
    ``cv2.cvtColor(frame, cv2.COLOR_YUV2BGR_NV12)``'s definition (BT.601 limited range, 20-bit fixed point) as the ring's kernel
    computes it.  Makes a private 2-slot ring, submits and copies back: a utility, not a hot path."""
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1 or rows % 2 or cols % 2:
        raise ValueError(f"stream 0: NV12 frames have positive even rows and cols, got {(rows, cols)}")
    f = np.ascontiguousarray(frame_nv12, dtype=np.uint8)
    if f.size != rows * cols * 3 // 2:
        raise ValueError(f"an NV12 frame of {rows} x {cols} has {rows * cols * 3 // 2} bytes, got {f.size}")
    ring = FrameRing(2, 1, rows, cols, fmt="nv12")
    try:
        ring.host_view(0, 0)[...] = f.reshape(rows * 3 // 2, cols)
        ring.submit(0)
        return ring.download(0, 0)
    finally:
        ring.close()
