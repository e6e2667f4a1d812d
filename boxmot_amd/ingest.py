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

The consumer that runs before the tracker is the caller's detector.  ``letterbox`` writes its input -- letterboxed, planar,
normalised fp16 / fp32, the form every YOLO-family detector takes -- for all streams of a slot with one kernel on the detector's
stream, straight from the slot's device frames (no second host copy, no second upload); ``LetterboxGeometry.to_frame`` maps the
detector's boxes back to frame coordinates:

    x = torch.empty((S, 3, 640, 640), dtype=torch.float16, device="cuda")
    geo = ring.letterbox(k, x, hip_stream=torch.cuda.current_stream().cuda_stream)
    dets = [g.to_frame(d) for g, d in zip(geo, my_detector(x))]       # the caller's detector and NMS
    rows = tracker.update_batch(dets, ring=ring, slot=k)

Large frames (a 4K frame shrinks six times on its way into 640 x 640): ``letterbox_tiles`` letterboxes ``T`` rectangles of every frame
-- ``tile_grid`` makes an overlapping grid, optionally with the whole frame as tile 0 -- as one batch of ``S * T`` tensors, and
``DetPost(tiles=T)`` merges the per-tile detections with one NMS per stream in frame coordinates:

    tiles = tile_grid(2160, 3840, grid=(2, 3), overlap=0.2)            # T = 7
    x = torch.empty((S * 7, 3, 640, 640), dtype=torch.float16, device="cuda")
    geo = ring.letterbox_tiles(k, x, tiles, hip_stream=st)             # per stream a list of TileGeometry

Everything is a thin ctypes wrapper over boxmot_hip_ingest_* (include/boxmot_hip.h).
"""
from __future__ import annotations

import ctypes
import math
import sys
from typing import NamedTuple

import numpy as np

from boxmot_amd import _lib

LETTERBOX_MODES = {"center": 0, "topleft": 1}


class LetterboxGeometry(NamedTuple):
    """Where a (rows, cols) frame lies inside an (H, W) letterboxed tensor: it is resized by ``gain`` to (new_h, new_w) and placed
    with its corner at (top, left).  ``rows, cols`` is the frame size itself (what ``to_frame`` clips to)."""
    gain: float
    new_w: int
    new_h: int
    top: int
    left: int
    rows: int = 0
    cols: int = 0

    def to_frame(self, boxes) -> np.ndarray:
        """Detector-space ``xyxy`` (columns 0..3 of an (N, >= 4) table) -> frame coordinates: ``((x - left) / gain, (y - top) /
        gain)`` clipped to ``[0, cols]`` and ``[0, rows]``, in float32.  Other columns are untouched; the input is not modified."""
        b = np.array(boxes, dtype=np.float32, ndmin=2)
        if b.shape[-1] < 4:
            raise ValueError(f"to_frame: boxes need at least the 4 xyxy columns, got shape {b.shape}")
        gain = np.float32(self.gain)
        b[:, [0, 2]] = np.clip((b[:, [0, 2]] - np.float32(self.left)) / gain, np.float32(0), np.float32(self.cols))
        b[:, [1, 3]] = np.clip((b[:, [1, 3]] - np.float32(self.top)) / gain, np.float32(0), np.float32(self.rows))
        return b


def _letterbox_size(size):
    if isinstance(size, (int, np.integer)):
        size = (size, size)
    size = tuple(int(v) for v in size)
    if len(size) != 2 or size[0] < 1 or size[1] < 1:
        raise ValueError(f"letterbox: size must be a positive (H, W), got {size}")
    return size


def letterbox_geometry(rows: int, cols: int, size, mode: str = "center") -> LetterboxGeometry:
    """The geometry ``FrameRing.letterbox`` uses for a (rows, cols) frame and an output ``size`` (H, W) -- equal to
    ``boxmot_hip_letterbox_geometry``.  ``mode="center"``: Ultralytics ``LetterBox(auto=False, scaleup=True, center=True)`` (sizes
    rounded half-to-even, an odd padding puts the extra line at the bottom / right); ``mode="topleft"``: YOLOX ``preproc`` (sizes
    truncated, picture in the top left corner).  A picture that would vanish (new size < 1) raises ``ValueError``."""
    rows, cols = int(rows), int(cols)
    H, W = _letterbox_size(size)
    if mode not in LETTERBOX_MODES:
        raise ValueError(f"letterbox: unknown mode {mode!r} (\"center\" or \"topleft\")")
    if rows < 1 or cols < 1:
        raise ValueError(f"letterbox: frame dimensions must be positive, got {(rows, cols)}")
    gain = min(H / rows, W / cols)
    if mode == "center":
        new_w, new_h = round(cols * gain), round(rows * gain)
        top, left = round((H - new_h) / 2 - 0.1), round((W - new_w) / 2 - 0.1)
    else:
        new_w, new_h = int(cols * gain), int(rows * gain)
        top = left = 0
    if new_w < 1 or new_h < 1:
        raise ValueError(f"letterbox of a {rows} x {cols} frame into {H} x {W} leaves no picture ({new_h} x {new_w})")
    return LetterboxGeometry(gain, new_w, new_h, top, left, rows, cols)


MAX_TILES = 64


class TileGeometry(NamedTuple):
    """Where the rectangle ``(x0, y0, cols, rows)`` of a frame lies inside an (H, W) letterboxed tensor: the rectangle is resized by
    ``gain`` to (new_h, new_w) and placed with its corner at (top, left).  ``rows, cols`` is the RECTANGLE's size (its h, w)."""
    gain: float
    new_w: int
    new_h: int
    top: int
    left: int
    rows: int
    cols: int
    x0: int
    y0: int

    def to_frame(self, boxes) -> np.ndarray:
        """Detector-space ``xyxy`` of this tile (columns 0..3 of an (N, >= 4) table) -> FRAME coordinates:
        ``clip((x - left) / gain, 0, cols) + x0`` and ``clip((y - top) / gain, 0, rows) + y0``, in float32 -- the arithmetic of
        the tiled ``DetPost``.  Other columns are untouched; the input is not modified."""
        b = np.array(boxes, dtype=np.float32, ndmin=2)
        if b.shape[-1] < 4:
            raise ValueError(f"to_frame: boxes need at least the 4 xyxy columns, got shape {b.shape}")
        gain = np.float32(self.gain)
        b[:, [0, 2]] = np.clip((b[:, [0, 2]] - np.float32(self.left)) / gain, np.float32(0), np.float32(self.cols)) + np.float32(self.x0)
        b[:, [1, 3]] = np.clip((b[:, [1, 3]] - np.float32(self.top)) / gain, np.float32(0), np.float32(self.rows)) + np.float32(self.y0)
        return b


def _tile_axis(L: int, n: int, o: float):
    if n == 1:
        return L, [0]
    size = min(L, math.ceil(L / (n - (n - 1) * o)))
    return size, [(i * (L - size)) // (n - 1) for i in range(n)]


def tile_grid(rows: int, cols: int, grid=(2, 2), overlap: float = 0.2, full: bool = True) -> list:
    """The rectangles ``(x0, y0, w, h)`` of an ``ny x nx`` grid of equal, overlapping tiles over a (rows, cols) frame, row-major,
    preceded by the whole frame ``(0, 0, cols, rows)`` when ``full`` -- what ``FrameRing.letterbox_tiles`` takes.  Per axis of
    length L with n tiles: ``size = min(L, ceil(L / (n - (n - 1) * overlap)))``, ``origin_i = (i * (L - size)) // (n - 1)``: the
    first tile starts at 0, the last ends at L, neighbours share about ``overlap`` of a tile.  The count, ``ny * nx + full``, does
    not depend on the frame size, so streams of different sizes share a call."""
    rows, cols = int(rows), int(cols)
    if rows < 1 or cols < 1:
        raise ValueError(f"tile_grid: frame dimensions must be positive, got {(rows, cols)}")
    try:
        ny, nx = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError(f"tile_grid: grid must be (ny, nx), got {grid!r}") from None
    if ny < 1 or nx < 1 or ny > rows or nx > cols:
        raise ValueError(f"tile_grid: grid {(ny, nx)} must be at least (1, 1) and at most the frame size {(rows, cols)}")
    overlap = float(overlap)
    if not 0.0 <= overlap <= 0.9:
        raise ValueError(f"tile_grid: overlap must be within [0, 0.9], got {overlap}")
    if ny * nx + bool(full) > MAX_TILES:
        raise ValueError(f"tile_grid: {ny * nx + bool(full)} tiles, more than the {MAX_TILES} a call takes")
    h, ys = _tile_axis(rows, ny, overlap)
    w, xs = _tile_axis(cols, nx, overlap)
    tiles = [(0, 0, cols, rows)] if full else []
    return tiles + [(x, y, w, h) for y in ys for x in xs]


def _tile_rect(r, s, t, rows, cols):
    try:
        rect = tuple(int(v) for v in r)
        exact = len(rect) == 4 and all(float(a) == b for a, b in zip(r, rect))
    except (TypeError, ValueError):
        exact = False
    if not exact:
        raise ValueError(f"stream {s} tile {t}: a tile is four integers (x0, y0, w, h), got {r!r}")
    x0, y0, w, h = rect
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > cols or y0 + h > rows:
        raise ValueError(f"stream {s} tile {t}: rectangle (x0 {x0}, y0 {y0}, w {w}, h {h}) must have w, h >= 1 and lie inside the {rows} x {cols} frame")
    return rect


def tile_geometry(rows: int, cols: int, rect, size, mode: str = "center") -> TileGeometry:
    """The geometry ``FrameRing.letterbox_tiles`` uses for the rectangle ``rect = (x0, y0, w, h)`` of a (rows, cols) frame:
    ``letterbox_geometry(h, w, size, mode)`` and the rectangle's origin -- equal to ``boxmot_hip_letterbox_tile_geometry``."""
    x0, y0, w, h = _tile_rect(rect, 0, 0, int(rows), int(cols))
    g = letterbox_geometry(h, w, size, mode)
    return TileGeometry(g.gain, g.new_w, g.new_h, g.top, g.left, h, w, x0, y0)


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

    def letterbox(self, slot: int, out, size=None, mode: str = "center", rgb: bool = True, unit: bool = True, pad: int = 114,
                  n_streams: int | None = None, hip_stream: int = 0):
        """Write the letterboxed detector input of the slot's first ``n_streams`` streams (default: all) into ``out``: a contiguous
        float16 / float32 device tensor of shape (N, 3, H, W), N >= n_streams, on the ring's device -- anything with ``data_ptr()``,
        ``dtype``, ``shape`` and ``is_contiguous()``; rows beyond ``n_streams`` are left alone.  ``size`` (H, W) defaults to
        ``out.shape[-2:]``; W must be a multiple of 8.  ``mode`` as ``letterbox_geometry``; plane order RGB (``rgb=True``,
        Ultralytics) or BGR (YOLOX); values ``v / 255`` (``unit=True``) or ``v``; ``pad``: the byte outside the picture.
        The kernel runs on ``hip_stream`` after the slot's upload (no host wait), so work queued there afterwards -- the
        detector -- sees the tensor; the slot's next ``submit`` waits for it.  Returns the streams' ``LetterboxGeometry``."""
        n = self.n_streams if n_streams is None else int(n_streams)
        if not 1 <= n <= self.n_streams:
            raise ValueError(f"letterbox: n_streams {n} out of range for a ring of {self.n_streams} streams")
        if mode not in LETTERBOX_MODES:
            raise ValueError(f"letterbox: unknown mode {mode!r} (\"center\" or \"topleft\")")
        shape = tuple(int(v) for v in out.shape)
        H, W = _letterbox_size(shape[-2:] if size is None else size)
        if len(shape) != 4 or shape[0] < n or shape[1:] != (3, H, W):
            raise ValueError(f"letterbox: out must have shape (N >= {n}, 3, {H}, {W}), got {shape}")
        dtype = {"float32": 0, "float16": 1}.get(str(out.dtype).split(".")[-1])
        if dtype is None:
            raise ValueError(f"letterbox: out must be float16 or float32, got {out.dtype}")
        if not out.is_contiguous():
            raise ValueError("letterbox: out must be contiguous")
        if W % 8:
            raise ValueError(f"letterbox: the output width must be a multiple of 8, got {W}")
        pad = int(pad)
        if not 0 <= pad <= 255:
            raise ValueError(f"letterbox: pad must be within 0..255, got {pad}")
        ptr = int(out.data_ptr())
        if not ptr or ptr % 16:
            raise ValueError(f"letterbox: out must be a non-null 16-byte aligned device address, got {ptr:#x}")
        geo = []
        for s in range(n):
            try:
                geo.append(letterbox_geometry(*self.sizes[s], (H, W), mode))
            except ValueError as e:
                raise ValueError(f"stream {s}: {e}") from None
        cfg = _lib.Letterbox(H, W, LETTERBOX_MODES[mode], dtype, int(bool(rgb)), int(bool(unit)), pad)
        _lib.check(self._lib.boxmot_hip_ingest_letterbox(self._handle, int(slot), n, ctypes.byref(cfg), ctypes.c_void_p(ptr),
                                                         ctypes.c_void_p(int(hip_stream))))
        return geo

    def _stream_tiles(self, tiles, n):
        """per stream the checked rectangles of ``tiles``: one list for all streams, or one list per stream"""
        try:
            tiles = list(tiles)
            one = len(tiles) > 0 and not hasattr(tiles[0][0], "__len__")
        except (TypeError, IndexError):
            raise ValueError(f"letterbox_tiles: tiles must be a list of (x0, y0, w, h) or one such list per stream, got {tiles!r}") from None
        if one:
            tiles = [tiles] * n
        elif len(tiles) < n:
            raise ValueError(f"letterbox_tiles: tiles has {len(tiles)} lists for {n} streams")
        per = [list(t) for t in tiles[:n]]
        T = len(per[0])
        for s, t in enumerate(per):
            if len(t) != T:
                raise ValueError(f"stream {s}: {len(t)} tiles where stream 0 has {T}: every stream of a call has the same number")
        if not 1 <= T <= MAX_TILES:
            raise ValueError(f"letterbox_tiles: the number of tiles per stream must be within 1..{MAX_TILES}, got {T}")
        return [[_tile_rect(r, s, t, *self.sizes[s]) for t, r in enumerate(rs)] for s, rs in enumerate(per)]

    def letterbox_tiles(self, slot: int, out, tiles, size=None, mode: str = "center", rgb: bool = True, unit: bool = True, pad: int = 114,
                        n_streams: int | None = None, hip_stream: int = 0):
        """Sliced inference on large frames: write the letterboxed detector input of ``T`` rectangles of each of the slot's first
        ``n_streams`` frames into ``out``, (N >= n_streams * T, 3, H, W), tensor ``s * T + t`` being exactly what ``letterbox``
        would write for a stand-alone frame equal to that rectangle.  ``tiles``: a list of ``(x0, y0, w, h)`` for all streams
        (``tile_grid(rows, cols, ...)`` on a uniform ring) or one list per stream; the same ``T`` (1..64) for every stream.
        Everything else -- ``size``, ``mode``, ``rgb``, ``unit``, ``pad``, the ordering on ``hip_stream`` -- as ``letterbox``.
        Returns, per stream, the list of the tiles' ``TileGeometry`` -- what ``DetPost(tiles=T).run`` takes."""
        n = self.n_streams if n_streams is None else int(n_streams)
        if not 1 <= n <= self.n_streams:
            raise ValueError(f"letterbox_tiles: n_streams {n} out of range for a ring of {self.n_streams} streams")
        if mode not in LETTERBOX_MODES:
            raise ValueError(f"letterbox_tiles: unknown mode {mode!r} (\"center\" or \"topleft\")")
        rects = self._stream_tiles(tiles, n)
        T = len(rects[0])
        shape = tuple(int(v) for v in out.shape)
        H, W = _letterbox_size(shape[-2:] if size is None else size)
        if len(shape) != 4 or shape[0] < n * T or shape[1:] != (3, H, W):
            raise ValueError(f"letterbox_tiles: out must have shape (N >= {n * T}, 3, {H}, {W}), got {shape}")
        dtype = {"float32": 0, "float16": 1}.get(str(out.dtype).split(".")[-1])
        if dtype is None:
            raise ValueError(f"letterbox_tiles: out must be float16 or float32, got {out.dtype}")
        if not out.is_contiguous():
            raise ValueError("letterbox_tiles: out must be contiguous")
        if W % 8:
            raise ValueError(f"letterbox_tiles: the output width must be a multiple of 8, got {W}")
        pad = int(pad)
        if not 0 <= pad <= 255:
            raise ValueError(f"letterbox_tiles: pad must be within 0..255, got {pad}")
        ptr = int(out.data_ptr())
        if not ptr or ptr % 16:
            raise ValueError(f"letterbox_tiles: out must be a non-null 16-byte aligned device address, got {ptr:#x}")
        geo = []
        for s in range(n):
            geo.append([])
            for t, (x0, y0, w, h) in enumerate(rects[s]):
                try:
                    g = letterbox_geometry(h, w, (H, W), mode)
                except ValueError as e:
                    raise ValueError(f"stream {s} tile {t}: {e}") from None
                geo[s].append(TileGeometry(g.gain, g.new_w, g.new_h, g.top, g.left, h, w, x0, y0))
        table = np.ascontiguousarray(np.array(rects, dtype=np.int32).reshape(n, T, 4))
        cfg = _lib.Letterbox(H, W, LETTERBOX_MODES[mode], dtype, int(bool(rgb)), int(bool(unit)), pad)
        _lib.check(self._lib.boxmot_hip_ingest_letterbox_tiles(self._handle, int(slot), n, T, table.ctypes.data, ctypes.byref(cfg),
                                                               ctypes.c_void_p(ptr), ctypes.c_void_p(int(hip_stream))))
        return geo

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
