"""Detection post-processing on the device: from a YOLO-family detector's raw prediction tensor to the ``d_dets`` / ``d_det_rows``
block the device-resident tracker steps read, in frame coordinates, with no host round trip (boxmot_hip_detpost_*,
include/boxmot_hip.h; the definition is at the top of csrc/det_post.hpp).  The detector stays the caller's:

    post = DetPost(S, n_anchors=8400, n_classes=80, layout="cn", conf=0.25, iou=0.45, max_det=256)
    d_dets = torch.empty((S, 256, 6), device="cuda"); d_rows = torch.empty(S, dtype=torch.int32, device="cuda")
    geo = ring.letterbox(k, x, hip_stream=st)
    post.run(my_detector(x), geo, d_dets, d_rows, hip_stream=st)          # confidence filter, top-K, NMS, frame coordinates
    trk.step_device(d_dets.data_ptr(), d_rows.data_ptr(), ...)            # after the tracker's stream has waited for ``st``

Stated plainly: this is greedy NMS with torchvision's IoU arithmetic in float32, ``IoU > iou`` suppresses; classes are kept apart by
COMPARING them, not by Ultralytics' ``cls * max_wh`` coordinate offset (which rounds differently); an anchor passes on ``conf >
conf_thres`` strictly (Ultralytics' rule, not YOLOX's ``>=``); candidates are the ``max_candidates`` best by (conf descending,
anchor index ascending), exactly.  It is compared bit for bit with a NumPy restatement of that definition -- parity with
torchvision or Ultralytics on real detector output is not pinned by any test.

Oriented heads: ``layout="cn_obb"`` reads the Ultralytics OBB raw head (S, 4 + n_classes + 1, n_anchors) -- the angle in radians is
the last row -- and writes 7-column rows ``[cx, cy, w, h, angle, conf, cls]``, not clipped, that ``MultiStreamBotSort(is_obb=True)``
reads through ``step_device`` (the definition is at the top of csrc/det_post_obb.hpp).  The NMS is rotated, by the ProbIoU closed
form in float32, ``ProbIoU >= iou`` suppresses; ``nms="greedy"`` drops a candidate that an earlier KEPT one suppresses,
``nms="fast"`` one that ANY earlier one suppresses (what Ultralytics ``nms_rotated`` computes).

Tiled detection for large frames (sliced inference): ``DetPost(..., tiles=T, merge="iou" | "ios")`` reads the detector's output on
the ``T`` tiles per stream that ``FrameRing.letterbox_tiles`` wrote -- ``pred`` is (S * T, ...), tile ``t`` of stream ``s`` at index
``s * T + t`` -- and merges them with ONE NMS per stream in frame coordinates (the definition is at the top of
csrc/det_post_tiled.hpp):

    tiles = tile_grid(2160, 3840, grid=(2, 3), overlap=0.2)              # the whole frame and 2 x 3 tiles: T = 7
    post = DetPost(S, n_anchors=8400, n_classes=80, tiles=len(tiles), merge="ios")
    geo = ring.letterbox_tiles(k, x, tiles, hip_stream=st)               # x: (S * 7, 3, 640, 640)
    post.run(my_detector(x), geo, d_dets, d_rows, hip_stream=st)

Stated plainly: the ``max_candidates`` best anchors of all of a stream's tiles by (conf descending, tile ascending, anchor
ascending) are mapped to the frame -- ``clip((x - left) / gain, 0, w) + x0`` -- BEFORE a merged greedy NMS in float32;
``merge="iou"`` suppresses on ``IoU > iou``, ``merge="ios"`` on ``inter / min(area_i, area_j) > iou`` (intersection over the
smaller box: a box cut by a tile's edge is absorbed by the whole one).  It is pinned against this repository's NumPy restatement
(tests/detpost_tiled_ref.py) only, not against SAHI or Ultralytics.

Pose and segmentation heads: ``DetPost(..., extra=E, extra_kind="raw" | "kpt2" | "kpt3")`` reads heads with ``E`` more values per
anchor after the class scores -- (S, 4 + n_classes + E, n_anchors) for ``"cn"``, (S, n_anchors, 5 + n_classes + E) for ``"nc_obj"``
-- and writes, beside the rows and in their order, the anchor each row came from and that anchor's extras (the definition is at
the top of csrc/det_post_extra.hpp); the tracker's ``det_ind`` column then finds the skeleton or the mask coefficients of a track:

    post = DetPost(S, n_anchors=8400, n_classes=1, layout="cn", extra=51, extra_kind="kpt3", max_det=256)   # "raw" for -seg coefficients
    d_kpts = torch.empty((S, 256, 51), device="cuda"); d_src = torch.empty((S, 256), dtype=torch.int32, device="cuda")
    post.run(pose_model(x), geo, d_dets, d_rows, hip_stream=st, d_extra=d_kpts, d_src=d_src)               # d_src optional
    trk.step_device(d_dets.data_ptr(), d_rows.data_ptr(), ...)
    kpts_of_tracks = d_kpts[s][d_out[s, :n_out, 7].long()]           # det_ind -> the skeleton of each track

Stated plainly: ``"kpt2"`` / ``"kpt3"`` map x and y to the frame with the arithmetic of the boxes, ``clip((v - left) / gain, 0, cols)``
(tiled: the row's own tile, clipped to it, then shifted), and copy the visibility; ``"raw"`` copies.  A NaN coordinate comes out as 0.
This is a reading of Ultralytics' ``scale_coords`` + ``clip_coords``, pinned against this repository's NumPy restatement
(tests/detpost_extra_ref.py) only.  Not for ``"cn_obb"``.

Segmentation masks: ``DetPost(..., extra=32, mask=(mask_h, mask_w), in_shape=(in_h, in_w))`` also decodes the masks of the emitted
rows on the device, from the ``"raw"`` coefficients and the model's prototype tensor (the definition is at the top of
csrc/det_post_mask.hpp); ``d_masks[s][det_ind]`` is then the mask of a track, as ``d_extra[s][det_ind]`` is its coefficients:

    post = DetPost(S, n_anchors=8400, n_classes=80, layout="cn", extra=32, mask=(160, 160), in_shape=(640, 640), max_det=256)
    d_coef = torch.empty((S, 256, 32), device="cuda"); d_masks = torch.empty((S, 256, 160, 160), dtype=torch.uint8, device="cuda")
    pred, proto = seg_model(x)                                          # (S, 4 + 80 + 32, 8400) and (S, 32, 160, 160), fp16 or fp32 each
    post.run(pred, geo, d_dets, d_rows, hip_stream=st, d_extra=d_coef, d_proto=proto, d_masks=d_masks)
    masks_of_tracks = d_masks[s][d_out[s, :n_out, 7].long()]

Stated plainly: a mask byte is 1 where the pixel lies in the row's letterbox-space box scaled to the prototypes' size -- ``x1 * wr <= j
< x2 * wr``, ``y1 * hr <= i < y2 * hr`` in float32, ``wr = mask_w / in_w``, ``hr = mask_h / in_h``, Ultralytics ``crop_mask``'s ``>=`` /
``<`` -- and ``sum_k coef[k] * proto[k, i, j] > 0``, a float32 chain over ascending ``k`` without fused multiply-add; else 0.  The mask
is at PROTOTYPE resolution in letterbox space (tiled: the letterbox of the row's own tile, ``d_src // n_anchors``, whose prototypes
are used): bilinear upsampling to the input or the frame size (``upsample=True``, ``scale_masks``) stays the caller's.  This is a
reading of ``process_mask(..., upsample=False)``, pinned against this repository's NumPy restatement (tests/detpost_mask_ref.py)
only, not against Ultralytics.  No masks for ``"cn_obb"``.

Frame-space label map: on an UNTILED mask handle ``labels`` turns the rows of a run into one int16 plane per stream at FRAME
resolution -- every pixel the row of ``d_dets`` that owns it, the tracker's ``det_ind``, or -1 (the definition is at the top of
csrc/det_post_labels.hpp) -- 4 MB per 1080p stream where dense per-row frame masks would take 530 MB:

    post.run(pred, geo, d_dets, d_rows, hip_stream=st, d_extra=d_coef, d_proto=proto, d_masks=d_masks)
    post.labels(geo, proto, d_dets, d_rows, d_coef, d_labels, hip_stream=st)                  # d_labels: (S, 1080, 1920) int16
    trk.step_device(d_dets.data_ptr(), d_rows.data_ptr(), ...)
    lut = torch.full((257,), -1.0, device="cuda"); lut[d_out[s, :n_out, 7].long()] = d_out[s, :n_out, 4]
    track_ids = lut[d_labels[s].long()]                               # lut[-1] is the last entry: no track

Stated plainly: a row covers a frame pixel when the pixel lies in the row's FRAME box (``x1 <= x < x2``, ``y1 <= y < y2``) and the
row's float logits, sampled bilinearly where the pixel's centre falls in the prototype plane -- ``pu = ((x + 0.5) * gain + left) * wr
- 0.5`` clamped to the plane, likewise ``pv`` -- are ``> 0``: upsampled before thresholding (``process_mask_native``'s order), every
float32 operation rounded on its own; the smallest such row wins, so the highest confidence does.  This is the exact inverse of the
handle's letterbox map with half-pixel centres composed with ``align_corners=False`` sampling; it is NOT Ultralytics ``scale_masks``'
integer-cropped interpolation, which shifts by a fraction of a prototype pixel, and it is pinned against this repository's NumPy
restatement (tests/detpost_labels_ref.py) only.  Out of scope: tiled handles, ``"cn_obb"``, dense per-row frame masks, polygons.
"""
from __future__ import annotations

import ctypes

import numpy as np

from boxmot_amd import _lib

LAYOUTS = {"cn": 0, "nc_obj": 1, "cn_obb": 0}          # the C ABI's layout code: "cn_obb" is "cn" through boxmot_hip_detpost_create_obb
NMS_MODES = {"greedy": 0, "fast": 1}
MERGES = {"iou": 0, "ios": 1}
MAX_TILES = 64
EXTRA_KINDS = {"raw": 0, "kpt2": 1, "kpt3": 2}
MAX_EXTRA = 1024
MAX_MASK_EXTRA = 256
MAX_MASK_DIM = 1024
MAX_LABEL_DET = 32767
_DTYPES = {"float32": 0, "float16": 1}


def _dtype_name(t) -> str:
    return str(t.dtype).split(".")[-1]


def _geometry_row(g, s):
    """(gain, top, left, rows, cols) of a ``LetterboxGeometry`` (or of a 5-sequence in that order)"""
    try:
        row = (g.gain, g.top, g.left, g.rows, g.cols) if hasattr(g, "gain") else tuple(g)
        row = tuple(float(v) for v in row)
    except (TypeError, ValueError):
        raise ValueError(f"stream {s}: geometry must be a LetterboxGeometry or (gain, top, left, rows, cols), got {g!r}") from None
    if len(row) != 5:
        raise ValueError(f"stream {s}: geometry must be a LetterboxGeometry or (gain, top, left, rows, cols), got {g!r}")
    if not (row[0] > 0 and np.isfinite(row[0])) or row[3] < 1 or row[4] < 1:
        raise ValueError(f"stream {s}: geometry needs gain > 0 and a frame of at least 1 x 1, got gain {row[0]}, rows {row[3]}, cols {row[4]}")
    return row


def _tile_geometry_row(g, s, t):
    """(gain, top, left, x0, y0, w, h) of a ``TileGeometry`` (or of a 7-sequence in that order)"""
    what = f"stream {s} tile {t}: geometry must be a TileGeometry or (gain, top, left, x0, y0, w, h), got {g!r}"
    try:
        row = (g.gain, g.top, g.left, g.x0, g.y0, g.cols, g.rows) if hasattr(g, "gain") else tuple(g)
        row = tuple(float(v) for v in row)
    except (TypeError, ValueError, AttributeError):
        raise ValueError(what) from None
    if len(row) != 7:
        raise ValueError(what)
    if not all(np.isfinite(row)) or not row[0] > 0 or row[5] < 1 or row[6] < 1:
        raise ValueError(f"stream {s} tile {t}: geometry needs finite values, gain > 0 and a tile of at least 1 x 1, got gain {row[0]}, w {row[5]}, "
                         f"h {row[6]}")
    return row


class DetPost:
    def __init__(self, n_streams: int, n_anchors: int, n_classes: int, layout: str = "cn", conf: float = 0.25, iou: float = 0.45,
                 max_det: int = 256, max_candidates: int = 1024, agnostic: bool = False, classes=None, nms: str | None = None,
                 regularize: bool | None = None, tiles: int | None = None, merge: str | None = None, extra: int | None = None,
                 extra_kind: str | None = None, mask=None, in_shape=None):
        """``layout``: ``"cn"`` -- (S, 4 + n_classes, n_anchors), the Ultralytics v8 / 11 raw head, conf = the best class score --
        ``"nc_obj"`` -- (S, n_anchors, 5 + n_classes), the YOLOX / YOLOv5 decoded head, conf = obj * the best class score -- or
        ``"cn_obb"`` -- (S, 4 + n_classes + 1, n_anchors), the Ultralytics OBB raw head, the angle in radians as the last row.
        ``classes``: an optional allow-list of class indices, applied to an anchor's best class.  ``nms`` (``"greedy"``, the
        default, or ``"fast"``) and ``regularize`` (w >= h and the angle within [0, pi] in the rows; default off) belong to
        ``"cn_obb"`` alone.  ``tiles``: the detector ran on that many tiles per stream (``FrameRing.letterbox_tiles``) and their
        detections are merged by one NMS per stream in frame coordinates, on ``merge="iou"`` (the default) or ``"ios"``,
        intersection over the smaller box; ``n_anchors`` stays the anchors of ONE tile tensor.  Not for ``"cn_obb"``.
        ``extra``: the head has that many more values per anchor after the class scores (1..1024) and ``run`` also writes
        ``d_extra`` / ``d_src``; ``extra_kind``: ``"raw"`` (the default) copies them, ``"kpt2"`` / ``"kpt3"`` map keypoints (x, y /
        x, y, visibility) to the frame.  With ``tiles`` or without; not for ``"cn_obb"``.
        ``mask=(mask_h, mask_w)`` (1..1024 each) with ``in_shape=(in_h, in_w)``, the detector's input size: the ``extra`` (1..256)
        values are ``"raw"`` mask coefficients and ``run`` also takes the prototypes ``d_proto`` and writes ``d_masks``, uint8 at
        prototype resolution in letterbox space.  Stated plainly: upsampling stays the caller's; pinned against this
        repository's NumPy restatement only.  With ``tiles`` or without; not for ``"cn_obb"``."""
        self._handle = None
        self._configure(n_streams, n_anchors, n_classes, layout, conf, iou, max_det, max_candidates, agnostic, classes, nms, regularize, tiles, merge,
                        extra, extra_kind, mask, in_shape)
        self._lib = _lib.load()
        allow = None
        if self.classes is not None:
            allow = np.zeros(self.n_classes, dtype=np.uint8)
            allow[self.classes] = 1
        cfg = _lib.DetPostConfig(self.n_streams, self.n_anchors, self.n_classes, LAYOUTS[self.layout], self.conf, self.iou, self.max_candidates,
                                 self.max_det, int(self.agnostic), None if allow is None else allow.ctypes.data)
        if self.mask is not None:
            ecfg = _lib.DetPostExtraConfig(cfg, self.tiles or 0, MERGES[self.merge or "iou"], self.extra, EXTRA_KINDS[self.extra_kind])
            mcfg = _lib.DetPostMaskConfig(ecfg, self.mask[0], self.mask[1], self.in_shape[0], self.in_shape[1])
            self._handle = self._lib.boxmot_hip_detpost_create_mask(ctypes.byref(mcfg))
        elif self.extra is not None:
            ecfg = _lib.DetPostExtraConfig(cfg, self.tiles or 0, MERGES[self.merge or "iou"], self.extra, EXTRA_KINDS[self.extra_kind])
            self._handle = self._lib.boxmot_hip_detpost_create_extra(ctypes.byref(ecfg))
        elif self.tiles is not None:
            tcfg = _lib.DetPostTiledConfig(cfg, self.tiles, MERGES[self.merge])
            self._handle = self._lib.boxmot_hip_detpost_create_tiled(ctypes.byref(tcfg))
        elif self.is_obb:
            ocfg = _lib.DetPostObbConfig(cfg, NMS_MODES[self.nms], int(self.regularize))
            self._handle = self._lib.boxmot_hip_detpost_create_obb(ctypes.byref(ocfg))
        else:
            self._handle = self._lib.boxmot_hip_detpost_create(ctypes.byref(cfg))      # (the table is copied by the call)
        if not self._handle:
            raise RuntimeError(_lib.last_error())

    def _configure(self, n_streams, n_anchors, n_classes, layout="cn", conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False,
                   classes=None, nms=None, regularize=None, tiles=None, merge=None, extra=None, extra_kind=None, mask=None, in_shape=None):
        """the options, checked; touches neither the library nor a device"""
        for name, v in (("n_streams", n_streams), ("n_anchors", n_anchors), ("n_classes", n_classes), ("max_det", max_det)):
            if int(v) != v or int(v) < 1:
                raise ValueError(f"DetPost: {name} must be an integer >= 1, got {v!r}")
        if layout not in LAYOUTS:
            raise ValueError(f"DetPost: unknown layout {layout!r} (\"cn\", \"nc_obj\" or \"cn_obb\")")
        is_obb = layout == "cn_obb"
        if not is_obb and (nms is not None or regularize is not None):
            raise ValueError(f"DetPost: nms= and regularize= belong to layout \"cn_obb\", not to {layout!r}")
        if tiles is None and merge is not None:
            raise ValueError("DetPost: merge= belongs to a tiled handle: give tiles= as well")
        if tiles is not None:
            if is_obb:
                raise ValueError("DetPost: layout \"cn_obb\" has no tiled form: tiles= is for \"cn\" and \"nc_obj\"")
            if int(tiles) != tiles or not 1 <= int(tiles) <= MAX_TILES:
                raise ValueError(f"DetPost: tiles must be an integer within 1..{MAX_TILES}, got {tiles!r}")
            merge = "iou" if merge is None else merge
            if merge not in MERGES:
                raise ValueError(f"DetPost: unknown merge {merge!r} (\"iou\" or \"ios\")")
        if mask is not None and is_obb:
            raise ValueError("DetPost: layout \"cn_obb\" has no masks: mask= is for \"cn\" and \"nc_obj\"")
        if extra is None and extra_kind is not None:
            raise ValueError("DetPost: extra_kind= belongs to a head with extras: give extra= as well")
        if extra is not None:
            if is_obb:
                raise ValueError("DetPost: layout \"cn_obb\" has no extras: extra= is for \"cn\" and \"nc_obj\"")
            if int(extra) != extra or not 1 <= int(extra) <= MAX_EXTRA:
                raise ValueError(f"DetPost: extra must be an integer within 1..{MAX_EXTRA}, got {extra!r}")
            extra_kind = "raw" if extra_kind is None else extra_kind
            if extra_kind not in EXTRA_KINDS:
                raise ValueError(f"DetPost: unknown extra_kind {extra_kind!r} (\"raw\", \"kpt2\" or \"kpt3\")")
            group = {"raw": 1, "kpt2": 2, "kpt3": 3}[extra_kind]
            if int(extra) % group:
                raise ValueError(f"DetPost: extra_kind {extra_kind!r} takes values in groups of {group}: extra = {extra} is no multiple")
        if mask is None and in_shape is not None:
            raise ValueError("DetPost: in_shape= belongs to a mask handle: give mask= as well")
        if mask is not None:
            if extra is None:
                raise ValueError("DetPost: mask= needs extra=, the number of mask coefficients per anchor")
            if in_shape is None:
                raise ValueError("DetPost: mask= needs in_shape=(in_h, in_w), the detector's input size")
            if extra_kind != "raw":
                raise ValueError(f"DetPost: mask= takes extra_kind \"raw\" (the mask coefficients), not extra_kind {extra_kind!r}")
            if int(extra) > MAX_MASK_EXTRA:
                raise ValueError(f"DetPost: mask= takes extra within 1..{MAX_MASK_EXTRA}, got {extra!r}")
            for name, v, hi in (("mask", mask, MAX_MASK_DIM), ("in_shape", in_shape, None)):
                try:
                    ok = len(v) == 2 and all(int(q) == q and int(q) >= 1 and (hi is None or int(q) <= hi) for q in v)
                except (TypeError, ValueError):
                    ok = False
                if not ok:
                    raise ValueError(f"DetPost: {name} must be two integers " + (f"within 1..{hi}" if hi else ">= 1") + f", got {v!r}")
        nms = "greedy" if nms is None else nms
        if nms not in NMS_MODES:
            raise ValueError(f"DetPost: unknown nms {nms!r} (\"greedy\" or \"fast\")")
        if not 0.0 <= float(conf) < 1.0:
            raise ValueError(f"DetPost: conf must be within [0, 1), got {conf!r}")
        if not 0.0 <= float(iou) <= 1.0:
            raise ValueError(f"DetPost: iou must be within [0, 1], got {iou!r}")
        if int(max_candidates) != max_candidates or not 64 <= int(max_candidates) <= 4096:
            raise ValueError(f"DetPost: max_candidates must be an integer within 64..4096, got {max_candidates!r}")
        if classes is not None:
            classes = [int(c) for c in classes]
            bad = [c for c in classes if not 0 <= c < int(n_classes)]
            if bad or not classes:
                raise ValueError(f"DetPost: classes must be a non-empty list of indices within 0..{int(n_classes) - 1}, got {classes}")
        self.n_streams, self.n_anchors, self.n_classes, self.layout = int(n_streams), int(n_anchors), int(n_classes), layout
        self.conf, self.iou = float(np.float32(conf)), float(np.float32(iou))          # the thresholds are float32 on the device
        self.max_det, self.max_candidates, self.agnostic, self.classes = int(max_det), int(max_candidates), bool(agnostic), classes
        self.is_obb, self.nms, self.regularize = is_obb, nms if is_obb else None, bool(regularize) if is_obb else None
        self.extra, self.extra_kind = (None, None) if extra is None else (int(extra), extra_kind)
        self.n_channels = (5 + self.n_classes if is_obb or layout == "nc_obj" else 4 + self.n_classes) + (self.extra or 0)    # per anchor, in the layout
        self.det_cols = 7 if is_obb else 6
        self.tiles, self.merge = (None, None) if tiles is None else (int(tiles), merge)
        self.mask, self.in_shape = (None, None) if mask is None else ((int(mask[0]), int(mask[1])), (int(in_shape[0]), int(in_shape[1])))

    def pred_shape(self, n: int | None = None) -> tuple:
        n = (self.n_streams if n is None else n) * (self.tiles or 1)
        return (n, self.n_anchors, self.n_channels) if self.layout == "nc_obj" else (n, self.n_channels, self.n_anchors)

    def _check_run(self, pred, geo, d_dets, d_det_rows, d_extra=None, d_src=None):
        """(n_streams, dtype code, geometry table) of a call; raises ValueError naming what is wrong"""
        n = len(geo)
        if not 1 <= n <= self.n_streams:
            raise ValueError(f"DetPost.run: geo has {n} entries for a handle of {self.n_streams} streams")
        T = self.tiles or 1
        if self.tiles is not None:
            for s, g in enumerate(geo):
                if hasattr(g, "gain") or not hasattr(g, "__len__") or len(g) != T:
                    raise ValueError(f"DetPost.run: stream {s}: a handle of tiles={T} takes a list of {T} TileGeometry per stream, got {g!r}")
        shape = tuple(int(v) for v in pred.shape)
        if len(shape) != 3 or shape[0] < n * T or shape[1:] != self.pred_shape()[1:]:
            raise ValueError(f"DetPost.run: pred must have shape {('N >= %d' % (n * T),) + self.pred_shape()[1:]} for layout {self.layout!r}, got {shape}")
        dtype = _DTYPES.get(_dtype_name(pred))
        if dtype is None:
            raise ValueError(f"DetPost.run: pred must be float16 or float32, got {pred.dtype}")
        if not pred.is_contiguous():
            raise ValueError("DetPost.run: pred must be contiguous")
        dshape = tuple(int(v) for v in d_dets.shape)
        if len(dshape) != 3 or dshape[0] < n or dshape[2] != self.det_cols:
            raise ValueError(f"DetPost.run: d_dets must have shape (N >= {n}, rows, {self.det_cols}), got {dshape}")
        if dshape[1] < self.max_det:
            raise ValueError(f"DetPost.run: d_dets holds {dshape[1]} rows per stream, fewer than max_det = {self.max_det}")
        if _dtype_name(d_dets) != "float32":
            raise ValueError(f"DetPost.run: d_dets must be float32, got {d_dets.dtype}")
        if not d_dets.is_contiguous():
            raise ValueError("DetPost.run: d_dets must be contiguous")
        rshape = tuple(int(v) for v in d_det_rows.shape)
        if len(rshape) != 1 or rshape[0] < n:
            raise ValueError(f"DetPost.run: d_det_rows must have shape (N >= {n},), got {rshape}")
        if _dtype_name(d_det_rows) != "int32":
            raise ValueError(f"DetPost.run: d_det_rows must be int32, got {d_det_rows.dtype}")
        if not d_det_rows.is_contiguous():
            raise ValueError("DetPost.run: d_det_rows must be contiguous")
        out = [("pred", pred), ("d_dets", d_dets), ("d_det_rows", d_det_rows)]
        if self.extra is None:
            if d_extra is not None or d_src is not None:
                raise ValueError("DetPost.run: d_extra and d_src belong to a handle with extras (extra=), which this one is not")
        else:
            if d_extra is None:
                raise ValueError(f"DetPost.run: a handle of extra={self.extra} needs d_extra")
            eshape = tuple(int(v) for v in d_extra.shape)
            if len(eshape) != 3 or eshape[0] < n or eshape[1] != dshape[1] or eshape[2] != self.extra:
                raise ValueError(f"DetPost.run: d_extra must have shape (N >= {n}, {dshape[1]}, {self.extra}), the rows of d_dets, got {eshape}")
            if _dtype_name(d_extra) != "float32":
                raise ValueError(f"DetPost.run: d_extra must be float32, got {d_extra.dtype}")
            if not d_extra.is_contiguous():
                raise ValueError("DetPost.run: d_extra must be contiguous")
            out.append(("d_extra", d_extra))
            if d_src is not None:
                sshape = tuple(int(v) for v in d_src.shape)
                if len(sshape) != 2 or sshape[0] < n or sshape[1] != dshape[1]:
                    raise ValueError(f"DetPost.run: d_src must have shape (N >= {n}, {dshape[1]}), the rows of d_dets, got {sshape}")
                if _dtype_name(d_src) != "int32":
                    raise ValueError(f"DetPost.run: d_src must be int32, got {d_src.dtype}")
                if not d_src.is_contiguous():
                    raise ValueError("DetPost.run: d_src must be contiguous")
                out.append(("d_src", d_src))
        for name, t in out:
            if not int(t.data_ptr()):
                raise ValueError(f"DetPost.run: {name} has a null device address")
        if self.tiles is not None:
            table = np.array([[_tile_geometry_row(g, s, t) for t, g in enumerate(gs)] for s, gs in enumerate(geo)], dtype=np.float64)
        else:
            table = np.array([_geometry_row(g, s) for s, g in enumerate(geo)], dtype=np.float64)
        return n, dtype, table, dshape[1]

    def _check_mask(self, n, rows, d_proto, d_masks):
        """the prototype dtype code of a call over ``n`` streams into blocks of ``rows`` rows per stream, or None on a handle without
        masks; raises ValueError naming what is wrong"""
        if self.mask is None:
            if d_proto is not None or d_masks is not None:
                raise ValueError("DetPost.run: d_proto and d_masks belong to a mask handle (mask=), which this one is not")
            return None
        if d_proto is None or d_masks is None:
            raise ValueError(f"DetPost.run: a handle of mask={self.mask} needs d_proto and d_masks")
        T = self.tiles or 1
        want = (self.extra,) + self.mask
        pshape = tuple(int(v) for v in d_proto.shape)
        if len(pshape) != 4 or pshape[0] < n * T or pshape[1:] != want:
            raise ValueError(f"DetPost.run: d_proto must have shape {('N >= %d' % (n * T),) + want}, got {pshape}")
        pdtype = _DTYPES.get(_dtype_name(d_proto))
        if pdtype is None:
            raise ValueError(f"DetPost.run: d_proto must be float16 or float32, got {d_proto.dtype}")
        if not d_proto.is_contiguous():
            raise ValueError("DetPost.run: d_proto must be contiguous")
        mshape = tuple(int(v) for v in d_masks.shape)
        if len(mshape) != 4 or mshape[0] < n or mshape[1] != rows or mshape[2:] != self.mask:
            raise ValueError(f"DetPost.run: d_masks must have shape {('N >= %d' % n, rows) + self.mask}, the rows of d_dets, got {mshape}")
        if _dtype_name(d_masks) != "uint8":
            raise ValueError(f"DetPost.run: d_masks must be uint8, got {d_masks.dtype}")
        if not d_masks.is_contiguous():
            raise ValueError("DetPost.run: d_masks must be contiguous")
        for name, t in (("d_proto", d_proto), ("d_masks", d_masks)):
            if not int(t.data_ptr()):
                raise ValueError(f"DetPost.run: {name} has a null device address")
        return pdtype

    def run(self, pred, geo, d_dets, d_det_rows, hip_stream: int = 0, d_extra=None, d_src=None, d_proto=None, d_masks=None) -> None:
        """``pred``: the detector's raw output of the first ``len(geo)`` streams, a contiguous float16 / float32 device tensor in
        the handle's layout -- anything with ``data_ptr()``, ``dtype``, ``shape`` and ``is_contiguous()``; ``geo``: what
        ``FrameRing.letterbox`` returned for them; ``d_dets``: (N, rows >= max_det, 6) float32, ``d_det_rows``: (N,) int32, on the
        same device.  Asynchronous on ``hip_stream``: rows ``[x1, y1, x2, y2, conf, cls]`` in frame coordinates and their count per
        stream; rows at and beyond the count, and streams beyond ``len(geo)``, are left alone.  Layout ``"cn_obb"``: ``d_dets`` is
        (N, rows >= max_det, 7), rows ``[cx, cy, w, h, angle, conf, cls]``, not clipped to the frame.  A handle of ``tiles=T``:
        ``pred`` holds ``len(geo) * T`` tensors and ``geo`` is what ``FrameRing.letterbox_tiles`` returned, per stream a list of
        ``T`` ``TileGeometry`` (or 7-sequences gain, top, left, x0, y0, w, h); ``d_dets`` / ``d_det_rows`` stay per stream.
        A handle of ``extra=E``: ``d_extra`` (N, rows of d_dets, E) float32 takes the extras of every row and, where given,
        ``d_src`` (N, rows of d_dets) int32 the anchor it came from (tiled: ``t * n_anchors + a``); rows beyond the count are left
        alone there too.  A handle of ``mask=(mask_h, mask_w)``: ``d_proto`` (N, E, mask_h, mask_w) float16 / float32, one tensor per
        stream (tiled: per (stream, tile), like ``pred``), and ``d_masks`` (N, rows of d_dets, mask_h, mask_w) uint8, which takes
        the 0 / 1 mask of every row at prototype resolution in letterbox space; both required there, refused elsewhere."""
        n, dtype, table, stride = self._check_run(pred, geo, d_dets, d_det_rows, d_extra, d_src)
        pdtype = self._check_mask(n, stride, d_proto, d_masks)
        if pdtype is not None:
            _lib.check(self._lib.boxmot_hip_detpost_run_mask(
                self._handle, n, ctypes.c_void_p(int(pred.data_ptr())), dtype, table.ctypes.data_as(_lib.c_double_p),
                ctypes.c_void_p(int(d_dets.data_ptr())), stride, ctypes.c_void_p(int(d_det_rows.data_ptr())), ctypes.c_void_p(int(d_extra.data_ptr())),
                None if d_src is None else ctypes.c_void_p(int(d_src.data_ptr())), ctypes.c_void_p(int(d_proto.data_ptr())), pdtype,
                ctypes.c_void_p(int(d_masks.data_ptr())), ctypes.c_void_p(int(hip_stream))))
            return
        if self.extra is not None:
            _lib.check(self._lib.boxmot_hip_detpost_run_extra(
                self._handle, n, ctypes.c_void_p(int(pred.data_ptr())), dtype, table.ctypes.data_as(_lib.c_double_p),
                ctypes.c_void_p(int(d_dets.data_ptr())), stride, ctypes.c_void_p(int(d_det_rows.data_ptr())), ctypes.c_void_p(int(d_extra.data_ptr())),
                None if d_src is None else ctypes.c_void_p(int(d_src.data_ptr())), ctypes.c_void_p(int(hip_stream))))
            return
        run = self._lib.boxmot_hip_detpost_run if self.tiles is None else self._lib.boxmot_hip_detpost_run_tiled
        _lib.check(run(self._handle, n, ctypes.c_void_p(int(pred.data_ptr())), dtype,
                       table.ctypes.data_as(_lib.c_double_p), ctypes.c_void_p(int(d_dets.data_ptr())), stride,
                       ctypes.c_void_p(int(d_det_rows.data_ptr())), ctypes.c_void_p(int(hip_stream))))

    def run_host(self, pred, geo, proto=None) -> list:
        """Convenience form: ``pred`` a device tensor or a host array (uploaded); returns the rows of each stream as an (n_s, 6)
        float32 array, (n_s, 7) for layout ``"cn_obb"``; on a handle of ``extra=E`` a tuple ``(rows, extras (n_s, E) float32, src (n_s,)
        int32)`` per stream; on a handle of ``mask=`` ``proto`` (a device tensor or a host array) is needed and the tuple is ``(rows,
        extras, src, masks (n_s, mask_h, mask_w) uint8)``.  Allocates its outputs with torch and waits for the result."""
        import torch
        if isinstance(pred, np.ndarray):
            pred = torch.from_numpy(np.ascontiguousarray(pred)).cuda()
        if self.mask is None and proto is not None:
            raise ValueError("DetPost.run_host: proto belongs to a mask handle (mask=), which this one is not")
        if self.mask is not None and proto is None:
            raise ValueError(f"DetPost.run_host: a handle of mask={self.mask} needs proto")
        if isinstance(proto, np.ndarray):
            proto = torch.from_numpy(np.ascontiguousarray(proto)).to(pred.device)
        n = len(geo)
        d_dets = torch.empty((max(n, 1), self.max_det, self.det_cols), dtype=torch.float32, device=pred.device)
        d_rows = torch.zeros(max(n, 1), dtype=torch.int32, device=pred.device)
        st = torch.cuda.current_stream(pred.device)
        if self.extra is None:
            self.run(pred, geo, d_dets, d_rows, hip_stream=st.cuda_stream)
            st.synchronize()
            rows, dets = d_rows.cpu().numpy(), d_dets.cpu().numpy()
            return [dets[s, :rows[s]].copy() for s in range(n)]
        d_extra = torch.empty((max(n, 1), self.max_det, self.extra), dtype=torch.float32, device=pred.device)
        d_src = torch.empty((max(n, 1), self.max_det), dtype=torch.int32, device=pred.device)
        if self.mask is not None:
            d_masks = torch.empty((max(n, 1), self.max_det) + self.mask, dtype=torch.uint8, device=pred.device)
            self.run(pred, geo, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_extra, d_src=d_src, d_proto=proto, d_masks=d_masks)
            st.synchronize()
            rows, dets, extras, src = d_rows.cpu().numpy(), d_dets.cpu().numpy(), d_extra.cpu().numpy(), d_src.cpu().numpy()
            return [(dets[s, :rows[s]].copy(), extras[s, :rows[s]].copy(), src[s, :rows[s]].copy(), d_masks[s, :rows[s]].cpu().numpy()) for s in range(n)]
        self.run(pred, geo, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_extra, d_src=d_src)
        st.synchronize()
        rows, dets, extras, src = d_rows.cpu().numpy(), d_dets.cpu().numpy(), d_extra.cpu().numpy(), d_src.cpu().numpy()
        return [(dets[s, :rows[s]].copy(), extras[s, :rows[s]].copy(), src[s, :rows[s]].copy()) for s in range(n)]

    def _check_labels(self, geo, d_proto, d_dets, d_det_rows, d_extra, d_labels):
        """(n_streams, prototype dtype code, geometry table, rows per stream of d_dets, label_rows, label_cols) of a ``labels`` call;
        raises ValueError naming what is wrong"""
        if self.mask is None:
            raise ValueError("DetPost.labels: label maps belong to a mask handle (mask=), which this one is not")
        if self.tiles is not None:
            raise ValueError("DetPost.labels: label maps of a tiled handle (tiles=) are out of scope: use an untiled mask handle")
        if self.max_det > MAX_LABEL_DET:
            raise ValueError(f"DetPost.labels: the labels are int16: max_det = {self.max_det} exceeds {MAX_LABEL_DET}")
        n = len(geo)
        if not 1 <= n <= self.n_streams:
            raise ValueError(f"DetPost.labels: geo has {n} entries for a handle of {self.n_streams} streams")
        want = (self.extra,) + self.mask
        pshape = tuple(int(v) for v in d_proto.shape)
        if len(pshape) != 4 or pshape[0] < n or pshape[1:] != want:
            raise ValueError(f"DetPost.labels: d_proto must have shape {('N >= %d' % n,) + want}, got {pshape}")
        pdtype = _DTYPES.get(_dtype_name(d_proto))
        if pdtype is None:
            raise ValueError(f"DetPost.labels: d_proto must be float16 or float32, got {d_proto.dtype}")
        dshape = tuple(int(v) for v in d_dets.shape)
        if len(dshape) != 3 or dshape[0] < n or dshape[2] != self.det_cols:
            raise ValueError(f"DetPost.labels: d_dets must have shape (N >= {n}, rows, {self.det_cols}), got {dshape}")
        if dshape[1] < self.max_det:
            raise ValueError(f"DetPost.labels: d_dets holds {dshape[1]} rows per stream, fewer than max_det = {self.max_det}")
        if _dtype_name(d_dets) != "float32":
            raise ValueError(f"DetPost.labels: d_dets must be float32, got {d_dets.dtype}")
        rshape = tuple(int(v) for v in d_det_rows.shape)
        if len(rshape) != 1 or rshape[0] < n:
            raise ValueError(f"DetPost.labels: d_det_rows must have shape (N >= {n},), got {rshape}")
        if _dtype_name(d_det_rows) != "int32":
            raise ValueError(f"DetPost.labels: d_det_rows must be int32, got {d_det_rows.dtype}")
        eshape = tuple(int(v) for v in d_extra.shape)
        if len(eshape) != 3 or eshape[0] < n or eshape[1] != dshape[1] or eshape[2] != self.extra:
            raise ValueError(f"DetPost.labels: d_extra must have shape (N >= {n}, {dshape[1]}, {self.extra}), the rows of d_dets, got {eshape}")
        if _dtype_name(d_extra) != "float32":
            raise ValueError(f"DetPost.labels: d_extra must be float32, got {d_extra.dtype}")
        lshape = tuple(int(v) for v in d_labels.shape)
        if len(lshape) != 3 or lshape[0] < n or lshape[1] < 1 or lshape[2] < 1:
            raise ValueError(f"DetPost.labels: d_labels must have shape (N >= {n}, H, W), got {lshape}")
        if _dtype_name(d_labels) != "int16":
            raise ValueError(f"DetPost.labels: d_labels must be int16, got {d_labels.dtype}")
        for name, t in (("d_proto", d_proto), ("d_dets", d_dets), ("d_det_rows", d_det_rows), ("d_extra", d_extra), ("d_labels", d_labels)):
            if not t.is_contiguous():
                raise ValueError(f"DetPost.labels: {name} must be contiguous")
            if not int(t.data_ptr()):
                raise ValueError(f"DetPost.labels: {name} has a null device address")
        table = np.array([_geometry_row(g, s) for s, g in enumerate(geo)], dtype=np.float64)
        for s, row in enumerate(table):
            if row[3] > lshape[1] or row[4] > lshape[2]:
                raise ValueError(f"DetPost.labels: stream {s}: the frame of {int(row[3])} x {int(row[4])} does not fit d_labels' planes of {lshape[1]} x {lshape[2]}")
        return n, pdtype, table, dshape[1], lshape[1], lshape[2]

    def labels(self, geo, d_proto, d_dets, d_det_rows, d_extra, d_labels, hip_stream: int = 0) -> None:
        """The frame-space instance label map of the rows a ``run`` on the same stream left in ``d_dets`` / ``d_det_rows`` /
        ``d_extra`` (the definition is step 10 at the top of csrc/det_post_labels.hpp); an untiled mask handle only.  ``geo`` and
        ``d_proto`` are the run's; ``d_labels``: (N >= len(geo), H, W) int16 with H, W at least every stream's frame.  Asynchronous on
        ``hip_stream``: ``d_labels[s, y, x]`` for every pixel of stream ``s``'s frame becomes the smallest row ``r < min(d_det_rows[s],
        max_det)`` that covers it -- ``x1 <= x < x2``, ``y1 <= y < y2`` on the row's frame box and the row's logits, sampled bilinearly
        at the pixel centre's position in the prototype plane, ``> 0`` -- or -1; the rest of a larger plane and streams beyond
        ``len(geo)`` are left alone.  Stated plainly: the exact inverse of the letterbox map with half-pixel centres composed with
        ``align_corners=False`` sampling, NOT Ultralytics ``scale_masks``' integer-cropped interpolation; pinned against this
        repository's NumPy restatement only."""
        n, pdtype, table, stride, rows, cols = self._check_labels(geo, d_proto, d_dets, d_det_rows, d_extra, d_labels)
        _lib.check(self._lib.boxmot_hip_detpost_labels(
            self._handle, n, table.ctypes.data_as(_lib.c_double_p), ctypes.c_void_p(int(d_proto.data_ptr())), pdtype, ctypes.c_void_p(int(d_dets.data_ptr())),
            stride, ctypes.c_void_p(int(d_det_rows.data_ptr())), ctypes.c_void_p(int(d_extra.data_ptr())), ctypes.c_void_p(int(d_labels.data_ptr())), rows, cols,
            ctypes.c_void_p(int(hip_stream))))

    def labels_host(self, pred, geo, proto) -> list:
        """Convenience form beside ``run_host``: ``run`` then ``labels`` on the current torch stream; returns per stream a tuple ``(rows,
        extras, src, labels (frame rows, frame cols) int16)``.  ``pred`` / ``proto``: device tensors or host arrays (uploaded).
        Allocates its outputs with torch and waits for the result."""
        import torch
        if self.mask is None:
            raise ValueError("DetPost.labels_host: label maps belong to a mask handle (mask=), which this one is not")
        if self.tiles is not None:
            raise ValueError("DetPost.labels_host: label maps of a tiled handle (tiles=) are out of scope: use an untiled mask handle")
        if isinstance(pred, np.ndarray):
            pred = torch.from_numpy(np.ascontiguousarray(pred)).cuda()
        if isinstance(proto, np.ndarray):
            proto = torch.from_numpy(np.ascontiguousarray(proto)).to(pred.device)
        n = len(geo)
        table = [_geometry_row(g, s) for s, g in enumerate(geo)]
        H, W = max([int(r[3]) for r in table] + [1]), max([int(r[4]) for r in table] + [1])
        d_dets = torch.empty((max(n, 1), self.max_det, self.det_cols), dtype=torch.float32, device=pred.device)
        d_rows = torch.zeros(max(n, 1), dtype=torch.int32, device=pred.device)
        d_extra = torch.empty((max(n, 1), self.max_det, self.extra), dtype=torch.float32, device=pred.device)
        d_src = torch.empty((max(n, 1), self.max_det), dtype=torch.int32, device=pred.device)
        d_masks = torch.empty((max(n, 1), self.max_det) + self.mask, dtype=torch.uint8, device=pred.device)
        d_labels = torch.empty((max(n, 1), H, W), dtype=torch.int16, device=pred.device)
        st = torch.cuda.current_stream(pred.device)
        self.run(pred, geo, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_extra, d_src=d_src, d_proto=proto, d_masks=d_masks)
        self.labels(geo, proto, d_dets, d_rows, d_extra, d_labels, hip_stream=st.cuda_stream)
        st.synchronize()
        rows, dets, extras, src, labels = d_rows.cpu().numpy(), d_dets.cpu().numpy(), d_extra.cpu().numpy(), d_src.cpu().numpy(), d_labels.cpu().numpy()
        return [(dets[s, :rows[s]].copy(), extras[s, :rows[s]].copy(), src[s, :rows[s]].copy(), labels[s, :int(table[s][3]), :int(table[s][4])].copy())
                for s in range(n)]

    def counters(self) -> np.ndarray:
        """(n_streams, 3) int32 of the last run, after waiting for it: anchors that passed the threshold, candidates after the
        top-K (``max_candidates`` when it bit), candidates NMS kept before the ``max_det`` cut."""
        out = np.zeros((self.n_streams, 3), dtype=np.int32)
        _lib.check(self._lib.boxmot_hip_detpost_counters(self._handle, out.ctypes.data, self.n_streams))
        return out

    def close(self) -> None:
        h = getattr(self, "_handle", None)
        if h:
            self._lib.boxmot_hip_detpost_destroy(h)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
