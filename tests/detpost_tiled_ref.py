"""NumPy float32 restatement of the TILED detection post-processing definition (boxmot_amd/csrc/det_post_tiled.hpp, steps 1-6 with 3b),
written from the definition and not from the kernels, and the table of cases the emulated and the device kernels are compared with,
bit for bit.

    rows, counters = detpost_tiled(preds, geos, layout, ...)         # one stream

``preds``: (T, 4 + nc, A) for layout "cn", (T, A, 5 + nc) for "nc_obj", float16 or float32.  ``geos``: T x (gain, top, left, x0, y0,
w, h).  ``rows``: (n, 6) float32 [x1, y1, x2, y2, conf, cls] in frame coordinates, ``counters``: int32 (passed, candidates, kept by
NMS).  ``nms_ge`` and ``tiles_high_first`` make the two WRONG references (``>=`` in the NMS test; conf ties to the higher tile) the
tests use as controls."""
from typing import NamedTuple

import numpy as np

import detpost_ref
import letterbox_ref

F = np.float32
LAYOUTS = detpost_ref.LAYOUTS
MERGES = {"iou": 0, "ios": 1}


def to_frame(xyxy, geo):
    """step 3b on an (n, 4) float32 table: one subtraction, one division, a clip to the tile, one addition"""
    gain, top, left, x0, y0, w, h = (F(v) for v in geo)
    out = np.array(xyxy, dtype=np.float32, ndmin=2)
    out[:, [0, 2]] = np.fmin(np.fmax((out[:, [0, 2]] - left) / gain, F(0)), w) + x0
    out[:, [1, 3]] = np.fmin(np.fmax((out[:, [1, 3]] - top) / gain, F(0)), h) + y0
    return out


def suppresses(kept_boxes, b, iou_thres, merge="iou", ge=False):
    """which of the (n, 4) float32 xyxy boxes suppress box b, by the metric of ``merge``"""
    with np.errstate(invalid="ignore", divide="ignore"):
        area_k = (kept_boxes[:, 2] - kept_boxes[:, 0]) * (kept_boxes[:, 3] - kept_boxes[:, 1])
        area_b = (b[2] - b[0]) * (b[3] - b[1])
        iw = np.fmax(np.fmin(b[2], kept_boxes[:, 2]) - np.fmax(b[0], kept_boxes[:, 0]), F(0))
        ih = np.fmax(np.fmin(b[3], kept_boxes[:, 3]) - np.fmax(b[1], kept_boxes[:, 1]), F(0))
        inter = iw * ih
        ratio = inter / (area_b + area_k - inter) if merge == "iou" else inter / np.fmin(area_b, area_k)
        return ratio >= F(iou_thres) if ge else ratio > F(iou_thres)


def detpost_tiled(preds, geos, layout="cn", conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False, classes=None, merge="iou",
                  nms_ge=False, tiles_high_first=False):
    T = len(preds)
    assert len(geos) == T and merge in MERGES
    half = F(0.5)
    tile, anchor, cls, cf, xyxy = [], [], [], [], []
    for t in range(T):
        box, _, _ = detpost_ref.split(preds[t], layout)
        c, f, passed = detpost_ref.score(preds[t], layout, conf, classes)                       # step 1, per tile tensor
        idx = np.nonzero(passed)[0]
        cx, cy, w, h = (box[idx, k] for k in range(4))
        b = np.stack([cx - w * half, cy - h * half, cx + w * half, cy + h * half], axis=1).astype(np.float32).reshape(-1, 4)
        tile.append(np.full(len(idx), t)); anchor.append(idx); cls.append(c[idx]); cf.append(f[idx])
        xyxy.append(to_frame(b, geos[t]).reshape(-1, 4))                                        # steps 3 and 3b
    tile, anchor, cls, cf, xyxy = (np.concatenate(v) for v in (tile, anchor, cls, cf, xyxy))
    n_pass = len(tile)
    order = np.lexsort((anchor, -tile if tiles_high_first else tile, -cf))[:max_candidates]     # conf descending, tile, anchor ascending
    cls, cf, xyxy = cls[order], cf[order], xyxy[order]
    kept = []
    for i in range(len(order)):
        if kept:
            k = np.array(kept)
            hit = suppresses(xyxy[k], xyxy[i], iou, merge, nms_ge)
            if not agnostic:
                hit &= cls[k] == cls[i]
            if hit.any():
                continue
        kept.append(i)
    counters = np.array([n_pass, len(order), len(kept)], dtype=np.int32)
    kept = kept[:max_det]
    rows = np.zeros((len(kept), 6), dtype=np.float32)
    if kept:
        rows[:, :4] = xyxy[kept]
        rows[:, 4] = cf[kept]
        rows[:, 5] = cls[kept].astype(np.float32)
    return rows, counters


# ---------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    preds: np.ndarray           # (S * T, 4 + nc, A) or (S * T, A, 5 + nc)
    geos: list                  # [S][T] of (gain, top, left, x0, y0, w, h)
    layout: str
    opts: dict                  # conf, iou, max_det, max_candidates, agnostic, classes, merge
    stride: int                 # rows per stream of the output block (>= max_det)

    @property
    def dims(self):             # S, T, A, nc
        s, T = self.preds.shape, len(self.geos[0])
        return (s[0] // T, T, s[2], s[1] - 4) if self.layout == "cn" else (s[0] // T, T, s[1], s[2] - 5)


def geo_of(rect, size=(64, 64), mode="center"):
    x0, y0, w, h = rect
    gain, _, _, top, left = letterbox_ref.geometry(h, w, size, mode)
    return (gain, top, left, x0, y0, w, h)


T = 3
# stream geometries: a 128 x 192 frame as the whole frame (gain 1 / 3: the division rounds; bars above and below) and two 128 x 128
# halves that overlap by 64 columns (gain 1 / 2: exact arithmetic); a 100 x 150 frame as the whole frame (gain 64 / 150, "topleft")
# and two unit-gain 64 x 64 corners
GEO_A = [geo_of((0, 0, 192, 128)), geo_of((0, 0, 128, 128)), geo_of((64, 0, 128, 128))]
GEO_B = [geo_of((0, 0, 150, 100), mode="topleft"), geo_of((0, 0, 64, 64)), geo_of((86, 36, 64, 64))]
TILE_UNIT = (1.0, 0, 0, 0, 0, 640, 640)         # T = 1: the untiled DetPost's GEO_UNIT


def in_tile(det, geo):
    """a frame-space detection (cx, cy, w, h, conf, cls) as the tile's detector would report it, in the tile's letterbox pixels"""
    gain, top, left, x0, y0 = geo[:5]
    return ((det[0] - x0) * gain + left, (det[1] - y0) * gain + top, det[2] * gain, det[3] * gain, det[4], det[5])


def pack_tiles(per_tile, A, nc, layout, dtype, seed, where=None):
    """(T, ...) tensors of one stream: ``per_tile[t]`` planted into tile t (detpost_ref.pack: sub-threshold clutter elsewhere)"""
    return np.stack([detpost_ref.pack(d, A, nc, layout, dtype, seed + 10 * t, None if where is None else where[t]) for t, d in enumerate(per_tile)])


def small_boxes(pred, layout):
    """detpost_ref.random_pred's boxes (made for a 640 x 640 input) at a tenth of their size: inside a 64 x 64 input"""
    p = pred.copy()
    if layout == "cn":
        p[:4] = (p[:4].astype(np.float32) * F(0.1)).astype(p.dtype)
    else:
        p[:, :4] = (p[:, :4].astype(np.float32) * F(0.1)).astype(p.dtype)
    return p


def _opts(**kw):
    return dict(dict(conf=0.25, iou=0.45, max_det=32, max_candidates=64, agnostic=False, classes=None, merge="iou"), **kw)


def grid_dets(n):
    """n frame-space detections of stream A's geometry with distinct confs in order, on a grid of disjoint 8 x 8 boxes, 10 to a row
    -- the left five columns are reported by tile 1, the right five by tile 2 -- except that every seventh from the 66th on repeats
    the box 66 places earlier, one pixel off and from whichever tile its own column belongs to: suppressions that cross an NMS chunk
    seam and a tile boundary.  Returns per tile the detections in the tile's letterbox pixels."""
    per = [[], [], []]
    for i in range(n):
        j = i - 66 if (i >= 66 and i % 7 == 3) else i
        det = (8 + 12 * (j % 10) + (i != j), 8 + 12 * (j // 10), 8, 8, 0.9 - i * 0.004, i % 3)
        t = 1 if i % 10 < 5 else 2
        if i != j and not (GEO_A[t][3] <= det[0] - 4 and det[0] + 4 <= GEO_A[t][3] + 128):
            t = 3 - t
        per[t].append(in_tile(det, GEO_A[t]))
    return per


def _build_cases():
    f16, f32 = np.float16, np.float32
    C = []

    def add(name, preds, geos, layout, stride=None, **kw):
        o = _opts(**kw)
        C.append(Case(name, np.ascontiguousarray(np.concatenate(preds)), list(geos), layout, o, stride or o["max_det"] + 3))

    # one object reported by two tiles (and, less sure, by the whole frame), kept once; stream B: by the whole frame and a corner
    obj_a = (90, 50, 40, 40, 0.9, 1)
    obj_b = (30, 30, 20, 24, 0.8, 2)
    far = (170, 100, 20, 20, 0.7, 0)
    a = [[in_tile(obj_a[:4] + (0.6, 1), GEO_A[0]), in_tile(far, GEO_A[0])], [in_tile(obj_a, GEO_A[1])], [in_tile(obj_a[:4] + (0.85, 1), GEO_A[2])]]
    b = [[in_tile(obj_b[:4] + (0.5, 2), GEO_B[0])], [in_tile(obj_b, GEO_B[1])], [in_tile((120, 70, 16, 16, 0.6, 0), GEO_B[2])]]
    for layout, dt in (("cn", f32), ("nc_obj", f16)):
        add(f"one_object_two_tiles_{layout}_{np.dtype(dt).name}", [pack_tiles(a, 64, 3, layout, dt, 100), pack_tiles(b, 64, 3, layout, dt, 200)],
            [GEO_A, GEO_B], layout)
    # a box cut by a tile's edge to 40 % of the whole box: frame box x 25..90, y 20..60 seen whole by tile 1 and from x = 64 on by
    # tile 2 (26 of 65 columns): IoU = 0.4 exactly, IOS = 1; at iou = 0.45 two rows under "iou", one under "ios".  Exact in fp16 too.
    whole, cut = (57.5, 40, 65, 40, 0.9, 0), (77, 40, 26, 40, 0.8, 0)
    c = [[], [in_tile(whole, GEO_A[1])], [in_tile(cut, GEO_A[2])]]
    cb = [[], [in_tile((32, 32, 40, 30, 0.9, 1), GEO_B[1])], []]
    for merge in ("iou", "ios"):
        add(f"cut_box_merge_{merge}", [pack_tiles(c, 65, 3, "cn", f16, 300), pack_tiles(cb, 65, 3, "cn", f16, 400)], [GEO_A, GEO_B], "cn", merge=merge)
    # ... and with the threshold AT the cut box's IOS of exactly 1: `>` keeps both rows (a `>=` would drop the second)
    add("cut_box_ios_exactly_at_the_threshold", [pack_tiles(c, 65, 3, "cn", f16, 300), pack_tiles(cb, 65, 3, "cn", f16, 400)], [GEO_A, GEO_B], "cn", merge="ios",
        iou=1.0)
    # equal confidences in different tiles: tile order decides which of two overlapping boxes is kept (the anchors are in the other
    # order); stream B: three equal confidences, one per tile
    e = [[], [in_tile((100, 60, 30, 30, 0.5, 1), GEO_A[1])], [in_tile((102, 60, 30, 30, 0.5, 1), GEO_A[2])]]
    eb = [[in_tile((30, 30, 20, 20, 0.5, 0), GEO_B[0])], [in_tile((31, 30, 20, 20, 0.5, 0), GEO_B[1])], [in_tile((120, 70, 16, 16, 0.5, 0), GEO_B[2])]]
    add("equal_conf_tile_order_decides", [pack_tiles(e, 64, 3, "cn", f32, 500, where=[[], [40], [3]]), pack_tiles(eb, 64, 3, "cn", f32, 600, where=[[9], [5], [1]])],
        [GEO_A, GEO_B], "cn")
    # more than K = 64 anchors pass across the tiles, confs in steps of 1 / 8: the ties at the K-th key straddle a tile boundary (the seed is
    # one at which the ties TAKEN come from more than one tile in both streams: tests/test_tiles_host.py checks it)
    for layout, dt, A in (("cn", f16, 100), ("nc_obj", f32, 300)):
        add(f"topk_ties_straddle_tiles_{layout}_A{A}",
            [np.stack([small_boxes(detpost_ref.random_pred(A, 3, layout, dt, 705 + 7 * s + t, 1.0, steps=8, n_obj=A // 8), layout) for t in range(T)])
             for s in range(2)],
            [GEO_A, GEO_B], layout, conf=0.2 if layout == "cn" else 0.0, max_det=64)
    # the same box from two tiles in different classes: class-aware keeps both, agnostic one
    k = [[], [in_tile((100, 60, 30, 30, 0.9, 0), GEO_A[1])], [in_tile((100, 60, 30, 30, 0.8, 2), GEO_A[2]), in_tile((150, 30, 20, 20, 0.7, 1), GEO_A[2])]]
    for agn in (False, True):
        add("classes_agnostic" if agn else "classes_kept_apart", [pack_tiles(k, 64, 3, "nc_obj", f32, 800), pack_tiles(b, 64, 3, "nc_obj", f32, 900)],
            [GEO_A, GEO_B], "nc_obj", agnostic=agn)
    # a tile with nothing passing (stream A's tile 1, stream B's tiles 0 and 2), and a stream with nothing at all
    n = [[in_tile(far, GEO_A[0])], [], [in_tile(obj_a, GEO_A[2])]]
    add("a_tile_with_nothing", [pack_tiles(n, 257, 3, "cn", f16, 1000), pack_tiles([[], [in_tile(obj_b, GEO_B[1])], []], 257, 3, "cn", f16, 1100)],
        [GEO_A, GEO_B], "cn")
    add("a_stream_with_nothing", [pack_tiles([[], [], []], 64, 3, "cn", f32, 1200), pack_tiles(b, 64, 3, "cn", f32, 1300)], [GEO_A, GEO_B], "cn")
    # boxes reaching beyond their tile -- over its left, right, top and bottom edges, into the letterbox bars of the whole frame --
    # are clipped to the tile BEFORE the NMS: the clipped box of tile 2 (frame x 64..84) lies inside tile 1's box of the same object
    # (x 30..84), IOS 1 where the unclipped one (x 30..84 too) would have IoU 1 -- and IoU 20 / 54 < 0.45 clipped: two rows under
    # "iou".  Given directly in letterbox pixels.
    p = [[(32, 5, 40, 20, 0.6, 0), (60, 50, 30, 20, 0.55, 1)],                # over the top bar / over the right edge and into the bottom bar
         [(28.5, 30, 27, 20, 0.9, 2), (2, 60, 10, 12, 0.5, 1)],               # frame x 30..84 | over the left and bottom edges
         [(-3.5, 30, 27, 20, 0.8, 2), (62, 2, 10, 10, 0.5, 0)]]               # frame x 30..84 before the clip, 64..84 after | over right and top
    pb = [[(70, 50, 30, 40, 0.9, 0)], [(60, 60, 20, 20, 0.8, 1)], [(0, 0, 20, 20, 0.7, 2)]]
    for merge in ("iou", "ios"):
        add(f"clip_to_the_tile_{merge}", [pack_tiles(p, 127, 3, "cn", f32, 1400), pack_tiles(pb, 127, 3, "cn", f32, 1500)], [GEO_A, GEO_B], "cn", merge=merge)
    # max_det cuts the rows while counter 2 counts on; > 64 candidates: suppressions across an NMS chunk seam and a tile boundary
    add("max_det_cuts_counter_2_does_not", [pack_tiles(grid_dets(100), 128, 3, "cn", f32, 1600), pack_tiles(b, 128, 3, "cn", f32, 1700)], [GEO_A, GEO_B], "cn",
        max_det=10, max_candidates=128, stride=12)
    add("seam_129_candidates_nc_obj_f16", [pack_tiles(grid_dets(129), 128, 3, "nc_obj", f16, 1800), pack_tiles(b, 128, 3, "nc_obj", f16, 1900)], [GEO_A, GEO_B],
        "nc_obj", max_det=130, max_candidates=256, stride=131)
    return C


CASES = _build_cases()
NAMES = [c.name for c in CASES]
_WANT = {}


def want(k, **wrong):
    """per stream (rows, counters) of CASES[k], computed once; treat as read-only"""
    key = (k, tuple(sorted(wrong.items())))
    if key not in _WANT:
        c = CASES[k]
        S, T_, _, _ = c.dims
        _WANT[key] = [detpost_tiled(c.preds[s * T_:(s + 1) * T_], c.geos[s], c.layout, **c.opts, **wrong) for s in range(S)]
    return _WANT[key]


# T = 1, unit gain, no padding, boxes inside the frame: the rows of the untiled DetPost (cases of detpost_ref, stream 0 only)
IDENTITY = ["more_survivors_than_max_det", "chain_frees_the_third", "classes_kept_apart", "argmax_and_conf_ties", "seam_129_obj_f16"]
