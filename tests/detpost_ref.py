"""NumPy float32 restatement of the detection post-processing definition (boxmot_amd/csrc/det_post.hpp, steps 1-6), written from
the definition and not from the kernels, and the table of cases the emulated and the device kernels are compared with, bit for bit.

    rows, counters = detpost(pred, geo, layout, ...)         # one stream

``pred``: (4 + nc, A) for layout "cn", (A, 5 + nc) for "nc_obj", float16 or float32.  ``geo``: (gain, top, left, rows, cols).
``rows``: (n, 6) float32 [x1, y1, x2, y2, conf, cls] in frame coordinates, ``counters``: int32 (passed, candidates, kept by NMS).
``nms_ge`` and ``ties_high_first`` make the two WRONG references (``>=`` in the NMS test; conf ties to the higher anchor index) the
tests use as controls."""
from typing import NamedTuple

import numpy as np

import letterbox_ref

F = np.float32
LAYOUTS = {"cn": 0, "nc_obj": 1}


def split(pred, layout):
    """float32 (A, 4) boxes cxcywh, (A, nc) scores, (A,) obj or None"""
    p = np.asarray(pred).astype(np.float32)            # (fp16 widens exactly)
    if layout == "cn":
        return p[:4].T, p[4:].T, None
    return p[:, :4], p[:, 5:], p[:, 4]


def score(pred, layout, conf_thres, classes=None):
    """step 1: (cls, conf, passed) per anchor"""
    _, sc, obj = split(pred, layout)
    sc = np.where(np.isnan(sc), F(-np.inf), sc)         # a NaN score is never the maximum
    cls = np.argmax(sc, axis=1)                         # (the first of equal maxima)
    best = sc[np.arange(len(sc)), cls]
    with np.errstate(invalid="ignore"):
        conf = best if obj is None else (obj * best).astype(np.float32)
        passed = conf > F(conf_thres)                   # strictly; NaN compares false
    if classes is not None:
        allow = np.zeros(sc.shape[1], dtype=bool)
        allow[list(classes)] = True
        passed &= allow[cls]
    return cls, conf, passed


def suppresses(kept_boxes, b, iou_thres, ge=False):
    """which of the (n, 4) float32 xyxy boxes suppress box b"""
    with np.errstate(invalid="ignore", divide="ignore"):
        area_k = (kept_boxes[:, 2] - kept_boxes[:, 0]) * (kept_boxes[:, 3] - kept_boxes[:, 1])
        area_b = (b[2] - b[0]) * (b[3] - b[1])
        iw = np.fmax(np.fmin(b[2], kept_boxes[:, 2]) - np.fmax(b[0], kept_boxes[:, 0]), F(0))
        ih = np.fmax(np.fmin(b[3], kept_boxes[:, 3]) - np.fmax(b[1], kept_boxes[:, 1]), F(0))
        inter = iw * ih
        iou = inter / (area_b + area_k - inter)
        return iou >= F(iou_thres) if ge else iou > F(iou_thres)


def to_frame(xyxy, geo):
    """step 5's coordinate arithmetic on an (n, 4) float32 table"""
    gain, top, left, rows, cols = geo
    out = np.array(xyxy, dtype=np.float32, ndmin=2)
    out[:, [0, 2]] = np.clip((out[:, [0, 2]] - F(left)) / F(gain), F(0), F(cols))
    out[:, [1, 3]] = np.clip((out[:, [1, 3]] - F(top)) / F(gain), F(0), F(rows))
    return out


def detpost(pred, geo, layout="cn", conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False, classes=None,
            nms_ge=False, ties_high_first=False):
    box, _, _ = split(pred, layout)
    cls, cf, passed = score(pred, layout, conf, classes)
    idx = np.nonzero(passed)[0]
    order = idx[np.lexsort((-idx if ties_high_first else idx, -cf[idx]))][:max_candidates]       # conf descending, anchor ascending
    half = F(0.5)
    cx, cy, w, h = (box[order, k] for k in range(4))
    xyxy = np.stack([cx - w * half, cy - h * half, cx + w * half, cy + h * half], axis=1).astype(np.float32).reshape(-1, 4)
    kept = []
    for i in range(len(order)):
        if kept:
            k = np.array(kept)
            hit = suppresses(xyxy[k], xyxy[i], iou, nms_ge)
            if not agnostic:
                hit &= cls[order[k]] == cls[order[i]]
            if hit.any():
                continue
        kept.append(i)
    counters = np.array([len(idx), len(order), len(kept)], dtype=np.int32)
    kept = kept[:max_det]
    rows = np.zeros((len(kept), 6), dtype=np.float32)
    if kept:
        rows[:, :4] = to_frame(xyxy[kept], geo)
        rows[:, 4] = cf[order[kept]]
        rows[:, 5] = cls[order[kept]].astype(np.float32)
    return rows, counters


# ---------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    preds: np.ndarray           # (S, 4 + nc, A) or (S, A, 5 + nc)
    geos: list                  # per stream (gain, top, left, rows, cols)
    layout: str
    opts: dict                  # conf, iou, max_det, max_candidates, agnostic, classes
    stride: int                 # rows per stream of the output block (>= max_det)

    @property
    def dims(self):             # S, A, nc
        s = self.preds.shape
        return (s[0], s[2], s[1] - 4) if self.layout == "cn" else (s[0], s[1], s[2] - 5)


def geo_of(rows, cols, size=(640, 640), mode="center"):
    gain, _, _, top, left = letterbox_ref.geometry(rows, cols, size, mode)
    return (gain, top, left, rows, cols)


GEO_UNIT = geo_of(640, 640)                             # gain 1, no padding
GEO_CENTER = geo_of(1080, 1920)                         # gain 1 / 3 (the division rounds), bars above and below
GEO_TOPLEFT = geo_of(1080, 1920, mode="topleft")
GEO_TALL = geo_of(700, 300, (64, 64))                   # bars left and right, an upscale-free odd gain


def pack(dets, A, nc, layout, dtype, seed=0, where=None, obj=None):
    """One stream's tensor with the detections ``dets`` = [(cx, cy, w, h, conf, cls)] planted at the anchors ``where`` (default: a
    seeded permutation) and sub-threshold clutter (scores <= 0.125) everywhere else; other classes of a planted anchor get
    conf / 4.  nc_obj: obj = ``obj`` (default 1) and the class score carries conf."""
    rng = np.random.default_rng(seed)
    box = np.stack([rng.integers(0, 640, A), rng.integers(0, 640, A), rng.integers(4, 200, A), rng.integers(4, 200, A)], 1).astype(np.float32)
    sc = rng.integers(0, 5, (A, nc)).astype(np.float32) / F(32)
    where = rng.permutation(A)[:len(dets)] if where is None else np.asarray(where)
    for a, d in zip(where, dets):
        box[a] = d[:4]
        sc[a] = F(d[4]) / F(4)
        sc[a, int(d[5])] = d[4]
    if layout == "cn":
        return np.concatenate([box.T, sc.T], 0).astype(dtype)
    o = np.full((A, 1), 1.0 if obj is None else obj, dtype=np.float32)
    return np.concatenate([box, o, sc], 1).astype(dtype)


def random_pred(A, nc, layout, dtype, seed, pass_rate=0.3, steps=128, n_obj=None):
    """Clustered boxes (so NMS has work), confs quantised to 1 / steps (so ties are plentiful), every class filled; an anchor is
    'active' with probability pass_rate, the rest stay under 0.15."""
    rng = np.random.default_rng(seed)
    n_obj = n_obj or max(1, A // 12)
    obj_box = np.stack([rng.integers(40, 600, n_obj), rng.integers(40, 600, n_obj), rng.integers(16, 160, n_obj), rng.integers(16, 160, n_obj)], 1)
    which = rng.integers(0, n_obj, A)
    box = (obj_box[which] + rng.integers(-24, 25, (A, 4)) / 4.0).astype(np.float32)
    cf = rng.integers(steps // 3, steps + 1, A).astype(np.float32) / F(steps)
    cf = np.where(rng.random(A) < pass_rate, cf, cf * F(0.125)).astype(np.float32)
    cls = (which + (rng.random(A) < 0.2)) % nc                                   # mostly the object's class
    sc = cf[:, None] * (rng.integers(0, 5, (A, nc)).astype(np.float32) / F(8))
    sc[np.arange(A), cls] = cf
    tie = rng.random(A) < 0.1                                                    # a second class with the same score: argmax ties
    sc[tie, (cls[tie] + 1 + rng.integers(0, nc, tie.sum())) % nc] = cf[tie]
    if layout == "cn":
        return np.concatenate([box.T, sc.T], 0).astype(dtype)
    o = (rng.integers(4, 9, (A, 1)) / 8.0).astype(np.float32)
    return np.concatenate([box, o, sc], 1).astype(dtype)


def seam_dets(n):
    """n detections, all above 0.25 with distinct confs in order, on a grid of disjoint cells -- except that every seventh from
    the 66th on repeats the box 66 places earlier, one pixel off: a suppression that crosses an NMS chunk seam"""
    out = []
    for i in range(n):
        j = i - 66 if (i >= 66 and i % 7 == 3) else i
        out.append((20 + 40 * (j % 16) + (i != j), 20 + 40 * (j // 16), 30, 30, 0.9 - i * 0.004, i % 3))
    return out


def _opts(**kw):
    return dict(dict(conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False, classes=None), **kw)


def _build_cases():
    f16, f32 = np.float16, np.float32
    C = []

    def add(name, preds, geos, layout, stride=None, **kw):
        o = _opts(**kw)
        C.append(Case(name, np.ascontiguousarray(np.stack(preds)), list(geos), layout, o, stride or o["max_det"] + 3))

    # shapes: A in {1, 63, 64, 65, 257, 1000}, nc in {1, 3, 80}, both layouts, both dtypes
    add("one_anchor_cn_f32", [pack([(32, 32, 20, 10, 0.5, 0)], 1, 1, "cn", f32)], [GEO_TALL], "cn", max_det=8)
    add("one_anchor_below_obj_f16", [pack([(32, 32, 20, 10, 0.5, 0)], 1, 1, "nc_obj", f16, obj=0.5)], [GEO_TALL], "nc_obj", max_det=8)
    for A, nc, layout, dt in [(63, 3, "cn", f16), (64, 80, "nc_obj", f32), (65, 1, "nc_obj", f16), (257, 3, "nc_obj", f16), (257, 80, "cn", f32),
                              (1000, 3, "cn", f16), (1000, 80, "nc_obj", f16)]:
        add(f"random_A{A}_nc{nc}_{layout}_{np.dtype(dt).name}", [random_pred(A, nc, layout, dt, A + nc, 0.5), random_pred(A, nc, layout, dt, A + nc + 1, 0.9)],
            [GEO_CENTER, GEO_TOPLEFT], layout, max_det=64)
    add("random_A8400_nc80_cn_f16_topk", [random_pred(8400, 80, "cn", f16, 8400, 0.3, n_obj=60)], [GEO_CENTER], "cn", max_det=300, stride=300)
    # nothing passes / everything passes with an exact top-K overflow and ties across the K boundary (confs in steps of 1 / 8)
    add("nothing_passes", [random_pred(257, 3, "cn", f16, 5, 0.0), random_pred(257, 3, "cn", f16, 6, 0.0)], [GEO_UNIT, GEO_UNIT], "cn", max_det=16)
    add("all_pass_A300_K64_ties_at_K", [random_pred(300, 3, "cn", f16, 7, 1.0, steps=8, n_obj=150)], [GEO_UNIT], "cn", max_candidates=64, max_det=64,
        conf=0.2)
    add("all_pass_A300_K64_nc_obj", [random_pred(300, 3, "nc_obj", f16, 8, 1.0, steps=8, n_obj=150)], [GEO_UNIT], "nc_obj", max_candidates=64, max_det=64,
        conf=0.0)
    add("more_survivors_than_max_det", [pack(seam_dets(100), 257, 3, "cn", f32, 9)], [GEO_UNIT], "cn", max_det=10, stride=12)
    # exact duplicates, and a chain a ~ b ~ c: IoU(a, b) = IoU(b, c) = 7 / 13, IoU(a, c) = 1 / 4: b's suppression frees c
    dup = [(100, 100, 40, 40, 0.9, 1)] * 3 + [(300, 300, 50, 20, 0.8, 0)] * 2
    add("exact_duplicates", [pack(dup, 63, 3, "cn", f32, 10), pack(dup, 63, 3, "cn", f32, 11)], [GEO_UNIT, GEO_CENTER], "cn", max_det=8)
    chain = [(105, 105, 10, 10, 0.9, 0), (108, 105, 10, 10, 0.8, 0), (111, 105, 10, 10, 0.7, 0), (114, 105, 10, 10, 0.6, 0)]
    add("chain_frees_the_third", [pack(chain, 64, 1, "cn", f32, 12)], [GEO_UNIT], "cn", max_det=8)
    add("chain_in_obj_layout", [pack(chain, 65, 3, "nc_obj", f32, 13, obj=0.75)], [GEO_UNIT], "nc_obj", max_det=8)
    # the same boxes in different classes, class-aware and agnostic
    two = [(200, 200, 60, 60, 0.9, 0), (200, 200, 60, 60, 0.8, 2), (201, 200, 60, 60, 0.7, 0), (400, 100, 30, 30, 0.6, 1)]
    add("classes_kept_apart", [pack(two, 64, 3, "cn", f16, 14)], [GEO_UNIT], "cn", max_det=8)
    add("classes_agnostic", [pack(two, 64, 3, "cn", f16, 14)], [GEO_UNIT], "cn", max_det=8, agnostic=True)
    add("allow_list", [random_pred(257, 80, "cn", f16, 15, 0.8), pack(two, 257, 80, "cn", f16, 16)], [GEO_CENTER, GEO_UNIT], "cn", max_det=32,
        classes=[0, 2, 17, 79])
    # argmax ties (the lowest class wins), conf ties (the lowest anchor first): equal boxes far apart, fixed anchors
    tie = pack([(100 + 50 * k, 100, 20, 20, 0.5, 2) for k in range(6)], 64, 3, "cn", f32, 17, where=[40, 3, 63, 0, 17, 5])
    tie[4 + 1, [3, 17]] = 0.5                               # anchors 3 and 17: class 1 ties class 2
    add("argmax_and_conf_ties", [tie], [GEO_UNIT], "cn", max_det=4, stride=6)
    # IoU exactly 1 / 2: (0, 0, 2, 2) and (0, 0, 2, 1); strict > keeps both at 0.5
    half = [(1, 1, 2, 2, 0.9, 0), (1, 0.5, 2, 1, 0.8, 0)]
    add("iou_exactly_half_kept", [pack(half, 63, 1, "cn", f32, 18)], [GEO_UNIT], "cn", max_det=8, iou=0.5)
    add("iou_exactly_half_suppressed", [pack(half, 63, 1, "cn", f32, 18)], [GEO_UNIT], "cn", max_det=8, iou=float(np.nextafter(F(0.5), F(0))))
    # NaN scores: alone in its anchor (never passes), beside a real score (ignored), and a NaN obj
    nan = pack([(100, 100, 20, 20, 0.9, 0), (200, 100, 20, 20, 0.8, 1), (300, 100, 20, 20, 0.7, 2)], 65, 3, "cn", f32, 19, where=[1, 2, 64])
    nan[4:, 1] = np.nan
    nan[4, 2] = np.nan
    add("nan_scores", [nan], [GEO_UNIT], "cn", max_det=8)
    nano = pack([(100, 100, 20, 20, 0.9, 0), (200, 100, 20, 20, 0.8, 1)], 65, 3, "nc_obj", f16, 20, where=[0, 64])
    nano[0, 4] = np.nan
    add("nan_obj", [nano], [GEO_UNIT], "nc_obj", max_det=8)
    # boxes over the frame's edges, in both letterbox modes' geometries and with bars left and right
    edge = [(5, 150, 40, 40, 0.9, 0), (635, 400, 40, 40, 0.8, 0), (320, 130, 100, 40, 0.7, 1), (320, 505, 60, 30, 0.6, 1), (300, 355, 700, 20, 0.5, 2)]
    add("clip_to_the_frame", [pack(edge, 63, 3, "cn", f32, 21), pack(edge, 63, 3, "cn", f32, 22), pack([(3, 3, 10, 10, 0.9, 0), (50, 60, 30, 20, 0.8, 1)], 63, 3, "cn", f32, 23)],
        [GEO_CENTER, GEO_TOPLEFT, GEO_TALL], "cn", max_det=8)
    # candidate counts at the NMS chunk seams
    for n in (63, 64, 65, 129):
        add(f"seam_{n}_candidates", [pack(seam_dets(n), 257, 3, "cn", f32, 30 + n)], [GEO_UNIT], "cn", max_det=130, stride=131)
    add("seam_129_obj_f16", [pack(seam_dets(129), 257, 3, "nc_obj", f16, 40)], [GEO_UNIT], "nc_obj", max_det=130, stride=131)
    return C


CASES = _build_cases()
_WANT = {}


def want(k, **wrong):
    """per stream (rows, counters) of CASES[k], computed once; treat as read-only"""
    key = (k, tuple(sorted(wrong.items())))
    if key not in _WANT:
        c = CASES[k]
        _WANT[key] = [detpost(c.preds[s], c.geos[s], c.layout, **c.opts, **wrong) for s in range(len(c.preds))]
    return _WANT[key]
