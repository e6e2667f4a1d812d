"""NumPy restatement of the ORIENTED detection post-processing definition (boxmot_amd/csrc/det_post_obb.hpp, steps 1-6), written
from the definition and not from the kernel, and the table of cases the emulated and the device kernels are compared with.

    rows, counters = detpost_obb(pred, geo, ...)             # one stream

``pred``: (4 + nc + 1, A), float16 or float32, the angle in the last row.  ``geo``: (gain, top, left, rows, cols).  ``rows``: (n, 7)
float32 [cx, cy, w, h, angle, conf, cls] in frame coordinates, ``counters``: int32 (passed, candidates, kept by NMS).

Every exactly computed quantity (score, selection, the emitted row) is float32, as on the device.  ProbIoU goes through cos, sin,
log and exp, which differ by units in the last place between NumPy, the CPU-thread emulation and the device: it is computed both in
float32 and in float64, the DECISIONS use float64, and every case has to satisfy ``check_margin``: no pair the NMS could compare lies
within MARGIN of the threshold, and float32 and float64 agree to FP32_ERR.  With that the decisions are the same in every
arithmetic, and rows, counts and counters can be compared bit for bit.

``angle_row`` and ``nms_gt`` make the two WRONG references (the angle read from channel 4; ``>`` in the NMS test) the tests use as
controls."""
from typing import NamedTuple

import numpy as np

from detpost_ref import GEO_CENTER, GEO_TALL, GEO_TOPLEFT, GEO_UNIT, geo_of, score

F = np.float32
MARGIN = 2e-3                   # no comparable pair may have |iou64 - iou_thres| below this
FP32_ERR = 2e-4                 # max |iou32 - iou64| over the comparable pairs
NMS_MODES = ("greedy", "fast")


def gaussians(box, angle, dtype):
    """step 3: (x, y, A, B, C) columns of the (n, 4) cxcywh boxes and (n,) angles, in ``dtype`` arithmetic from the float32 inputs"""
    t = np.dtype(dtype).type
    x, y, w, h = (np.asarray(box[:, k], dtype=np.float32).astype(dtype) for k in range(4))
    ang = np.asarray(angle, dtype=np.float32).astype(dtype)
    a, b = w * w / t(12), h * h / t(12)
    c, s = np.cos(ang), np.sin(ang)
    c2, s2 = c * c, s * s
    return np.stack([x, y, a * c2 + b * s2, a * s2 + b * c2, ((a - b) * c) * s], axis=1).astype(dtype)


def probiou(g1, g2):
    """step 4: ProbIoU of the earlier candidates g1 and the later ones g2 ((..., 5) tables that broadcast), in their own dtype"""
    t = g1.dtype.type
    eps = t(F(1e-7))
    x1, y1, a1, b1, c1 = (g1[..., k] for k in range(5))
    x2, y2, a2, b2, c2 = (g2[..., k] for k in range(5))
    with np.errstate(all="ignore"):
        den = (a1 + a2) * (b1 + b2) - (c1 + c2) * (c1 + c2)
        t1 = (((a1 + a2) * ((y1 - y2) * (y1 - y2)) + (b1 + b2) * ((x1 - x2) * (x1 - x2))) / (den + eps)) * t(0.25)
        t2 = ((((c1 + c2) * (x2 - x1)) * (y1 - y2)) / (den + eps)) * t(0.5)
        t3 = np.log(den / (t(4) * np.sqrt(np.fmax(a1 * b1 - c1 * c1, t(0)) * np.fmax(a2 * b2 - c2 * c2, t(0))) + eps) + eps) * t(0.5)
        bd = np.fmin(np.fmax(t1 + t2 + t3, eps), t(100))
        return t(1) - np.sqrt(t(1) - np.exp(-bd) + eps)


class Pairs(NamedTuple):
    order: np.ndarray           # the candidates' anchors, in order
    cls: np.ndarray             # per anchor
    conf: np.ndarray            # per anchor
    n_pass: int
    sup: np.ndarray             # (n, n) bool: sup[j, i], j < i: "j suppresses i" (classes included)
    margin: float               # min |iou64 - iou_thres| over the comparable pairs (inf when there is none)
    err32: float                # max |iou32 - iou64| over them


def pairs(pred, conf=0.25, iou=0.45, max_candidates=1024, agnostic=False, classes=None, angle_row=None, nms_gt=False, **_):
    """steps 1-4 of one stream: the candidates and who suppresses whom, decided in float64, with the margins of those decisions"""
    p = np.asarray(pred).astype(np.float32)             # (fp16 widens exactly)
    nc = p.shape[0] - 5
    box, angle = p[:4].T, p[-1 if angle_row is None else angle_row]
    cls, cf, passed = score(p[:4 + nc], "cn", conf, classes)
    passed = passed & np.isfinite(p[-1])                # a NaN or +-inf angle never passes
    idx = np.nonzero(passed)[0]
    order = idx[np.lexsort((idx, -cf[idx]))][:max_candidates]       # conf descending, anchor ascending
    n = len(order)
    g64, g32 = gaussians(box[order], angle[order], np.float64), gaussians(box[order], angle[order], np.float32)
    thr = np.float64(F(iou))
    sup = np.zeros((n, n), dtype=bool)
    margin, err32 = np.inf, 0.0
    for j0 in range(0, n, 256):                         # rows j0 .. j1 of the upper triangle, a block at a time
        j1 = min(j0 + 256, n)
        i64 = probiou(g64[j0:j1, None, :], g64[None, :, :])
        i32 = probiou(g32[j0:j1, None, :], g32[None, :, :])
        can = np.arange(j0, j1)[:, None] < np.arange(n)[None, :]
        if not agnostic:
            can &= cls[order[j0:j1]][:, None] == cls[order][None, :]
        with np.errstate(invalid="ignore"):
            sup[j0:j1] = can & ((i64 > thr) if nms_gt else (i64 >= thr))
        if can.any():
            margin = min(margin, float(np.abs(i64[can] - thr).min()))
            err32 = max(err32, float(np.abs(i32[can].astype(np.float64) - i64[can]).max()))
    return Pairs(order, cls, cf, len(idx), sup, margin, err32)


def nms(sup, mode):
    """step 5: the kept candidates' positions"""
    n = len(sup)
    if mode == "fast":
        return [i for i in np.nonzero(~sup.any(axis=0))[0]]
    assert mode == "greedy", mode
    alive = np.ones(n, dtype=bool)
    kept = []
    for i in range(n):
        if alive[i]:
            kept.append(i)
            alive &= ~sup[i]
    return kept


def regularized(w, h, angle):
    """step 6's regularisation of float32 columns"""
    swap = h > w
    w, h = np.where(swap, h, w), np.where(swap, w, h)
    angle = np.where(swap, angle + F(np.pi / 2), angle).astype(np.float32)
    angle = np.fmod(angle, F(np.pi)).astype(np.float32)
    angle = np.where(angle < 0, angle + F(np.pi), angle).astype(np.float32)
    return w, h, angle


def detpost_obb(pred, geo, conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False, classes=None, nms_mode="greedy",
                regularize=False, angle_row=None, nms_gt=False, found=None):
    """``found``: what ``pairs`` gave for the same arguments, to save computing it again"""
    pr = found or pairs(pred, conf, iou, max_candidates, agnostic, classes, angle_row, nms_gt)
    kept = nms(pr.sup, nms_mode)
    counters = np.array([pr.n_pass, len(pr.order), len(kept)], dtype=np.int32)
    at = pr.order[kept[:max_det]]
    p = np.asarray(pred).astype(np.float32)
    gain, top, left = F(geo[0]), F(geo[1]), F(geo[2])
    cx, cy, w, h = (p[k, at] for k in range(4))
    angle = p[-1 if angle_row is None else angle_row, at]
    if regularize:
        w, h, angle = regularized(w, h, angle)
    rows = np.stack([(cx - left) / gain, (cy - top) / gain, w / gain, h / gain, angle, pr.conf[at], pr.cls[at].astype(np.float32)], axis=1)
    return rows.astype(np.float32).reshape(-1, 7), counters


# ---------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    preds: np.ndarray           # (S, 4 + nc + 1, A)
    geos: list                  # per stream (gain, top, left, rows, cols)
    opts: dict                  # conf, iou, max_det, max_candidates, agnostic, classes, nms_mode, regularize
    stride: int                 # rows per stream of the output block (>= max_det)

    @property
    def dims(self):             # S, A, nc
        s = self.preds.shape
        return s[0], s[2], s[1] - 5


GEO_WIDE = geo_of(300, 500, (64, 64))                   # bars above and below, gain 0.128


def pack(dets, A, nc, dtype, seed=0, where=None):
    """One stream's tensor with the detections ``dets`` = [(cx, cy, w, h, angle, conf, cls)] planted at the anchors ``where``
    (default: a seeded permutation) and sub-threshold clutter (scores <= 0.125) everywhere else; the other classes of a planted
    anchor get conf / 4."""
    rng = np.random.default_rng(seed)
    box = np.stack([rng.integers(0, 640, A), rng.integers(0, 640, A), rng.integers(4, 80, A), rng.integers(4, 80, A)], 1).astype(np.float32)
    ang = (rng.integers(-50, 51, A) / 32.0).astype(np.float32)
    sc = rng.integers(0, 5, (A, nc)).astype(np.float32) / F(32)
    where = rng.permutation(A)[:len(dets)] if where is None else np.asarray(where)
    for a, d in zip(where, dets):
        box[a] = d[:4]
        ang[a] = d[4]
        sc[a] = F(d[5]) / F(4)
        sc[a, int(d[6])] = d[5]
    return np.concatenate([box.T, sc.T, ang[None]], 0).astype(dtype)


def clusters(n_obj, members, nc, seed, spacing=90, confs=None):
    """n_obj objects far apart (ProbIoU between two of them is ~ 0), sides 8..80 px with an aspect ratio <= 8, each with ``members``
    detections: near-duplicates (a jitter of a fraction of a pixel and of a degree: ProbIoU ~ 0.9 and more), links of a chain -- the
    object moved by 0.3 and by 0.6 of its short side, where ProbIoU is ~ 0.65 and ~ 0.35 -- and the object turned by a right angle.
    Confidences are distinct unless ``confs`` gives them."""
    rng = np.random.default_rng(seed)
    per_row = max(1, 640 // spacing)
    out = []
    for o in range(n_obj):
        cx, cy = 40 + spacing * (o % per_row), 40 + spacing * (o // per_row)
        short = float(rng.integers(8, 41))
        long_ = float(min(80, short * rng.integers(1, 9)))
        w, h = (long_, short) if rng.random() < 0.5 else (short, long_)
        ang = float(rng.integers(-48, 49)) / 32.0
        cls = int(rng.integers(0, nc))
        for m in range(members):
            kind = int(rng.integers(0, 6)) if m else 0
            dx = dy = 0.0
            a = ang
            if kind in (1, 2):                          # a link of the chain, along the box's own axes' diagonal
                dx, dy = (0.3 * kind * short * np.cos(ang + 0.7), 0.3 * kind * short * np.sin(ang + 0.7))
            elif kind == 3:
                a = ang + float(np.pi / 2)
            jit = rng.integers(-2, 3, 2) / 8.0
            out.append((cx + dx + jit[0], cy + dy + jit[1], w, h, a + float(rng.integers(-2, 3)) / 256.0, 0.0,
                        cls if rng.random() < 0.85 else int(rng.integers(0, nc))))
    n = len(out)
    cf = (0.3 + 0.69 * rng.permutation(n) / max(n - 1, 1)) if confs is None else confs(rng, n)
    return [d[:5] + (float(c),) + d[6:] for d, c in zip(out, cf)]


def _opts(**kw):
    return dict(dict(conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False, classes=None, nms_mode="greedy", regularize=False), **kw)


def check_margin(c):
    """(min margin, max float32 error) over the streams of a case"""
    found = [_pairs_of(c, s) for s in range(len(c.preds))]
    return min(f.margin for f in found), max(f.err32 for f in found)


_PAIRS = {}


def _pairs_of(c, s, **wrong):
    key = (c.name, s, tuple(sorted(wrong.items())))
    if key not in _PAIRS:
        _PAIRS[key] = pairs(c.preds[s], **dict(c.opts, **wrong))
    return _PAIRS[key]


HALF_PI = float(np.pi / 2)
# the hand-worked table: two identical boxes (ProbIoU 1 - sqrt(2e-7)), one far away (~ 0), and a cross of two 40 x 10 boxes with one
# centre and perpendicular angles (1 - sqrt(9 / 17) = 0.2724: both stay at 0.45)
TABLE = [(100, 100, 40, 20, 0.5, 0.9, 0), (100, 100, 40, 20, 0.5, 0.8, 0), (400, 300, 30, 30, 0.0, 0.7, 0),
         (250, 500, 40, 10, 0.0, 0.6, 0), (250, 500, 40, 10, HALF_PI, 0.5, 0)]
# a chain: ProbIoU(a, b) = ProbIoU(b, c) ~ 0.64, ProbIoU(a, c) ~ 0.35: greedy keeps c (b is gone), fast drops it; d stands apart
CHAIN = [(100, 100, 40, 40, 0.25, 0.9, 0), (112, 100, 40, 40, 0.25, 0.8, 0), (124, 100, 40, 40, 0.25, 0.7, 0), (300, 100, 40, 40, 0.25, 0.6, 0)]
TWO = [(200, 200, 60, 20, 0.5, 0.9, 0), (200, 200, 60, 20, 0.5, 0.8, 2), (201, 200, 60, 20, 0.5, 0.7, 0), (400, 100, 30, 12, -0.5, 0.6, 1)]
# h > w, a negative angle, an angle >= pi, one that needs nothing, and h > w with an angle that passes pi after the quarter turn
REG = [(100, 100, 10, 40, 0.5, 0.9, 0), (200, 100, 40, 10, -0.75, 0.8, 0), (300, 100, 40, 10, 3.5, 0.7, 0), (400, 100, 40, 10, 1.0, 0.6, 0),
       (500, 100, 10, 40, 2.0, 0.55, 0), (100, 300, 10, 40, -2.0, 0.5, 0)]


def _build_cases():
    f16, f32 = np.float16, np.float32
    C = []

    def add(name, preds, geos, stride=None, **kw):
        o = _opts(**kw)
        c = Case(name, np.ascontiguousarray(np.stack(preds)), list(geos), o, stride or o["max_det"] + 3)
        C.append(c)
        return c

    def add_sampled(name, make, geos, stride=None, **kw):
        """``make(seed)`` -> the streams' tensors: the first seed whose candidates keep the margin"""
        for seed in range(40):
            c = Case(name, np.ascontiguousarray(np.stack(make(seed))), list(geos), _opts(**kw), stride or _opts(**kw)["max_det"] + 3)
            m, e = check_margin(c)
            if m >= MARGIN and e <= FP32_ERR:
                C.append(c)
                return c
            for s in range(len(c.preds)):
                _PAIRS.pop((name, s, ()), None)
        raise AssertionError(f"{name}: no seed keeps the margin")

    add("hand_worked_table", [pack(TABLE, 63, 1, f32, 1)], [GEO_UNIT], max_det=8)
    for mode in NMS_MODES:
        add(f"chain_{mode}", [pack(CHAIN, 64, 1, f32, 2)], [GEO_UNIT], max_det=8, nms_mode=mode)
    add("classes_kept_apart", [pack(TWO, 64, 3, f16, 3)], [GEO_UNIT], max_det=8)
    add("classes_agnostic", [pack(TWO, 64, 3, f16, 3)], [GEO_UNIT], max_det=8, agnostic=True)
    add_sampled("allow_list_nc15", lambda seed: [pack(clusters(12, 4, 15, seed), 257, 15, f16, seed), pack(TWO, 257, 15, f16, 4)],
                [GEO_CENTER, GEO_UNIT], max_det=32, classes=[0, 2, 7, 14])
    # the angle is the LAST row: channel 4 is the first class's score (a reference that reads the angle there differs)
    add("angle_in_the_last_row", [pack(TWO + [(500, 400, 60, 8, 1.25, 0.5, 1), (500, 400, 60, 8, -0.3, 0.4, 1)], 63, 3, f32, 5)], [GEO_UNIT], max_det=8)
    # NaN, +inf and -inf angles on the three best anchors: they never pass; wide (A = 64, fp16) and narrow (A = 63, fp32) score kernel
    for A, dt in ((64, f16), (63, f32)):
        bad = pack(CHAIN + [(500, 500, 20, 20, 0.0, 0.95, 0), (520, 500, 20, 20, 0.0, 0.94, 0), (540, 500, 20, 20, 0.0, 0.93, 0)], A, 1, dt, 6,
                   where=[3, 9, 17, 30, 0, 33, A - 1])
        bad[-1, [0, 33, A - 1]] = [np.nan, np.inf, -np.inf]
        add(f"non_finite_angle_A{A}_{np.dtype(dt).name}", [bad], [GEO_UNIT], max_det=8)
    # more than K pass, with ties across the K boundary: confs in steps of 1 / 8
    add_sampled("all_pass_A600_K64_ties_at_K",
                lambda seed: [pack(clusters(150, 4, 3, seed, spacing=48, confs=lambda rng, n: rng.integers(3, 9, n) / 8.0), 600, 3, f16, seed)],
                [GEO_UNIT], max_candidates=64, max_det=64)
    # ~ 200 candidates: several 64-chunks and the cross-chunk path, in both modes
    for mode in NMS_MODES:
        for A, dt in ((600, f16), (257, f32)):
            add_sampled(f"clusters_200_{mode}_A{A}_{np.dtype(dt).name}", lambda seed, A=A, dt=dt: [pack(clusters(40, 5, 3, seed), A, 3, dt, seed)],
                        [GEO_UNIT], nms_mode=mode, max_det=128, stride=130)
    add_sampled("more_survivors_than_max_det", lambda seed: [pack(clusters(40, 5, 3, seed), 257, 3, f32, seed)], [GEO_UNIT], max_det=10, stride=12)
    # three streams, three geometries (bars left and right; above and below with gain 1 / 3; above and below with gain 0.128); the
    # first detection of each stream has its centre in the padding: it is emitted outside the frame, unclipped
    add_sampled("three_geometries_unclipped", lambda seed: [
        pack([(3, 30, 20, 8, 0.5, 0.9, 0), (40, 30, 12, 18, 0.25, 0.8, 1)] + clusters(4, 3, 3, seed, spacing=16)[:10], 63, 3, f32, seed),
        pack([(320, 20, 60, 30, 1.0, 0.9, 0)] + clusters(20, 3, 3, seed + 1), 63, 3, f32, seed + 1),
        pack([(30, 4, 20, 6, -0.5, 0.9, 2), (30, 40, 10, 10, 0.0, 0.8, 0)], 63, 3, f32, seed + 2)], [GEO_TALL, GEO_CENTER, GEO_WIDE], max_det=16)
    add("regularize", [pack(REG, 63, 1, f32, 7), pack(REG, 63, 1, f32, 8)], [GEO_UNIT, GEO_TOPLEFT], max_det=8, regularize=True)
    add("regularize_off", [pack(REG, 63, 1, f32, 7)], [GEO_UNIT], max_det=8)

    # K = 4096: the largest LDS table.  4504 anchors on a 9-pixel grid with sides 2..5 px (neighbours: ProbIoU < 0.01); every fifth
    # repeats the one before it a quarter of a pixel off
    def big(seed):
        rng = np.random.default_rng(seed)
        A = 4504
        k = np.arange(A)
        k = np.where(k % 5 == 4, k - 1, k)
        box = np.stack([12 + 9 * (k % 68) + 0.25 * (np.arange(A) % 5 == 4), 12 + 9 * (k // 68), rng.integers(2, 6, A)[k], rng.integers(2, 6, A)[k]], 1)
        ang = (rng.integers(-48, 49, A) / 32.0)[k]
        cf = rng.integers(300, 1000, A) / 1000.0
        return [np.concatenate([box.T, cf[None], ang[None]], 0).astype(f16)]
    add_sampled("K4096_A4504", big, [GEO_UNIT], max_candidates=4096, max_det=300, stride=300)
    return C


CASES = _build_cases()
NAMES = [c.name for c in CASES]
_WANT = {}


def want(k, **wrong):
    """per stream (rows, counters) of CASES[k], computed once; treat as read-only"""
    key = (k, tuple(sorted(wrong.items())))
    if key not in _WANT:
        c = CASES[k]
        _WANT[key] = [detpost_obb(c.preds[s], c.geos[s], **c.opts, **wrong, found=_pairs_of(c, s, **wrong)) for s in range(len(c.preds))]
    return _WANT[key]
