"""NumPy float32 restatement of steps 7-8 of the detection post-processing with per-anchor extras (boxmot_amd/csrc/det_post_extra.hpp),
written from the definition and not from the kernels, and the table of cases the emulated and the device kernels are compared with,
bit for bit.

    rows, counters, extras, src = detpost_extra(pred, geo, layout, nc, E, kind, ...)              # one stream
    rows, counters, extras, src = detpost_extra_tiled(preds, geos, layout, nc, E, kind, ...)      # one stream of T tiles

``pred``: (4 + nc + E, A) for layout "cn", (A, 5 + nc + E) for "nc_obj", float16 or float32.  ``rows`` and ``counters`` come from the
EXISTING references, ``detpost_ref.detpost`` / ``detpost_tiled_ref.detpost_tiled``, run on the tensor with the extra channels cut
away: extras disturb nothing.  ``src`` (n,) int32 is restated here -- steps 1-4 once more, keeping the anchors -- and ``extras``
(n, E) float32 with ``np.fmax`` / ``np.fmin`` (a NaN coordinate comes out as 0, as fmaxf gives it).  ``candidate_order`` and
``visibility_is_a_coordinate`` make the two WRONG references the tests use as controls: the extras of the first n CANDIDATES,
ignoring what NMS dropped; the third value of a "kpt3" group mapped like an x."""
from typing import NamedTuple

import numpy as np

import detpost_ref
import detpost_tiled_ref as tiled_ref
from detpost_ref import GEO_CENTER, GEO_TALL, GEO_UNIT

F = np.float32
LAYOUTS = detpost_ref.LAYOUTS
KINDS = {"raw": 0, "kpt2": 1, "kpt3": 2}
GROUP = {"raw": 1, "kpt2": 2, "kpt3": 3}


def cut(pred, layout, nc):
    """the tensor without its extra channels: what the existing references read"""
    return pred[:4 + nc] if layout == "cn" else pred[:, :5 + nc]


def extras_of(pred, layout, nc):
    """(A, E) float32: the extra values per anchor (fp16 widens exactly)"""
    p = np.asarray(pred).astype(np.float32)
    return p[4 + nc:].T if layout == "cn" else p[:, 5 + nc:]


def kept_anchors(pred, layout, conf, iou, max_candidates, agnostic, classes):
    """steps 1-4 of det_post.hpp once more, keeping the anchors: (order, kept) -- the candidates' anchors, and which of them NMS keeps"""
    box, _, _ = detpost_ref.split(pred, layout)
    cls, cf, passed = detpost_ref.score(pred, layout, conf, classes)
    idx = np.nonzero(passed)[0]
    order = idx[np.lexsort((idx, -cf[idx]))][:max_candidates]
    half = F(0.5)
    cx, cy, w, h = (box[order, k] for k in range(4))
    xyxy = np.stack([cx - w * half, cy - h * half, cx + w * half, cy + h * half], axis=1).astype(np.float32).reshape(-1, 4)
    kept = []
    for i in range(len(order)):
        if kept:
            k = np.array(kept)
            hit = detpost_ref.suppresses(xyxy[k], xyxy[i], iou)
            if not agnostic:
                hit &= cls[order[k]] == cls[order[i]]
            if hit.any():
                continue
        kept.append(i)
    return order, kept


def map_extras(v, kind, off_x, off_y, gain, hi_x, hi_y, x0=None, y0=None, visibility_is_a_coordinate=False):
    """step 8 on an (n, E) float32 table: x through (left, cols | w, x0), y through (top, rows | h, y0), everything else copied"""
    out = np.array(v, dtype=np.float32, ndmin=2).copy()
    if kind == "raw" or out.shape[0] == 0:
        return out
    g = GROUP[kind]
    with np.errstate(invalid="ignore"):
        for comp, off, hi, origin in ((0, off_x, hi_x, x0), (1, off_y, hi_y, y0)) + (((2, off_x, hi_x, x0),) if visibility_is_a_coordinate and g == 3 else ()):
            m = np.fmin(np.fmax((out[:, comp::g] - F(off)) / F(gain), F(0)), F(hi))
            out[:, comp::g] = m if origin is None else m + F(origin)
    return out


def detpost_extra(pred, geo, layout, nc, E, kind, conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False, classes=None,
                  candidate_order=False, visibility_is_a_coordinate=False):
    assert extras_of(pred, layout, nc).shape[1] == E and E % GROUP[kind] == 0
    base = np.ascontiguousarray(cut(pred, layout, nc))
    rows, counters = detpost_ref.detpost(base, geo, layout, conf, iou, max_det, max_candidates, agnostic, classes)
    order, kept = kept_anchors(base, layout, conf, iou, max_candidates, agnostic, classes)
    assert counters.tolist()[1:] == [len(order), len(kept)]
    n = len(rows)
    src = (order[:n] if candidate_order else order[kept[:max_det]]).astype(np.int32).reshape(-1)
    assert len(src) == n
    gain, top, left, frows, fcols = geo
    extras = map_extras(extras_of(pred, layout, nc)[src].reshape(-1, E), kind, left, top, gain, fcols, frows,
                        visibility_is_a_coordinate=visibility_is_a_coordinate)
    return rows, counters, extras, src


def detpost_extra_tiled(preds, geos, layout, nc, E, kind, conf=0.25, iou=0.45, max_det=256, max_candidates=1024, agnostic=False, classes=None,
                        merge="iou", candidate_order=False, visibility_is_a_coordinate=False):
    T = len(preds)
    A = preds.shape[2] if layout == "cn" else preds.shape[1]
    base = np.ascontiguousarray(np.stack([cut(p, layout, nc) for p in preds]))
    rows, counters = tiled_ref.detpost_tiled(base, geos, layout, conf, iou, max_det, max_candidates, agnostic, classes, merge)
    # steps 1-4 of det_post_tiled.hpp once more, keeping (tile, anchor)
    half = F(0.5)
    tile, anchor, cls, cf, xyxy = [], [], [], [], []
    for t in range(T):
        box, _, _ = detpost_ref.split(base[t], layout)
        c, f, passed = detpost_ref.score(base[t], layout, conf, classes)
        idx = np.nonzero(passed)[0]
        cx, cy, w, h = (box[idx, k] for k in range(4))
        b = np.stack([cx - w * half, cy - h * half, cx + w * half, cy + h * half], axis=1).astype(np.float32).reshape(-1, 4)
        tile.append(np.full(len(idx), t)); anchor.append(idx); cls.append(c[idx]); cf.append(f[idx])
        xyxy.append(tiled_ref.to_frame(b, geos[t]).reshape(-1, 4))
    tile, anchor, cls, cf, xyxy = (np.concatenate(v) for v in (tile, anchor, cls, cf, xyxy))
    order = np.lexsort((anchor, tile, -cf))[:max_candidates]
    tile, anchor, cls, xyxy = tile[order], anchor[order], cls[order], xyxy[order]
    kept = []
    for i in range(len(order)):
        if kept:
            k = np.array(kept)
            hit = tiled_ref.suppresses(xyxy[k], xyxy[i], iou, merge)
            if not agnostic:
                hit &= cls[k] == cls[i]
            if hit.any():
                continue
        kept.append(i)
    assert counters.tolist()[1:] == [len(order), len(kept)]
    n = len(rows)
    take = np.arange(n) if candidate_order else np.array(kept[:max_det], dtype=np.int64)
    assert len(take) == n
    src = (tile[take] * A + anchor[take]).astype(np.int32).reshape(-1)
    extras = np.zeros((n, E), dtype=np.float32)
    for r in range(n):                                  # the geometry of the row's OWN tile
        t, a = int(tile[take[r]]), int(anchor[take[r]])
        gain, top, left, x0, y0, w, h = geos[t]
        extras[r] = map_extras(extras_of(preds[t], layout, nc)[a], kind, left, top, gain, w, h, x0, y0, visibility_is_a_coordinate)[0]
    return rows, counters, extras, src


# ---------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    preds: np.ndarray           # (S [* T], 4 + nc + E, A) or (S [* T], A, 5 + nc + E)
    geos: list                  # per stream (gain, top, left, rows, cols); tiled: [S][T] of (gain, top, left, x0, y0, w, h)
    layout: str
    nc: int
    E: int
    kind: str
    opts: dict                  # conf, iou, max_det, max_candidates, agnostic, classes (+ merge when tiled)
    stride: int                 # rows per stream of the output blocks (>= max_det)
    tiles: int                  # 0: untiled

    @property
    def dims(self):             # S, A
        s = self.preds.shape
        return s[0] // (self.tiles or 1), (s[2] if self.layout == "cn" else s[1])


def with_extras(base, layout, extras, dtype):
    """one tensor: ``base`` (4 + nc, A) / (A, 5 + nc) with the (A, E) ``extras`` appended"""
    return np.concatenate([base, extras.T.astype(dtype)], 0) if layout == "cn" else np.concatenate([base, extras.astype(dtype)], 1)


def make_extras(A, E, kind, seed, lo=-100, hi=800):
    """raw: values within +-8 in steps of 1 / 64; keypoints: coordinates within lo..hi in steps of 1 / 4 -- beyond the letterbox
    picture on every side, so the clip works -- and visibilities within 0..1"""
    rng = np.random.default_rng(seed)
    if kind == "raw":
        return (rng.integers(-512, 513, (A, E)) / 64.0).astype(np.float32)
    v = (rng.integers(4 * lo, 4 * hi + 1, (A, E)) / 4.0).astype(np.float32)
    if kind == "kpt3":
        v[:, 2::3] = (rng.integers(0, 65, (A, E // 3)) / 64.0).astype(np.float32)
    return v


def _opts(**kw):
    return dict(dict(conf=0.25, iou=0.45, max_det=32, max_candidates=1024, agnostic=False, classes=None), **kw)


GEOS = [GEO_UNIT, GEO_CENTER, GEO_TALL]                 # S = 3: gain 1; gain 1 / 3 (the division rounds); bars left and right


def _build_cases():
    f16, f32 = np.float16, np.float32
    C = []

    def add(name, bases, layout, nc, E, kind, dt, extras=None, geos=GEOS, tiles=0, stride=None, lo=-100, hi=800, **kw):
        """bases: per tensor the extra-less tensor; extras: per tensor an (A, E) table, default seeded random ones"""
        o = _opts(**kw)
        if tiles:
            o.setdefault("merge", "iou")
        A = bases[0].shape[1] if layout == "cn" else bases[0].shape[0]
        if extras is None:
            extras = [make_extras(A, E, kind, 7000 + 13 * len(C) + q, lo, hi) for q in range(len(bases))]
        preds = [with_extras(b.astype(dt), layout, x, dt) for b, x in zip(bases, extras)]
        C.append(Case(name, np.ascontiguousarray(np.stack(preds)), list(geos), layout, nc, E, kind, o, stride or o["max_det"] + 3, tiles))

    rp, pack = detpost_ref.random_pred, detpost_ref.pack
    # the table: both layouts x both dtypes x the four (E, kind); nc alternates; A = 100 (fp16: no multiple of 8, the narrow score
    # kernel; fp32: the wide one), 127 (narrow for both), 96, 200, 257, 320
    sizes = [96, 100, 127, 200, 257, 320]
    k = 0
    for layout in ("cn", "nc_obj"):
        for dt in (f16, f32):
            for E, kind in ((1, "raw"), (32, "raw"), (34, "kpt2"), (51, "kpt3")):
                A, nc = sizes[k % len(sizes)], (1, 3)[k % 2]
                add(f"table_A{A}_nc{nc}_{layout}_{np.dtype(dt).name}_E{E}_{kind}", [rp(A, nc, layout, dt, 100 + 3 * k + s, 0.4) for s in range(3)], layout, nc, E,
                    kind, dt)
                k += 1
    add("narrow_score_kernel_A127_cn_f16", [rp(127, 3, "cn", f16, 200 + s, 0.5) for s in range(3)], "cn", 3, 51, "kpt3", f16)
    # raw fp32 values that encode (stream, anchor, channel): any mis-gather shows
    for layout, A in (("cn", 200), ("nc_obj", 131)):
        enc = [((s * 320 + np.arange(A))[:, None] * 32 + np.arange(7)[None, :]).astype(np.float32) for s in range(3)]
        add(f"raw_encodes_stream_anchor_channel_{layout}", [rp(A, 3, layout, f32, 300 + s, 0.5) for s in range(3)], layout, 3, 7, "raw", f32, extras=enc)
    # more than 64 survive NMS: ranks cross a chunk boundary (95 of seam_dets(100) survive); and more survive than max_det
    seam = [pack(detpost_ref.seam_dets(100), 257, 3, "cn", f32, 400 + s) for s in range(3)]
    add("survivors_cross_a_chunk", seam, "cn", 3, 51, "kpt3", f32, max_det=130)
    add("more_survivors_than_max_det", seam, "cn", 3, 6, "kpt3", f32, max_det=10, stride=12)
    add("survivors_cross_a_chunk_nc_obj_f16", [pack(detpost_ref.seam_dets(100), 257, 3, "nc_obj", f16, 410 + s) for s in range(3)], "nc_obj", 3, 32, "raw", f16,
        max_det=130)
    # A > K = 64: the exact top-K bites, with ties at the K-th key (confs in steps of 1 / 8)
    add("A300_K64_topk_bites", [rp(300, 3, "cn", f16, 500 + s, 1.0, steps=8, n_obj=150) for s in range(3)], "cn", 3, 34, "kpt2", f16, max_candidates=64,
        max_det=64, conf=0.2)
    # equal confs far apart: src shows the lower anchor first
    tie = [pack([(100 + 50 * q, 100 + 40 * s, 20, 20, 0.5, 0) for q in range(6)], 96, 1, "cn", f32, 600 + s, where=[40, 3, 63, 0, 17, 5]) for s in range(3)]
    add("equal_confs_lower_anchor_first", tie, "cn", 1, 4, "kpt2", f32, max_det=4, stride=6)
    # stacks of duplicates: the best of a stack sits at a middle anchor (stack 1), equal confs leave the lowest anchor (stack 2)
    stack = [(100, 100, 40, 40, 0.7, 1), (100, 100, 40, 40, 0.9, 1), (100, 100, 40, 40, 0.8, 1), (300, 300, 50, 20, 0.6, 0), (300, 300, 50, 20, 0.6, 0)]
    add("stacks_of_duplicates", [pack(stack, 96, 3, "nc_obj", f32, 700 + s, where=[5, 50, 20, 70, 30]) for s in range(3)], "nc_obj", 3, 3, "kpt3", f32, max_det=8)
    add("nothing_passes", [rp(127, 3, "cn", f16, 800 + s, 0.0) for s in range(3)], "cn", 3, 51, "kpt3", f16, max_det=16)
    # a NaN and an inf keypoint on emitted rows (anchors 1, 2, 64: three boxes far apart), x and y, and a NaN visibility
    for dt in (f32, f16):
        dets = [(100, 100, 20, 20, 0.9, 0), (200, 100, 20, 20, 0.8, 1), (300, 100, 20, 20, 0.7, 2)]
        ex = []
        for s in range(3):
            x = make_extras(100, 6, "kpt3", 900 + s)
            x[1, :] = [np.nan, 50, 0.5, 60, np.nan, np.nan]
            x[2, :] = [np.inf, -np.inf, 1.0, -np.inf, np.inf, 0.25]
            ex.append(x)
        add(f"nan_and_inf_keypoints_{np.dtype(dt).name}", [pack(dets, 100, 3, "cn", dt, 910 + s, where=[1, 2, 64]) for s in range(3)], "cn", 3, 6, "kpt3", dt,
            extras=ex, max_det=8)
    # tiled, T = 3, both merges (the geometries and scenes of tests/detpost_tiled_ref.py): survivors from different tiles, src = t * A + a,
    # keypoints clipped to their own tile and then shifted (coordinates within -20 .. 90 of a 64 x 64 letterbox)
    GA, GB, in_tile = tiled_ref.GEO_A, tiled_ref.GEO_B, tiled_ref.in_tile
    obj_a, obj_b, far = (90, 50, 40, 40, 0.9, 1), (30, 30, 20, 24, 0.8, 2), (170, 100, 20, 20, 0.7, 0)
    a = [[in_tile(obj_a[:4] + (0.6, 1), GA[0]), in_tile(far, GA[0])], [in_tile(obj_a, GA[1])], [in_tile(obj_a[:4] + (0.85, 1), GA[2]), in_tile((150, 30, 20, 20, 0.5, 0), GA[2])]]
    b = [[in_tile(obj_b[:4] + (0.5, 2), GB[0])], [in_tile(obj_b, GB[1])], [in_tile((120, 70, 16, 16, 0.6, 0), GB[2])]]
    for merge in ("iou", "ios"):
        for layout, dt, A in (("cn", f32, 96), ("nc_obj", f16, 127)):
            bases = list(tiled_ref.pack_tiles(a, A, 3, layout, dt, 1000)) + list(tiled_ref.pack_tiles(b, A, 3, layout, dt, 1100))
            add(f"tiled_{merge}_{layout}_{np.dtype(dt).name}", bases, layout, 3, 6, "kpt3", dt, geos=[GA, GB], tiles=3, merge=merge, lo=-20, hi=90)
    grid = list(tiled_ref.pack_tiles(tiled_ref.grid_dets(100), 128, 3, "cn", f32, 1600)) + list(tiled_ref.pack_tiles(b, 128, 3, "cn", f32, 1700))
    add("tiled_survivors_cross_a_chunk", grid, "cn", 3, 34, "kpt2", f32, geos=[GA, GB], tiles=3, merge="ios", max_det=130, max_candidates=128, lo=-20, hi=90)
    add("tiled_raw_f16", grid, "cn", 3, 32, "raw", f16, geos=[GA, GB], tiles=3, merge="iou", max_det=10, max_candidates=128, stride=12)
    return C


CASES = _build_cases()
NAMES = [c.name for c in CASES]
_WANT = {}


def want(k, **wrong):
    """per stream (rows, counters, extras, src) of CASES[k], computed once; treat as read-only"""
    key = (k, tuple(sorted(wrong.items())))
    if key not in _WANT:
        c = CASES[k]
        S, T = c.dims[0], c.tiles
        if T:
            _WANT[key] = [detpost_extra_tiled(c.preds[s * T:(s + 1) * T], c.geos[s], c.layout, c.nc, c.E, c.kind, **c.opts, **wrong) for s in range(S)]
        else:
            _WANT[key] = [detpost_extra(c.preds[s], c.geos[s], c.layout, c.nc, c.E, c.kind, **c.opts, **wrong) for s in range(S)]
    return _WANT[key]
