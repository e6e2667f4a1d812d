"""NumPy float32 restatement of step 10 of the detection post-processing, the frame-space instance label map
(boxmot_amd/csrc/det_post_labels.hpp), written from the definition and not from the kernel, and the table of cases the emulated
and the device kernels are compared with, bit for bit.

    per stream: labels (rows, cols) int16 = want(k)[s]

Step 10 reads what a run left on the device -- the rows in frame coordinates, their count, the raw coefficients -- and the
prototypes, so the cases give those blocks directly: no detector head is involved.  ``labels_of`` restates the step per row, over
the whole frame at once: the logits of the row at PROTOTYPE resolution by a float32 accumulator array ``acc = acc + c[k] * p[k]``
in a Python loop over ascending ``k``, the two taps and the weight per column and per line from ``tap``, the four gathers, the
blend with every ``1 - l``, product and sum an array operation of its own (NumPy rounds each to float32), the window compared
with the row's frame box, and first-wins by only labelling pixels that are still -1.  Every comparison with the kernel is exact.

Subnormals are kept out, as in detpost_mask_ref (``vals``): coefficients and prototype values are 0 or fp16-representable numbers
of magnitude within [2^-6, 60], so the logits are 0 or multiples of 2^-32 and a product with a bilinear weight (0 or >= 2^-24)
stays far above the subnormal range.

The keyword switches of ``labels_of`` make the WRONG references the tests use as controls: ``corner`` (no ``+ 0.5`` / ``- 0.5``:
pixel corners instead of centres), ``last_wins``, ``threshold_first`` (threshold at prototype resolution, then nearest
upsampling), ``letterbox_window`` (the window from the letterbox-space box ``x * gain + left`` instead of the frame row),
``inclusive_edge`` (``<=`` at the right and bottom edge) and ``float64_acc``."""
from typing import NamedTuple

import numpy as np

F = np.float32


def vals(rng, shape):
    """float32 values that are fp16-representable and 0 (one in eight) or of magnitude within [2^-6, 60]: +-m * 2^e, m in 8..15, e in -9..2
    (detpost_mask_ref's)"""
    m = rng.integers(8, 16, shape).astype(np.float32)
    e = rng.integers(-9, 3, shape).astype(np.float32)
    sign = np.where(rng.random(shape) < 0.5, F(-1), F(1))
    return np.where(rng.random(shape) < 0.125, F(0), sign * m * np.exp2(e)).astype(np.float32)


WRONG = ("corner", "last_wins", "threshold_first", "letterbox_window", "inclusive_edge", "float64_acc")
TILE_W, TILE_H, PATCH = 64, 16, 2048            # the kernel's tile and LDS patch budget: only ``patch_of`` (which path a case takes) reads them


def tap(n, gain, off, ratio, size, corner=False):
    """(t0, t1, l) of the n frame coordinates 0 .. n - 1 along one axis: the definition's map, float32 throughout"""
    x = np.arange(n, dtype=np.float32)
    gain, off, ratio = F(gain), F(off), F(ratio)
    with np.errstate(all="ignore"):
        p = (x * gain + off) * ratio if corner else ((x + F(0.5)) * gain + off) * ratio - F(0.5)
        p = np.minimum(np.maximum(p, F(0)), F(size - 1))
    t0 = p.astype(np.int32)
    t1 = np.minimum(t0 + 1, size - 1)
    return t0, t1, p - t0.astype(np.float32)


def logits_of(c, proto, float64_acc=False):
    """(mask_h, mask_w) logits of one row: the chain over ascending k"""
    p = proto.astype(np.float64 if float64_acc else np.float32)             # (fp16 widens exactly)
    c = c.astype(p.dtype)
    acc = np.zeros(p.shape[1:], dtype=p.dtype)
    with np.errstate(all="ignore"):
        for k in range(p.shape[0]):
            acc = acc + c[k] * p[k]
    return acc


def labels_of(geo, dets, n_rows, coefs, proto, mask, in_shape, max_det, corner=False, last_wins=False, threshold_first=False, letterbox_window=False,
              inclusive_edge=False, float64_acc=False):
    """labels (rows, cols) int16 of one stream.  geo: (gain, top, left, rows, cols); dets: (stride, 6) float32, frame coordinates;
    n_rows: what d_det_rows holds; coefs: (stride, E) float32; proto: (E, mask_h, mask_w)"""
    gain, top, left = F(geo[0]), F(geo[1]), F(geo[2])
    rows, cols = int(F(geo[3])), int(F(geo[4]))
    mh, mw = mask
    wr, hr = F(mw) / F(in_shape[1]), F(mh) / F(in_shape[0])
    n = min(int(n_rows), max_det)
    j0, j1, lx = tap(cols, gain, left, wr, mw, corner)
    i0, i1, ly = tap(rows, gain, top, hr, mh, corner)
    lx, ly = lx[None, :], ly[:, None]
    xs, ys = np.arange(cols, dtype=np.float32)[None, :], np.arange(rows, dtype=np.float32)[:, None]
    out = np.full((rows, cols), -1, dtype=np.int16)
    one = F(1)
    for r in range(max(n, 0)):
        g = logits_of(coefs[r], proto, float64_acc)
        x1, y1, x2, y2 = (F(v) for v in dets[r, :4])
        with np.errstate(all="ignore"):
            if threshold_first:
                jn = np.minimum(np.maximum(np.floor(((xs[0] + F(0.5)) * gain + left) * wr), 0), mw - 1).astype(np.int32)
                im = np.minimum(np.maximum(np.floor(((ys[:, 0] + F(0.5)) * gain + top) * hr), 0), mh - 1).astype(np.int32)
                on = (g > 0)[im][:, jn]
            else:
                g00, g01, g10, g11 = g[i0][:, j0], g[i0][:, j1], g[i1][:, j0], g[i1][:, j1]
                wx, wy = one - lx, one - ly
                upper = wx * g00 + lx * g01
                lower = wx * g10 + lx * g11
                on = (wy * upper + ly * lower) > 0
            if letterbox_window:
                x1, y1, x2, y2 = x1 * gain + left, y1 * gain + top, x2 * gain + left, y2 * gain + top
            right, bottom = (xs <= x2, ys <= y2) if inclusive_edge else (xs < x2, ys < y2)
            covers = (xs >= x1) & right & (ys >= y1) & bottom & on
        if last_wins:
            out[covers] = r
        else:
            out[covers & (out < 0)] = r
    return out


def patch_of(geo, mask, in_shape, tile_x=0, tile_y=0):
    """(patch_h, patch_w) of prototype pixels a tile of the frame maps to: more than PATCH of them and the kernel takes the fallback path"""
    rows, cols = int(F(geo[3])), int(F(geo[4]))
    wr, hr = F(mask[1]) / F(in_shape[1]), F(mask[0]) / F(in_shape[0])
    j0, j1, _ = tap(cols, geo[0], geo[2], wr, mask[1])
    i0, i1, _ = tap(rows, geo[0], geo[1], hr, mask[0])
    xa, xb = tile_x * TILE_W, min((tile_x + 1) * TILE_W, cols) - 1
    ya, yb = tile_y * TILE_H, min((tile_y + 1) * TILE_H, rows) - 1
    return int(i1[yb] - i0[ya] + 1), int(j1[xb] - j0[xa] + 1)


# ---------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    geos: list                  # per stream (gain, top, left, rows, cols)
    dets: np.ndarray            # (S, stride, 6) float32: rows in frame coordinates; beyond the count: garbage that must not be read as rows
    n_rows: np.ndarray          # (S,) int32: what d_det_rows holds (may exceed max_det)
    coefs: np.ndarray           # (S, stride, E) float32
    protos: np.ndarray          # (S, E, mask_h, mask_w), float16 or float32
    mask: tuple                 # (mask_h, mask_w)
    in_shape: tuple             # (in_h, in_w)
    max_det: int
    plane: tuple                # (H, W) of the label block, >= every frame

    @property
    def E(self):
        return self.protos.shape[1]

    @property
    def stride(self):
        return self.dets.shape[1]


def geometry(frame, in_shape, centre):
    """(gain, top, left, rows, cols) of a frame letterboxed into in_shape, the picture in the centre or at the top left"""
    rows, cols = frame
    gain = min(in_shape[0] / rows, in_shape[1] / cols)
    top = (in_shape[0] - round(rows * gain)) // 2 if centre else 0
    left = (in_shape[1] - round(cols * gain)) // 2 if centre else 0
    return (float(F(gain)), float(top), float(left), float(rows), float(cols))


def scene(frame):
    """six rows by descending confidence, in quarter pixels: two overlapping, one nested in the first (and over the second), one
    flush with the frame's right and bottom edge, one of zero area, and the whole frame underneath"""
    r, c = frame
    q = lambda v: round(v * 4) / 4
    boxes = [(0.1 * c, 0.1 * r, 0.6 * c, 0.7 * r), (0.3 * c, 0.2 * r, 0.9 * c, 0.8 * r), (0.2 * c, 0.3 * r, 0.5 * c, 0.6 * r), (0.5 * c, 0.5 * r, c, r),
             (0.4 * c, 0.4 * r, 0.4 * c, 0.9 * r), (0, 0, c, r)]
    return [(q(x1), q(y1), q(x2), q(y2), 0.9 - 0.1 * k, k % 3) for k, (x1, y1, x2, y2) in enumerate(boxes)]


SHAPES = [((8, 8), (32, 32)), ((7, 9), (28, 30)), ((12, 20), (40, 64))]
SMALL = {(8, 8): (7, 6), (7, 9): (6, 7), (12, 20): (10, 17)}           # frames smaller than the input: gain * wr > 1 and gain * hr > 1
GARBAGE = F(-3.0e4)


def _build_cases():
    f16, f32 = np.float16, np.float32
    C = []

    def add(name, frames, boxes, mask, in_shape, E=32, qdt=f32, centre=True, coefs=None, protos=None, max_det=8, stride=10, n_rows=None, plane=None, geos=None):
        """frames: per stream (rows, cols); boxes: per stream the rows; coefs: per stream (len(boxes), E), default ``vals``; protos:
        (S, E, mh, mw), default ``vals``"""
        rng = np.random.default_rng(7000 + 13 * len(C))
        S = len(frames)
        geos = [geometry(f, in_shape, centre) for f in frames] if geos is None else geos
        dets = np.full((S, stride, 6), GARBAGE, dtype=np.float32)
        cf = vals(rng, (S, stride, E))                  # (beyond the count too: values that would label if they were read)
        for s in range(S):
            b = np.array(boxes[s], dtype=np.float32).reshape(-1, 6)
            dets[s, :len(b)] = b
            dets[s, len(b):, :4] = (0, 0, 1e4, 1e4)       # rows beyond the count cover everything
            if coefs is not None:
                cf[s, :len(b)] = coefs[s]
        if protos is None:
            protos = vals(rng, (S, E) + tuple(mask))
        if n_rows is None:
            n_rows = [len(b) for b in boxes]
        if plane is None:
            plane = (max(f[0] for f in frames), max(f[1] for f in frames))
        C.append(Case(name, geos, dets, np.array(n_rows, dtype=np.int32), cf, np.ascontiguousarray(np.asarray(protos).astype(qdt)), tuple(mask), tuple(in_shape),
                      max_det, tuple(plane)))

    # the table: three shapes x three frames (24 x 40, 50 x 31, one smaller than the input) x centre / top-left; E = 32 / 5 and
    # fp16 / fp32 prototypes in turn
    k = 0
    for mask, in_shape in SHAPES:
        for frame in ((24, 40), (50, 31), SMALL[mask]):
            for centre in (True, False):
                E, qdt = (32, 5)[k % 2], (f16, f32)[(k // 2) % 2]
                add(f"table_{mask[0]}x{mask[1]}_frame_{frame[0]}x{frame[1]}_{'centre' if centre else 'topleft'}_E{E}_{np.dtype(qdt).name}", [frame], [scene(frame)],
                    mask, in_shape, E=E, qdt=qdt, centre=centre)
                k += 1
    # three streams of different sizes (one wider than a tile) into one block larger than every frame
    frames = [(24, 40), (20, 70), (50, 31)]
    for qdt in (f16, f32):
        add(f"three_streams_{np.dtype(qdt).name}", frames, [scene(f) for f in frames], (12, 20), (40, 64), E=32, qdt=qdt, plane=(56, 72))

    def ones(S, E, mask):
        p = np.zeros((S, E) + tuple(mask), dtype=np.float32)
        p[:, 0] = 1
        return p

    def unit(n, E, first=1.0):
        c = np.zeros((n, E), dtype=np.float32)
        c[:, 0] = first
        return c

    frame, mask, in_shape = (24, 40), (8, 8), (32, 32)
    whole = (0, 0, 40, 24)
    # positive logits everywhere: the label is the window alone.  Two and three overlapping boxes, nested boxes: first-wins
    add("first_wins_two", [frame], [[(4, 4, 30, 20, 0.9, 0), (10, 2, 38, 22, 0.8, 0)]], mask, in_shape, E=5, coefs=[unit(2, 5)], protos=ones(1, 5, mask))
    add("first_wins_three", [frame], [[(4, 4, 30, 20, 0.9, 0), (10, 2, 38, 22, 0.8, 0), (0, 8, 40, 16, 0.7, 1)]], mask, in_shape, E=5, coefs=[unit(3, 5)],
        protos=ones(1, 5, mask))
    add("nested", [frame], [[(12, 8, 20, 14, 0.9, 0), (6, 4, 30, 20, 0.8, 0), whole + (0.7, 1)]], mask, in_shape, E=5, coefs=[unit(3, 5)], protos=ones(1, 5, mask))
    # edges exactly on integers: x1 = 8 includes x = 8, x2 = 20 excludes x = 20; likewise y 4 .. 12; flush with the right and bottom edge
    add("edges_on_integers", [frame], [[(8, 4, 20, 12, 0.9, 0), (30, 16, 40, 24, 0.8, 0)]], mask, in_shape, E=5, coefs=[unit(2, 5)], protos=ones(1, 5, mask))
    add("zero_area", [frame], [[(10, 4, 10, 20, 0.9, 0), (4, 12, 30, 12, 0.8, 0), whole + (0.7, 1)]], mask, in_shape, E=5, coefs=[unit(3, 5)], protos=ones(1, 5, mask))
    add("zero_rows", [frame, frame], [[], [whole + (0.9, 0)]], mask, in_shape, E=5, coefs=[unit(0, 5), unit(1, 5)], protos=ones(2, 5, mask), n_rows=[0, 1])
    # more kept than max_det: the count says 6, max_det = 4: rows 4 and 5 cover the whole frame and must not label
    many = [(0, 0, 10, 10, 0.9, 0), (10, 0, 20, 10, 0.8, 0), (20, 0, 30, 10, 0.7, 0), (30, 0, 40, 10, 0.6, 0), whole + (0.5, 0), whole + (0.4, 0)]
    add("more_kept_than_max_det", [frame], [many], mask, in_shape, E=5, coefs=[unit(6, 5)], protos=ones(1, 5, mask), max_det=4, n_rows=[6])
    # NaN coefficients: row 0 covers nothing, row 1 shows through.  A NaN prototype: every pixel with a tap on it is -1 for every row
    nan_c = unit(2, 5)
    nan_c[0, 3] = np.nan
    add("nan_coefficients", [frame], [[whole + (0.9, 0), (4, 4, 36, 20, 0.8, 0)]], mask, in_shape, E=5, coefs=[nan_c], protos=ones(1, 5, mask))
    nan_p = ones(1, 5, mask)
    nan_p[0, 2, 3, 4] = np.nan
    for qdt in (f32, f16):
        add(f"nan_prototype_{np.dtype(qdt).name}", [frame], [[whole + (0.9, 0), whole + (0.8, 0)]], mask, in_shape, E=5, qdt=qdt, coefs=[unit(2, 5)], protos=nan_p)
    # a NaN box edge: the row covers nothing
    add("nan_box", [frame], [[(np.nan, 0, 40, 24, 0.9, 0), (0, 0, 40, np.nan, 0.8, 0), (4, 4, 36, 20, 0.7, 0)]], mask, in_shape, E=5, coefs=[unit(3, 5)],
        protos=ones(1, 5, mask))
    # logits of exactly +-0: all prototypes 0 under coefficients of both signs (+0 and -0 products) -- row 0 covers nothing
    zero_c = np.array([[2, -1, 1, -3, 0.5], [1, 0, 0, 0, 0]], dtype=np.float32)
    zero_p = np.zeros((1, 5) + mask, dtype=np.float32)
    add("signed_zero_logits_row_0", [frame], [[whole + (0.9, 0)]], mask, in_shape, E=5, coefs=[zero_c[:1]], protos=zero_p)
    half = ones(1, 5, mask)
    half[0, :, :, :4] = 0                               # the left half: logits +0, and a blend that reaches exactly 0 stays uncovered
    add("signed_zero_logits_left_half", [frame], [[whole + (0.9, 0), whole + (0.8, 1)]], mask, in_shape, E=5, coefs=[np.array([[1, -1, 1, -1, 1], [-1, 0, 0, 0, 0]], dtype=np.float32)],
        protos=half)
    # the order of the chain: terms 1, 2^27, -2^27 -- ascending in float32 gives 0 (uncovered), float64 gives 1
    order_c = np.tile(np.array([1.0, 2.0 ** 14, -2.0 ** 14], dtype=np.float32), (1, 1))
    order_p = np.ones((1, 3) + mask, dtype=np.float32) * np.array([1.0, 2.0 ** 13, 2.0 ** 13], dtype=np.float32)[None, :, None, None]
    add("order_of_the_chain", [frame], [[whole + (0.9, 0)]], mask, in_shape, E=3, qdt=f16, coefs=[order_c], protos=order_p)
    # more rows than one staged chunk of 256: 270 small boxes on a grid, the whole frame last
    grid = [(2 * (q % 20), (q // 20), 2 * (q % 20) + 2.5, (q // 20) + 1.5, 0.9, 0) for q in range(269)] + [whole + (0.1, 0)]
    add("more_rows_than_a_chunk", [frame], [grid], mask, in_shape, E=5, max_det=300, stride=300)
    # prototypes as large as the input, a frame half its size: a tile maps to more than PATCH prototype pixels and the kernel takes
    # the fallback path by itself
    add("patch_beyond_the_budget", [(30, 38)], [scene((30, 38))], (60, 76), (60, 76), E=5, qdt=f16, centre=False)
    return C


CASES = _build_cases()
NAMES = [c.name for c in CASES]
_WANT = {}


def want(k, **wrong):
    """per stream the labels (rows, cols) int16 of CASES[k], computed once; treat as read-only"""
    key = (k, tuple(sorted(wrong.items())))
    if key not in _WANT:
        c = CASES[k]
        _WANT[key] = [labels_of(c.geos[s], c.dets[s], c.n_rows[s], c.coefs[s], c.protos[s], c.mask, c.in_shape, c.max_det, **wrong) for s in range(len(c.geos))]
    return _WANT[key]
