"""TEST-ONLY NumPy reference of the letterboxed tiles the ingest ring writes on the device (boxmot_amd/csrc/ingest_letterbox_tiles.hpp has
the definition), written from that definition: tensor ``s * T + t`` is ``letterbox_ref.letterbox`` of the slice
``frame[y0:y0 + h, x0:x0 + w]`` as a frame of its own.  Plus the frames, the rectangles and the output sizes the emulated and the
device tests share."""
from __future__ import annotations

import math

import numpy as np

import letterbox_ref

# two streams of different sizes in one call
SIZES = [(97, 131), (128, 200)]                         # (rows, cols)
FRAMES = [letterbox_ref.make_frame(r, c, "random", 500 + s) for s, (r, c) in enumerate(SIZES)]
OUT_SIZES = [(64, 64), (32, 64)]                        # (H, W)
# (x0, y0, w, h) per stream, the same count for both; what each rectangle is there for, at 64 x 64 | at 32 x 64:
TILES = [
    [(0, 0, 131, 97),           # the whole frame
     (3, 5, 64, 64),            # copy | bilinear, bars left and right
     (1, 20, 128, 64),          # exact 2 x, bars above and below | exact 2 x, no bars; odd x0: rows at any byte alignment
     (81, 57, 50, 40),          # flush with the right and bottom edges: the last row pair and column pair are the frame's last
     (7, 11, 33, 20),           # odd x0, odd w: an upscale
     (130, 10, 1, 20),          # one column, the frame's last: the 3-byte path
     (10, 50, 40, 1),           # one row
     (5, 9, 64, 32)],           # copy with bars | copy
    [(0, 0, 200, 128),
     (101, 33, 64, 64),
     (71, 0, 128, 128),         # exact 2 x | bilinear downscale by 4
     (123, 78, 77, 50),         # flush with the right and bottom edges, odd w
     (13, 9, 45, 31),
     (0, 30, 1, 20),            # one column, the frame's first
     (150, 127, 40, 1),         # one row, the frame's last
     (99, 77, 64, 32)],
]
T = len(TILES[0])
assert all(len(t) == T for t in TILES)


def tile_axis(L, n, o):
    """the definition of tile_grid per axis: (size, origins)"""
    if n == 1:
        return L, [0]
    size = min(L, math.ceil(L / (n - (n - 1) * o)))
    return size, [(i * (L - size)) // (n - 1) for i in range(n)]


def tile_grid(rows, cols, grid, overlap=0.2, full=True):
    h, ys = tile_axis(rows, grid[0], overlap)
    w, xs = tile_axis(cols, grid[1], overlap)
    return ([(0, 0, cols, rows)] if full else []) + [(x, y, w, h) for y in ys for x in xs]


def geometry(rect, size, mode="center"):
    """(gain, new_w, new_h, top, left, rows, cols, x0, y0) of a rectangle, or None where its picture would vanish"""
    x0, y0, w, h = rect
    g = letterbox_ref.geometry(h, w, size, mode)
    return None if g is None else g + (h, w, x0, y0)


def letterbox_tiles(frames, tiles, size, mode="center", rgb=True, unit=True, pad=114, dtype=np.float32) -> np.ndarray:
    """(S * T, 3, H, W) ``dtype`` of the streams' frames and their per-stream rectangles"""
    out = [letterbox_ref.letterbox(np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w]), size, mode, rgb, unit, pad, dtype)
           for f, rects in zip(frames, tiles) for (x0, y0, w, h) in rects]
    return np.stack(out)


_WANT = {}


def want(size, mode="center", rgb=True, unit=True, pad=114, dtype=np.float32) -> np.ndarray:
    """the reference of FRAMES x TILES, computed once per configuration; treat the result as read-only"""
    key = (tuple(size), mode, rgb, unit, pad, np.dtype(dtype).str)
    if key not in _WANT:
        w = letterbox_tiles(FRAMES, TILES, size, mode, rgb, unit, pad, dtype)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]
