"""Shared by tests/test_obb_reid_emu.py and tests/test_gpu_obb_reid.py (test infrastructure, no tests here): the pool of oriented
boxes the crop geometry is checked on, the oracle's geometry table, and the (hi, lo) fp16 RGBX planes the fp32-grade ReID family
takes as its input, restated in NumPy from oracle.crops."""
from __future__ import annotations

import functools

import numpy as np

# the nine fixed boxes of tests/test_gpu_reid.py::test_oriented_box_crops_bit_exact_and_features_in_both_modes
FIXED = np.array([[320, 240, 80, 160, 0.3], [10, 20, 60, 90, -1.2], [630, 470, 50, 120, 2.0], [300, 200, 33.4, 71.6, 0.77],
                  [200, 200, 128, 256, 0.0], [200.5, 100.5, 256, 512, 0.0], [100, 300, 0.2, 40, 0.5], [400, 100, 300.5, 20.5, 1.5708],
                  [-50, -60, 40, 40, 0.1]], dtype=np.float32)

BLANK_GEOMETRY = np.array([1.0, 1.0, 0.0, 0.0, -1.0e6, 0.0, 0.0, -1.0e6])      # obb_crop_geometry.hpp: a box with a non-finite field


@functools.lru_cache(maxsize=None)
def geometry_pool() -> np.ndarray:
    """(N, 5) float32 [cx, cy, w, h, angle]: the nine fixed boxes plus 200 with seed 21 -- angles 0, +-pi/2, +-pi among them, sizes
    below 1, exact half-integer sizes (2.5, 3.5: round-half-to-even), centres outside a 641 x 480 frame."""
    rng = np.random.default_rng(21)
    n = 200
    b = np.stack([rng.uniform(-80, 720, n), rng.uniform(-80, 560, n), rng.uniform(0.05, 300, n), rng.uniform(0.05, 500, n),
                  rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    special = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi], dtype=np.float32)
    b[0:25, 4] = np.tile(special, 5)
    b[25:35, 2] = np.float32([2.5, 3.5, 0.5, 1.5, 4.5, 2.5, 3.5, 0.3, 0.99, 1.0])
    b[30:40, 3] = np.float32([2.5, 3.5, 0.5, 1.5, 4.5, 2.5, 3.5, 0.3, 0.99, 1.0])
    b[40:45, 0] = np.float32([-500, 2000, 320, 320, -1])
    b[40:45, 1] = np.float32([240, 240, -400, 1500, -1])
    out = np.concatenate([FIXED, b]).astype(np.float32)
    out.setflags(write=False)
    return out


def non_finite_boxes() -> np.ndarray:
    """one non-finite field per box, every field and NaN / +inf / -inf covered"""
    rows = []
    for k in range(5):
        for bad in (np.nan, np.inf, -np.inf):
            r = np.array([100, 80, 40, 60, 0.3], dtype=np.float32)
            r[k] = bad
            rows.append(r)
    return np.stack(rows)


def oracle_geometry(boxes) -> np.ndarray:
    """(N, 8) float64: out_w, out_h, inverse 2x3 map of oracle.crops.obb_crop_geometry (finite boxes only)"""
    from oracle.crops import obb_crop_geometry

    geo = np.empty((len(boxes), 8), dtype=np.float64)
    for i, b in enumerate(boxes):
        ow, oh, im = obb_crop_geometry(b[:5])
        geo[i, 0], geo[i, 1], geo[i, 2:] = ow, oh, im
    return geo


def expected_planes(boxes, img, preprocess: str):
    """(hi, lo) float16 (N, 262, 136, 4): oracle.crops.get_crops_u8 -> the fp32 normalisation table -> hi = fp16(f), lo = fp16(f - hi),
    in the 256 x 128 interior of the stem's padded RGBX layout; border and X channel zero."""
    from oracle.crops import get_crops_u8, normalization_lut

    u8 = get_crops_u8(np.asarray(boxes, dtype=np.float32), img, preprocess=preprocess)          # (N, 256, 128, 3) RGB
    lut = normalization_lut()
    f = np.stack([lut[c][u8[..., c]] for c in range(3)], -1).astype(np.float32)
    hi = f.astype(np.float16)
    lo = (f - hi.astype(np.float32)).astype(np.float16)
    ph = np.zeros((len(u8), 262, 136, 4), dtype=np.float16)
    pl = np.zeros_like(ph)
    ph[:, 3:259, 3:131, :3] = hi
    pl[:, 3:259, 3:131, :3] = lo
    return ph, pl


def same_bits(a, b) -> bool:
    """bit equality of two float arrays of one dtype (NaN payloads and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
