"""TEST-ONLY NumPy reference of the NV12 -> BGR conversion the ingest ring runs on the device (boxmot_amd/csrc/ingest_nv12.hpp):
``cv2.cvtColor(frame, cv2.COLOR_YUV2BGR_NV12)`` restated -- BT.601 limited range, 20-bit fixed point, int32 throughout.  Pinned
on hand-computed pixels by tests/test_nv12_ref.py (OpenCV itself is absent offline: parity with it is stated, not tested)."""
from __future__ import annotations

import numpy as np

CY, CUB, CUG, CVG, CVR, SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20


def nv12_to_bgr_planes(y: np.ndarray, uv: np.ndarray) -> np.ndarray:
    """``y``: (rows, >= cols) uint8 Y plane; ``uv``: (rows // 2, >= cols) uint8 plane of interleaved U, V pairs; the planes may
    be wider than the picture (a pitch), the picture is ``cols = `` the narrower of the two.  Returns (rows, cols, 3) uint8 BGR."""
    rows = y.shape[0]
    cols = min(y.shape[1], uv.shape[1])
    assert rows % 2 == 0 and cols % 2 == 0 and uv.shape[0] == rows // 2
    y = y[:, :cols].astype(np.int32)
    u = uv[:, 0:cols:2].astype(np.int32) - 128
    v = uv[:, 1:cols:2].astype(np.int32) - 128
    u = np.repeat(np.repeat(u, 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)
    yy = np.maximum(y - 16, 0) * np.int32(CY) + np.int32(1 << (SHIFT - 1))
    out = np.empty((rows, cols, 3), dtype=np.uint8)
    out[..., 0] = np.clip((yy + np.int32(CUB) * u) >> SHIFT, 0, 255)
    out[..., 1] = np.clip((yy + np.int32(CVG) * v + np.int32(CUG) * u) >> SHIFT, 0, 255)
    out[..., 2] = np.clip((yy + np.int32(CVR) * v) >> SHIFT, 0, 255)
    return out


def nv12_to_bgr(frame: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """``frame``: a tightly packed NV12 frame, (rows * 3 // 2, cols) uint8 (or those bytes flat)."""
    f = np.asarray(frame, dtype=np.uint8).reshape(rows * 3 // 2, cols)
    return nv12_to_bgr_planes(f[:rows], f[rows:])


def exhaustive_frame() -> np.ndarray:
    """The (4096 * 3 // 2, 4096) NV12 frame that holds every one of the 2^24 (Y, U, V) byte triples exactly once: chroma position
    k = i * 2048 + j carries the pair (U, V) = (k % 65536 % 256, k % 65536 // 256) and its four luma samples carry
    4 * (k // 65536) + 2 * dy + dx."""
    n = 4096
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    pair = k % 65536
    f = np.empty((n * 3 // 2, n), dtype=np.uint8)
    f[n:, 0::2] = pair % 256
    f[n:, 1::2] = pair // 256
    base = 4 * (k // 65536)
    for dy in range(2):
        for dx in range(2):
            f[dy:n:2, dx::2] = base + 2 * dy + dx
    return f


def random_frame(rows: int, cols: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (rows * 3 // 2, cols), dtype=np.uint8)


def bgr_to_nv12(img: np.ndarray) -> np.ndarray:
    """A plausible NV12 frame of a BGR picture (BT.601 limited range in floating point, 2 x 2 chroma means): test input only --
    nothing checks this direction."""
    rows, cols = img.shape[0] // 2 * 2, img.shape[1] // 2 * 2
    b, g, r = (img[:rows, :cols, c].astype(np.float32) for c in range(3))
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    f = np.empty((rows * 3 // 2, cols), dtype=np.uint8)
    f[:rows] = np.clip(np.rint(y), 0, 255)
    sub = lambda p: p.reshape(rows // 2, 2, cols // 2, 2).mean(axis=(1, 3))
    f[rows:, 0::2] = np.clip(np.rint(sub(u)), 0, 255)
    f[rows:, 1::2] = np.clip(np.rint(sub(v)), 0, 255)
    return f
