"""TEST-ONLY NumPy reference of the letterboxed detector input the ingest ring writes on the device
(boxmot_amd/csrc/ingest_letterbox.hpp has the definition), on top of ``oracle.crops.cv2_resize_linear_u8``; plus the frames and
the shapes the letterbox tests share.  Pinned by tests/test_letterbox_ref.py (OpenCV itself is absent offline: parity with it is as
unpinned as the crops')."""
from __future__ import annotations

import numpy as np

from oracle.crops import cv2_resize_linear_u8

# (rows, cols) -> (H, W), the "center" geometry (new_w, new_h, top, left), the branch it reaches: the smallest shapes that reach
# every branch
SHAPES = [
    ((36, 64), (32, 32), (32, 18, 7, 0)),        # exact 2x, wide
    ((64, 36), (32, 32), (18, 32, 0, 7)),        # exact 2x, tall
    ((64, 96), (32, 48), (48, 32, 0, 0)),        # 2x, no pad
    ((32, 32), (32, 32), (32, 32, 0, 0)),        # copy
    ((24, 32), (32, 32), (32, 24, 4, 0)),        # copy plus pad
    ((37, 53), (32, 48), (46, 32, 0, 1)),        # general downscale
    ((50, 131), (40, 72), (72, 27, 6, 0)),       # odd padding: 6 above and 7 below
    ((20, 30), (32, 48), (48, 32, 0, 0)),        # upscale 1.6
    ((9, 7), (32, 48), (25, 32, 0, 11)),         # upscale 3.6, odd padding
    ((1, 1), (8, 8), (8, 8, 0, 0)),              # one-pixel frame
]
# where "topleft" differs in more than top = left = 0
TOPLEFT_NEW_W = {(37, 53): 45, (9, 7): 24}
# The kernel tiles the flattened (H, W) plane: a thread owns 8 columns of one row, a workgroup 256 such threads in row-major order
# (2048 elements).  Two shapes put work just past a workgroup's span:
#   (10, 700) -> (4, 520)   65 thread columns x 4 rows = 260 threads: 4 threads of a second workgroup, and 65 threads a row means
#                           every wavefront straddles two output rows (picture row and padding mixed in one wavefront)
#   (33, 70) -> (63, 136)   17 thread columns x 63 rows = 1071 threads: four full workgroups and 47 threads of a fifth
OWN_SHAPES = [
    ((10, 700), (4, 520), (280, 4, 0, 120)),
    ((33, 70), (63, 136), (134, 63, 0, 1)),      # 70 * 63 / 33 = 133.6...
]
TOPLEFT_NEW_W[(33, 70)] = 133
ALL_SHAPES = SHAPES + OWN_SHAPES


def geometry(rows: int, cols: int, size, mode: str = "center"):
    """(gain, new_w, new_h, top, left), or None where the picture would vanish"""
    H, W = size
    gain = min(H / rows, W / cols)
    if mode == "center":
        new_w, new_h = round(cols * gain), round(rows * gain)
        top, left = round((H - new_h) / 2 - 0.1), round((W - new_w) / 2 - 0.1)
    else:
        assert mode == "topleft"
        new_w, new_h, top, left = int(cols * gain), int(rows * gain), 0, 0
    if new_w < 1 or new_h < 1:
        return None
    return gain, new_w, new_h, top, left


def table(unit: bool, dtype) -> np.ndarray:
    """the 256 values a byte becomes"""
    v = np.arange(256, dtype=np.float32)
    if unit:
        v = v / np.float32(255)
    return v.astype(dtype)


def letterbox_u8(frame: np.ndarray, size, mode: str = "center", pad: int = 114) -> np.ndarray:
    """(H, W, 3) uint8 BGR: the resized picture on the pad colour"""
    H, W = size
    rows, cols = frame.shape[:2]
    _, new_w, new_h, top, left = geometry(rows, cols, size, mode)
    out = np.full((H, W, 3), pad, dtype=np.uint8)
    out[top:top + new_h, left:left + new_w] = cv2_resize_linear_u8(frame, (new_w, new_h))
    return out


def letterbox(frame: np.ndarray, size, mode: str = "center", rgb: bool = True, unit: bool = True, pad: int = 114,
              dtype=np.float32) -> np.ndarray:
    """(3, H, W) ``dtype`` tensor of one (rows, cols, 3) uint8 BGR frame"""
    chw = letterbox_u8(frame, size, mode, pad).transpose(2, 0, 1)
    if rgb:
        chw = chw[::-1]
    return table(unit, dtype)[chw]


def make_frame(rows: int, cols: int, kind: str = "random", seed: int = 0) -> np.ndarray:
    """``random`` bytes; ``checker``: 0 / 255 in a checkerboard (the largest coefficient sums); ``ramp``: every byte value"""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if kind == "checker":
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    assert kind == "ramp"
    f = ((yy * cols + xx)[:, :, None] * 3 + np.arange(3)[None, None, :]) * 7 + seed
    return (f & 255).astype(np.uint8)


def _build_cases():
    """(name, frame, size): every shape with random bytes, and the checkerboard and the every-byte frame on a 2x, a general
    downscale, an upscale and the wide own shape; the references are computed once (``want``) and shared"""
    cases = []
    for k, ((r, c), size, _) in enumerate(ALL_SHAPES):
        cases.append((f"{r}x{c}->{size[0]}x{size[1]}", make_frame(r, c, "random", 100 + k), size))
    for (r, c), size in (((36, 64), (32, 32)), ((37, 53), (32, 48)), ((20, 30), (32, 48)), ((10, 700), (4, 520))):
        cases.append((f"checker {r}x{c}->{size[0]}x{size[1]}", make_frame(r, c, "checker"), size))
        cases.append((f"ramp {r}x{c}->{size[0]}x{size[1]}", make_frame(r, c, "ramp", 3), size))
    return cases


CASES = _build_cases()
EVEN_CASES = [c for c in CASES if c[1].shape[0] % 2 == 0 and c[1].shape[1] % 2 == 0]      # what an NV12 ring can hold

_WANT = {}


def want(case_index: int, mode="center", rgb=True, unit=True, pad=114, dtype=np.float32) -> np.ndarray:
    """the reference of CASES[case_index], computed once per configuration; treat the result as read-only"""
    key = (case_index, mode, rgb, unit, pad, np.dtype(dtype).str)
    if key not in _WANT:
        _, frame, size = CASES[case_index]
        w = letterbox(frame, size, mode, rgb, unit, pad, dtype)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]
