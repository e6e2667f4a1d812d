"""Per-stream frame sizes in the crop kernels: the table forms (k_crop_resize_sized<float>, k_crop_resize_rgbx_hl_sized,
k_stem_sized_fused_hp -- device source, unchanged, on CPU threads: tests/host_emu/emu_reid_sized.cpp) take the crops of four frames
of different sizes in ONE launch and must equal, bit for bit, (a) oracle.crops on each frame alone and (b) the scalar-form kernel
launched once per frame.  Every frame has boxes clipped by each of its own four borders, and the smaller frames have a box that
is interior in 1080 x 1920 but clipped in them, so a kernel that took another frame's size cannot pass.  Not a product path."""
import ctypes
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent / "host_emu"
CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
SIZES = [(480, 640), (487, 651), (720, 1280), (1080, 1920)]          # (rows, cols); 651 * 3 bytes: rows start at every dword offset

_VP, _I = ctypes.c_void_p, ctypes.c_int


def _build(sanitize=False):
    out = HERE / ("libemu_reid_sized_asan.so" if sanitize else "libemu_reid_sized.so")
    deps = [HERE / "emu_reid_sized.cpp", HERE / "emu_reid.cpp", HERE / "hip_shim.hpp"] + list((HERE.parent.parent / "boxmot_amd" / "csrc").glob("*.hpp"))
    if not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps):
        flags = ["-fsanitize=address", "-shared-libasan", "-fno-omit-frame-pointer", "-g"] if sanitize else []
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-DEMU_DEFER_GLDS=1",
                               *flags, "-o", str(out), str(HERE / "emu_reid_sized.cpp")])
    return out


def _frame(rows, cols, seed):
    """seeded noise on a smooth gradient (noise alone makes the resize insensitive to an off-by-one tap)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    g = np.stack([x * 200.0 / cols, y * 200.0 / rows, (x + y) * 200.0 / (rows + cols)], axis=2)
    return np.ascontiguousarray(np.clip(g + rng.integers(0, 56, (rows, cols, 3)), 0, 255).astype(np.uint8))


def _boxes(rows, cols):
    W, H = float(cols), float(rows)
    b = [[0.1 * W + 0.2, 0.2 * H + 0.7, 0.3 * W + 0.1, 0.7 * H + 0.3],       # interior
         [-20.0, 0.3 * H, 50.4, 0.6 * H],                                     # clipped by the left border
         [0.4 * W, -15.5, 0.5 * W, 100.2],                                    # top
         [W - 60.4, 0.2 * H, W + 30.0, 0.5 * H],                              # right
         [0.5 * W, H - 80.7, 0.6 * W, H + 25.0],                              # bottom
         [10, 10, 138, 266],                                                  # identity-sized
         [20, 8, 276, 520],                                                   # exact 2x where the frame is tall enough
         [0, 0, W, H]]                                                        # the whole frame
    if (rows, cols) in ((480, 640), (487, 651)):
        b.append([600.3, 300.2, 900.6, 700.1])                                # interior in 1080 x 1920, clipped right and bottom here
    elif (rows, cols) == (720, 1280):
        b.append([1100.3, 500.2, 1500.6, 900.1])
    else:
        b.append([1500.2, 800.4, 1800.1, 1060.3])
    return np.array(b, dtype=np.float32)


# boxes of _boxes() the (slow: 512 threads per crop) stem runs on: interior, bottom-clipped, and the other-frame's-interior box
STEM_ROWS = [0, 4, 8]


def _check(sanitize=False, stem_rows=STEM_ROWS, crop_rows=None):
    from boxmot_amd.reid_weights import pack_osnet, random_osnet_state_dict
    from oracle.crops import get_crops

    lib = ctypes.CDLL(str(_build(sanitize)))
    lib.emu_sized_crop_f32.argtypes = [_VP, _VP, _VP, _I, _VP, _I, _I, _I, _VP]
    lib.emu_sized_crop_hl.argtypes = [_VP, _VP, _VP, _I, _VP, _I, _I, _I, _VP, _VP]
    lib.emu_sized_stem_hp.argtypes = [_VP, ctypes.c_long, _VP, _VP, _VP, _I, _VP, _I, _I, _VP, _VP, _VP]
    frames = [_frame(r, c, 11 + k) for k, (r, c) in enumerate(SIZES)]
    fptr = (ctypes.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    dims = np.array([[c, r] for r, c in SIZES], dtype=np.int32)              # {W, H} per stream
    per = [_boxes(r, c) for r, c in SIZES]
    if crop_rows is not None:
        per = [b[crop_rows] for b in per]

    def tables(sel):
        bx = [b if sel is None else b[sel] for b in per]
        boxes = np.ascontiguousarray(np.concatenate(bx))
        stream = np.repeat(np.arange(len(SIZES), dtype=np.int32), [len(b) for b in bx]).astype(np.int32)
        order = np.random.default_rng(3).permutation(len(boxes))              # crops of the frames interleaved in the launch
        return np.ascontiguousarray(boxes[order]), np.ascontiguousarray(stream[order])

    # ---- k_crop_resize<float>, both preprocess modes ----
    boxes, stream = tables(None)
    n = len(boxes)
    for pad in (0, 1):
        mixed = np.zeros((n, 256, 128, 3), np.float32)
        assert lib.emu_sized_crop_f32(fptr, stream.ctypes.data, boxes.ctypes.data, n, dims.ctypes.data, 0, 0, pad, mixed.ctypes.data) == 0
        for s, (r, c) in enumerate(SIZES):
            idx = np.flatnonzero(stream == s)
            bs, ss = np.ascontiguousarray(boxes[idx]), np.ascontiguousarray(stream[idx])
            want = get_crops(bs, frames[s], preprocess="resize_pad" if pad else "resize").transpose(0, 2, 3, 1)
            assert np.array_equal(mixed[idx], want), (pad, s)                                   # (a) the oracle on this frame alone
            one = np.zeros((len(idx), 256, 128, 3), np.float32)
            assert lib.emu_sized_crop_f32(fptr, ss.ctypes.data, bs.ctypes.data, len(idx), None, c, r, pad, one.ctypes.data) == 0
            assert np.array_equal(mixed[idx], one), (pad, s)                                    # (b) the scalar form on this frame alone
    # ---- k_crop_resize_rgbx_hl: (hi, lo) fp16 planes, interior of a zero-bordered (262, 136, 4) buffer ----
    mh, ml = np.zeros((n, 262, 136, 4), np.uint16), np.zeros((n, 262, 136, 4), np.uint16)
    assert lib.emu_sized_crop_hl(fptr, stream.ctypes.data, boxes.ctypes.data, n, dims.ctypes.data, 0, 0, 0, mh.ctypes.data, ml.ctypes.data) == 0
    for s, (r, c) in enumerate(SIZES):
        idx = np.flatnonzero(stream == s)
        bs, ss = np.ascontiguousarray(boxes[idx]), np.ascontiguousarray(stream[idx])
        f = get_crops(bs, frames[s]).transpose(0, 2, 3, 1)
        hi = f.astype(np.float16)
        lo = (f - hi.astype(np.float32)).astype(np.float16)
        assert np.array_equal(mh[idx][:, 3:259, 3:131, :3], hi.view(np.uint16)), s
        assert np.array_equal(ml[idx][:, 3:259, 3:131, :3], lo.view(np.uint16)), s
        oh, ol = np.zeros((len(idx), 262, 136, 4), np.uint16), np.zeros((len(idx), 262, 136, 4), np.uint16)
        assert lib.emu_sized_crop_hl(fptr, ss.ctypes.data, bs.ctypes.data, len(idx), None, c, r, 0, oh.ctypes.data, ol.ctypes.data) == 0
        assert np.array_equal(mh[idx], oh) and np.array_equal(ml[idx], ol), s
    # ---- k_stem_resize_fused_hp: crop + resize + stem + maxpool in one kernel ----
    if not stem_rows:
        return
    import torch

    from oracle.osnet import osnet_forward
    sd = random_osnet_state_dict("osnet_x0_25", seed=0)
    blob = pack_osnet(sd)
    boxes, stream = tables(stem_rows if crop_rows is None else list(range(len(stem_rows))))
    n = len(boxes)
    mh, ml = np.zeros((n, 2048, 16), np.uint16), np.zeros((n, 2048, 16), np.uint16)
    mf = np.zeros((n, 2048, 16), np.float32)
    assert lib.emu_sized_stem_hp(blob.ctypes.data, blob.size, fptr, stream.ctypes.data, boxes.ctypes.data, n, dims.ctypes.data, 0, 0,
                                 mh.ctypes.data, ml.ctypes.data, mf.ctypes.data) == 0
    for s, (r, c) in enumerate(SIZES):
        idx = np.flatnonzero(stream == s)
        bs, ss = np.ascontiguousarray(boxes[idx]), np.ascontiguousarray(stream[idx])
        oh, ol = np.zeros((len(idx), 2048, 16), np.uint16), np.zeros((len(idx), 2048, 16), np.uint16)
        assert lib.emu_sized_stem_hp(blob.ctypes.data, blob.size, fptr, ss.ctypes.data, bs.ctypes.data, len(idx), None, c, r,
                                     oh.ctypes.data, ol.ctypes.data, None) == 0
        assert np.array_equal(mh[idx], oh) and np.array_equal(ml[idx], ol), s                   # (b) bit for bit
        # (a) the oracle's crops of this frame alone through the oracle's stem: the convolution is not bit-comparable with torch, so
        # the bound is the one tests/test_reid_emu.py holds the scalar kernel to (1e-4 of the stage's largest value)
        _, st = osnet_forward(sd, torch.from_numpy(get_crops(bs, frames[s])), return_stages=True)
        ref = st["maxpool"].numpy().transpose(0, 2, 3, 1).reshape(len(idx), 2048, 16)
        err = np.abs(mf[idx] - ref).max() / np.abs(ref).max()
        print(f"stem, frame {r}x{c}: rel max err vs oracle {err:.2e}")
        assert err < 1e-4, (s, err)


@pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")
def test_table_form_crop_kernels_equal_oracle_and_scalar_form_on_four_frame_sizes_emulated():
    _check()


@pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")
def test_table_form_crop_kernels_clean_under_asan():
    """the same launches (fewer crops: every frame's interior, bottom-clipped and other-frame's-interior box) with the harness and the
    kernels built with AddressSanitizer: a read past the end of a small frame -- what a wrong frame size does -- is an error here"""
    rt = subprocess.run([CLANG, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not rt or not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("the host clang has no shared AddressSanitizer runtime")
    code = ("import sys; sys.path[:0]=['.', 'tests']\n"
            "from test_reid_sized_emu import _check\n"
            "_check(sanitize=True, crop_rows=[0, 4, 8], stem_rows=[0, 1, 2])\nprint('ASAN-OK')\n")
    pre = os.environ.get("LD_PRELOAD", "")
    env = dict(os.environ, LD_PRELOAD=rt + (" " + pre if pre else ""), ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500,
                       cwd=str(Path(__file__).resolve().parents[1]))
    assert "ASAN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
