"""Runs the ingest ring's letterbox DEVICE kernel (boxmot_amd/csrc/ingest_letterbox.hpp, unchanged) on CPU threads through
tests/host_emu/emu_letterbox.cpp, with the grid and the geometry the library uses, and compares it bit for bit with
tests/letterbox_ref.py: every shape of the definition's table, shapes one thread / one workgroup past a workgroup's span, both
modes, both dtypes, rgb and unit on and off, streams of different frame sizes in one launch, canary bytes behind the block.  Test
infrastructure for the kernel logic -- the shipped library has no CPU path."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import letterbox_ref as ref

HERE = Path(__file__).resolve().parent / "host_emu"
CANARY = 0xA5
MODES = {"center": 0, "topleft": 1}


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_letterbox.so"
    csrc = HERE.parent.parent / "boxmot_amd" / "csrc"
    deps = [HERE / "emu_letterbox.cpp", HERE / "hip_shim.hpp", csrc / "ingest_letterbox.hpp", csrc / "reid_kernels_v1.hpp",
            csrc / "reid_layout.hpp", csrc / "kernel_macros.hpp"]
    if not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-w", "-o", str(out),
                               str(HERE / "emu_letterbox.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_letterbox_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + \
                                     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.emu_letterbox_geometry.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return lib


def _lut(unit, dtype):
    """the table as the library passes it: one 32-bit word per byte value holding the element's bits"""
    t = ref.table(unit, dtype)
    return t.view(np.uint32).copy() if dtype == np.float32 else t.view(np.uint16).astype(np.uint32)


def _run(lib, frames, size, mode="center", dtype=np.float32, rgb=True, unit=True, pad=114, n_out=None, os_threads=4):
    """frames: (rows, cols, 3) uint8 arrays, one per stream.  Returns the (n_out, 3, H, W) block (n_out >= the stream count: the
    rows beyond must stay canary) and grid.x; asserts the canary bytes behind the block."""
    n, (H, W) = len(frames), size
    n_out = n_out or n
    elt = np.dtype(dtype).itemsize
    nbytes = n_out * 3 * H * W * elt
    raw = np.full(nbytes + 64 + 256, CANARY, dtype=np.uint8)
    start = (-raw.ctypes.data) % 64
    buf = raw[start:start + nbytes + 256]                                   # 64-byte aligned, 256 canary bytes behind the block
    keep = [np.ascontiguousarray(f) for f in frames]
    ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in keep])
    rows = np.array([f.shape[0] for f in keep], dtype=np.int32)
    cols = np.array([f.shape[1] for f in keep], dtype=np.int32)
    lut = _lut(unit, dtype)
    gx = lib.emu_letterbox_run(n, ctypes.addressof(ptrs), rows.ctypes.data, cols.ctypes.data, H, W, MODES[mode], int(dtype == np.float16),
                               int(rgb), pad, lut.ctypes.data, buf.ctypes.data, os_threads)
    assert (buf[nbytes:] == CANARY).all(), "the kernel wrote past the block"
    assert (raw[:start] == CANARY).all()
    out = buf[:nbytes].view(dtype).reshape(n_out, 3, H, W)
    if n_out > n:
        assert (buf[n * 3 * H * W * elt:nbytes] == CANARY).all(), "the kernel wrote rows beyond the stream count"
    return out, gx


def _same(got, want):
    """bit for bit (an fp16 0.0 and a -0.0, or two NaNs, would not pass as equal values do)"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("mode", ["center", "topleft"])
@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=[c[0] for c in ref.CASES])
def test_kernel_on_cpu_threads_equals_the_reference(emu, k, mode):
    _, frame, size = ref.CASES[k]
    for dtype in (np.float16, np.float32):
        got, gx = _run(emu, [frame], size, mode, dtype)
        assert gx == -(-size[0] * (size[1] // 8) // 256)
        assert _same(got[0], ref.want(k, mode, dtype=dtype)), (mode, dtype)


@pytest.mark.parametrize("rgb,unit,pad", [(False, True, 114), (True, False, 114), (False, False, 0), (True, True, 255)])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_plane_order_scale_and_pad_value(emu, rgb, unit, pad, dtype):
    for k in (0, 5, 8, 10):                 # a 2x, a general downscale, an upscale with padding left and right, the wide own shape
        _, frame, size = ref.CASES[k]
        got, _ = _run(emu, [frame], size, "center", dtype, rgb, unit, pad)
        assert _same(got[0], ref.want(k, "center", rgb, unit, pad, dtype)), ref.CASES[k][0]


@pytest.mark.parametrize("mode", ["center", "topleft"])
def test_streams_of_different_frame_sizes_share_one_launch(emu, mode):
    """every frame of the table as a stream of ONE launch into a common (40, 72), where none of them is special-cased by its own
    output size; two rows of the block beyond the stream count stay untouched"""
    frames = [c[1] for c in ref.CASES[:len(ref.ALL_SHAPES)]]
    for dtype in (np.float16, np.float32):
        got, gx = _run(emu, frames, (40, 72), mode, dtype, n_out=len(frames) + 2)
        assert gx == 2                      # 40 rows x 9 thread columns = 360 threads
        for s, f in enumerate(frames):
            assert _same(got[s], ref.letterbox(f, (40, 72), mode, dtype=dtype)), (s, f.shape)


def test_geometry_of_the_device_header_equals_the_reference(emu):
    rng = np.random.default_rng(0)
    sizes = [(f, s) for f, s, _ in ref.ALL_SHAPES] + [((3, 200), (16, 64)), ((720, 1280), (640, 640)), ((1080, 1920), (640, 640))]
    sizes += [((int(a), int(b)), (int(c), int(d) * 8)) for a, b, c, d in zip(rng.integers(1, 2200, 300), rng.integers(1, 4000, 300),
                                                                            rng.integers(1, 1300, 300), rng.integers(1, 160, 300))]
    out = np.zeros(5)
    for (rows, cols), size in sizes:
        for mode in ("center", "topleft"):
            ok = emu.emu_letterbox_geometry(rows, cols, size[0], size[1], MODES[mode], out.ctypes.data)
            want = ref.geometry(rows, cols, size, mode)
            assert bool(ok) == (want is not None), (rows, cols, size, mode)
            if want:
                assert tuple(out) == want, (rows, cols, size, mode)


def test_a_degenerate_stream_is_refused(emu):
    frames = [ref.make_frame(8, 8), ref.make_frame(3, 200)]
    lut = _lut(True, np.float32)
    ptrs = (ctypes.c_void_p * 2)(*[f.ctypes.data for f in frames])
    rows, cols = np.array([8, 3], np.int32), np.array([8, 200], np.int32)
    out = np.zeros(2 * 3 * 16 * 64, np.float32)
    assert emu.emu_letterbox_run(2, ctypes.addressof(ptrs), rows.ctypes.data, cols.ctypes.data, 16, 64, 1, 0, 1, 114, lut.ctypes.data,
                                 out.ctypes.data, 1) == -2       # stream 1
    assert (out == 0).all()
