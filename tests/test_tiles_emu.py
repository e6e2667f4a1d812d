"""Runs the two tiled-detection DEVICE kernels -- k_letterbox_tiles (boxmot_amd/csrc/ingest_letterbox_tiles.hpp) and the tiled
post-processing (boxmot_amd/csrc/det_post_tiled.hpp), both unchanged -- on CPU threads through tests/host_emu/emu_tiles.cpp, with
the library's grids, geometry and kernel sequence, and compares them bit for bit with tests/letterbox_tiles_ref.py and
tests/detpost_tiled_ref.py.  A last test builds tests/host_emu/tiles_asan_main.cpp, a stand-alone program, with
-fsanitize=address,undefined and runs it as a child process over the same shapes.  Test infrastructure for the kernel logic -- the
shipped library has no CPU path."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detpost_ref
import detpost_tiled_ref as dref
import letterbox_ref
import letterbox_tiles_ref as lref

HERE = Path(__file__).resolve().parent / "host_emu"
CSRC = HERE.parent.parent / "boxmot_amd" / "csrc"
DEPS = [HERE / "emu_tiles.cpp", HERE / "emu_detpost.cpp", HERE / "hip_shim.hpp"] + [CSRC / n for n in ("ingest_letterbox_tiles.hpp", "ingest_letterbox.hpp", "reid_kernels_v1.hpp",
                                                                             "reid_layout.hpp", "det_post_tiled.hpp", "det_post.hpp", "det_post_obb.hpp",
                                                                             "kernel_macros.hpp")]
CXX = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or "g++"       # (a compiler with _Float16)
CANARY = 0xA5
SENTINEL = np.float32(-12345.5)
MODES = {"center": 0, "topleft": 1}


def _stale(out, deps):
    return not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps)


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_tiles.so"
    if _stale(out, DEPS):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-w", "-o", str(out),
                               str(HERE / "emu_tiles.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_letterbox_tiles_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.emu_letterbox_tile_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.emu_detpost_tiled_run.restype = ctypes.c_long
    lib.emu_detpost_tiled_run.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + \
                                         [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


# ---- k_letterbox_tiles -------------------------------------------------------------------------------------------------------------
def _lut(unit, dtype):
    t = letterbox_ref.table(unit, dtype)
    return t.view(np.uint32).copy() if dtype == np.float32 else t.view(np.uint16).astype(np.uint32)


def run_letterbox(lib, frames, tiles, size, mode="center", dtype=np.float32, rgb=True, unit=True, pad=114, n_extra=0, os_threads=4):
    """the (n * T + n_extra, 3, H, W) block, canary-filled before the call (the n_extra tensors beyond must stay canary), and what the
    call returned; asserts the canary bytes behind the block"""
    n, T, (H, W) = len(frames), len(tiles[0]), size
    elt = np.dtype(dtype).itemsize
    nbytes = (n * T + n_extra) * 3 * H * W * elt
    raw = np.full(nbytes + 64 + 256, CANARY, dtype=np.uint8)
    start = (-raw.ctypes.data) % 64
    buf = raw[start:start + nbytes + 256]
    keep = [np.ascontiguousarray(f) for f in frames]
    ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in keep])
    rows = np.array([f.shape[0] for f in keep], dtype=np.int32)
    cols = np.array([f.shape[1] for f in keep], dtype=np.int32)
    rects = np.ascontiguousarray(np.array(tiles, dtype=np.int32).reshape(n, T, 4))
    lut = _lut(unit, dtype)
    rc = lib.emu_letterbox_tiles_run(n, T, ctypes.addressof(ptrs), rows.ctypes.data, cols.ctypes.data, rects.ctypes.data, H, W, MODES[mode],
                                     int(dtype == np.float16), int(rgb), pad, lut.ctypes.data, buf.ctypes.data, os_threads)
    assert (buf[nbytes:] == CANARY).all() and (raw[:start] == CANARY).all(), "the kernel wrote past the block"
    used = n * T * 3 * H * W * elt
    assert (buf[used:nbytes] == CANARY).all(), "the kernel wrote tensors beyond n_streams * T"
    return buf[:used].view(dtype).reshape(n * T, 3, H, W), rc


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("mode", ["center", "topleft"])
@pytest.mark.parametrize("size", lref.OUT_SIZES, ids=["64x64", "32x64"])
def test_tiles_on_cpu_threads_equal_the_reference(emu, size, mode, dtype):
    got, gx = run_letterbox(emu, lref.FRAMES, lref.TILES, size, mode, dtype, n_extra=2)
    assert gx == -(-size[0] * (size[1] // 8) // 256)
    want = lref.want(size, mode, dtype=dtype)
    for k in range(len(want)):
        assert _same(got[k], want[k]), (size, mode, dtype, "stream", k // lref.T, "tile", lref.TILES[k // lref.T][k % lref.T])


def test_plane_order_scale_and_pad_value(emu):
    for rgb, unit, pad, dtype in [(False, True, 0, np.float16), (True, False, 255, np.float32), (False, False, 7, np.float16)]:
        got, _ = run_letterbox(emu, lref.FRAMES, lref.TILES, (64, 64), "center", dtype, rgb, unit, pad)
        assert _same(got, lref.want((64, 64), "center", rgb, unit, pad, dtype)), (rgb, unit, pad)


def test_the_single_whole_frame_tile_is_the_untiled_letterbox(emu):
    """against letterbox_ref of the frames themselves: T = 1 and the rectangle (0, 0, cols, rows)"""
    whole = [[(0, 0, c, r)] for r, c in lref.SIZES]
    for size in lref.OUT_SIZES:
        for mode in ("center", "topleft"):
            got, _ = run_letterbox(emu, lref.FRAMES, whole, size, mode, np.float16)
            for s, f in enumerate(lref.FRAMES):
                assert _same(got[s], letterbox_ref.letterbox(f, size, mode, dtype=np.float16)), (size, mode, s)


def test_geometry_of_the_device_header_equals_the_reference(emu):
    out = np.zeros(5)
    for rects, (rows, cols) in zip(lref.TILES, lref.SIZES):
        for rect in rects:
            for size in lref.OUT_SIZES + [(640, 640)]:
                for mode in ("center", "topleft"):
                    r = np.array(rect, dtype=np.int32)
                    assert emu.emu_letterbox_tile_geometry(rows, cols, r.ctypes.data, size[0], size[1], MODES[mode], out.ctypes.data) == 1
                    assert tuple(out) == lref.geometry(rect, size, mode)[:5], (rect, size, mode)
    for rect in [(100, 0, 32, 10), (0, 90, 10, 8), (-1, 0, 10, 10), (0, 0, 0, 5), (0, 0, 132, 97)]:         # not inside a 97 x 131 frame
        r = np.array(rect, dtype=np.int32)
        assert emu.emu_letterbox_tile_geometry(97, 131, r.ctypes.data, 64, 64, 0, out.ctypes.data) == -1, rect
    r = np.array((0, 0, 131, 1), dtype=np.int32)                                                            # 1 x 131: no line is left
    assert emu.emu_letterbox_tile_geometry(97, 131, r.ctypes.data, 64, 64, 0, out.ctypes.data) == 0


def test_a_bad_rectangle_is_refused_before_anything_is_written(emu):
    tiles = [list(t) for t in lref.TILES]
    tiles[1][3] = (150, 100, 60, 28)                       # 150 + 60 > 200: outside stream 1's frame
    got, rc = run_letterbox(emu, lref.FRAMES, tiles, (64, 64))
    assert rc == -1 - (1 * lref.T + 3) and (got.view(np.uint8) == CANARY).all()
    tiles[1][3] = (0, 0, 200, 1)                           # a vanishing picture
    got, rc = run_letterbox(emu, lref.FRAMES, tiles, (64, 64))
    assert rc == -1 - (1 * lref.T + 3) and (got.view(np.uint8) == CANARY).all()


# ---- tiled post-processing ----------------------------------------------------------------------------------------------------------
def run_detpost(lib, c, n_streams=None, **over):
    """(dets (S, stride, 6), det_rows (S,), counters (S, 3)) of a case, the outputs pre-filled with sentinels"""
    S, T, A, nc = c.dims
    n = S if n_streams is None else n_streams
    o = dict(c.opts, **over)
    preds = np.ascontiguousarray(c.preds)
    geom = np.ascontiguousarray(np.array(c.geos, dtype=np.float32).reshape(S, T, 7))
    allow = None
    if o["classes"] is not None:
        allow = np.zeros(nc, dtype=np.uint8)
        allow[list(o["classes"])] = 1
    dets = np.full((S, c.stride, 6), SENTINEL, dtype=np.float32)
    rows = np.full(S, -77, dtype=np.int32)
    counters = np.full((S, 3), -77, dtype=np.int32)
    lds = lib.emu_detpost_tiled_run(n, T, A, nc, dref.LAYOUTS[c.layout], int(preds.dtype == np.float16), preds.ctypes.data, geom.ctypes.data,
                                    None if allow is None else allow.ctypes.data, o["max_candidates"], o["max_det"], int(o["agnostic"]),
                                    dref.MERGES[o["merge"]], np.float32(o["conf"]), np.float32(o["iou"]), dets.ctypes.data, c.stride, rows.ctypes.data,
                                    counters.ctypes.data)
    assert 0 < lds <= 160 * 1024
    return dets, rows, counters


def assert_equals_reference(c, want, dets, rows, counters, n_streams=None):
    S = c.dims[0]
    n = S if n_streams is None else n_streams
    for s in range(n):
        w_rows, w_cnt = want[s]
        assert rows[s] == len(w_rows), (c.name, s, rows[s], len(w_rows))
        assert counters[s].tolist() == w_cnt.tolist(), (c.name, s)
        assert np.array_equal(dets[s, :rows[s]].view(np.uint32), w_rows.view(np.uint32)), (c.name, s)
        assert (dets[s, rows[s]:] == SENTINEL).all(), (c.name, s, "rows beyond the count were written")
    for s in range(n, S):
        assert (dets[s] == SENTINEL).all() and rows[s] == -77 and (counters[s] == -77).all(), (c.name, s, "a stream beyond the call's was written")


@pytest.mark.parametrize("k", range(len(dref.CASES)), ids=dref.NAMES)
def test_tiled_kernels_on_cpu_threads_equal_the_reference(emu, k):
    c = dref.CASES[k]
    assert_equals_reference(c, dref.want(k), *run_detpost(emu, c))


def test_fewer_streams_than_the_tensor_leave_the_rest_alone(emu):
    k = dref.NAMES.index("clip_to_the_tile_ios")
    c = dref.CASES[k]
    assert_equals_reference(c, dref.want(k), *run_detpost(emu, c, n_streams=1), n_streams=1)


def test_one_unit_tile_gives_the_untiled_rows(emu):
    """T = 1, unit gain, no padding, boxes inside the frame: the bytes of the untiled definition's reference"""
    for name in dref.IDENTITY:
        k = [c.name for c in detpost_ref.CASES].index(name)
        u = detpost_ref.CASES[k]
        assert u.geos[0] == detpost_ref.GEO_UNIT
        c = dref.Case(name, u.preds[:1], [[dref.TILE_UNIT]], u.layout, dict(u.opts, merge="iou"), u.stride)
        assert_equals_reference(c, [detpost_ref.want(k)[0]], *run_detpost(emu, c))


def test_the_comparison_bites(emu):
    """the two wrong references differ from the kernels on the cases built for them"""
    k = dref.NAMES.index("cut_box_ios_exactly_at_the_threshold")
    dets, rows, _ = run_detpost(emu, dref.CASES[k])
    assert rows[0] == 2 and len(dref.want(k, nms_ge=True)[0][0]) == 1
    k = dref.NAMES.index("equal_conf_tile_order_decides")
    dets, rows, _ = run_detpost(emu, dref.CASES[k])
    wrong = dref.want(k, tiles_high_first=True)[0][0]
    assert rows[0] == len(wrong) == 1 and not np.array_equal(dets[0, :1], wrong)


# ---- both, under the sanitizers -------------------------------------------------------------------------------------------------------
def test_the_sanitizer_program_runs_clean():
    """address + undefined-behaviour sanitizers on the emulated kernels, as a stand-alone child process (nothing is loaded into this
    interpreter): the letterbox shapes of letterbox_tiles_ref (frames as heap blocks of exactly their size, so a tap past a rectangle
    that is flush with the frame's end is an error) and the shapes of detpost_tiled_ref's cases"""
    exe = HERE / "tiles_asan_main"
    if _stale(exe, DEPS + [HERE / "tiles_asan_main.cpp"]):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "tiles_asan_main.cpp")])
    args, runs = [], 0
    for H, W in lref.OUT_SIZES:
        for mode, fp16 in ((0, 1), (1, 0)):
            args += ["L", len(lref.SIZES), lref.T, H, W, mode, fp16] + [v for sz in lref.SIZES for v in sz] + [v for rects in lref.TILES for r in rects for v in r]
            runs += 1
    shapes = []
    for c in dref.CASES:
        S, T, A, nc = c.dims
        shape = (S, T, A, nc, dref.LAYOUTS[c.layout], int(c.preds.dtype == np.float16), c.opts["max_candidates"], c.opts["max_det"], dref.MERGES[c.opts["merge"]])
        if shape not in shapes:
            shapes.append(shape)
    for shape in shapes:
        args += ["D", *shape, 80]
        runs += 1
    r = subprocess.run([str(exe), *[str(v) for v in args]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{runs} runs" in r.stdout
