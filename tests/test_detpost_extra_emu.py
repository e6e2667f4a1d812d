"""Runs the detection post-processing DEVICE kernels of a head with per-anchor extras (boxmot_amd/csrc/det_post_extra.hpp with
det_post.hpp and det_post_tiled.hpp, unchanged) on CPU threads through tests/host_emu/emu_detpost_extra.cpp, with the library's
grids and kernel sequences, and compares every case of tests/detpost_extra_ref.py bit for bit: rows, counts, counters, extras and
source anchors, and the sentinels beyond the count and in the streams beyond the call's, in all four blocks.  A second test builds
tests/host_emu/detpost_extra_asan_main.cpp, a stand-alone program, with -fsanitize=address,undefined and runs it as a child process
over the cases' shapes.  Test infrastructure for the kernel logic -- the shipped library has no CPU path."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detpost_extra_ref as ref

HERE = Path(__file__).resolve().parent / "host_emu"
CSRC = HERE.parent.parent / "boxmot_amd" / "csrc"
DEPS = [HERE / "emu_detpost_extra.cpp", HERE / "emu_detpost.cpp", HERE / "hip_shim.hpp", CSRC / "det_post.hpp", CSRC / "det_post_obb.hpp",
        CSRC / "det_post_tiled.hpp", CSRC / "det_post_extra.hpp", CSRC / "det_post_select_body.hpp", CSRC / "det_post_tiled_select_body.hpp",
        CSRC / "kernel_macros.hpp"]
CXX = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or "g++"       # (a compiler with _Float16)
SENTINEL = np.float32(-12345.5)
SRC_SENTINEL = -99


def _stale(out, deps):
    return not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps)


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_detpost_extra.so"
    if _stale(out, DEPS):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-w", "-o", str(out),
                               str(HERE / "emu_detpost_extra.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_detpost_extra_run.restype = ctypes.c_long
    lib.emu_detpost_extra_run.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + \
                                         [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p]
    return lib


def run_case(lib, c, n_streams=None, with_src=True, geos=None):
    """(dets (S, stride, 6), det_rows (S,), counters (S, 3), extra (S, stride, E), src (S, stride)) of a case, the outputs pre-filled
    with sentinels"""
    S, A = c.dims
    n = S if n_streams is None else n_streams
    o = c.opts
    preds = np.ascontiguousarray(c.preds)
    geom = np.ascontiguousarray(np.array(c.geos if geos is None else geos, dtype=np.float32))
    allow = None
    if o["classes"] is not None:
        allow = np.zeros(c.nc, dtype=np.uint8)
        allow[list(o["classes"])] = 1
    dets = np.full((S, c.stride, 6), SENTINEL, dtype=np.float32)
    rows = np.full(S, -77, dtype=np.int32)
    counters = np.full((S, 3), -77, dtype=np.int32)
    extra = np.full((S, c.stride, c.E), SENTINEL, dtype=np.float32)
    src = np.full((S, c.stride), SRC_SENTINEL, dtype=np.int32)
    lds = lib.emu_detpost_extra_run(n, c.tiles, A, c.nc, ref.LAYOUTS[c.layout], int(preds.dtype == np.float16), preds.ctypes.data, geom.ctypes.data,
                                    None if allow is None else allow.ctypes.data, o["max_candidates"], o["max_det"], int(o["agnostic"]),
                                    tiled_merge(c), np.float32(o["conf"]), np.float32(o["iou"]), dets.ctypes.data, c.stride, rows.ctypes.data,
                                    counters.ctypes.data, c.E, ref.KINDS[c.kind], extra.ctypes.data, src.ctypes.data if with_src else None)
    assert 0 < lds <= 160 * 1024
    return dets, rows, counters, extra, src


def tiled_merge(c):
    return {"iou": 0, "ios": 1}[c.opts["merge"]] if c.tiles else 0


def assert_equals_reference(c, want, dets, rows, counters, extra, src, n_streams=None, with_src=True):
    S = c.dims[0]
    n = S if n_streams is None else n_streams
    for s in range(n):
        w_rows, w_cnt, w_extra, w_src = want[s]
        k = len(w_rows)
        assert rows[s] == k, (c.name, s, rows[s], k)
        assert counters[s].tolist() == w_cnt.tolist(), (c.name, s)
        assert np.array_equal(dets[s, :k].view(np.uint32), w_rows.view(np.uint32)), (c.name, s)
        assert np.array_equal(extra[s, :k].view(np.uint32), w_extra.view(np.uint32)), (c.name, s, "extras")
        assert (dets[s, k:] == SENTINEL).all() and (extra[s, k:] == SENTINEL).all(), (c.name, s, "rows beyond the count were written")
        if with_src:
            assert np.array_equal(src[s, :k], w_src) and (src[s, k:] == SRC_SENTINEL).all(), (c.name, s, "src")
    for s in range(n, S):
        assert (dets[s] == SENTINEL).all() and rows[s] == -77 and (counters[s] == -77).all() and (extra[s] == SENTINEL).all(), \
            (c.name, s, "a stream beyond the call's was written")
    if not with_src:
        assert (src == SRC_SENTINEL).all()
    else:
        assert (src[n:] == SRC_SENTINEL).all()


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_kernels_on_cpu_threads_equal_the_reference(emu, k):
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), *run_case(emu, c))


@pytest.mark.parametrize("name", ["survivors_cross_a_chunk", "table_A127_nc1_cn_float16_E34_kpt2", "tiled_ios_nc_obj_float16"])
def test_without_a_src_block_the_extras_are_the_same(emu, name):
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), *run_case(emu, c, with_src=False), with_src=False)


@pytest.mark.parametrize("name", ["raw_encodes_stream_anchor_channel_cn", "tiled_iou_cn_float32"])
def test_fewer_streams_than_the_tensor_leave_the_rest_alone(emu, name):
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    n = c.dims[0] - 1
    assert_equals_reference(c, ref.want(k), *run_case(emu, c, n_streams=n), n_streams=n)


def test_the_comparison_bites(emu):
    """the two wrong references differ from the kernels on the cases built for them"""
    k = ref.NAMES.index("survivors_cross_a_chunk")
    c = ref.CASES[k]
    dets, rows, _, extra, src = run_case(emu, c)
    for wrong in (ref.want(k, candidate_order=True), ref.want(k, visibility_is_a_coordinate=True)):
        w_rows, _, w_extra, w_src = wrong[1]
        assert rows[1] == len(w_rows) and not np.array_equal(extra[1, :rows[1]], w_extra)
    assert not np.array_equal(src[1, :rows[1]], ref.want(k, candidate_order=True)[1][3])


def test_the_sanitizer_program_runs_clean():
    """address + undefined-behaviour sanitizers on the emulated kernels, as a stand-alone child process (nothing is loaded into this
    interpreter): the shapes of the cases, S T A nc layout fp16 K max_det E kind and a pass rate each"""
    exe = HERE / "detpost_extra_asan_main"
    if _stale(exe, DEPS + [HERE / "detpost_extra_asan_main.cpp"]):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "detpost_extra_asan_main.cpp")])
    shapes = []
    for c in ref.CASES:
        S, A = c.dims
        shape = (min(S, 2), c.tiles, A, c.nc, ref.LAYOUTS[c.layout], int(c.preds.dtype == np.float16), c.opts["max_candidates"], c.opts["max_det"], c.E,
                 ref.KINDS[c.kind])
        if shape not in [s[:10] for s in shapes]:
            shapes.append(shape + (90,))
    args = [str(v) for s in shapes for v in s]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(shapes)} runs" in r.stdout
