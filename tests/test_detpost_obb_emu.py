"""Runs the ORIENTED detection post-processing DEVICE kernels (boxmot_amd/csrc/det_post.hpp + det_post_obb.hpp, unchanged) on CPU
threads through tests/host_emu/emu_detpost_obb.cpp, with the library's grids and kernel sequence, and compares every case of
tests/detpost_obb_ref.py bit for bit: rows, counts, counters and the sentinel rows beyond the count.  (The cases keep a margin
around the NMS threshold, so the decisions do not depend on the last bits of cosf / sinf / logf / expf; everything else in a row is
computed exactly.)  A second test builds tests/host_emu/detpost_obb_asan_main.cpp, a stand-alone program, with
-fsanitize=address,undefined and runs it as a child process over the cases' shapes.  Test infrastructure for the kernel logic --
the shipped library has no CPU path."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detpost_obb_ref as ref

HERE = Path(__file__).resolve().parent / "host_emu"
CSRC = HERE.parent.parent / "boxmot_amd" / "csrc"
DEPS = [HERE / "emu_detpost_obb.cpp", HERE / "emu_detpost.cpp", HERE / "hip_shim.hpp", CSRC / "det_post.hpp", CSRC / "det_post_obb.hpp",
        CSRC / "kernel_macros.hpp"]
CXX = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or "g++"       # (a compiler with _Float16)
SENTINEL = np.float32(-12345.5)
MODES = {"greedy": 0, "fast": 1}


def _stale(out, deps):
    return not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps)


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_detpost_obb.so"
    if _stale(out, DEPS):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-w", "-o", str(out),
                               str(HERE / "emu_detpost_obb.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_detpost_obb_run.restype = ctypes.c_long
    lib.emu_detpost_obb_run.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_float] * 2 + \
                                       [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def run_case(lib, c, n_streams=None, **over):
    """(dets (S, stride, 7), det_rows (S,), counters (S, 3)) of a case, the outputs pre-filled with sentinels"""
    S, A, nc = c.dims
    n = S if n_streams is None else n_streams
    o = dict(c.opts, **over)
    preds = np.ascontiguousarray(c.preds)
    geom = np.array([[g[0], g[1], g[2], g[3], g[4]] for g in c.geos], dtype=np.float32)
    allow = None
    if o["classes"] is not None:
        allow = np.zeros(nc, dtype=np.uint8)
        allow[list(o["classes"])] = 1
    dets = np.full((S, c.stride, 7), SENTINEL, dtype=np.float32)
    rows = np.full(S, -77, dtype=np.int32)
    counters = np.full((S, 3), -77, dtype=np.int32)
    lds = lib.emu_detpost_obb_run(n, A, nc, int(preds.dtype == np.float16), preds.ctypes.data, geom.ctypes.data,
                                  None if allow is None else allow.ctypes.data, o["max_candidates"], o["max_det"], int(o["agnostic"]),
                                  MODES[o["nms_mode"]], int(o["regularize"]), np.float32(o["conf"]), np.float32(o["iou"]), dets.ctypes.data, c.stride,
                                  rows.ctypes.data, counters.ctypes.data)
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


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_kernels_on_cpu_threads_equal_the_reference(emu, k):
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), *run_case(emu, c))


def test_the_largest_table_is_the_lds_the_design_states(emu):
    """8 + 20 + 4 + 1 bytes per slot plus the fixed 1648: 136 816 bytes at K = 4096, whatever the tensor's size"""
    small = ref.CASES[ref.NAMES.index("hand_worked_table")]
    geom = np.array([small.geos[0]], dtype=np.float32)
    dets, rows, counters = np.zeros((1, 8, 7), np.float32), np.zeros(1, np.int32), np.zeros((1, 3), np.int32)
    lds = emu.emu_detpost_obb_run(1, 63, 1, 0, np.ascontiguousarray(small.preds).ctypes.data, geom.ctypes.data, None, 4096, 8, 0, 0, 0,
                                  np.float32(0.25), np.float32(0.45), dets.ctypes.data, 8, rows.ctypes.data, counters.ctypes.data)
    assert lds == 4096 * 33 + 1648 == 136816 and rows[0] == 4


def test_fewer_streams_than_the_tensor_leave_the_rest_alone(emu):
    k = ref.NAMES.index("three_geometries_unclipped")
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), *run_case(emu, c, n_streams=2), n_streams=2)


def test_an_unaligned_tensor_takes_the_narrow_score_kernel(emu):
    """the 16-byte loads of k_detpost_score_cn_vec need a 16-byte aligned tensor: one element off, the same case goes through
    k_detpost_score and gives the same bytes -- the finite-angle test included"""
    for name in ("clusters_200_greedy_A600_float16", "non_finite_angle_A64_float16"):
        k = ref.NAMES.index(name)
        c = ref.CASES[k]
        assert c.dims[1] % 8 == 0
        buf = np.zeros(c.preds.size + 16, dtype=c.preds.dtype)
        off = 1 + (-buf.ctypes.data // buf.itemsize) % (16 // buf.itemsize)       # one element past a 16-byte boundary
        view = buf[off:off + c.preds.size].reshape(c.preds.shape)
        view[...] = c.preds
        assert view.ctypes.data % 16 == buf.itemsize and c.preds.ctypes.data % 16 == 0
        assert_equals_reference(c, ref.want(k), *run_case(emu, c._replace(preds=view)))


def test_the_comparison_bites(emu):
    """the mode swap: the chain run in the other mode gives the other mode's reference and not its own; and the reference that
    reads the angle from channel 4 differs from the kernels on the case built for it"""
    kg, kf = ref.NAMES.index("chain_greedy"), ref.NAMES.index("chain_fast")
    for k, other, mode in ((kg, kf, "fast"), (kf, kg, "greedy")):
        dets, rows, counters = run_case(emu, ref.CASES[k], nms_mode=mode)
        assert_equals_reference(ref.CASES[other], ref.want(other), dets, rows, counters)
        assert rows[0] != len(ref.want(k)[0][0])
    k = ref.NAMES.index("angle_in_the_last_row")
    dets, rows, _ = run_case(emu, ref.CASES[k])
    wrong = ref.want(k, angle_row=4)[0][0]
    assert rows[0] != len(wrong) or not np.array_equal(dets[0, :rows[0]], wrong)


def test_the_sanitizer_program_runs_clean():
    """address + undefined-behaviour sanitizers on the emulated kernels, as a stand-alone child process (nothing is loaded into this
    interpreter): the shapes of the cases, S A nc fp16 K max_det nms_mode and a pass rate each"""
    exe = HERE / "detpost_obb_asan_main"
    if _stale(exe, DEPS + [HERE / "detpost_obb_asan_main.cpp"]):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "detpost_obb_asan_main.cpp")])
    shapes = []
    for c in ref.CASES:
        S, A, nc = c.dims
        shape = (min(S, 2), A, nc, int(c.preds.dtype == np.float16), c.opts["max_candidates"], c.opts["max_det"], MODES[c.opts["nms_mode"]])
        if shape not in [s[:7] for s in shapes]:
            shapes.append(shape + (90 if A <= 1000 else 30,))
    args = [str(v) for s in shapes for v in s]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(shapes)} runs" in r.stdout
