"""Runs the label-map DEVICE kernel (boxmot_amd/csrc/det_post_labels.hpp, unchanged) on CPU threads through
tests/host_emu/emu_detpost_labels.cpp, with the library's grid, and compares every case of tests/detpost_labels_ref.py bit for bit,
the sentinels beyond the frames and in the streams beyond the call's included (the label blocks are pre-filled with -21931).  Every
case runs twice, on the path the kernel chooses (LDS patch, or the fallback where the patch passes the budget) and with the
fallback forced, and both give the reference's bytes.  A second test builds tests/host_emu/detpost_labels_asan_main.cpp, a
stand-alone program, with -fsanitize=address,undefined and runs it as a child process: nothing is loaded into this interpreter
under a sanitizer.  Test infrastructure for the kernel logic -- the shipped library has no CPU path."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detpost_labels_ref as ref

HERE = Path(__file__).resolve().parent / "host_emu"
CSRC = HERE.parent.parent / "boxmot_amd" / "csrc"
DEPS = [HERE / "emu_detpost_labels.cpp", HERE / "emu_detpost.cpp", HERE / "hip_shim.hpp", CSRC / "det_post.hpp", CSRC / "det_post_obb.hpp",
        CSRC / "det_post_tiled.hpp", CSRC / "det_post_extra.hpp", CSRC / "det_post_mask.hpp", CSRC / "det_post_labels.hpp", CSRC / "det_post_select_body.hpp",
        CSRC / "det_post_tiled_select_body.hpp", CSRC / "kernel_macros.hpp"]
CXX = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or "g++"       # (a compiler with _Float16)
SENTINEL = -21931


def _stale(out, deps):
    return not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps)


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_detpost_labels.so"
    if _stale(out, DEPS):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-w", "-o", str(out),
                               str(HERE / "emu_detpost_labels.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_detpost_labels_run.restype = ctypes.c_long
    lib.emu_detpost_labels_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 9
    return lib


def run_case(lib, c, n_streams=None, protos=None, fallback=0, shift=0):
    """labels (S, H, W) int16 of a case, pre-filled with the sentinel.  shift = 1: the prototypes and the labels start one element
    into their blocks, off every wider alignment"""
    S = len(c.geos)
    n = S if n_streams is None else n_streams
    protos = np.ascontiguousarray(c.protos if protos is None else protos)
    proto_block = np.concatenate([np.zeros(shift, dtype=protos.dtype), protos.reshape(-1)])
    geom = np.ascontiguousarray(np.array(c.geos, dtype=np.float32))
    H, W = c.plane
    block = np.full(shift + S * H * W, SENTINEL, dtype=np.int16)
    groups = lib.emu_detpost_labels_run(n, geom.ctypes.data, proto_block.ctypes.data + shift * protos.itemsize, int(protos.dtype == np.float16),
                                        c.dets.ctypes.data, c.stride, c.n_rows.ctypes.data, c.coefs.ctypes.data, block.ctypes.data + 2 * shift, H, W, c.max_det,
                                        c.E, c.mask[0], c.mask[1], c.in_shape[0], c.in_shape[1], fallback)
    assert groups >= n
    assert (block[:shift] == SENTINEL).all()
    return block[shift:].reshape(S, H, W)


def assert_equals_reference(c, want, labels, n_streams=None):
    S = len(c.geos)
    n = S if n_streams is None else n_streams
    for s in range(n):
        rows, cols = want[s].shape
        got = labels[s, :rows, :cols]
        assert got.tobytes() == want[s].tobytes(), (c.name, s, np.argwhere(got != want[s])[:8].tolist())
        rest = labels[s].copy()
        rest[:rows, :cols] = SENTINEL
        assert (rest == SENTINEL).all(), (c.name, s, "a pixel beyond the frame was written")
    for s in range(n, S):
        assert (labels[s] == SENTINEL).all(), (c.name, s, "a stream beyond the call's was written")


@pytest.mark.parametrize("fallback", [0, 1], ids=["chosen_path", "forced_fallback"])
@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_kernel_on_cpu_threads_equals_the_reference(emu, k, fallback):
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), run_case(emu, c, fallback=fallback))


def test_the_chosen_path_is_the_lds_patch_except_where_the_budget_is_passed():
    """what `chosen_path` above ran: every case's tiles fit the patch, but those of patch_beyond_the_budget"""
    for c in ref.CASES:
        for g in c.geos:
            tiles = [(ty, tx) for ty in range(-(-int(g[3]) // ref.TILE_H)) for tx in range(-(-int(g[4]) // ref.TILE_W))]
            over = [np.prod(ref.patch_of(g, c.mask, c.in_shape, tx, ty)) > ref.PATCH for ty, tx in tiles]
            assert all(over) if c.name == "patch_beyond_the_budget" else not any(over), c.name


@pytest.mark.parametrize("name", ["three_streams_float16", "three_streams_float32"])
def test_fewer_streams_than_the_block_leave_the_rest_alone(emu, name):
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), run_case(emu, c, n_streams=2), n_streams=2)


@pytest.mark.parametrize("name", ["three_streams_float16", "table_7x9_frame_24x40_centre_E32_float32", "patch_beyond_the_budget"])
def test_blocks_off_every_wider_alignment_give_the_same(emu, name):
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), run_case(emu, c, shift=1))


WRONG_ON = {"corner": "table_8x8_frame_24x40_centre_E32_float16", "last_wins": "first_wins_three", "threshold_first": "table_12x20_frame_50x31_topleft_E5_float32",
            "letterbox_window": "table_7x9_frame_24x40_centre_E32_float32", "inclusive_edge": "edges_on_integers", "float64_acc": "order_of_the_chain"}


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_the_comparison_bites(emu, wrong):
    """each wrong reference differs from the kernel on the case named for it"""
    k = ref.NAMES.index(WRONG_ON[wrong])
    c = ref.CASES[k]
    labels = run_case(emu, c)
    rows, cols = ref.want(k)[0].shape
    assert labels[0, :rows, :cols].tobytes() == ref.want(k)[0].tobytes()
    assert labels[0, :rows, :cols].tobytes() != ref.want(k, **{wrong: True})[0].tobytes(), wrong


def test_the_sanitizer_program_runs_clean():
    """address + undefined-behaviour sanitizers on the emulated kernel, as a stand-alone child process (nothing is loaded into this
    interpreter): groups of S E proto_fp16 mask_h mask_w in_h in_w rows cols centre n_rows max_det, the shapes of the cases"""
    exe = HERE / "detpost_labels_asan_main"
    if _stale(exe, DEPS + [HERE / "detpost_labels_asan_main.cpp"]):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "detpost_labels_asan_main.cpp")])
    shapes = []
    for c in ref.CASES:
        rows, cols = int(c.geos[0][3]), int(c.geos[0][4])
        shape = (min(len(c.geos), 2), c.E, int(c.protos.dtype == np.float16)) + c.mask + c.in_shape + (rows, cols, int(c.geos[0][2] > 0 or c.geos[0][1] > 0),
                                                                                                   min(int(c.n_rows.max()), c.max_det), c.max_det)
        if shape not in shapes:
            shapes.append(shape)
    shapes.append((1, 5, 1, 12, 20, 40, 64, 20, 70, 1, 8, 8))          # wider than a tile
    args = [str(v) for s in shapes for v in s]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(shapes)} runs" in r.stdout
