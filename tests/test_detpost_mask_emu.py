"""Runs the detection post-processing DEVICE kernels of a mask handle (boxmot_amd/csrc/det_post_mask.hpp with det_post.hpp,
det_post_tiled.hpp and det_post_extra.hpp, unchanged) on CPU threads through tests/host_emu/emu_detpost_mask.cpp, with the library's
grids and kernel sequences, and compares every case of tests/detpost_mask_ref.py bit for bit in all five blocks: rows, counts,
counters, extras, source anchors and masks, and the sentinels beyond the count and in the streams beyond the call's (the masks are
pre-filled with 0xA5).  A second test builds tests/host_emu/detpost_mask_asan_main.cpp, a stand-alone program, with
-fsanitize=address,undefined and runs it as a child process over the cases' shapes: nothing is loaded into this interpreter under
a sanitizer.  Test infrastructure for the kernel logic -- the shipped library has no CPU path."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import detpost_mask_ref as ref

HERE = Path(__file__).resolve().parent / "host_emu"
CSRC = HERE.parent.parent / "boxmot_amd" / "csrc"
DEPS = [HERE / "emu_detpost_mask.cpp", HERE / "emu_detpost.cpp", HERE / "hip_shim.hpp", CSRC / "det_post.hpp", CSRC / "det_post_obb.hpp",
        CSRC / "det_post_tiled.hpp", CSRC / "det_post_extra.hpp", CSRC / "det_post_mask.hpp", CSRC / "det_post_select_body.hpp",
        CSRC / "det_post_tiled_select_body.hpp", CSRC / "kernel_macros.hpp"]
CXX = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++") or "g++"       # (a compiler with _Float16)
SENTINEL = np.float32(-12345.5)
SRC_SENTINEL = -99
MASK_SENTINEL = 0xA5


def _stale(out, deps):
    return not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps)


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_detpost_mask.so"
    if _stale(out, DEPS):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-w", "-o", str(out),
                               str(HERE / "emu_detpost_mask.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_detpost_mask_run.restype = ctypes.c_long
    lib.emu_detpost_mask_run.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + \
                                        [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 4
    return lib


def run_case(lib, c, n_streams=None, with_src=True, protos=None, shift=0):
    """(dets (S, stride, 6), det_rows (S,), counters (S, 3), extra (S, stride, E), src (S, stride), masks (S, stride, mh, mw)) of a
    case, the outputs pre-filled with sentinels.  shift = 1: the prototypes and the masks start one element / one byte into their
    blocks, so the launch takes the byte path whatever the width"""
    S, A = c.dims
    n = S if n_streams is None else n_streams
    o = c.opts
    preds = np.ascontiguousarray(c.preds)
    protos = np.ascontiguousarray(c.protos if protos is None else protos)
    proto_block = np.concatenate([np.zeros(shift, dtype=protos.dtype), protos.reshape(-1)])
    geom = np.ascontiguousarray(np.array(c.geos, dtype=np.float32))
    dets = np.full((S, c.stride, 6), SENTINEL, dtype=np.float32)
    rows = np.full(S, -77, dtype=np.int32)
    counters = np.full((S, 3), -77, dtype=np.int32)
    extra = np.full((S, c.stride, c.E), SENTINEL, dtype=np.float32)
    src = np.full((S, c.stride), SRC_SENTINEL, dtype=np.int32)
    mask_block = np.full(shift + S * c.stride * c.mask[0] * c.mask[1], MASK_SENTINEL, dtype=np.uint8)
    lds = lib.emu_detpost_mask_run(n, c.tiles, A, c.nc, ref.LAYOUTS[c.layout], int(preds.dtype == np.float16), preds.ctypes.data, geom.ctypes.data, None,
                                   o["max_candidates"], o["max_det"], int(o["agnostic"]), {"iou": 0, "ios": 1}[o["merge"]] if c.tiles else 0,
                                   np.float32(o["conf"]), np.float32(o["iou"]), dets.ctypes.data, c.stride, rows.ctypes.data, counters.ctypes.data, c.E,
                                   extra.ctypes.data, src.ctypes.data if with_src else None, proto_block.ctypes.data + shift * protos.itemsize,
                                   int(protos.dtype == np.float16), mask_block.ctypes.data + shift, c.mask[0], c.mask[1], c.in_shape[0], c.in_shape[1])
    assert 0 < lds <= 160 * 1024
    assert (mask_block[:shift] == MASK_SENTINEL).all()
    return dets, rows, counters, extra, src, mask_block[shift:].reshape((S, c.stride) + c.mask)


def assert_equals_reference(c, want, dets, rows, counters, extra, src, masks, n_streams=None, with_src=True):
    S = c.dims[0]
    n = S if n_streams is None else n_streams
    for s in range(n):
        w_rows, w_cnt, w_extra, w_src, w_masks = want[s]
        k = len(w_rows)
        assert rows[s] == k, (c.name, s, rows[s], k)
        assert counters[s].tolist() == w_cnt.tolist(), (c.name, s)
        assert np.array_equal(dets[s, :k].view(np.uint32), w_rows.view(np.uint32)), (c.name, s)
        assert np.array_equal(extra[s, :k].view(np.uint32), w_extra.view(np.uint32)), (c.name, s, "extras")
        assert masks[s, :k].tobytes() == w_masks.tobytes(), (c.name, s, "masks", np.argwhere(masks[s, :k] != w_masks)[:8].tolist())
        assert (dets[s, k:] == SENTINEL).all() and (extra[s, k:] == SENTINEL).all() and (masks[s, k:] == MASK_SENTINEL).all(), \
            (c.name, s, "rows beyond the count were written")
        if with_src:
            assert np.array_equal(src[s, :k], w_src) and (src[s, k:] == SRC_SENTINEL).all(), (c.name, s, "src")
    for s in range(n, S):
        assert (dets[s] == SENTINEL).all() and rows[s] == -77 and (counters[s] == -77).all() and (extra[s] == SENTINEL).all() and \
            (masks[s] == MASK_SENTINEL).all(), (c.name, s, "a stream beyond the call's was written")
    if not with_src:
        assert (src == SRC_SENTINEL).all()
    else:
        assert (src[n:] == SRC_SENTINEL).all()


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_kernels_on_cpu_threads_equal_the_reference(emu, k):
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), *run_case(emu, c))


@pytest.mark.parametrize("name", ["table_8x8_cn_E32_pred_float16_proto_float16", "table_40x72_nc_obj_E32_pred_float32_proto_float32", "tiled_T2_ios",
                                  "more_survivors_than_max_det"])
def test_blocks_off_the_wide_alignment_take_the_byte_path_and_give_the_same(emu, name):
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    assert c.mask[1] % 4 == 0
    assert_equals_reference(c, ref.want(k), *run_case(emu, c, shift=1))


@pytest.mark.parametrize("name", ["table_7x9_cn_E3_pred_float16_proto_float16", "encoding_prototypes_nc_obj", "tiled_T3_ios_cn"])
def test_without_a_src_block_the_masks_are_the_same(emu, name):
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    assert_equals_reference(c, ref.want(k), *run_case(emu, c, with_src=False), with_src=False)


@pytest.mark.parametrize("name", ["encoding_prototypes_cn", "tiled_T2_iou"])
def test_fewer_streams_than_the_tensor_leave_the_rest_alone(emu, name):
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    n = c.dims[0] - 1
    assert_equals_reference(c, ref.want(k), *run_case(emu, c, n_streams=n), n_streams=n)


WRONG_ON = {"descending_k": "order_of_the_chain", "float64_acc": "order_of_the_chain", "inclusive_edge": "window_edges_on_integers",
            "frame_box": "table_8x8_cn_E3_pred_float32_proto_float16", "tile0_protos": "tiled_T2_iou", "ge_zero": "special_logits_proto_float32"}


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_the_comparison_bites(emu, wrong):
    """each wrong reference differs from the kernels on the case built for it"""
    k = ref.NAMES.index(WRONG_ON[wrong])
    c = ref.CASES[k]
    masks = run_case(emu, c)[5]
    differs = False
    for s in range(c.dims[0]):
        n = len(ref.want(k)[s][0])
        assert masks[s, :n].tobytes() == ref.want(k)[s][4].tobytes()
        differs = differs or masks[s, :n].tobytes() != ref.want(k, **{wrong: True})[s][4].tobytes()
    assert differs, wrong


def test_the_sanitizer_program_runs_clean():
    """address + undefined-behaviour sanitizers on the emulated kernels, as a stand-alone child process (nothing is loaded into this
    interpreter): the shapes of the cases, S T A nc layout fp16 K max_det E proto_fp16 mask_h mask_w in_h in_w and a pass rate each"""
    exe = HERE / "detpost_mask_asan_main"
    if _stale(exe, DEPS + [HERE / "detpost_mask_asan_main.cpp"]):
        subprocess.check_call([CXX, "-x", "c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "detpost_mask_asan_main.cpp")])
    shapes = []
    for c in ref.CASES:
        S, A = c.dims
        shape = (min(S, 2), c.tiles, A, c.nc, ref.LAYOUTS[c.layout], int(c.preds.dtype == np.float16), c.opts["max_candidates"], c.opts["max_det"], c.E,
                 int(c.protos.dtype == np.float16)) + c.mask + c.in_shape
        if shape not in [s[:14] for s in shapes]:
            shapes.append(shape + (20,))
    args = [str(v) for s in shapes for v in s]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(shapes)} runs" in r.stdout
