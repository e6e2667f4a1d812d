"""The oriented ReID front end's DEVICE sources on CPU threads (tests/host_emu/emu_obb_reid.cpp): the crop geometry function, the
oriented crop-list kernel and the (hi, lo) oriented crop kernels of the fp32-grade family, each against oracle.crops -- bit for bit
(both sides use the host's libm here).  Validates the logic without a GPU; the shipped library has no CPU path."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from obb_reid_common import BLANK_GEOMETRY, expected_planes, geometry_pool, non_finite_boxes, oracle_geometry, same_bits

HERE = Path(__file__).resolve().parent / "host_emu"
CSRC = HERE.parent.parent / "boxmot_amd" / "csrc"
CLANG = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CLANG is None, reason="needs a host clang with _Float16")
VP, I = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_obb_reid.so"
    deps = [HERE / "emu_obb_reid.cpp", HERE / "hip_shim.hpp"] + list(CSRC.glob("*.hpp"))
    if not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-o", str(out),
                               str(HERE / "emu_obb_reid.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_obb_geometry.argtypes = [VP, I, I, VP]
    lib.emu_build_crop_list_obb.argtypes = [VP, VP, I, I, ctypes.c_double, I, I, VP, VP, VP, VP]
    lib.emu_crop_resize_obb_hl.argtypes = [VP, VP, VP, I, I, I, VP, I, I, VP, VP]
    return lib


def _geometry(lib, boxes, stride=5):
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    geo = np.full((len(b), 8), -77.0, dtype=np.float64)
    assert lib.emu_obb_geometry(b.ctypes.data, stride, len(b), geo.ctypes.data) == 0
    return geo


def test_crop_geometry_function_is_bit_equal_to_the_oracle(emu):
    """obb_crop_geometry (the one host / device function) on the pool: all 8 doubles of every box bit-equal to
    oracle.crops.obb_crop_geometry -- special angles, sizes below 1, half-integer sizes (half to even), centres outside the frame."""
    pool = geometry_pool()
    assert len(pool) >= 200 and {0.0, np.float32(np.pi), np.float32(-np.pi / 2)} <= set(pool[:, 4].tolist())
    got = _geometry(emu, pool)
    want = oracle_geometry(pool)
    bad = [i for i in range(len(pool)) if not same_bits(got[i], want[i])]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])
    assert got[9 + 25, 0] == 2 and got[9 + 26, 0] == 4          # w = 2.5 -> 2, 3.5 -> 4: round half to even


def test_non_finite_boxes_get_the_blank_geometry(emu):
    """a NaN or an infinity in any of cx, cy, w, h, angle: out_w = out_h = 1 and a map that sends every pixel outside any frame"""
    bad = non_finite_boxes()
    got = _geometry(emu, bad)
    assert np.array_equal(got, np.tile(BLANK_GEOMETRY, (len(bad), 1)))
    # ... and a finite neighbour in the same launch is untouched by the rule
    mixed = np.concatenate([bad[:2], geometry_pool()[:3]])
    assert same_bits(_geometry(emu, mixed)[2:], oracle_geometry(mixed[2:]))


@pytest.mark.parametrize("inclusive", [0, 1])
def test_oriented_crop_list_kernel_equals_a_numpy_restatement(emu, inclusive):
    """build_crop_list_obb_kernel over 5 streams (one with 0 detections, one with count -1, one with more detections than the
    workgroup has threads): count, the set of (stream, row) pairs and each pair's geometry (bit for bit) against NumPy; rows with
    conf == thresh separate the two `inclusive` settings."""
    rng = np.random.default_rng(21)
    S, nd, thresh = 5, 300, 0.5
    counts = np.array([7, 0, -1, 300, 12], dtype=np.int32)
    pool = geometry_pool()
    dets = np.zeros((S, nd, 7), dtype=np.float32)
    for s in range(S):
        dets[s, :, :5] = pool[rng.integers(0, len(pool), nd)]
        dets[s, :, 5] = rng.choice(np.float32([0.2, 0.5, 0.5, 0.8, 0.49999, 0.50001]), nd)
        dets[s, :, 6] = rng.integers(0, 3, nd)
    dets[4, 3, 0] = np.nan                                       # a non-finite box that passes: blank geometry
    dets[4, 3, 5] = 0.9
    cap = S * nd
    count = np.full(1, -5, dtype=np.int32)
    stream = np.full(cap, -7, dtype=np.int32)
    row = np.full(cap, -7, dtype=np.int32)
    geo = np.full((cap, 8), -77.0, dtype=np.float64)
    assert emu.emu_build_crop_list_obb(dets.ctypes.data, counts.ctypes.data, S, nd, thresh, inclusive, 0, count.ctypes.data, stream.ctypes.data,
                                       row.ctypes.data, geo.ctypes.data) == 0
    want = {}
    for s in range(S):
        for j in range(max(int(counts[s]), 0)):
            cf = float(dets[s, j, 5])
            if (cf >= thresh) if inclusive else (cf > thresh):
                want[(s, s * nd + j)] = dets[s, j, :5]
    n = int(count[0])
    assert n == len(want)
    got = list(zip(stream[:n].tolist(), row[:n].tolist()))
    assert len(set(got)) == n and set(got) == set(want)
    for k, key in enumerate(got):
        box = want[key]
        w = np.tile(BLANK_GEOMETRY, 1) if not np.isfinite(box).all() else oracle_geometry(box[None])[0]
        assert same_bits(geo[k], w), (key, geo[k], w)
    assert (stream[n:] == -7).all() and (row[n:] == -7).all() and (geo[n:] == -77.0).all()       # nothing beyond the count
    assert sum(1 for s, _ in got if s in (1, 2)) == 0
    assert inclusive == 0 or n > sum(1 for key in want if float(dets[key[0], key[1] - key[0] * nd, 5]) > thresh)


FRAME_BOXES = np.array([[100, 80, 40, 90, 0.3], [10, 12, 30, 50, -1.2], [190, 150, 50, 60, 2.0], [96.5, 70.5, 33.4, 71.6, 0.77],
                        [100, 80, 64, 128, 0.0], [100.5, 80.5, 256, 512, 0.0], [60, 100, 0.2, 40, 0.5], [120, 40, 150.5, 20.5, 1.5708],
                        [-30, -40, 40, 40, 0.1], [np.nan, 50, 20, 30, 0.0]], dtype=np.float32)


def _geo_of(boxes):
    ok = np.isfinite(boxes).all(1)
    geo = np.tile(BLANK_GEOMETRY, (len(boxes), 1))
    geo[ok] = oracle_geometry(boxes[ok])
    return geo


@pytest.fixture(scope="module")
def frame_case():
    """a 160 x 200 frame, the boxes above and the expected planes of both preprocess modes (made once; never modified)"""
    img = np.random.default_rng(6).integers(0, 255, (160, 200, 3), dtype=np.uint8)
    finite = FRAME_BOXES[:-1]
    want = {}
    for pre in ("resize", "resize_pad"):
        h, l = expected_planes(finite, img, pre)
        h.setflags(write=False); l.setflags(write=False)
        want[pre] = (h, l)
    return img, want


def _run_hl(lib, imgs, crop_stream, geo, n, dims, count, pad, W=0, H=0, fill=None):
    ptrs = (ctypes.c_void_p * len(imgs))(*[a.ctypes.data for a in imgs])
    cs = np.ascontiguousarray(crop_stream, dtype=np.int32)
    hi = np.zeros((n, 262, 136, 4), dtype=np.float16) if fill is None else np.full((n, 262, 136, 4), fill, dtype=np.float16)
    lo = hi.copy()
    d = None if dims is None else np.ascontiguousarray(dims, dtype=np.int32)
    assert lib.emu_crop_resize_obb_hl(ptrs, cs.ctypes.data, geo.ctypes.data, n, W, H, None if d is None else d.ctypes.data, count, pad,
                                      hi.ctypes.data, lo.ctypes.data) == 0
    return hi, lo


@pytest.mark.parametrize("pre", ["resize", "resize_pad"])
def test_hi_lo_oriented_crop_kernel_equals_the_oracle(emu, frame_case, pre):
    """k_crop_resize_obb_rgbx_hl: planes bit-equal to get_crops_u8 -> LUT -> (hi, lo) split; X channel and border zero; a box with a
    non-finite field is an all-zero crop under "resize"; with count = k < n the planes of crops >= k stay untouched."""
    img, want = frame_case
    wh, wl = want[pre]
    pad = int(pre == "resize_pad")
    geo = _geo_of(FRAME_BOXES)
    n = len(FRAME_BOXES)
    hi, lo = _run_hl(emu, [img], np.zeros(n), geo, n, None, -1, pad, W=200, H=160)
    assert same_bits(hi[:-1], wh) and same_bits(lo[:-1], wl)
    for p in (hi, lo):
        assert not p[..., 3].any() and not p[:, :3].any() and not p[:, 259:].any() and not p[:, :, :3].any() and not p[:, :, 131:].any()
    if not pad:
        zh, zl = expected_planes(np.array([[50, 50, 50, 50]], dtype=np.float32), img, pre)      # an empty axis-aligned box: the all-zero crop
        assert same_bits(hi[-1:], zh) and same_bits(lo[-1:], zl)
    assert np.isfinite(hi[-1].astype(np.float32)).all()
    k = 3
    hi2, lo2 = _run_hl(emu, [img], np.zeros(n), geo, n, None, k, pad, W=200, H=160, fill=7.0)
    assert same_bits(hi2[:k, 3:259, 3:131], wh[:k, 3:259, 3:131]) and same_bits(lo2[:k, 3:259, 3:131], wl[:k, 3:259, 3:131])
    assert (hi2[k:] == np.float16(7.0)).all() and (lo2[k:] == np.float16(7.0)).all()


@pytest.mark.parametrize("pre", ["resize", "resize_pad"])
def test_hi_lo_oriented_crop_kernel_table_form_takes_each_crops_own_frame_size(emu, frame_case, pre):
    """k_crop_resize_obb_rgbx_hl_sized: crops of two frames of different sizes in one launch, each equal to the scalar form's result
    on its own frame; the count works the same way."""
    img, want = frame_case
    img2 = np.ascontiguousarray(np.random.default_rng(7).integers(0, 255, (96, 128, 3), dtype=np.uint8))
    pad = int(pre == "resize_pad")
    boxes = FRAME_BOXES[:6]
    geo = _geo_of(boxes)
    cs = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    dims = np.array([[200, 160], [128, 96]], dtype=np.int32)
    hi, lo = _run_hl(emu, [img, img2], cs, geo, 6, dims, -1, pad)
    wh2, wl2 = expected_planes(boxes, img2, pre)
    for i in range(6):
        eh, el = (want[pre][0][i], want[pre][1][i]) if cs[i] == 0 else (wh2[i], wl2[i])
        assert same_bits(hi[i], eh) and same_bits(lo[i], el), i
    hi2, lo2 = _run_hl(emu, [img, img2], cs, geo, 6, dims, 2, pad, fill=7.0)
    assert same_bits(hi2[:2, 3:259, 3:131], hi[:2, 3:259, 3:131]) and (hi2[2:] == np.float16(7.0)).all() and (lo2[2:] == np.float16(7.0)).all()


def test_the_sanitizer_program_runs_clean():
    """address + undefined-behaviour sanitizers on the emulated crop-list and oriented crop kernels, as a stand-alone child process
    (nothing is loaded into this interpreter): heap buffers of exactly the library's sizes, boxes hanging over every frame edge,
    non-finite fields, an empty stream and a stream with count -1, counted launches"""
    exe = HERE / "obb_reid_asan_main"
    deps = [HERE / "obb_reid_asan_main.cpp", HERE / "emu_obb_reid.cpp", HERE / "hip_shim.hpp"] + list(CSRC.glob("*.hpp"))
    if not exe.exists() or any(d.stat().st_mtime > exe.stat().st_mtime for d in deps):
        subprocess.check_call([CLANG, "-x", "c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-w", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", str(exe), str(HERE / "obb_reid_asan_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "2 runs" in r.stdout
