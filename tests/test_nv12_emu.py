"""Runs the ingest ring's NV12 -> BGR DEVICE kernel (boxmot_amd/csrc/ingest_nv12.hpp, unchanged) on CPU threads through
tests/host_emu/emu_nv12.cpp, with the grid the library launches, and compares it bit for bit with tests/nv12_ref.py: both
paths (2 x 8 and 2 x 2 pixels per thread), pitches, misaligned bases, sizes one thread-column / one tile past a workgroup, streams
of different sizes in one launch, and every (Y, U, V) triple.  Test infrastructure for the kernel logic -- the shipped library
has no CPU path."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nv12_ref import exhaustive_frame, nv12_to_bgr, random_frame

HERE = Path(__file__).resolve().parent / "host_emu"
CANARY = 0xA5


@pytest.fixture(scope="module")
def emu():
    out = HERE / "libemu_nv12.so"
    csrc = HERE.parent.parent / "boxmot_amd" / "csrc"
    deps = [HERE / "emu_nv12.cpp", HERE / "hip_shim.hpp", csrc / "ingest_nv12.hpp", csrc / "kernel_macros.hpp"]
    if not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-pthread", "-o", str(out),
                               str(HERE / "emu_nv12.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.emu_nv12_run.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 8 + [ctypes.c_int]
    return lib


def _aligned(nbytes, offset=0, fill=0):
    """uint8 buffer of nbytes whose address is ``offset`` past a multiple of 64"""
    raw = np.full(nbytes + 128, fill, dtype=np.uint8)
    start = (-raw.ctypes.data) % 64 + offset
    return raw[start:start + nbytes]


def _convert(lib, streams, os_threads=4):
    """streams: dicts with frame (tight NV12), rows, cols and optionally pitch_y, pitch_uv, off_y, off_uv, off_dst (bytes past an
    aligned address).  Returns ([BGR per stream], [wide flag per stream], grid.x)."""
    n = len(streams)
    keep, ys, uvs, dsts = [], [], [], []
    for st in streams:
        r, c = st["rows"], st["cols"]
        py, pu = st.get("pitch_y", c), st.get("pitch_uv", c)
        f = np.asarray(st["frame"], np.uint8).reshape(r * 3 // 2, c)
        y = _aligned(r * py, st.get("off_y", 0), 0x11).reshape(r, py)
        uv = _aligned(r // 2 * pu, st.get("off_uv", 0), 0x22).reshape(r // 2, pu)
        y[:, :c] = f[:r]
        uv[:, :c] = f[r:]
        dst = _aligned(r * c * 3 + 64, st.get("off_dst", 0), CANARY)       # 64 canary bytes behind the frame
        ys.append(y); uvs.append(uv); dsts.append(dst)
    arr = lambda v: np.array(v, dtype=np.int32)
    ptrs = lambda v: (ctypes.c_void_p * n)(*[a.ctypes.data for a in v])
    rows, cols = arr([s["rows"] for s in streams]), arr([s["cols"] for s in streams])
    py, pu = arr([y.shape[1] for y in ys]), arr([u.shape[1] for u in uvs])
    yp, up, dp = ptrs(ys), ptrs(uvs), ptrs(dsts)
    wide = np.zeros(n, dtype=np.int32)
    gx = lib.emu_nv12_run(n, ctypes.addressof(yp), ctypes.addressof(up), py.ctypes.data, pu.ctypes.data, rows.ctypes.data, cols.ctypes.data,
                          ctypes.addressof(dp), wide.ctypes.data, os_threads)
    outs = []
    for st, d in zip(streams, dsts):
        nb = st["rows"] * st["cols"] * 3
        assert (d[nb:] == CANARY).all(), "the kernel wrote past the frame"
        outs.append(d[:nb].reshape(st["rows"], st["cols"], 3).copy())
    return outs, wide.tolist(), gx


def _case(rows, cols, seed, **kw):
    return dict(frame=random_frame(rows, cols, seed), rows=rows, cols=cols, **kw)


# rows, cols, pitch_y, pitch_uv, takes the 2 x 8 path.  64 thread columns x 4 thread rows per workgroup: 520 = 8 * 65 and 130 = 2 * 65
# columns need one thread column more than a workgroup spans, 10 rows (5 thread rows) one more tile in y
SHAPES = [
    (2, 2, 2, 2, False),
    (6, 10, 10, 10, False),
    (18, 34, 48, 40, False),
    (16, 64, 64, 64, True),
    (10, 72, 128, 128, True),
    (4, 520, 520, 520, True),
    (4, 130, 130, 130, False),
    (10, 6, 6, 6, False),
    (10, 1032, 1040, 1032, True),        # 129 thread columns: three tiles in x, two in y
    (8, 64, 68, 64, False),              # a Y pitch that is no multiple of 8 rules the wide path out
    (8, 64, 64, 100, False),
]


@pytest.mark.parametrize("rows,cols,pitch_y,pitch_uv,wide", SHAPES)
def test_kernel_on_cpu_threads_equals_the_reference(emu, rows, cols, pitch_y, pitch_uv, wide):
    st = _case(rows, cols, rows * 1000 + cols, pitch_y=pitch_y, pitch_uv=pitch_uv)
    (got,), (w,), _ = _convert(emu, [st])
    assert bool(w) == wide
    assert np.array_equal(got, nv12_to_bgr(st["frame"], rows, cols))


@pytest.mark.parametrize("which", ["off_y", "off_uv", "off_dst"])
def test_a_misaligned_base_takes_the_narrow_path_and_gives_the_same_bytes(emu, which):
    st = _case(12, 136, 7)
    (a,), (wa,), _ = _convert(emu, [st])
    (b,), (wb,), _ = _convert(emu, [dict(st, **{which: 4})])
    assert wa == 1 and wb == 0
    assert np.array_equal(a, b) and np.array_equal(a, nv12_to_bgr(st["frame"], 12, 136))


def test_streams_of_different_sizes_share_one_launch(emu):
    sts = [_case(24, 1040, 1), _case(6, 10, 2), _case(122, 166, 3), _case(16, 64, 4, pitch_y=72, pitch_uv=80)]
    outs, wide, gx = _convert(emu, sts)
    assert wide == [1, 0, 0, 1]
    # tiles: 24 x 1040 wide = 3 x 3, 6 x 10 narrow = 1, 122 x 166 narrow = ceil(83 / 64) x ceil(61 / 4) = 2 x 16, 16 x 64 wide = 1 x 2
    assert gx == 32
    for st, got in zip(sts, outs):
        assert np.array_equal(got, nv12_to_bgr(st["frame"], st["rows"], st["cols"])), (st["rows"], st["cols"])


def test_every_yuv_triple(emu):
    """The exhaustive 4096 x 4096 frame (every one of the 2^24 (Y, U, V) byte triples once), whole -- not a corner of it: the
    emulated threads of this kernel run as plain loops, a few seconds in all.  Wide path, then the same frame through the narrow
    path (a destination 4 bytes off alignment) on its first 128 rows."""
    f = exhaustive_frame()
    want = nv12_to_bgr(f, 4096, 4096)
    assert 0.15 < (want == 255).mean() < 0.25 and 0.15 < (want == 0).mean() < 0.25       # about a fifth saturates either way
    (got,), (w,), _ = _convert(emu, [dict(frame=f, rows=4096, cols=4096)], os_threads=8)
    assert w == 1
    assert np.array_equal(got, want)
    top = np.concatenate([f[:128], f[4096:4096 + 64]])
    (got,), (w,), _ = _convert(emu, [dict(frame=top, rows=128, cols=4096, off_dst=4)])
    assert w == 0
    assert np.array_equal(got, want[:128])
