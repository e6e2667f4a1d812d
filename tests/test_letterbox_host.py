"""Host side of ``FrameRing.letterbox`` without a device: the wrapper's validation against a stand-in library (nothing reaches the
library on bad input, a good call passes the right struct), the declaration of the two entry points in include/boxmot_hip.h and
boxmot_amd/_lib.py, and ``boxmot_hip_letterbox_geometry`` -- which needs no device -- against the Python function."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import letterbox_ref as ref

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("boxmot_hip_letterbox_geometry", "boxmot_hip_ingest_letterbox")


class _FakeLib:
    """records every call"""
    def __init__(self):
        self.calls = []

    def boxmot_hip_ingest_create(self, n_slots, n_streams, rows, cols):
        self.calls.append(("create", n_slots, n_streams, rows, cols))
        return 1

    def boxmot_hip_ingest_create_sized(self, n_slots, n_streams, rows_ptr, cols_ptr):
        self.calls.append(("create_sized", n_slots, n_streams))
        return 1

    def boxmot_hip_ingest_letterbox(self, h, slot, n, cfg, d_out, stream):
        c = cfg._obj
        self.calls.append(("letterbox", slot, n, (c.out_rows, c.out_cols, c.mode, c.dtype, c.rgb, c.unit, c.pad_value), d_out.value, stream.value))
        return 1

    def boxmot_hip_ingest_destroy(self, h):
        self.calls.append(("destroy",))


class _Out:
    """what ``letterbox`` needs of a tensor: data_ptr(), dtype, shape, is_contiguous() -- e.g. a torch tensor"""
    def __init__(self, shape, dtype="torch.float16", ptr=0x7F0000001000, contiguous=True):
        self.shape, self.dtype, self._ptr, self._c = shape, dtype, ptr, contiguous

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return self._c


@pytest.fixture
def ring(monkeypatch):
    from boxmot_amd import ingest
    fake = _FakeLib()
    monkeypatch.setattr(ingest._lib, "load", lambda: fake)
    r = ingest.FrameRing(2, 3, sizes=[(36, 64), (37, 53), (9, 7)])
    fake.calls.clear()
    yield r, fake
    r.close()


def test_a_good_call_passes_the_config_and_returns_the_geometry(ring):
    r, fake = ring
    geo = r.letterbox(1, _Out((3, 3, 32, 48)), hip_stream=0x1234)
    assert fake.calls == [("letterbox", 1, 3, (32, 48, 0, 1, 1, 1, 114), 0x7F0000001000, 0x1234)]
    assert [tuple(g)[1:] for g in geo] == [(48, 27, 2, 0, 36, 64), (46, 32, 0, 1, 37, 53), (25, 32, 0, 11, 9, 7)]
    fake.calls.clear()
    # numpy-style dtype names, YOLOX conventions, fewer streams than the block has rows, an explicit size
    geo = r.letterbox(0, _Out((3, 3, 32, 48), np.dtype(np.float32)), size=(32, 48), mode="topleft", rgb=False, unit=False, pad=0, n_streams=2)
    assert fake.calls == [("letterbox", 0, 2, (32, 48, 1, 0, 0, 0, 0), 0x7F0000001000, None)]
    assert [tuple(g)[1:5] for g in geo] == [(48, 27, 0, 0), (45, 32, 0, 0)]
    assert geo[0] == r.letterbox(0, _Out((2, 3, 32, 48), "float32"), mode="topleft", n_streams=2)[0]


@pytest.mark.parametrize("out,kw,word", [
    (_Out((3, 3, 32, 48), "torch.float64"), {}, "float16 or float32"),
    (_Out((3, 3, 32, 48), "torch.uint8"), {}, "float16 or float32"),
    (_Out((3, 3, 32, 48), contiguous=False), {}, "contiguous"),
    (_Out((2, 3, 32, 48)), {}, "shape"),                                  # fewer rows than streams
    (_Out((3, 32, 48)), {}, "shape"),
    (_Out((3, 1, 32, 48)), {}, "shape"),
    (_Out((3, 3, 32, 48)), dict(size=(32, 40)), "shape"),                 # size and tensor disagree
    (_Out((3, 3, 32, 44)), {}, "multiple of 8"),
    (_Out((3, 3, 32, 48), ptr=0x7F0000001008), {}, "16-byte"),
    (_Out((3, 3, 32, 48), ptr=0), {}, "16-byte"),
    (_Out((3, 3, 32, 48)), dict(mode="middle"), "mode"),
    (_Out((3, 3, 32, 48)), dict(pad=256), "pad"),
    (_Out((3, 3, 32, 48)), dict(pad=-1), "pad"),
    (_Out((3, 3, 32, 48)), dict(n_streams=4), "n_streams"),
    (_Out((3, 3, 32, 48)), dict(n_streams=0), "n_streams"),
])
def test_bad_input_raises_before_the_library_is_reached(ring, out, kw, word):
    r, fake = ring
    with pytest.raises(ValueError, match=word):
        r.letterbox(0, out, **kw)
    assert fake.calls == []


def test_a_degenerate_stream_is_named_before_the_library_is_reached(monkeypatch):
    from boxmot_amd import ingest
    fake = _FakeLib()
    monkeypatch.setattr(ingest._lib, "load", lambda: fake)
    r = ingest.FrameRing(2, 2, sizes=[(8, 8), (3, 200)])
    fake.calls.clear()
    with pytest.raises(ValueError, match="stream 1.*no picture"):
        r.letterbox(0, _Out((2, 3, 16, 64)), mode="topleft")
    assert fake.calls == []
    assert len(r.letterbox(0, _Out((2, 3, 16, 64)), mode="topleft", n_streams=1)) == 1        # the stream is not asked for
    assert len(r.letterbox(0, _Out((2, 3, 16, 64)), mode="center")) == 2                      # center rounds 0.96 up to one line
    r.close()


def test_ingest_module_does_not_import_torch():
    text = (ROOT / "boxmot_amd" / "ingest.py").read_text()
    assert not re.search(r"^\s*(import|from)\s+torch\b", text, flags=re.M)


def test_new_symbols_are_declared_and_bound():
    from boxmot_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "boxmot_hip.h").read_text(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), f"{n} is not declared in include/boxmot_hip.h"
        assert n in _lib.SIGNATURES
    m = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*BoxMOTHipLetterbox\s*;", text, re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1)) == [f[0] for f in _lib.Letterbox._fields_]
    assert ctypes.sizeof(_lib.Letterbox) == 28
    m = re.search(r"boxmot_hip_ingest_letterbox\s*\((.*?)\)\s*;", text, re.S)
    assert " ".join(m.group(1).split()) == ("BoxMOTHipIngest* handle, int slot, int n_streams, const BoxMOTHipLetterbox* cfg, void* d_out, "
                                            "void* consumer_hip_stream")
    assert len(_lib.SIGNATURES["boxmot_hip_ingest_letterbox"][1]) == 6 and len(_lib.SIGNATURES["boxmot_hip_letterbox_geometry"][1]) == 4
    assert (ROOT / "boxmot_amd" / "csrc" / "ingest_letterbox.hpp").exists()


def test_library_geometry_equals_the_python_function():
    """boxmot_hip_letterbox_geometry takes no handle and no device: the table of the definition, then a few hundred random sizes"""
    import __graft_entry__ as g
    g.build()
    from boxmot_amd import _lib
    from boxmot_amd.ingest import letterbox_geometry
    lib = _lib.load()
    rng = np.random.default_rng(1)
    sizes = [(f, s) for f, s, _ in ref.ALL_SHAPES] + [((720, 1280), (640, 640)), ((1080, 1920), (640, 640)), ((2160, 3840), (384, 640))]
    sizes += [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in zip(rng.integers(1, 2200, 400), rng.integers(1, 4000, 400),
                                                                        rng.integers(1, 1300, 400), rng.integers(1, 1300, 400))]
    # thin frames into small outputs, where the picture shrinks to nothing
    sizes += [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in zip(rng.integers(1, 7, 100), rng.integers(300, 4000, 100),
                                                                        rng.integers(1, 40, 100), rng.integers(8, 600, 100))]
    out = (ctypes.c_double * 5)()
    bad = 0
    for (rows, cols), (H, W) in sizes:
        for mode, m in (("center", 0), ("topleft", 1)):
            cfg = _lib.Letterbox(H, W, m, 0, 1, 1, 114)
            ok = lib.boxmot_hip_letterbox_geometry(rows, cols, ctypes.byref(cfg), out)
            try:
                want = letterbox_geometry(rows, cols, (H, W), mode)
            except ValueError:
                bad += 1
                assert not ok and "no picture" in _lib.last_error(), (rows, cols, H, W, mode)
                continue
            assert ok and tuple(out) == tuple(want)[:5], (rows, cols, H, W, mode)
            assert want[1:5] == ref.geometry(rows, cols, (H, W), mode)[1:]
    assert bad > 0                                                        # the random sizes include pictures that vanish
    cfg = _lib.Letterbox(16, 64, 1, 0, 1, 1, 114)
    assert not lib.boxmot_hip_letterbox_geometry(3, 200, ctypes.byref(cfg), out) and "3 x 200" in _lib.last_error()
    assert tuple(out)[1:] == (64.0, 0.0, 0.0, 0.0)                        # filled even so
    cfg.mode = 2
    assert not lib.boxmot_hip_letterbox_geometry(8, 8, ctypes.byref(cfg), out) and "mode" in _lib.last_error()
    assert not lib.boxmot_hip_letterbox_geometry(8, 8, None, out) and "null" in _lib.last_error()
    assert not lib.boxmot_hip_letterbox_geometry(0, 8, ctypes.byref(_lib.Letterbox(16, 64, 0, 0, 1, 1, 114)), out)
