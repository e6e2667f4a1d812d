"""Host side of the NV12 ingest ring without a device: ``FrameRing(fmt="nv12")``'s validation (before the library is reached),
its shapes against a stand-in library, the unchanged library calls of the default format, and the declaration of the new entry
points in include/boxmot_hip.h and boxmot_amd/_lib.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("boxmot_hip_ingest_create_nv12", "boxmot_hip_ingest_submit_device_nv12", "boxmot_hip_ingest_format",
               "boxmot_hip_ingest_download")


class _NoLib:
    """stands in for the loaded library: reaching it is the failure"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the inputs were validated")


class _FakeLib:
    """records every call; host memory laid out as the library lays out a slot (frames at 256-byte aligned offsets)"""
    def __init__(self):
        self.calls, self.bufs, self.offs = [], {}, None

    def _sizes(self, n, rows_ptr, cols_ptr):
        r = np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(rows_ptr)).tolist()
        c = np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(cols_ptr)).tolist()
        return r, c

    def boxmot_hip_ingest_create(self, n_slots, n_streams, rows, cols):
        self.calls.append(("create", n_slots, n_streams, rows, cols))
        self.offs = [s * rows * cols * 3 for s in range(n_streams + 1)]
        return 1

    def boxmot_hip_ingest_create_sized(self, n_slots, n_streams, rows_ptr, cols_ptr):
        r, c = self._sizes(n_streams, rows_ptr, cols_ptr)
        self.calls.append(("create_sized", n_slots, n_streams, r, c))
        self.offs = [0]
        for a, b in zip(r, c):
            self.offs.append((self.offs[-1] + a * b * 3 + 255) // 256 * 256)
        return 1

    def boxmot_hip_ingest_create_nv12(self, n_slots, n_streams, rows_ptr, cols_ptr):
        r, c = self._sizes(n_streams, rows_ptr, cols_ptr)
        self.calls.append(("create_nv12", n_slots, n_streams, r, c))
        self.offs = [0]
        for a, b in zip(r, c):
            self.offs.append((self.offs[-1] + a * b * 3 // 2 + 255) // 256 * 256)
        return 1

    def boxmot_hip_ingest_host_ptr(self, h, slot, stream):
        self.calls.append(("host_ptr", slot, stream))
        self.bufs.setdefault(slot, (ctypes.c_uint8 * self.offs[-1])())
        return ctypes.addressof(self.bufs[slot]) + self.offs[stream]

    def boxmot_hip_ingest_submit(self, h, slot, n):
        self.calls.append(("submit", slot, n))
        return 1

    def boxmot_hip_ingest_submit_device_nv12(self, h, slot, n, yp, up, py, pu):
        rd = lambda p, t: list((t * n).from_address(p))
        self.calls.append(("submit_device_nv12", slot, n, rd(yp, ctypes.c_uint64), rd(up, ctypes.c_uint64), rd(py, ctypes.c_int32), rd(pu, ctypes.c_int32)))
        return 1

    def boxmot_hip_ingest_destroy(self, h):
        self.calls.append(("destroy",))


def _fake(monkeypatch):
    from boxmot_amd import ingest
    fake = _FakeLib()
    monkeypatch.setattr(ingest._lib, "load", lambda: fake)
    return ingest, fake


def test_default_format_makes_the_library_calls_it_made_before(monkeypatch):
    ingest, fake = _fake(monkeypatch)
    ring = ingest.FrameRing(2, 3, 4, 5)
    assert ring.fmt == "bgr" and fake.calls == [("create", 2, 3, 4, 5)]
    assert ring.host_view(0).shape == (3, 4, 5, 3)
    ring.submit(1)
    ring.close()
    assert fake.calls == [("create", 2, 3, 4, 5), ("host_ptr", 0, 0), ("submit", 1, 3), ("destroy",)]
    fake.calls.clear()
    ring = ingest.FrameRing(2, 2, sizes=[(4, 6), (3, 5)], fmt="bgr")
    assert ring.host_view(1, 1).shape == (3, 5, 3)
    ring.close()
    assert fake.calls == [("create_sized", 2, 2, [4, 3], [6, 5]), ("host_ptr", 1, 1), ("destroy",)]
    # an odd size is fine for BGR frames
    ingest.FrameRing(2, 1, 5, 7).close()


def test_nv12_ring_shapes_and_calls(monkeypatch):
    ingest, fake = _fake(monkeypatch)
    ring = ingest.FrameRing(3, 2, rows=6, cols=10, fmt="nv12")          # a uniform ring still passes a size per stream
    assert fake.calls == [("create_nv12", 3, 2, [6, 6], [10, 10])]
    assert ring.sizes == [(6, 10), (6, 10)] and (ring.rows, ring.cols) == (6, 10) and not ring.mixed     # image sizes, not NV12 sizes
    v = ring.host_view(1)
    assert v.shape == (2, 9, 10) and v.dtype == np.uint8
    assert ring.host_view(1, 1).shape == (9, 10)
    v[0] = 1
    ring.host_view(1, 1)[...] = np.arange(90, dtype=np.uint8).reshape(9, 10)
    raw = np.frombuffer(fake.bufs[1], dtype=np.uint8)
    assert (raw[:90] == 1).all() and (raw[90:256] == 0).all()            # 90 bytes per frame, the second at the 256-byte offset
    assert np.array_equal(raw[256:346], np.arange(90, dtype=np.uint8))
    del v, raw
    held = ring.host_view(0)[1]                                          # a held slice blocks close(), as for BGR
    with pytest.raises(RuntimeError, match="still referenced"):
        ring.close()
    del held
    ring.close()
    assert fake.calls[-1] == ("destroy",)
    # different sizes: per-stream views only
    ring = ingest.FrameRing(2, 2, sizes=[(4, 6), (8, 2)], fmt="nv12")
    assert ring.mixed and ring.host_view(0, 0).shape == (6, 6) and ring.host_view(0, 1).shape == (12, 2)
    with pytest.raises(ValueError, match="use host_view"):
        ring.host_view(0)
    with pytest.raises(ValueError, match="out of range"):
        ring.host_view(0, 2)
    ring.close()


@pytest.mark.parametrize("kw,word", [
    (dict(rows=5, cols=8), "stream 0"),
    (dict(rows=4, cols=7), "stream 0"),
    (dict(sizes=[(4, 8), (6, 9)]), "stream 1"),
    (dict(sizes=[(4, 8), (3, 8)]), "stream 1"),
])
def test_odd_nv12_sizes_raise_before_the_library_is_called(monkeypatch, kw, word):
    from boxmot_amd import _lib
    from boxmot_amd.ingest import FrameRing, nv12_to_bgr
    monkeypatch.setattr(_lib, "load", lambda: _NoLib())
    with pytest.raises(ValueError, match=word):
        FrameRing(2, 2, fmt="nv12", **kw)
    with pytest.raises(ValueError, match="stream 0"):
        nv12_to_bgr(np.zeros((3, 3), np.uint8), 2, 3)
    with pytest.raises(ValueError, match="bytes"):
        nv12_to_bgr(np.zeros((4, 4), np.uint8), 4, 4)


def test_unknown_format_raises_before_the_library_is_called(monkeypatch):
    from boxmot_amd import _lib
    from boxmot_amd.ingest import FrameRing
    monkeypatch.setattr(_lib, "load", lambda: _NoLib())
    for fmt in ("NV12", "i420", "", None):
        with pytest.raises(ValueError, match="fmt"):
            FrameRing(2, 1, 4, 4, fmt=fmt)


def test_submit_device_nv12_validates_then_passes_the_tables(monkeypatch):
    ingest, fake = _fake(monkeypatch)
    ring = ingest.FrameRing(2, 2, sizes=[(4, 8), (6, 10)])               # a BGR ring: only the device side is needed
    fake.calls.clear()
    good = dict(y_ptrs=[4096, 8192], uv_ptrs=[5000, 9000], pitch_y=[8, 16], pitch_uv=[8, 10])
    for name in good:
        for bad in (good[name][:1], good[name] + [1]):
            with pytest.raises(ValueError, match=f"{name} has {len(bad)} entries for 2 streams"):
                ring.submit_device_nv12(0, **dict(good, **{name: bad}))
    with pytest.raises(ValueError, match="stream 1.*pitch"):
        ring.submit_device_nv12(0, **dict(good, pitch_y=[8, 9]))
    with pytest.raises(ValueError, match="stream 0.*pitch"):
        ring.submit_device_nv12(0, **dict(good, pitch_uv=[6, 10]))
    with pytest.raises(ValueError, match="stream 1"):
        ring.submit_device_nv12(0, **dict(good, uv_ptrs=[5000, 0]))
    assert fake.calls == []                                              # nothing reached the library
    ring.submit_device_nv12(1, **good)
    assert fake.calls == [("submit_device_nv12", 1, 2, [4096, 8192], [5000, 9000], [8, 16], [8, 10])]
    ring.close()
    odd = ingest.FrameRing(2, 2, sizes=[(4, 8), (5, 10)])
    fake.calls.clear()
    with pytest.raises(ValueError, match="stream 1"):
        odd.submit_device_nv12(0, **good)
    assert fake.calls == []
    odd.close()


def test_new_symbols_are_declared_and_bound():
    from boxmot_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "boxmot_hip.h").read_text(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b(?:int|BoxMOTHipIngest\*)\s+%s\s*\(" % n, text), f"{n} is not declared in include/boxmot_hip.h"
        assert n in _lib.SIGNATURES
    m = re.search(r"boxmot_hip_ingest_submit_device_nv12\s*\((.*?)\)\s*;", text, re.S)
    assert " ".join(m.group(1).split()) == ("BoxMOTHipIngest* handle, int slot, int n_streams, const uint8_t* const* d_y, "
                                            "const uint8_t* const* d_uv, const int* pitch_y, const int* pitch_uv")
    assert len(_lib.SIGNATURES["boxmot_hip_ingest_submit_device_nv12"][1]) == 7
    assert (ROOT / "boxmot_amd" / "csrc" / "ingest_nv12.hpp").exists()
