"""Argument checking of boxmot_amd.detpost.DetPost for the oriented layout "cn_obb", without a device: every bad option or shape
raises a ValueError that names what is wrong, before anything goes down to the library."""
import ctypes

import pytest

from boxmot_amd import _lib
from boxmot_amd.detpost import LAYOUTS, NMS_MODES, DetPost
from boxmot_amd.ingest import letterbox_geometry


class Fake:
    """the four things run() asks of a tensor"""

    def __init__(self, shape, dtype="float32", contiguous=True, ptr=0x1000):
        self.shape, self.dtype, self._c, self._p = shape, "torch." + dtype, contiguous, ptr

    def data_ptr(self):
        return self._p

    def is_contiguous(self):
        return self._c


BASE = dict(n_streams=3, n_anchors=100, n_classes=5, max_det=16)


def configured(**kw):
    """the options checked as the constructor checks them, but no handle (there is no device here)"""
    d = DetPost.__new__(DetPost)
    d._handle = None
    d._configure(**dict(BASE, **kw))
    return d


def test_the_oriented_layout_and_its_options():
    assert "cn_obb" in LAYOUTS and NMS_MODES == {"greedy": 0, "fast": 1}
    d = configured(layout="cn_obb")
    assert d.is_obb and d.nms == "greedy" and d.regularize is False and d.det_cols == 7
    assert d.pred_shape() == (3, 10, 100) and d.pred_shape(2) == (2, 10, 100)          # 4 + 5 classes + the angle row
    d = configured(layout="cn_obb", nms="fast", regularize=1)
    assert d.nms == "fast" and d.regularize is True
    assert configured().det_cols == 6 and configured().is_obb is False and configured(layout="nc_obj").pred_shape() == (3, 100, 10)


@pytest.mark.parametrize("kw,word", [
    (dict(layout="cn_obb", nms="soft"), "unknown nms 'soft'"), (dict(layout="cn_obb", nms=1), "unknown nms 1"),
    (dict(layout="cn", nms="greedy"), "belong to layout \"cn_obb\", not to 'cn'"), (dict(layout="nc_obj", nms="fast"), "not to 'nc_obj'"),
    (dict(layout="cn", regularize=False), "belong to layout \"cn_obb\""), (dict(layout="nc_obj", regularize=True), "belong to layout \"cn_obb\""),
    (dict(layout="obb"), "unknown layout 'obb'"), (dict(layout="cn_obb", conf=1.0), "conf"), (dict(layout="cn_obb", max_candidates=4097), "max_candidates"),
    (dict(layout="cn_obb", classes=[5]), "classes"),
])
def test_bad_options(kw, word):
    with pytest.raises(ValueError, match=word):
        configured(**kw)
    with pytest.raises(ValueError, match=word):             # the constructor checks before it looks for a device
        DetPost(**dict(BASE, **kw))


GEO = [letterbox_geometry(480, 640, (64, 64))] * 3


def good():
    return dict(pred=Fake((3, 10, 100), "float16"), geo=GEO, d_dets=Fake((3, 16, 7)), d_det_rows=Fake((3,), "int32"))


@pytest.mark.parametrize("change,word", [
    (dict(pred=Fake((3, 9, 100))), r"pred must have shape \('N >= 3', 10, 100\) for layout 'cn_obb'"), (dict(pred=Fake((3, 100, 10))), "pred must have shape"),
    (dict(pred=Fake((3, 11, 100))), "pred must have shape"), (dict(pred=Fake((3, 10, 100), "float64")), "float16 or float32"),
    (dict(d_dets=Fake((3, 16, 6))), r"d_dets must have shape \(N >= 3, rows, 7\)"), (dict(d_dets=Fake((3, 16, 9))), "rows, 7"),
    (dict(d_dets=Fake((3, 15, 7))), "fewer than max_det = 16"), (dict(d_dets=Fake((2, 16, 7))), "d_dets must have shape"),
    (dict(d_det_rows=Fake((3,), "int64")), "d_det_rows must be int32"), (dict(geo=GEO + GEO), "geo has 6 entries"),
])
def test_bad_run_arguments(change, word):
    d = configured(layout="cn_obb")
    with pytest.raises(ValueError, match=word):
        d.run(**dict(good(), **change))


def test_good_arguments_pass_the_checks():
    d = configured(layout="cn_obb", nms="fast")
    n, dtype, table, stride = d._check_run(**good())
    assert (n, dtype, stride) == (3, 1, 16) and table.shape == (3, 5)
    n, dtype, table, stride = d._check_run(**dict(good(), geo=GEO[:2], pred=Fake((3, 10, 100)), d_dets=Fake((4, 20, 7))))
    assert (n, dtype, stride) == (2, 0, 20)
    with pytest.raises(ValueError, match="rows, 6"):        # and an axis-aligned handle still wants 6 columns
        configured()._check_run(**dict(good(), pred=Fake((3, 9, 100))))


def test_the_c_abi_struct_and_symbol():
    """BoxMOTHipDetPostObbConfig { base; nms_mode; regularize } as include/boxmot_hip.h lays it out, and the entry point's signature"""
    assert [f[0] for f in _lib.DetPostObbConfig._fields_] == ["base", "nms_mode", "regularize"]
    assert _lib.DetPostObbConfig.base.size == ctypes.sizeof(_lib.DetPostConfig) and _lib.DetPostObbConfig.base.offset == 0
    assert _lib.DetPostObbConfig.nms_mode.offset == ctypes.sizeof(_lib.DetPostConfig)
    restype, argtypes = _lib.SIGNATURES["boxmot_hip_detpost_create_obb"]
    assert restype is ctypes.c_void_p and len(argtypes) == 1
    header = (__import__("pathlib").Path(_lib.__file__).resolve().parent.parent / "include" / "boxmot_hip.h").read_text()
    assert "boxmot_hip_detpost_create_obb(const BoxMOTHipDetPostObbConfig* config)" in header
