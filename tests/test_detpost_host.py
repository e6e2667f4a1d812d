"""Argument checking of boxmot_amd.detpost.DetPost, without a device: every bad option, shape, dtype or geometry raises a
ValueError that names what is wrong, before anything goes down to the library."""
from collections import namedtuple

import pytest

from boxmot_amd.detpost import DetPost
from boxmot_amd.ingest import letterbox_geometry


class Fake:
    """the four things run() asks of a tensor"""

    def __init__(self, shape, dtype="float32", contiguous=True, ptr=0x1000):
        self.shape, self.dtype, self._c, self._p = shape, "torch." + dtype, contiguous, ptr

    def data_ptr(self):
        return self._p

    def is_contiguous(self):
        return self._c


def configured(**kw):
    """the options checked as the constructor checks them, but no handle (there is no device here)"""
    d = DetPost.__new__(DetPost)
    d._handle = None
    d._configure(**dict(dict(n_streams=3, n_anchors=100, n_classes=5, max_det=16), **kw))
    return d


@pytest.mark.parametrize("kw,word", [
    (dict(n_streams=0), "n_streams"), (dict(n_anchors=0), "n_anchors"), (dict(n_classes=0), "n_classes"), (dict(n_anchors=2.5), "n_anchors"),
    (dict(max_det=0), "max_det"), (dict(layout="nc"), "layout"), (dict(conf=1.0), "conf"), (dict(conf=-0.1), "conf"), (dict(conf=float("nan")), "conf"),
    (dict(iou=1.5), "iou"), (dict(iou=-1), "iou"), (dict(max_candidates=63), "max_candidates"), (dict(max_candidates=4097), "max_candidates"),
    (dict(max_candidates=100.5), "max_candidates"), (dict(classes=[5]), "classes"), (dict(classes=[-1]), "classes"), (dict(classes=[]), "classes"),
])
def test_bad_options(kw, word):
    with pytest.raises(ValueError, match=word):
        configured(**kw)
    with pytest.raises(ValueError, match=word):             # the constructor checks before it looks for a device
        DetPost(**dict(dict(n_streams=3, n_anchors=100, n_classes=5, max_det=16), **kw))


def test_options_are_kept_as_the_device_sees_them():
    import numpy as np
    d = configured(conf=0.3, iou=0.45, classes=(1, 4), agnostic=1, layout="nc_obj", max_candidates=64)
    assert d.conf == float(np.float32(0.3)) and d.iou == float(np.float32(0.45)) and d.classes == [1, 4] and d.agnostic is True
    assert d.pred_shape() == (3, 100, 10) and configured().pred_shape(2) == (2, 9, 100)


GEO = [letterbox_geometry(480, 640, (64, 64))] * 3


def good():
    return dict(pred=Fake((3, 9, 100), "float16"), geo=GEO, d_dets=Fake((3, 16, 6)), d_det_rows=Fake((3,), "int32"))


@pytest.mark.parametrize("change,word", [
    (dict(pred=Fake((3, 100, 9))), "pred must have shape"), (dict(pred=Fake((2, 9, 100))), "pred must have shape"),
    (dict(pred=Fake((3, 9, 101))), "pred must have shape"), (dict(pred=Fake((9, 100))), "pred must have shape"),
    (dict(pred=Fake((3, 9, 100), "float64")), "float16 or float32"), (dict(pred=Fake((3, 9, 100), "bfloat16")), "float16 or float32"),
    (dict(pred=Fake((3, 9, 100), contiguous=False)), "pred must be contiguous"), (dict(pred=Fake((3, 9, 100), ptr=0)), "pred has a null"),
    (dict(d_dets=Fake((3, 16, 5))), "d_dets must have shape"), (dict(d_dets=Fake((2, 16, 6))), "d_dets must have shape"),
    (dict(d_dets=Fake((3, 15, 6))), "fewer than max_det = 16"), (dict(d_dets=Fake((3, 16, 6), "float16")), "d_dets must be float32"),
    (dict(d_dets=Fake((3, 16, 6), contiguous=False)), "d_dets must be contiguous"), (dict(d_dets=Fake((3, 16, 6), ptr=0)), "d_dets has a null"),
    (dict(d_det_rows=Fake((2,), "int32")), "d_det_rows must have shape"), (dict(d_det_rows=Fake((3, 1), "int32")), "d_det_rows must have shape"),
    (dict(d_det_rows=Fake((3,), "int64")), "d_det_rows must be int32"), (dict(d_det_rows=Fake((3,), "int32", contiguous=False)), "d_det_rows must be contiguous"),
    (dict(geo=[]), "geo has 0 entries"), (dict(geo=GEO + GEO), "geo has 6 entries"),
    (dict(geo=GEO[:2] + [(1.0, 0, 0, 480)]), "stream 2: geometry"), (dict(geo=[GEO[0], (0.0, 0, 0, 480, 640), GEO[0]]), "stream 1: geometry needs gain > 0"),
    (dict(geo=[GEO[0], GEO[0], (0.5, 0, 0, 0, 640)]), "stream 2: geometry needs"), (dict(geo=["abc", GEO[0], GEO[0]]), "stream 0: geometry"),
])
def test_bad_run_arguments(change, word):
    d = configured()
    with pytest.raises(ValueError, match=word):
        d.run(**dict(good(), **change))


def test_good_arguments_pass_the_checks_and_fewer_streams_are_allowed():
    d = configured()
    n, dtype, table, stride = d._check_run(**good())
    assert (n, dtype, stride) == (3, 1, 16) and table.shape == (3, 5)
    g = GEO[0]
    assert table[0].tolist() == [g.gain, g.top, g.left, 480, 640]
    five = namedtuple("five", "a b c d e")(0.5, 1, 2, 30, 40)
    n, dtype, table, stride = d._check_run(**dict(good(), geo=[GEO[0], five], pred=Fake((3, 9, 100)), d_dets=Fake((4, 20, 6))))
    assert (n, dtype, stride) == (2, 0, 20) and table[1].tolist() == [0.5, 1, 2, 30, 40]
    nc_obj = configured(layout="nc_obj")
    with pytest.raises(ValueError, match="nc_obj"):
        nc_obj.run(**good())
    assert nc_obj._check_run(**dict(good(), pred=Fake((3, 100, 10))))[0] == 3


def test_exported():
    import boxmot_amd
    assert boxmot_amd.DetPost is DetPost and "DetPost" in boxmot_amd.__all__
