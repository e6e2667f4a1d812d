"""Argument checking of boxmot_amd.detpost.DetPost.labels, without a device: every bad shape, dtype, layout or address raises a
ValueError that names what is wrong, before anything goes down to the library; a handle without masks and a tiled mask handle
are refused; the ctypes signature is the header's; ``_check_run`` and ``_check_mask`` keep their signatures."""
import inspect

import pytest

from boxmot_amd import _lib
from boxmot_amd.detpost import MAX_LABEL_DET, DetPost
from boxmot_amd.ingest import letterbox_geometry


class Fake:
    """the four things labels() asks of a tensor"""

    def __init__(self, shape, dtype="float32", contiguous=True, ptr=0x1000):
        self.shape, self.dtype, self._c, self._p = shape, "torch." + dtype, contiguous, ptr

    def data_ptr(self):
        return self._p

    def is_contiguous(self):
        return self._c


BASE = dict(n_streams=2, n_anchors=100, n_classes=5, max_det=16)
MASK = dict(extra=32, mask=(12, 20), in_shape=(40, 64))


def configured(**kw):
    """the options checked as the constructor checks them, but no handle (there is no device here)"""
    d = DetPost.__new__(DetPost)
    d._handle = None
    d._configure(**dict(BASE, **kw))
    return d


GEO = [letterbox_geometry(480, 640, (40, 64)), letterbox_geometry(360, 500, (40, 64))]


def good():
    return dict(geo=GEO, d_proto=Fake((2, 32, 12, 20), "float16"), d_dets=Fake((2, 20, 6)), d_det_rows=Fake((2,), "int32"), d_extra=Fake((2, 20, 32)),
                d_labels=Fake((2, 480, 640), "int16"))


@pytest.mark.parametrize("change,word", [
    (dict(geo=[]), "geo has 0 entries"), (dict(geo=GEO * 2), "geo has 4 entries"), (dict(geo=[GEO[0], (1.0, 0, 0)]), "stream 1: geometry must be"),
    (dict(geo=[(0.0, 0, 0, 480, 640)]), "stream 0: geometry needs gain > 0"),
    (dict(d_proto=Fake((1, 32, 12, 20))), "d_proto must have shape"), (dict(d_proto=Fake((2, 31, 12, 20))), "d_proto must have shape"),
    (dict(d_proto=Fake((2, 32, 20, 12))), "d_proto must have shape"), (dict(d_proto=Fake((2, 32, 240))), "d_proto must have shape"),
    (dict(d_proto=Fake((2, 32, 12, 20), "bfloat16")), "d_proto must be float16 or float32"), (dict(d_proto=Fake((2, 32, 12, 20), contiguous=False)), "d_proto must be contiguous"),
    (dict(d_proto=Fake((2, 32, 12, 20), ptr=0)), "d_proto has a null"),
    (dict(d_dets=Fake((1, 20, 6))), "d_dets must have shape"), (dict(d_dets=Fake((2, 20, 7))), "d_dets must have shape"), (dict(d_dets=Fake((2, 120))), "d_dets must have shape"),
    (dict(d_dets=Fake((2, 15, 6)), d_extra=Fake((2, 15, 32))), "fewer than max_det = 16"), (dict(d_dets=Fake((2, 20, 6), "float16")), "d_dets must be float32"),
    (dict(d_dets=Fake((2, 20, 6), contiguous=False)), "d_dets must be contiguous"), (dict(d_dets=Fake((2, 20, 6), ptr=0)), "d_dets has a null"),
    (dict(d_det_rows=Fake((1,), "int32")), "d_det_rows must have shape"), (dict(d_det_rows=Fake((2, 1), "int32")), "d_det_rows must have shape"),
    (dict(d_det_rows=Fake((2,), "int64")), "d_det_rows must be int32"), (dict(d_det_rows=Fake((2,), "int32", contiguous=False)), "d_det_rows must be contiguous"),
    (dict(d_det_rows=Fake((2,), "int32", ptr=0)), "d_det_rows has a null"),
    (dict(d_extra=Fake((1, 20, 32))), "d_extra must have shape"), (dict(d_extra=Fake((2, 16, 32))), "d_extra must have shape"), (dict(d_extra=Fake((2, 20, 31))), "d_extra must have shape"),
    (dict(d_extra=Fake((2, 20, 32), "float16")), "d_extra must be float32"), (dict(d_extra=Fake((2, 20, 32), contiguous=False)), "d_extra must be contiguous"),
    (dict(d_extra=Fake((2, 20, 32), ptr=0)), "d_extra has a null"),
    (dict(d_labels=Fake((1, 480, 640), "int16")), "d_labels must have shape"), (dict(d_labels=Fake((2, 480 * 640), "int16")), "d_labels must have shape"),
    (dict(d_labels=Fake((2, 0, 640), "int16")), "d_labels must have shape"), (dict(d_labels=Fake((2, 480, 640), "int32")), "d_labels must be int16"),
    (dict(d_labels=Fake((2, 480, 640), "uint8")), "d_labels must be int16"), (dict(d_labels=Fake((2, 480, 640), "int16", contiguous=False)), "d_labels must be contiguous"),
    (dict(d_labels=Fake((2, 480, 640), "int16", ptr=0)), "d_labels has a null"),
    (dict(d_labels=Fake((2, 479, 640), "int16")), "stream 0: the frame of 480 x 640 does not fit"), (dict(d_labels=Fake((2, 480, 639), "int16")), "stream 0: the frame of 480 x 640 does not fit"),
    (dict(geo=GEO[::-1], d_labels=Fake((2, 400, 640), "int16")), "stream 1: the frame of 480 x 640 does not fit"),
])
def test_bad_labels_arguments(change, word):
    d = configured(**MASK)
    with pytest.raises(ValueError, match=word) as e:
        d.labels(**dict(good(), **change))
    assert str(e.value).startswith("DetPost.labels: ") or "geometry" in word          # (the geometry rows' messages are _geometry_row's)


def test_good_arguments_pass_the_checks():
    d = configured(**MASK)
    n, pdtype, table, stride, rows, cols = d._check_labels(**good())
    assert (n, pdtype, stride, rows, cols) == (2, 1, 20, 480, 640) and table.shape == (2, 5) and table[1, 3:].tolist() == [360.0, 500.0]
    g = dict(good(), geo=GEO[1:], d_proto=Fake((3, 32, 12, 20), "float32"), d_labels=Fake((4, 361, 501), "int16"))     # fewer streams, larger blocks
    assert d._check_labels(**g)[:2] == (1, 0) and d._check_labels(**g)[4:] == (361, 501)
    assert configured(**dict(MASK, max_det=MAX_LABEL_DET))._check_labels(**dict(good(), d_dets=Fake((2, MAX_LABEL_DET, 6)), d_extra=Fake((2, MAX_LABEL_DET, 32))))[0] == 2


@pytest.mark.parametrize("kw,word", [
    (dict(), "belong to a mask handle"), (dict(extra=32), "belong to a mask handle"), (dict(extra=51, extra_kind="kpt3"), "belong to a mask handle"),
    (dict(tiles=2), "belong to a mask handle"), (dict(layout="cn_obb"), "belong to a mask handle"),
    (dict(MASK, tiles=3), "tiled handle.*out of scope"), (dict(MASK, tiles=1, merge="ios"), "tiled handle.*out of scope"),
    (dict(MASK, max_det=MAX_LABEL_DET + 1), "int16: max_det = 32768 exceeds 32767"),
])
def test_handles_that_have_no_label_maps_are_refused(kw, word):
    d = configured(**kw)
    with pytest.raises(ValueError, match=word):
        d.labels(**good())
    if "max_det" not in kw:
        with pytest.raises(ValueError, match=word):         # ... before anything is uploaded
            d.labels_host(None, GEO, None)


def test_the_signature_is_the_headers_and_the_older_checks_keep_theirs():
    res, args = _lib.SIGNATURES["boxmot_hip_detpost_labels"]
    assert res is _lib.SIGNATURES["boxmot_hip_detpost_run_mask"][0] and len(args) == 13 and args[2] is _lib.c_double_p
    assert list(inspect.signature(DetPost._check_run).parameters) == ["self", "pred", "geo", "d_dets", "d_det_rows", "d_extra", "d_src"]
    assert list(inspect.signature(DetPost._check_mask).parameters) == ["self", "n", "rows", "d_proto", "d_masks"]
    assert list(inspect.signature(DetPost.labels).parameters) == ["self", "geo", "d_proto", "d_dets", "d_det_rows", "d_extra", "d_labels", "hip_stream"]
