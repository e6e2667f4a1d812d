"""Argument checking of boxmot_amd.detpost.DetPost(mask=...), without a device: every bad option or shape of the mask decoding
raises a ValueError that names what is wrong, before anything goes down to the library; handles without masks refuse the two new
blocks; the ctypes table and the config struct are the header's."""
import ctypes

import pytest

from boxmot_amd import _lib
from boxmot_amd.detpost import DetPost
from boxmot_amd.ingest import letterbox_geometry, tile_geometry, tile_grid


class Fake:
    """the four things run() asks of a tensor"""

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


@pytest.mark.parametrize("kw,word", [
    (dict(mask=(12, 20), in_shape=(40, 64)), "mask= needs extra="), (dict(extra=32, mask=(12, 20)), "mask= needs in_shape="),
    (dict(extra=32, in_shape=(40, 64)), "in_shape= belongs to a mask handle"), (dict(MASK, extra_kind="kpt2"), "extra_kind 'kpt2'"),
    (dict(MASK, extra=33, extra_kind="kpt3"), "extra_kind 'kpt3'"), (dict(MASK, layout="cn_obb"), "cn_obb.*mask="), (dict(MASK, extra=257), "mask= takes extra within 1..256"),
    (dict(MASK, mask=(0, 20)), "mask must be two integers within 1..1024"), (dict(MASK, mask=(12, 1025)), "mask must be two integers within 1..1024"),
    (dict(MASK, mask=(12,)), "mask must be two integers"), (dict(MASK, mask=12), "mask must be two integers"), (dict(MASK, mask=(12.5, 20)), "mask must be two integers"),
    (dict(MASK, in_shape=(0, 64)), "in_shape must be two integers >= 1"), (dict(MASK, in_shape=(40, -1)), "in_shape must be two integers >= 1"),
    (dict(MASK, in_shape=(40, 64, 3)), "in_shape must be two integers"), (dict(MASK, in_shape="640"), "in_shape must be two integers"),
])
def test_bad_mask_options(kw, word):
    with pytest.raises(ValueError, match=word):
        configured(**kw)
    with pytest.raises(ValueError, match=word):             # the constructor checks before it looks for a device
        DetPost(**dict(BASE, **kw))


def test_mask_options_and_shapes():
    d = configured(**MASK)
    assert (d.extra, d.extra_kind, d.mask, d.in_shape, d.n_channels) == (32, "raw", (12, 20), (40, 64), 41) and d.pred_shape() == (2, 41, 100)
    assert configured(**dict(MASK, extra_kind="raw")).extra_kind == "raw" and configured(**dict(MASK, extra=256, mask=(1024, 1), in_shape=(1, 7))).mask == (1024, 1)
    t = configured(**dict(MASK, tiles=3, merge="ios", layout="nc_obj"))
    assert (t.tiles, t.merge, t.mask) == (3, "ios", (12, 20)) and t.pred_shape() == (6, 100, 42)
    for other in (configured(), configured(extra=51, extra_kind="kpt3"), configured(tiles=2), configured(layout="cn_obb")):
        assert other.mask is None and other.in_shape is None


def test_the_config_struct_and_the_signatures_are_the_headers():
    assert [n for n, _ in _lib.DetPostMaskConfig._fields_] == ["extra", "mask_h", "mask_w", "in_h", "in_w"]
    assert ctypes.sizeof(_lib.DetPostMaskConfig) == ctypes.sizeof(_lib.DetPostExtraConfig) + 16
    assert [n for n, _ in _lib.DetPostExtraConfig._fields_] == ["base", "n_tiles", "merge", "n_extra", "extra_kind"]
    assert len(_lib.SIGNATURES["boxmot_hip_detpost_create_mask"][1]) == 1 and len(_lib.SIGNATURES["boxmot_hip_detpost_run_mask"][1]) == 14
    assert len(_lib.SIGNATURES["boxmot_hip_detpost_run_extra"][1]) == 11


GEO = [letterbox_geometry(480, 640, (40, 64))] * 2


def good():
    return dict(pred=Fake((2, 41, 100), "float16"), geo=GEO, d_dets=Fake((2, 20, 6)), d_det_rows=Fake((2,), "int32"), d_extra=Fake((2, 20, 32)),
                d_src=Fake((2, 20), "int32"), d_proto=Fake((2, 32, 12, 20), "float16"), d_masks=Fake((2, 20, 12, 20), "uint8"))


@pytest.mark.parametrize("change,word", [
    (dict(d_proto=None), "needs d_proto and d_masks"), (dict(d_masks=None), "needs d_proto and d_masks"), (dict(d_proto=None, d_masks=None), "needs d_proto and d_masks"),
    (dict(d_proto=Fake((1, 32, 12, 20))), "d_proto must have shape"), (dict(d_proto=Fake((2, 31, 12, 20))), "d_proto must have shape"),
    (dict(d_proto=Fake((2, 32, 20, 12))), "d_proto must have shape"), (dict(d_proto=Fake((2, 32, 240))), "d_proto must have shape"),
    (dict(d_proto=Fake((2, 32, 12, 20), "bfloat16")), "d_proto must be float16 or float32"), (dict(d_proto=Fake((2, 32, 12, 20), contiguous=False)), "d_proto must be contiguous"),
    (dict(d_proto=Fake((2, 32, 12, 20), ptr=0)), "d_proto has a null"), (dict(d_masks=Fake((1, 20, 12, 20), "uint8")), "d_masks must have shape"),
    (dict(d_masks=Fake((2, 16, 12, 20), "uint8")), "d_masks must have shape"), (dict(d_masks=Fake((2, 20, 12, 21), "uint8")), "d_masks must have shape"),
    (dict(d_masks=Fake((2, 20, 240), "uint8")), "d_masks must have shape"), (dict(d_masks=Fake((2, 20, 12, 20), "bool")), "d_masks must be uint8"),
    (dict(d_masks=Fake((2, 20, 12, 20), "float32")), "d_masks must be uint8"), (dict(d_masks=Fake((2, 20, 12, 20), "uint8", contiguous=False)), "d_masks must be contiguous"),
    (dict(d_masks=Fake((2, 20, 12, 20), "uint8", ptr=0)), "d_masks has a null"), (dict(d_extra=None), "needs d_extra"),
    (dict(d_extra=Fake((2, 20, 31))), "d_extra must have shape"), (dict(pred=Fake((2, 9, 100))), "pred must have shape"),
])
def test_bad_mask_run_arguments(change, word):
    d = configured(**MASK)
    with pytest.raises(ValueError, match=word):
        d.run(**dict(good(), **change))


def test_good_arguments_pass_the_checks():
    d = configured(**MASK)
    g = good()
    n, dtype, table, stride = d._check_run(**{k: g[k] for k in ("pred", "geo", "d_dets", "d_det_rows", "d_extra", "d_src")})     # unchanged: a 4-tuple
    assert (n, dtype, stride) == (2, 1, 20) and table.shape == (2, 5)
    assert d._check_mask(2, 20, g["d_proto"], g["d_masks"]) == 1
    assert d._check_mask(2, 20, Fake((2, 32, 12, 20), "float32"), g["d_masks"]) == 0                       # proto's dtype is its own
    assert d._check_mask(1, 20, Fake((3, 32, 12, 20)), Fake((3, 20, 12, 20), "uint8")) == 0                # fewer streams, larger blocks
    tg = [[tile_geometry(480, 640, r, (40, 64)) for r in tile_grid(480, 640, grid=(1, 2))]] * 2             # T = 3
    t = configured(**dict(MASK, tiles=3))
    assert t._check_mask(2, 20, Fake((6, 32, 12, 20)), g["d_masks"]) == 0
    with pytest.raises(ValueError, match="N >= 6"):
        t.run(**dict(good(), pred=Fake((6, 41, 100)), geo=tg))                                              # prototypes of 2 tensors for 6


def test_handles_without_masks_refuse_the_blocks():
    plain = dict(pred=Fake((2, 9, 100), "float16"), geo=GEO, d_dets=Fake((2, 20, 6)), d_det_rows=Fake((2,), "int32"))
    extras = dict(plain, pred=Fake((2, 41, 100), "float16"), d_extra=Fake((2, 20, 32)))
    for d, base in ((configured(), plain), (configured(extra=32), extras)):
        assert d._check_mask(2, 20, None, None) is None
        for kw in (dict(d_proto=Fake((2, 32, 12, 20))), dict(d_masks=Fake((2, 20, 12, 20), "uint8")),
                   dict(d_proto=Fake((2, 32, 12, 20)), d_masks=Fake((2, 20, 12, 20), "uint8"))):
            with pytest.raises(ValueError, match="mask="):
                d.run(**dict(base, **kw))
        with pytest.raises(ValueError, match="mask="):
            d._check_mask(2, 20, Fake((2, 32, 12, 20)), None)
