"""Argument checking of boxmot_amd.detpost.DetPost(extra=...), without a device: every bad option or shape of the per-anchor extras
raises a ValueError that names what is wrong, before anything goes down to the library; handles without extras refuse the two new
blocks."""
import pytest

from boxmot_amd import _lib
from boxmot_amd.detpost import EXTRA_KINDS, DetPost
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


def configured(**kw):
    """the options checked as the constructor checks them, but no handle (there is no device here)"""
    d = DetPost.__new__(DetPost)
    d._handle = None
    d._configure(**dict(BASE, **kw))
    return d


@pytest.mark.parametrize("kw,word", [
    (dict(extra_kind="kpt3"), "extra="), (dict(extra_kind="raw"), "extra="), (dict(extra=0), "extra must be"), (dict(extra=1025), "extra must be"),
    (dict(extra=-3), "extra must be"), (dict(extra=2.5), "extra must be"), (dict(extra=6, extra_kind="kpt4"), "extra_kind"),
    (dict(extra=51, extra_kind="kpt2"), "groups of 2"), (dict(extra=32, extra_kind="kpt3"), "groups of 3"), (dict(extra=6, layout="cn_obb"), "cn_obb"),
    (dict(extra=6, extra_kind="kpt3", layout="cn_obb"), "cn_obb"),
])
def test_bad_extra_options(kw, word):
    with pytest.raises(ValueError, match=word):
        configured(**kw)
    with pytest.raises(ValueError, match=word):             # the constructor checks before it looks for a device
        DetPost(**dict(BASE, **kw))


def test_extra_options_and_shapes():
    d = configured(extra=51, extra_kind="kpt3")
    assert (d.extra, d.extra_kind, d.n_channels) == (51, "kpt3", 60) and d.pred_shape() == (2, 60, 100) and d.pred_shape(1) == (1, 60, 100)
    assert configured(extra=32).extra_kind == "raw" and configured(extra=1024).extra == 1024 and configured(extra=34, extra_kind="kpt2").n_channels == 43
    assert configured(extra=32, layout="nc_obj").pred_shape() == (2, 100, 42)
    t = configured(extra=6, extra_kind="kpt3", tiles=3, merge="ios")
    assert (t.tiles, t.merge, t.extra) == (3, "ios", 6) and t.pred_shape() == (6, 15, 100)
    u = configured()
    assert (u.extra, u.extra_kind) == (None, None) and u.pred_shape() == (2, 9, 100)
    assert EXTRA_KINDS == {"raw": 0, "kpt2": 1, "kpt3": 2}


def test_the_config_struct_is_the_headers():
    import ctypes
    f = [n for n, _ in _lib.DetPostExtraConfig._fields_]
    assert f == ["base", "n_tiles", "merge", "n_extra", "extra_kind"]
    assert ctypes.sizeof(_lib.DetPostExtraConfig) == ctypes.sizeof(_lib.DetPostConfig) + 16
    assert "boxmot_hip_detpost_create_extra" in _lib.SIGNATURES and len(_lib.SIGNATURES["boxmot_hip_detpost_run_extra"][1]) == 11


GEO = [letterbox_geometry(480, 640, (64, 64))] * 2


def good():
    return dict(pred=Fake((2, 15, 100), "float16"), geo=GEO, d_dets=Fake((2, 20, 6)), d_det_rows=Fake((2,), "int32"), d_extra=Fake((2, 20, 6)),
                d_src=Fake((2, 20), "int32"))


@pytest.mark.parametrize("change,word", [
    (dict(pred=Fake((2, 9, 100))), "pred must have shape"), (dict(pred=Fake((2, 100, 15))), "pred must have shape"), (dict(d_extra=None), "needs d_extra"),
    (dict(d_extra=Fake((2, 20, 5))), "d_extra must have shape"), (dict(d_extra=Fake((2, 16, 6))), "d_extra must have shape"),
    (dict(d_extra=Fake((1, 20, 6))), "d_extra must have shape"), (dict(d_extra=Fake((2, 120))), "d_extra must have shape"),
    (dict(d_extra=Fake((2, 20, 6), "float16")), "d_extra must be float32"), (dict(d_extra=Fake((2, 20, 6), contiguous=False)), "d_extra must be contiguous"),
    (dict(d_extra=Fake((2, 20, 6), ptr=0)), "d_extra has a null"), (dict(d_src=Fake((2, 16), "int32")), "d_src must have shape"),
    (dict(d_src=Fake((1, 20), "int32")), "d_src must have shape"), (dict(d_src=Fake((2, 20, 1), "int32")), "d_src must have shape"),
    (dict(d_src=Fake((2, 20), "int64")), "d_src must be int32"), (dict(d_src=Fake((2, 20), "int32", contiguous=False)), "d_src must be contiguous"),
    (dict(d_src=Fake((2, 20), "int32", ptr=0)), "d_src has a null"), (dict(d_dets=Fake((2, 15, 6))), "fewer than max_det = 16"),
])
def test_bad_extra_run_arguments(change, word):
    d = configured(extra=6, extra_kind="kpt3")
    with pytest.raises(ValueError, match=word):
        d.run(**dict(good(), **change))


def test_good_arguments_pass_the_checks():
    d = configured(extra=6, extra_kind="kpt3")
    n, dtype, table, stride = d._check_run(**good())
    assert (n, dtype, stride) == (2, 1, 20) and table.shape == (2, 5)
    assert d._check_run(**dict(good(), d_src=None))[0] == 2                                         # d_src is optional
    n, _, _, stride = d._check_run(**dict(good(), geo=GEO[:1], d_extra=Fake((3, 20, 6))))           # fewer streams, a larger block
    assert (n, stride) == (1, 20)
    tg = [[tile_geometry(480, 640, r, (64, 64)) for r in tile_grid(480, 640, grid=(1, 2))]] * 2     # T = 3
    t = configured(extra=6, extra_kind="kpt3", tiles=3)
    n, _, table, _ = t._check_run(**dict(good(), pred=Fake((6, 15, 100)), geo=tg))
    assert n == 2 and table.shape == (2, 3, 7)
    with pytest.raises(ValueError, match="N >= 6"):
        t.run(**dict(good(), geo=tg))


def test_a_handle_without_extras_refuses_the_blocks():
    base = dict(pred=Fake((2, 9, 100), "float16"), geo=GEO, d_dets=Fake((2, 20, 6)), d_det_rows=Fake((2,), "int32"))
    assert configured()._check_run(**base)[0] == 2
    for kw in (dict(d_extra=Fake((2, 20, 6))), dict(d_src=Fake((2, 20), "int32")), dict(d_extra=Fake((2, 20, 6)), d_src=Fake((2, 20), "int32"))):
        with pytest.raises(ValueError, match="extra="):
            configured().run(**dict(base, **kw))
    with pytest.raises(ValueError, match="pred must have shape"):                                   # ... and a head with extras
        configured().run(**dict(base, pred=Fake((2, 15, 100))))
