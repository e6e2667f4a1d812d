"""The host side of tiled detection, without a device: tile_grid's rectangles, the rules for explicit rectangles, TileGeometry, the
argument checks of DetPost(tiles=...) -- every error a ValueError naming the stream and tile before anything goes down to the
library -- and checks of the two NumPy references themselves (tests/letterbox_tiles_ref.py, tests/detpost_tiled_ref.py): that the
cases are what their names say."""
import numpy as np
import pytest

import detpost_ref
import detpost_tiled_ref as dref
import letterbox_tiles_ref as lref
from boxmot_amd.detpost import DetPost
from boxmot_amd.ingest import FrameRing, TileGeometry, letterbox_geometry, tile_geometry, tile_grid
from test_detpost_host import Fake


# ---- tile_grid and the rectangles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n,o,size,origins", [(3840, 3, 0.2, 1477, [0, 1181, 2363]), (131, 3, 0.2, 51, [0, 40, 80]), (64, 2, 0, 32, [0, 32])])
def test_tile_grid_axis_values(L, n, o, size, origins):
    assert lref.tile_axis(L, n, o) == (size, origins)
    across = tile_grid(10, L, grid=(1, n), overlap=o, full=False)
    assert across == [(x, 0, size, 10) for x in origins]
    down = tile_grid(L, 10, grid=(n, 1), overlap=o, full=False)
    assert down == [(0, y, 10, size) for y in origins]
    assert origins[0] == 0 and origins[-1] + size == L


def test_tile_grid_order_count_and_the_whole_frame():
    t = tile_grid(2160, 3840, grid=(2, 3), overlap=0.2)
    assert len(t) == 7 and t[0] == (0, 0, 3840, 2160)
    assert t[1:] == [(x, y, 1477, 1200) for y in (0, 960) for x in (0, 1181, 2363)]                 # row-major
    assert t == lref.tile_grid(2160, 3840, (2, 3), 0.2)
    assert tile_grid(97, 131, grid=(1, 1), full=False) == [(0, 0, 131, 97)]
    for rows, cols in ((2160, 3840), (97, 131), (1080, 1920)):                                       # T does not depend on the frame size
        g = tile_grid(rows, cols, grid=(2, 3), overlap=0.5)
        assert len(g) == 7 and all(x >= 0 and y >= 0 and x + w <= cols and y + h <= rows and w >= 1 and h >= 1 for x, y, w, h in g)


@pytest.mark.parametrize("kw,word", [(dict(grid=(0, 2)), "grid"), (dict(grid=3), "grid"), (dict(overlap=0.95), "overlap"), (dict(overlap=-0.1), "overlap"),
                                     (dict(grid=(8, 8)), "tiles"), (dict(rows=0), "positive"), (dict(grid=(200, 1)), "grid")])
def test_tile_grid_errors(kw, word):
    with pytest.raises(ValueError, match=word):
        tile_grid(**dict(dict(rows=97, cols=131, grid=(2, 2)), **kw))


def _ring(sizes):
    """a FrameRing's host-side checks without its handle (there is no device here)"""
    r = FrameRing.__new__(FrameRing)
    r._handle, r.n_streams, r.sizes = None, len(sizes), list(sizes)
    return r


def test_rectangles_one_list_or_one_per_stream():
    r = _ring(lref.SIZES)
    assert r._stream_tiles(lref.TILES, 2) == lref.TILES
    shared = [(0, 0, 64, 64), (10, 20, 30, 40)]
    assert r._stream_tiles(shared, 2) == [shared, shared]
    assert r._stream_tiles(np.array(shared), 1) == [shared]


@pytest.mark.parametrize("tiles,word", [
    ([[(0, 0, 10, 10)], [(150, 100, 60, 28)]], "stream 1 tile 0"),                      # outside the 128 x 200 frame
    ([[(0, 0, 10, 10), (100, 0, 32, 10)], [(0, 0, 10, 10)] * 2], "stream 0 tile 1"),    # 100 + 32 > 131
    ([[(0, 0, 10, 0)], [(0, 0, 10, 10)]], "stream 0 tile 0"), ([[(-1, 0, 10, 10)], [(0, 0, 10, 10)]], "stream 0 tile 0"),
    ([[(0, 0, 10.5, 10)], [(0, 0, 10, 10)]], "four integers"), ([[(0, 0, 10)], [(0, 0, 10, 10)]], "four integers"),
    ([[(0, 0, 10, 10)] * 2, [(0, 0, 10, 10)]], "stream 1: 1 tiles where stream 0 has 2"),
    ([[(0, 0, 10, 10)] * 65] * 2, "1..64"), ([[], []], "tiles"), ([[(0, 0, 10, 10)]], "1 lists for 2 streams"),
])
def test_bad_rectangles_name_the_stream_and_tile(tiles, word):
    with pytest.raises(ValueError, match=word):
        _ring(lref.SIZES)._stream_tiles(tiles, 2)


def test_tile_geometry_is_the_rectangle_s_letterbox_geometry():
    for rects, (rows, cols) in zip(lref.TILES, lref.SIZES):
        for rect in rects:
            for size in lref.OUT_SIZES:
                for mode in ("center", "topleft"):
                    g = tile_geometry(rows, cols, rect, size, mode)
                    assert tuple(g) == lref.geometry(rect, size, mode)
                    assert tuple(g)[:7] == tuple(letterbox_geometry(rect[3], rect[2], size, mode))
    with pytest.raises(ValueError, match="no picture"):
        tile_geometry(97, 131, (0, 0, 131, 1), (64, 64))


def test_to_frame_is_the_tiled_detposts_arithmetic():
    g = TileGeometry(1 / 3, 64, 43, 10, 0, 128, 192, 7, 5)
    boxes = np.array([[-4.0, 3.0, 70.0, 60.0, 0.9, 1.0], [10.5, 20.25, 30.0, 40.0, 0.5, 2.0]], dtype=np.float32)
    got = g.to_frame(boxes)
    want = dref.to_frame(boxes[:, :4], (g.gain, g.top, g.left, g.x0, g.y0, g.cols, g.rows))
    assert got.dtype == np.float32 and np.array_equal(got[:, :4].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[:, 4:], boxes[:, 4:])
    assert got[0, 0] == 7.0 and got[0, 2] == 199.0 and boxes[0, 0] == -4.0                          # clipped to the tile, then shifted; input untouched


# ---- DetPost(tiles=...) ---------------------------------------------------------------------------------------------------------------
def configured(**kw):
    d = DetPost.__new__(DetPost)
    d._handle = None
    d._configure(**dict(dict(n_streams=2, n_anchors=100, n_classes=5, max_det=16), **kw))
    return d


@pytest.mark.parametrize("kw,word", [(dict(merge="ios"), "tiles"), (dict(tiles=3, merge="giou"), "merge"), (dict(tiles=0), "tiles"), (dict(tiles=65), "tiles"),
                                     (dict(tiles=2.5), "tiles"), (dict(tiles=3, layout="cn_obb"), "cn_obb")])
def test_bad_tiled_options(kw, word):
    with pytest.raises(ValueError, match=word):
        configured(**kw)
    with pytest.raises(ValueError, match=word):             # the constructor checks before it looks for a device
        DetPost(**dict(dict(n_streams=2, n_anchors=100, n_classes=5, max_det=16), **kw))


def test_tiled_options_and_shapes():
    d = configured(tiles=3)
    assert (d.tiles, d.merge) == (3, "iou") and configured(tiles=3, merge="ios").merge == "ios"
    assert d.pred_shape() == (6, 9, 100) and d.pred_shape(1) == (3, 9, 100) and configured(tiles=3, layout="nc_obj").pred_shape() == (6, 100, 10)
    u = configured()
    assert (u.tiles, u.merge) == (None, None) and u.pred_shape() == (2, 9, 100)


TG = [[tile_geometry(480, 640, r, (64, 64)) for r in tile_grid(480, 640, grid=(1, 2))]] * 2       # T = 3


def good():
    return dict(pred=Fake((6, 9, 100), "float16"), geo=TG, d_dets=Fake((2, 16, 6)), d_det_rows=Fake((2,), "int32"))


@pytest.mark.parametrize("change,word", [
    (dict(pred=Fake((5, 9, 100))), "N >= 6"), (dict(pred=Fake((2, 9, 100))), "N >= 6"), (dict(geo=[TG[0], TG[0][:2]]), "stream 1: a handle of tiles=3"),
    (dict(geo=[TG[0][0], TG[0][0]]), "stream 0: a handle of tiles=3"), (dict(geo=[letterbox_geometry(480, 640, (64, 64))] * 2), "stream 0: a handle of tiles=3"),
    (dict(geo=[TG[0], [TG[0][0], (1.0, 0, 0, 0, 0, 64), TG[0][2]]]), "stream 1 tile 1: geometry must be"),
    (dict(geo=[[TG[0][0], TG[0][1], (0.0, 0, 0, 0, 0, 64, 64)], TG[0]]), "stream 0 tile 2: geometry needs"),
    (dict(geo=[TG[0], [TG[0][0], (1.0, 0, 0, 0, 0, 0, 64), TG[0][2]]]), "stream 1 tile 1: geometry needs"),
    (dict(geo=[TG[0], [TG[0][0], (1.0, 0, float("nan"), 0, 0, 64, 64), TG[0][2]]]), "stream 1 tile 1: geometry needs"),
    (dict(geo=TG + TG), "geo has 4 entries"), (dict(d_dets=Fake((1, 16, 6))), "d_dets must have shape"),
])
def test_bad_tiled_run_arguments(change, word):
    with pytest.raises(ValueError, match=word):
        configured(tiles=3).run(**dict(good(), **change))


def test_good_tiled_arguments_pass_the_checks():
    d = configured(tiles=3)
    n, dtype, table, stride = d._check_run(**good())
    assert (n, dtype, stride) == (2, 1, 16) and table.shape == (2, 3, 7)
    g = TG[0][2]
    assert table[1, 2].tolist() == [g.gain, g.top, g.left, g.x0, g.y0, g.cols, g.rows]
    seven = [(0.5, 1, 2, 3, 4, 50, 60)] * 3
    n, _, table, _ = d._check_run(**dict(good(), geo=[seven], pred=Fake((3, 9, 100))))             # fewer streams, 7-sequences
    assert n == 1 and table[0, 1].tolist() == [0.5, 1, 2, 3, 4, 50, 60]
    with pytest.raises(ValueError, match="geometry"):                                               # an untiled handle takes no tile lists
        configured().run(**dict(good(), pred=Fake((2, 9, 100))))


# ---- the references are what the cases' names say ------------------------------------------------------------------------------------------
def test_the_cut_box_is_40_percent_of_the_whole_one():
    k = dref.NAMES.index("cut_box_merge_iou")
    rows = dref.want(k)[0][0]
    assert rows[:, :4].tolist() == [[25, 20, 90, 60], [64, 20, 90, 60]]
    whole, cut = rows[0, :4], rows[1, :4]
    area = lambda b: (b[2] - b[0]) * (b[3] - b[1])
    assert area(cut) / area(whole) == np.float32(0.4)
    assert not dref.suppresses(whole[None], cut, 0.45, "iou")[0] and dref.suppresses(whole[None], cut, 0.45, "ios")[0]
    assert dref.suppresses(whole[None], cut, np.nextafter(np.float32(0.4), np.float32(0)), "iou")[0] and not dref.suppresses(whole[None], cut, 0.4, "iou")[0]
    assert not dref.suppresses(whole[None], cut, 1.0, "ios")[0] and dref.suppresses(whole[None], cut, 1.0, "ios", ge=True)[0]
    assert len(dref.want(dref.NAMES.index("cut_box_merge_ios"))[0][0]) == 1
    zero = np.zeros(4, dtype=np.float32)
    assert not dref.suppresses(zero[None], zero, 0.0, "iou")[0] and not dref.suppresses(zero[None], zero, 0.0, "ios")[0]        # 0 / 0


def test_the_top_k_ties_straddle_a_tile_boundary():
    for name in ("topk_ties_straddle_tiles_cn_A100", "topk_ties_straddle_tiles_nc_obj_A300"):
        c = dref.CASES[dref.NAMES.index(name)]
        S, T, A, nc = c.dims
        for s in range(S):
            cf = np.concatenate([np.where(p, f, -1) for _, f, p in (detpost_ref.score(c.preds[s * T + t], c.layout, c.opts["conf"]) for t in range(T))])
            order = np.lexsort((np.arange(T * A), -cf))
            K = c.opts["max_candidates"]
            assert (cf > 0).sum() > K
            kth = cf[order[K - 1]]
            tied = np.nonzero(cf == kth)[0]
            taken = np.intersect1d(tied, order[:K])
            assert 0 < len(taken) < len(tied)                                   # the boundary cuts through the ties ...
            assert len(set(taken // A)) > 1, (name, s)                          # ... and the ties taken come from more than one tile
            assert taken.max() < np.setdiff1d(tied, taken).min()                # the lowest (tile, anchor) first


def test_the_wrong_references_differ_where_they_should():
    k = dref.NAMES.index("cut_box_ios_exactly_at_the_threshold")
    assert len(dref.want(k)[0][0]) == 2 and len(dref.want(k, nms_ge=True)[0][0]) == 1
    k = dref.NAMES.index("equal_conf_tile_order_decides")
    assert not np.array_equal(dref.want(k)[0][0], dref.want(k, tiles_high_first=True)[0][0])
    assert dref.want(k)[0][0][0, :4].tolist() == [85, 45, 115, 75]              # tile 1's box, not tile 2's two pixels to the right


def test_what_the_cases_cover():
    got = {n: [(len(r), c.tolist()) for r, c in dref.want(k)] for k, n in enumerate(dref.NAMES)}
    assert got["one_object_two_tiles_cn_float32"][0] == (2, [4, 4, 2])          # three reports of one object and one other: two rows
    assert got["classes_kept_apart"][0][0] == 3 and got["classes_agnostic"][0][0] == 2
    assert got["a_stream_with_nothing"][0] == (0, [0, 0, 0])
    assert got["clip_to_the_tile_iou"][0][0] == 6 and got["clip_to_the_tile_ios"][0][0] == 5
    n, (p, c, kept) = got["max_det_cuts_counter_2_does_not"][0]
    assert n == 10 and p == c == 100 and 10 < kept < 100
    assert got["seam_129_candidates_nc_obj_f16"][0][1][1] == 129
    layouts = {(c.layout, c.preds.dtype.name) for c in dref.CASES}
    assert layouts == {("cn", "float16"), ("cn", "float32"), ("nc_obj", "float16"), ("nc_obj", "float32")}
    assert all(c.dims[0] == 2 and c.dims[1] == 3 and 64 <= c.dims[2] <= 300 and c.dims[3] == 3 for c in dref.CASES)


def test_one_unit_tile_is_the_untiled_definition():
    names = [c.name for c in detpost_ref.CASES]
    for name in dref.IDENTITY:
        k = names.index(name)
        u = detpost_ref.CASES[k]
        rows, counters = dref.detpost_tiled(u.preds[:1], [dref.TILE_UNIT], u.layout, **u.opts)
        w_rows, w_counters = detpost_ref.want(k)[0]
        assert np.array_equal(rows.view(np.uint32), w_rows.view(np.uint32)) and counters.tolist() == w_counters.tolist(), name
