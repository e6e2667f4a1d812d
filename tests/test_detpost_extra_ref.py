"""The cases of tests/detpost_extra_ref.py are what their names claim, and the comparison with its reference bites: two wrong
references -- extras in candidate order, ignoring NMS; the visibility treated as a coordinate -- differ from the right one on the
cases built for them.  No device, no kernel."""
import numpy as np
import pytest

import detpost_extra_ref as ref


def case(name):
    k = ref.NAMES.index(name)
    return ref.CASES[k], ref.want(k), k


def test_the_table_covers_what_the_definition_distinguishes():
    table = [c for c in ref.CASES if c.name.startswith("table_")]
    assert {(c.layout, c.preds.dtype.name, c.E, c.kind) for c in table} == {
        (lay, dt, E, kind) for lay in ("cn", "nc_obj") for dt in ("float16", "float32") for E, kind in ((1, "raw"), (32, "raw"), (34, "kpt2"), (51, "kpt3"))}
    assert {c.nc for c in table} == {1, 3}
    for c in ref.CASES:
        S, A = c.dims
        assert 96 <= A <= 320 and c.stride >= c.opts["max_det"] and 1 <= c.E <= 1024 and c.E % ref.GROUP[c.kind] == 0, c.name
        assert S == (2 if c.tiles else 3) and c.tiles in (0, 3), c.name
        if not c.tiles:
            assert c.geos == [ref.GEO_UNIT, ref.GEO_CENTER, ref.GEO_TALL], c.name
        assert c.preds.shape[1 if c.layout == "cn" else 2] == (4 if c.layout == "cn" else 5) + c.nc + c.E, c.name
    # both score kernels: an fp16 "cn" tensor of A % 8 != 0 and an fp32 one of A % 4 != 0 take the narrow one
    cn = [(c.preds.dtype.name, c.dims[1]) for c in ref.CASES if c.layout == "cn"]
    assert any(d == "float16" and A % 8 for d, A in cn) and any(d == "float16" and A % 8 == 0 for d, A in cn)
    assert any(d == "float32" and A % 4 for d, A in cn) and any(d == "float32" and A % 4 == 0 for d, A in cn)
    assert any(c.tiles and c.opts["merge"] == m for c in ref.CASES for m in ("iou",)) and any(c.tiles and c.opts["merge"] == "ios" for c in ref.CASES)


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_shapes_and_source_anchors(k):
    """src names an anchor that the existing reference's row came from: its conf and class are that anchor's"""
    c = ref.CASES[k]
    S, A = c.dims
    T = c.tiles or 1
    for s, (rows, counters, extras, src) in enumerate(ref.want(k)):
        n = len(rows)
        assert extras.shape == (n, c.E) and extras.dtype == np.float32 and src.shape == (n,) and src.dtype == np.int32
        assert n == min(counters[2], c.opts["max_det"]) and len(set(src.tolist())) == n and ((0 <= src) & (src < T * A)).all()
        for r in range(n):
            t, a = divmod(int(src[r]), A)
            cls, conf, passed = ref.detpost_ref.score(ref.cut(c.preds[s * T + t], c.layout, c.nc), c.layout, c.opts["conf"], c.opts["classes"])
            assert passed[a] and conf[a] == rows[r, 4] and cls[a] == rows[r, 5]
        if c.kind == "raw":
            for r in range(n):
                t, a = divmod(int(src[r]), A)
                assert np.array_equal(extras[r], ref.extras_of(c.preds[s * T + t], c.layout, c.nc)[a], equal_nan=True)


def test_raw_values_name_their_stream_anchor_and_channel():
    for name in ("raw_encodes_stream_anchor_channel_cn", "raw_encodes_stream_anchor_channel_nc_obj"):
        c, want, _ = case(name)
        for s, (rows, _, extras, src) in enumerate(want):
            assert len(rows) >= 5
            v = extras.astype(np.int64)
            assert np.array_equal(v % 32, np.tile(np.arange(c.E), (len(src), 1))) and np.array_equal(v // 32, np.tile((s * 320 + src)[:, None], (1, c.E)))


def test_survivor_counts_are_what_the_names_say():
    for name in ("survivors_cross_a_chunk", "survivors_cross_a_chunk_nc_obj_f16"):
        for rows, counters, _, _ in case(name)[1]:
            assert len(rows) >= 65 and counters[1] > counters[2] >= 65           # and NMS dropped some
    c, want, _ = case("more_survivors_than_max_det")
    for rows, counters, extras, src in want:
        assert counters[2] > c.opts["max_det"] == len(rows) == len(src) == len(extras)
    for rows, counters, extras, src in case("nothing_passes")[1]:
        assert len(rows) == len(src) == len(extras) == 0 and counters.tolist() == [0, 0, 0]
    c, want, _ = case("A300_K64_topk_bites")
    for rows, counters, _, _ in want:
        assert c.dims[1] > 64 and counters[0] > 64 == counters[1] and len(rows) > 0
    rows, counters, _, src = case("tiled_survivors_cross_a_chunk")[1][0]
    assert len(rows) >= 65 and counters[1] > counters[2]


def test_ties_and_stacks_show_in_src():
    for rows, _, _, src in case("equal_confs_lower_anchor_first")[1]:
        assert (rows[:, 4] == np.float32(0.5)).all() and src.tolist() == [0, 3, 5, 17]      # of the anchors 40, 3, 63, 0, 17, 5; max_det = 4
    for rows, counters, _, src in case("stacks_of_duplicates")[1]:
        assert counters.tolist() == [5, 5, 2] and src.tolist() == [50, 30]                  # the best of stack 1; the lower anchor of stack 2


def test_keypoints_are_clipped_and_nan_comes_out_as_zero():
    kpt =[k for k, c in enumerate(ref.CASES) if c.kind != "raw" and not c.tiles and c.name.startswith("table_")]
    assert kpt
    for k in kpt:
        c = ref.CASES[k]
        g = ref.GROUP[c.kind]
        for s, (rows, _, extras, src) in enumerate(ref.want(k)):
            gain, top, left, frows, fcols = c.geos[s]
            raw = ref.extras_of(c.preds[s], c.layout, c.nc)[src]
            x, y = extras[:, 0::g], extras[:, 1::g]
            assert ((0 <= x) & (x <= fcols)).all() and ((0 <= y) & (y <= frows)).all()
            assert (x == 0).any() and (x == fcols).any() and (y == 0).any() and (y == frows).any(), (c.name, s, "no keypoint was clipped")
            inside = (x > 0) & (x < fcols)
            assert inside.any() and np.array_equal(x[inside], ((raw[:, 0::g] - np.float32(left)) / np.float32(gain))[inside])
            if g == 3:
                assert np.array_equal(extras[:, 2::3], raw[:, 2::3])                         # the visibility is copied
    for name in ("nan_and_inf_keypoints_float32", "nan_and_inf_keypoints_float16"):
        c, want, _ = case(name)
        for s, (rows, _, extras, src) in enumerate(want):
            gain, top, left, frows, fcols = c.geos[s]
            assert src.tolist() == [1, 2, 64]
            raw = ref.extras_of(c.preds[s], c.layout, c.nc)[src]
            assert np.isnan(raw[0, [0, 4, 5]]).all() and np.isinf(raw[1, [0, 1, 3, 4]]).all()
            assert extras[0, 0] == 0 and extras[0, 4] == 0 and np.isnan(extras[0, 5])        # NaN x, NaN y -> 0; a NaN visibility is copied
            assert extras[1].tolist() == [fcols, 0, 1.0, 0, frows, 0.25]                    # +inf -> the frame's edge, -inf -> 0


def test_tiled_rows_come_from_several_tiles_with_their_own_geometry():
    for name in [n for n in ref.NAMES if n.startswith("tiled_")]:
        c, want, _ = case(name)
        S, A = c.dims
        tiles_seen = set()
        for s, (rows, _, extras, src) in enumerate(want):
            tiles_seen |= {(s, int(t)) for t in src // A}
        assert len({t for s, t in tiles_seen if s == 0}) >= 2, (name, "stream 0's rows come from one tile")
    hit = 0
    for name in [n for n in ref.NAMES if n.startswith("tiled_") and ref.CASES[ref.NAMES.index(n)].kind != "raw"]:
        c, want, _ = case(name)
        S, A = c.dims
        g = ref.GROUP[c.kind]
        for s, (rows, _, extras, src) in enumerate(want):
            for r in range(len(src)):
                gain, top, left, x0, y0, w, h = c.geos[s][int(src[r]) // A]
                x, y = extras[r, 0::g], extras[r, 1::g]
                assert ((x0 <= x) & (x <= x0 + w)).all() and ((y0 <= y) & (y <= y0 + h)).all()
                hit += int(x0 > 0 and ((x == x0) | (x == x0 + w)).any())
    assert hit >= 2, "no keypoint was clipped to a tile that does not start at the frame's origin"


def test_wrong_references_differ_where_the_cases_say():
    # extras in candidate order, ignoring NMS: from the first suppressed candidate on, src and the extras are another anchor's
    for name in ("survivors_cross_a_chunk", "tiled_survivors_cross_a_chunk", "stacks_of_duplicates"):
        c, want, k = case(name)
        wrong = ref.want(k, candidate_order=True)
        for (rows, _, extras, src), (w_rows, _, w_extras, w_src) in zip(want[:1], wrong[:1]):
            assert np.array_equal(rows, w_rows) and not np.array_equal(src, w_src) and not np.array_equal(extras, w_extras, equal_nan=True)
    # the visibility treated as a coordinate
    for name in ("survivors_cross_a_chunk", "tiled_iou_cn_float32"):
        c, want, k = case(name)
        wrong = ref.want(k, visibility_is_a_coordinate=True)
        for s, ((rows, _, extras, src), (_, _, w_extras, w_src)) in enumerate(zip(want, wrong)):
            assert np.array_equal(src, w_src) and np.array_equal(extras[:, 0::3], w_extras[:, 0::3]) and np.array_equal(extras[:, 1::3], w_extras[:, 1::3])
            if c.tiles or s > 0:        # (stream 0 of the untiled cases has gain 1 and no padding: there a visibility within 0..1 maps to itself)
                assert not np.array_equal(extras[:, 2::3], w_extras[:, 2::3])
