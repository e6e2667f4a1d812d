"""Self-checks of tests/detpost_mask_ref.py, the NumPy restatement of the device mask decoding (csrc/det_post_mask.hpp) and its table
of cases: every case is what its name says, every wrong reference differs on the case built for it, and the random inputs have
the magnitudes that keep subnormals out.  No library, no device."""
import numpy as np
import pytest

import detpost_mask_ref as ref

F = np.float32


def case(name):
    k = ref.NAMES.index(name)
    return k, ref.CASES[k]


def boxes(c, s):
    """the letterbox-space boxes of stream s's emitted rows (untiled)"""
    return [ref.box_of(c.preds[s], c.layout, int(a)) for a in ref.want(ref.NAMES.index(c.name))[s][3]]


def test_the_table_covers_what_it_should():
    names = ref.NAMES
    assert len(set(names)) == len(names)
    table = [c for c in ref.CASES if c.name.startswith("table_")]
    assert {(c.mask, c.in_shape) for c in table} == set(ref.SHAPES)
    for shape in ref.SHAPES:
        assert {(c.preds.dtype.name, c.protos.dtype.name) for c in table if c.mask == shape[0]} == \
            {(p, q) for p in ("float16", "float32") for q in ("float16", "float32")}
    assert {c.layout for c in table} == {"cn", "nc_obj"} and {c.E for c in table} == {1, 3, 32} and {c.nc for c in table} == {1, 3}
    for c in ref.CASES:
        S, A = c.dims
        assert 96 <= A <= 128 and c.opts["max_det"] == 16 and c.stride == 20 and c.opts["max_candidates"] == 64 and S in (2, 3)
        assert c.protos.shape == (S * (c.tiles or 1), c.E) + c.mask
    assert {c.tiles for c in ref.CASES} == {0, 2, 3}
    assert {c.opts["merge"] for c in ref.CASES if c.tiles == 2} == {"iou", "ios"} == {c.opts["merge"] for c in ref.CASES if c.tiles == 3}


def test_the_ratios_round_where_the_table_says():
    """(8, 8) / (32, 32) is exact; 12 / 40 is no float32, and a product with it rounds"""
    assert F(8) / F(32) == 0.25 and F(20) / F(64) == 0.3125
    hr = F(12) / F(40)
    assert float(hr) != 0.3 and float(F(25.25) * hr) != 25.25 * float(hr)


def test_random_inputs_keep_subnormals_out():
    """the coefficients and the prototypes of the random cases are fp16-representable and 0 or of magnitude within [2^-6, 2^6], so
    every product is 0 or at least 2^-12 and a multiple of 2^-18, and every partial sum a multiple of 2^-18 below 2^17: exact or
    rounded, never subnormal"""
    n = 0
    for k, c in enumerate(ref.CASES):
        if not c.random:
            continue
        n += 1
        for s in range(c.dims[0]):
            coef = ref.want(k)[s][2]
            for v in (coef, c.protos.astype(np.float32)):
                assert np.array_equal(v, v.astype(np.float16).astype(np.float32))
                mag = np.abs(v[v != 0])
                assert mag.size == 0 or (mag.min() >= 2.0 ** -6 and mag.max() <= 2.0 ** 6)
    assert n >= 19
    rng = np.random.default_rng(0)
    v = ref.vals(rng, (4096,))
    assert (v == 0).any() and (v > 0).any() and (v < 0).any()


@pytest.mark.parametrize("k", [0, 1, 31])
def test_impulse_prototypes_give_the_window_iff_the_coefficient_is_positive(k):
    kk, c = case(f"impulse_plane_{k}")
    seen = set()
    for s in range(3):
        _, _, coef, _, masks = ref.want(kk)[s]
        for r, box in enumerate(boxes(c, s)):
            win = ref.window_of(box, c.mask, c.in_shape)
            assert np.array_equal(masks[r].astype(bool), win if coef[r, k] > 0 else np.zeros_like(win))
            seen.add(bool(coef[r, k] > 0) and bool(win.any()))
    assert seen == {True, False}


def test_encoding_prototypes_are_integers_and_differ_per_tensor_plane_and_pixel():
    for name in ("encoding_prototypes_cn", "encoding_prototypes_nc_obj", "tiled_T2_iou"):
        k, c = case(name)
        p = c.protos
        assert np.array_equal(p, np.round(p)) and np.abs(p).max() <= 5
        assert all(not np.array_equal(p[0], p[q]) for q in range(1, len(p))) and not np.array_equal(p[0, 0], p[0, 1])
        assert not np.array_equal(p[0, 0, 0], p[0, 0, 1]) and not np.array_equal(p[0, 0, :, 0], p[0, 0, :, 1])
        coef = np.concatenate([ref.want(k)[s][2] for s in range(c.dims[0])])
        assert np.array_equal(coef, np.round(coef)) and np.abs(coef).max() <= 3
        masks = np.concatenate([ref.want(k)[s][4].reshape(-1) for s in range(c.dims[0])])
        assert 0 < masks.sum() < masks.size


def test_the_order_case_flips_under_the_other_orders():
    k, c = case("order_of_the_chain")
    for s in range(3):
        rows, _, coef, _, masks = ref.want(k)[s]
        assert len(rows) == 2 and coef[0].tolist() == [1.0, 2.0 ** 14, -2.0 ** 14]
        terms = coef[0] * c.protos[s, :, 0, 0].astype(np.float32)
        assert terms.tolist() == [1.0, 2.0 ** 27, -2.0 ** 27]
        assert (F(0) + terms[0] + terms[1]) + terms[2] == 0 and (F(0) + terms[2] + terms[1]) + terms[0] == 1
        assert (terms[0] + terms[1]) + (terms[2] + F(0)) == 0 and terms.astype(np.float64).sum() == 1          # pairwise of these three: 0 as well
        assert masks.sum() == 0
        win = [ref.window_of(b, c.mask, c.in_shape) for b in boxes(c, s)]
        assert win[0].all() and 0 < win[1].sum() < 64
        for wrong in ("descending_k", "float64_acc"):
            w = ref.want(k, **{wrong: True})[s][4]
            assert np.array_equal(w[0].astype(bool), win[0]) and np.array_equal(w[1].astype(bool), win[1]), wrong


def test_window_edges_on_integers_include_the_left_and_exclude_the_right():
    k, c = case("window_edges_on_integers")
    for s in range(3):
        (x1, y1, x2, y2), = boxes(c, s)
        assert (x1 * F(0.25), x2 * F(0.25), y1 * F(0.25), y2 * F(0.25)) == (2.0, 6.0, 1.0, 7.0)
        m = ref.want(k)[s][4][0]
        want = np.zeros((8, 8), dtype=np.uint8)
        want[1:7, 2:6] = 1
        assert np.array_equal(m, want)
        inc = ref.want(k, inclusive_edge=True)[s][4][0]
        want[1:8, 2:7] = 1
        assert np.array_equal(inc, want)


def test_degenerate_windows():
    k, c = case("degenerate_windows")
    for s in range(3):
        rows, _, _, _, masks = ref.want(k)[s]
        assert len(rows) == 6
        assert [int(m.sum()) for m in masks] == [0, 0, 0, 0, 0, 64]
        b = boxes(c, s)
        assert b[0][2] < 0 and b[1][3] < 0 and b[2][0] * F(0.25) >= 8 and b[3][1] * F(0.25) >= 8 and b[4][0] == b[4][2]


@pytest.mark.parametrize("name", ["nan_box_float32", "nan_box_float16"])
def test_a_nan_box_is_kept_and_gives_an_all_zero_mask(name):
    k, c = case(name)
    for s in range(3):
        rows, counters, _, src, masks = ref.want(k)[s]
        assert counters.tolist() == [2, 2, 2] and len(rows) == 2
        b = boxes(c, s)[0]
        assert np.isnan(b[0]) and np.isnan(b[2]) and not np.isnan(b[1])
        assert masks[0].sum() == 0 and masks[1].sum() == 64 and not np.isnan(rows).any()


@pytest.mark.parametrize("name", ["special_logits_proto_float32", "special_logits_proto_float16"])
def test_special_logits_give_zero(name):
    k, c = case(name)
    for s in range(3):
        coef, masks = ref.want(k)[s][2], ref.want(k)[s][4]
        assert coef[0].tolist() == [2.0, -1.0, 1.0]
        p = c.protos[s].astype(np.float32)
        prod = coef[0] * p[:, 2, 3]
        assert (prod == 0).all() and np.signbit(prod).tolist() == [False, True, False]             # +0, -0, +0: the chain gives +0
        assert np.isnan(p[1, 4, 4])
        want = np.ones((8, 8), dtype=np.uint8)
        want[2, 3] = want[4, 4] = 0
        assert np.array_equal(masks[0], want)
        ge = ref.want(k, ge_zero=True)[s][4][0]
        assert ge[2, 3] == 1 and ge[4, 4] == 0 and ge.sum() == 63


def test_sentinel_cases():
    k, c = case("more_survivors_than_max_det")
    w = ref.want(k)
    assert [len(x[0]) for x in w] == [16, 16, 0] and [x[1].tolist() for x in w] == [[24, 24, 24], [24, 24, 24], [0, 0, 0]]
    assert c.mask[1] > 64 and c.mask[0] * c.mask[1] == 2880
    assert sum(len(ref.want(kk)[c2.dims[0] - 1][0]) == 0 for kk, c2 in enumerate(ref.CASES)) >= 8       # streams where nothing passes


def test_tiled_cases_take_rows_from_different_tiles_with_their_own_boxes_and_prototypes():
    for name in ("tiled_T2_iou", "tiled_T2_ios", "tiled_T3_iou_nc_obj", "tiled_T3_ios_cn"):
        k, c = case(name)
        S, A = c.dims
        T = c.tiles
        tiles_seen = set()
        for s in range(S):
            src = ref.want(k)[s][3]
            tiles_seen |= set((src // A).tolist())
            assert all(not np.array_equal(c.protos[s * T], c.protos[s * T + t]) for t in range(1, T))
        assert len(tiles_seen) == T, (name, tiles_seen)
    k, c = case("tiled_T2_iou")
    for s in range(3):                                          # the same anchor, another box in the other tile
        assert ref.box_of(c.preds[2 * s], "cn", 5) != ref.box_of(c.preds[2 * s + 1], "cn", 5)
        src = ref.want(k)[s][3].tolist()
        assert 5 in src and 96 + 5 in src


WRONG_ON = {"descending_k": "order_of_the_chain", "float64_acc": "order_of_the_chain", "inclusive_edge": "window_edges_on_integers",
            "frame_box": "table_8x8_cn_E3_pred_float32_proto_float16", "tile0_protos": "tiled_T2_iou", "ge_zero": "special_logits_proto_float32"}


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_each_wrong_reference_differs_where_intended(wrong):
    k, c = case(WRONG_ON[wrong])
    true, other = ref.want(k), ref.want(k, **{wrong: True})
    assert any(a[4].tobytes() != b[4].tobytes() for a, b in zip(true, other)), wrong
    for a, b in zip(true, other):                               # ... and only in the masks
        assert all(np.array_equal(a[q], b[q], equal_nan=True) for q in range(4))


def test_tile0_prototypes_change_only_rows_of_other_tiles():
    k, c = case("tiled_T2_iou")
    A = c.dims[1]
    for a, b in zip(ref.want(k), ref.want(k, tile0_protos=True)):
        for r, anchor in enumerate(a[3]):
            if anchor < A:
                assert np.array_equal(a[4][r], b[4][r])
