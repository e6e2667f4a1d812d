"""Self-checks of tests/detpost_labels_ref.py, the NumPy restatement of the frame-space label map (csrc/det_post_labels.hpp) and
its table of cases: every case is what its name says, every wrong reference changes at least one pixel on the case named for it,
and the random inputs have the magnitudes that keep subnormals out.  No library, no device."""
import numpy as np
import pytest

import detpost_labels_ref as ref

F = np.float32


def case(name):
    k = ref.NAMES.index(name)
    return k, ref.CASES[k]


def test_the_table_covers_what_it_should():
    names = ref.NAMES
    assert len(set(names)) == len(names)
    table = [c for c in ref.CASES if c.name.startswith("table_")]
    assert len(table) == 18 and {(c.mask, c.in_shape) for c in table} == set(ref.SHAPES)
    for mask, in_shape in ref.SHAPES:
        mine = [c for c in table if c.mask == mask]
        assert {(int(c.geos[0][3]), int(c.geos[0][4])) for c in mine} == {(24, 40), (50, 31), ref.SMALL[mask]}
        assert {c.geos[0][1] > 0 or c.geos[0][2] > 0 for c in mine} == {True, False}              # centre and top-left
        assert {c.E for c in mine} == {32, 5} and {c.protos.dtype.name for c in mine} == {"float16", "float32"}
    for c in ref.CASES:
        S = len(c.geos)
        assert c.dets.shape == (S, c.stride, 6) and c.coefs.shape == (S, c.stride, c.E) and c.protos.shape == (S, c.E) + c.mask
        assert c.stride >= c.max_det and c.max_det <= 32767
        for g in c.geos:
            assert g[3] <= c.plane[0] and g[4] <= c.plane[1]


def test_the_small_frames_have_a_gain_that_passes_the_prototype_pitch():
    """gain > 1, gain * wr > 1 and gain * hr > 1: neighbouring frame pixels are more than a prototype pixel apart"""
    for c in ref.CASES:
        rows, cols = int(c.geos[0][3]), int(c.geos[0][4])
        if c.name.startswith("table_") and (rows, cols) == ref.SMALL[c.mask]:
            gain = c.geos[0][0]
            assert gain > 1 and gain * c.mask[1] / c.in_shape[1] > 1 and gain * c.mask[0] / c.in_shape[0] > 1, c.name
            j0 = ref.tap(cols, gain, c.geos[0][2], F(c.mask[1]) / F(c.in_shape[1]), c.mask[1])[0]
            assert (np.diff(j0) >= 1).all(), c.name                       # no two columns share their first tap


def test_the_odd_shape_clamps_its_second_tap():
    """(7, 9) for (28, 30): the last columns and lines have j1 == j0 == mask_w - 1 (i likewise) with weight 0 ... and the first ones pu
    clamped at 0"""
    _, c = case("table_7x9_frame_24x40_topleft_E5_float32")
    g = c.geos[0]
    j0, j1, lx = ref.tap(40, g[0], g[2], F(9) / F(30), 9)
    assert j0[-1] == j1[-1] == 8 and lx[-1] == 0 and j0[0] == 0 and lx[0] == 0
    assert (np.diff(j0) >= 0).all() and (j1 - j0 <= 1).all() and (lx >= 0).all() and (lx < 1).all()
    _, c = case("table_7x9_frame_50x31_topleft_E5_float16")            # (the frame that fills the input's height)
    g = c.geos[0]
    i0, i1, ly = ref.tap(50, g[0], g[1], F(7) / F(28), 7)
    assert i0[-1] == i1[-1] == 6 and ly[-1] == 0 and i0[0] == 0 and ly[0] == 0


def test_the_ratios_and_the_map_round_where_the_table_says():
    assert F(8) / F(32) == 0.25 and F(20) / F(64) == 0.3125
    wr = F(9) / F(30)
    assert float(wr) != 0.3
    pu = ref.tap(40, F(0.7), F(1), wr, 9)[2]
    exact = ((np.arange(40) + 0.5) * float(F(0.7)) + 1.0) * float(wr) - 0.5
    assert (np.abs(pu - (exact - np.floor(exact))) > 0).any()               # float32 rounding is visible in the weights


def test_random_inputs_keep_subnormals_out():
    n = 0
    for c in ref.CASES:
        if not (c.name.startswith("table_") or c.name.startswith("three_streams") or c.name in ("more_rows_than_a_chunk", "patch_beyond_the_budget")):
            continue
        n += 1
        for v in (c.coefs, c.protos.astype(np.float32)):
            assert np.array_equal(v, v.astype(np.float16).astype(np.float32))
            mag = np.abs(v[v != 0])
            assert mag.size == 0 or (mag.min() >= 2.0 ** -6 and mag.max() <= 2.0 ** 6)
    assert n == 22


def test_every_frame_pixel_is_a_row_below_the_count_or_minus_one():
    for k, c in enumerate(ref.CASES):
        for s, lab in enumerate(ref.want(k)):
            n = min(int(c.n_rows[s]), c.max_det)
            assert lab.dtype == np.int16 and lab.shape == (int(c.geos[s][3]), int(c.geos[s][4]))
            assert lab.min() >= -1 and lab.max() < max(n, 0) or (n == 0 and (lab == -1).all()), c.name


def test_the_table_cases_show_the_rows_that_can_show():
    """the scene's rows 0, 1, 3 and 5 own pixels (the whole-frame row shows through where the others' logits are <= 0); row 2 is nested
    and may be shadowed; row 4 has no area"""
    shows_2 = 0
    for k, c in enumerate(ref.CASES):
        rows, cols = int(c.geos[0][3]), int(c.geos[0][4])
        if c.name.startswith("table_") and rows * cols > 100:
            seen = set(np.unique(ref.want(k)[0]).tolist())
            assert seen - {2} == {-1, 0, 1, 3, 5}, (c.name, seen)
            shows_2 += 2 in seen
    assert shows_2 >= 6


def test_first_wins():
    k, c = case("first_wins_two")
    lab = ref.want(k)[0]
    assert (lab[4:20, 4:30] == 0).all() and (lab[2:22, 30:38] == 1).all() and (lab[2:4, 10:38] == 1).all() and (lab[:, :4] == -1).all()
    k, c = case("first_wins_three")
    lab = ref.want(k)[0]
    assert (lab[8:16, :4] == 2).all() and (lab[8:16, 38:] == 2).all() and (lab[8:16, 4:30] == 0).all() and (lab[8:16, 30:38] == 1).all()
    k, c = case("nested")
    lab = ref.want(k)[0]
    assert (lab[8:14, 12:20] == 0).all() and (lab[4:8, 6:30] == 1).all() and (lab[0:4] == 2).all() and set(np.unique(lab).tolist()) == {0, 1, 2}


def test_edges():
    k, c = case("edges_on_integers")
    lab = ref.want(k)[0]
    assert (lab[4:12, 8:20] == 0).all() and (lab[4:12, 7] == -1).all() and (lab[4:12, 20] == -1).all() and (lab[3, 8:20] == -1).all() and (lab[12, 8:20] == -1).all()
    assert (lab[16:24, 30:40] == 1).all() and (lab == 1).sum() == 80               # flush with the right and bottom edge
    k, c = case("zero_area")
    assert (ref.want(k)[0] == 2).all()
    k, c = case("zero_rows")
    assert (ref.want(k)[0] == -1).all() and (ref.want(k)[1] == 0).all()
    k, c = case("more_kept_than_max_det")
    lab = ref.want(k)[0]
    assert c.n_rows[0] == 6 > c.max_det == 4 and (lab[10:] == -1).all() and [int(lab[5, 5 + 10 * q]) for q in range(4)] == [0, 1, 2, 3]


def test_nans_and_zeros():
    k, c = case("nan_coefficients")
    lab = ref.want(k)[0]
    assert np.isnan(c.coefs[0, 0]).any() and (lab[4:20, 4:36] == 1).all() and (lab == 0).sum() == 0 and (lab == -1).sum() == 24 * 40 - 16 * 32
    for name in ("nan_prototype_float32", "nan_prototype_float16"):
        k, c = case(name)
        lab = ref.want(k)[0]
        hole = np.argwhere(lab == -1)
        assert np.isnan(c.protos[0, 2, 3, 4]) and 0 < len(hole) < lab.size / 4 and (lab[lab >= 0] == 0).all()
        # the hole is where a tap falls on prototype (3, 4): frame pixels whose centre maps within one prototype pixel of it
        g = c.geos[0]
        j0, j1, _ = ref.tap(40, g[0], g[2], F(0.25), 8)
        i0, i1, _ = ref.tap(24, g[0], g[1], F(0.25), 8)
        on = ((i0 == 3) | (i1 == 3))[:, None] & ((j0 == 4) | (j1 == 4))[None, :]
        assert np.array_equal(lab == -1, on)
    k, c = case("nan_box")
    lab = ref.want(k)[0]
    assert (lab[4:20, 4:36] == 2).all() and set(np.unique(lab).tolist()) == {-1, 2}
    k, c = case("signed_zero_logits_row_0")
    assert (ref.want(k)[0] == -1).all()
    g = ref.logits_of(c.coefs[0, 0], c.protos[0])
    assert (g == 0).all() and not np.signbit(g).any()                      # 0 + (+-0) is +0 in round-to-nearest
    k, c = case("signed_zero_logits_left_half")
    lab = ref.want(k)[0]
    assert set(np.unique(lab).tolist()) == {-1, 0} and (lab[:, :10] == -1).all() and (lab[:, 30:] == 0).all()


def test_more_rows_than_a_chunk_and_the_budget_case():
    k, c = case("more_rows_than_a_chunk")
    lab = ref.want(k)[0]
    assert c.n_rows[0] == 270 and lab.max() == 269 and (np.unique(lab) > 256).sum() >= 5          # rows of the second chunk own pixels
    k, c = case("patch_beyond_the_budget")
    ph, pw = ref.patch_of(c.geos[0], c.mask, c.in_shape, 0, 0)
    assert ph * pw > ref.PATCH and c.geos[0][0] == 2.0


WRONG_ON = {"corner": "table_8x8_frame_24x40_centre_E32_float16", "last_wins": "first_wins_three", "threshold_first": "table_12x20_frame_50x31_topleft_E5_float32",
            "letterbox_window": "table_7x9_frame_24x40_centre_E32_float32", "inclusive_edge": "edges_on_integers", "float64_acc": "order_of_the_chain"}


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_every_wrong_reference_changes_a_pixel_on_its_case(wrong):
    k, _ = case(WRONG_ON[wrong])
    right, other = ref.want(k)[0], ref.want(k, **{wrong: True})[0]
    assert right.shape == other.shape and (right != other).any(), wrong


def test_the_named_controls_change_what_they_should():
    k, _ = case("edges_on_integers")
    other = ref.want(k, inclusive_edge=True)[0]
    assert (other[4:13, 20] == 0).all() and (other[12, 8:21] == 0).all() and (ref.want(k)[0][12, 8:21] == -1).all()
    k, _ = case("order_of_the_chain")
    assert (ref.want(k)[0] == -1).all() and (ref.want(k, float64_acc=True)[0] == 0).all()
    k, _ = case("first_wins_three")
    assert (ref.want(k, last_wins=True)[0][8:16] == 2).all()
