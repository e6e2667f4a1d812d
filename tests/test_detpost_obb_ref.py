"""The NumPy restatement of the oriented detection post-processing (tests/detpost_obb_ref.py) against hand-worked values, the
margin every case has to keep for its decisions to be the same in every arithmetic, and the two NMS modes on the chain."""
import numpy as np
import pytest

import detpost_obb_ref as ref

F = np.float32


def _iou(b1, b2, dtype=np.float64):
    """ProbIoU of two (cx, cy, w, h, angle) boxes"""
    g = ref.gaussians(np.array([b1[:4], b2[:4]], dtype=np.float32), np.array([b1[4], b2[4]], dtype=np.float32), dtype)
    return float(ref.probiou(g[0], g[1]))


def test_hand_worked_gaussian():
    """w = 4, h = 2: a = 4 / 3, b = 1 / 3; at angle 0 the Gaussian is (a, b, 0), at a quarter turn (b, a, ~0), and at 45 degrees
    A = B = (a + b) / 2, C = (a - b) / 2"""
    box = np.array([[7, 9, 4, 2]] * 3, dtype=np.float32)
    g = ref.gaussians(box, np.array([0, np.pi / 2, np.pi / 4], dtype=np.float32), np.float64)
    assert np.allclose(g[0], [7, 9, 4 / 3, 1 / 3, 0], atol=1e-12)
    assert np.allclose(g[1], [7, 9, 1 / 3, 4 / 3, 0], atol=1e-7)
    assert np.allclose(g[2], [7, 9, 5 / 6, 5 / 6, 1 / 2], atol=1e-7)
    g32 = ref.gaussians(box, np.array([0, np.pi / 2, np.pi / 4], dtype=np.float32), np.float32)
    assert g32.dtype == np.float32 and np.allclose(g32, g, atol=1e-6)


def test_hand_worked_probiou():
    """identical boxes: the distance is clamped to eps = 1e-7 and ProbIoU = 1 - sqrt(1 - exp(-eps) + eps) = 1 - sqrt(2e-7); distant
    boxes: the distance is clamped to 100 and ProbIoU = 1 - sqrt(1 + eps) < 0; a cross of two w x h boxes with one centre: the centre
    terms vanish and exp(-bd) = 2 sqrt(a b) / (a + b) = 2 w h / (w^2 + h^2): 8 / 17 for 40 x 10, so ProbIoU = 1 - sqrt(9 / 17)"""
    t = ref.TABLE
    assert abs(_iou(t[0], t[1]) - (1 - np.sqrt(2e-7))) < 1e-6
    assert -1e-6 < _iou(t[0], t[2]) < 0 and -1e-6 < _iou(t[2], t[3]) < 0
    assert abs(_iou(t[3], t[4]) - (1 - np.sqrt(9 / 17))) < 1e-6
    assert abs(_iou(t[3], t[4], np.float32) - (1 - np.sqrt(9 / 17))) < 1e-4
    # a shift d of a w x w box along x: bd = d^2 / (8 w^2 / 12): the chain's links, 12 and 24 px of a 40 px box
    for d, k in ((12, 1), (24, 2)):
        bd = d * d / (8 * 1600 / 12)
        assert abs(_iou(ref.CHAIN[0], ref.CHAIN[k]) - (1 - np.sqrt(1 - np.exp(-bd) + 1e-7))) < 1e-6
    assert _iou(ref.CHAIN[0], ref.CHAIN[1]) > 0.6 and _iou(ref.CHAIN[0], ref.CHAIN[2]) < 0.4
    # ProbIoU does not see the regularisation: (w, h, angle) and (h, w, angle + pi / 2) are one Gaussian
    assert abs(_iou((10, 10, 30, 8, 0.4), (14, 12, 8, 30, 0.4 + np.pi / 2)) - _iou((10, 10, 30, 8, 0.4), (14, 12, 30, 8, 0.4))) < 1e-6


def test_hand_worked_table_rows():
    k = ref.NAMES.index("hand_worked_table")
    rows, counters = ref.want(k)[0]
    assert counters.tolist() == [5, 5, 4] and rows.dtype == np.float32 and rows.shape == (4, 7)
    assert rows[:, 5].tolist() == [F(0.9), F(0.7), F(0.6), F(0.5)]              # the duplicate is gone, both arms of the cross stay
    assert rows[0].tolist() == [100, 100, 40, 20, 0.5, F(0.9), 0] and rows[3, 4] == F(np.pi / 2)


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_every_case_keeps_the_margin(k):
    """no pair the NMS could compare within 2e-3 of the threshold -- none, not a share -- and float32 within 2e-4 of float64"""
    c = ref.CASES[k]
    margin, err32 = ref.check_margin(c)
    print(c.name, "margin", margin, "float32 error", err32)
    assert margin >= ref.MARGIN == 2e-3 and err32 <= ref.FP32_ERR == 2e-4
    S, A, nc = c.dims
    if c.name != "K4096_A4504":
        assert S <= 3 and A <= 600 and nc in (1, 3, 15)
    p = c.preds.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        passing = p[:, 4:4 + nc].max(axis=1) > 0.25
        aspect = np.maximum(p[:, 2] / p[:, 3], p[:, 3] / p[:, 2])
    assert aspect[passing].max() <= 16


def test_the_modes_differ_exactly_on_the_third_of_the_chain():
    kg, kf = ref.NAMES.index("chain_greedy"), ref.NAMES.index("chain_fast")
    assert np.array_equal(ref.CASES[kg].preds, ref.CASES[kf].preds)
    (g_rows, g_cnt), (f_rows, f_cnt) = ref.want(kg)[0], ref.want(kf)[0]
    assert g_cnt.tolist() == [4, 4, 3] and f_cnt.tolist() == [4, 4, 2]
    assert g_rows[:, 5].tolist() == [F(0.9), F(0.7), F(0.6)] and f_rows[:, 5].tolist() == [F(0.9), F(0.6)]
    assert g_rows[1, 0] == 124                                                  # c, which b would have suppressed
    # and somewhere in the ~ 200 candidates too
    a, b = (ref.want(ref.NAMES.index(f"clusters_200_{m}_A600_float16"))[0][1] for m in ref.NMS_MODES)
    assert a[2] > b[2] and a[:2].tolist() == b[:2].tolist() == [200, 200]


def test_the_cases_cover_what_they_are_named_for():
    n = ref.NAMES.index
    # classes
    assert ref.want(n("classes_kept_apart"))[0][1][2] == 3 and ref.want(n("classes_agnostic"))[0][1][2] == 2
    k = n("allow_list_nc15")
    assert set(np.concatenate([w[0][:, 6] for w in ref.want(k)]).astype(int)) <= {0, 2, 7, 14}
    assert ref.detpost_obb(ref.CASES[k].preds[0], ref.CASES[k].geos[0], **dict(ref.CASES[k].opts, classes=None))[1][0] > ref.want(k)[0][1][0]
    # the angle is in the last row: read from channel 4 the result differs
    k = n("angle_in_the_last_row")
    assert not np.array_equal(ref.want(k)[0][0], ref.want(k, angle_row=4)[0][0])
    # non-finite angles never pass: three anchors better than everything else are absent
    for name in ("non_finite_angle_A64_float16", "non_finite_angle_A63_float32"):
        rows, cnt = ref.want(n(name))[0]
        assert cnt.tolist() == [4, 4, 3] and rows[:, 5].max() == F(ref.CASES[n(name)].preds.dtype.type(0.9)) and np.isfinite(rows).all()
    # top-K with ties at the boundary
    k = n("all_pass_A600_K64_ties_at_K")
    pr = ref.pairs(ref.CASES[k].preds[0], **ref.CASES[k].opts)
    assert pr.n_pass == 600 and len(pr.order) == 64
    last = pr.conf[pr.order[-1]]
    assert (pr.conf == last).sum() > (pr.conf[pr.order] == last).sum() > 0      # the K boundary cuts through equal confs ...
    tied = np.nonzero(pr.conf == last)[0]
    assert pr.order[pr.conf[pr.order] == last].tolist() == tied[:(pr.conf[pr.order] == last).sum()].tolist()     # ... lowest anchors first
    # max_det cuts, counter 2 is taken before
    rows, cnt = ref.want(n("more_survivors_than_max_det"))[0]
    assert len(rows) == 10 < cnt[2]
    # a centre outside the frame stays outside
    w = ref.want(n("three_geometries_unclipped"))
    assert (w[0][0][:, 0] < 0).sum() == 1 and w[2][0][0, 1] < 0 and len({c for c in ref.CASES[n("three_geometries_unclipped")].geos}) == 3
    # regularize: w >= h, the angle within [0, pi], and the same boxes without it have h > w and angles outside
    rows = ref.want(n("regularize"))[0][0]
    assert (rows[:, 2] >= rows[:, 3]).all() and (rows[:, 4] >= 0).all() and (rows[:, 4] <= F(np.pi)).all()
    off = ref.want(n("regularize_off"))[0][0]
    assert (off[:, 3] > off[:, 2]).sum() == 3 and (off[:, 4] < 0).sum() == 2 and (off[:, 4] >= F(np.pi)).sum() == 1
    assert rows[0].tolist() == [100, 100, 40, 10, F(F(0.5) + F(np.pi / 2)), F(0.9), 0]
    assert rows[1, 4] == F(F(-0.75) + F(np.pi)) and rows[2, 4] == np.fmod(F(3.5), F(np.pi))
    # the largest table
    assert ref.want(n("K4096_A4504"))[0][1][:2].tolist() == [4504, 4096]


def test_the_threshold_decides_the_chain():
    """above the links' ProbIoU (~ 0.64) nothing is suppressed; below the ends' (~ 0.35) a suppresses b and c, whatever the mode"""
    k = ref.NAMES.index("chain_greedy")
    c = ref.CASES[k]
    assert ref.detpost_obb(c.preds[0], c.geos[0], **dict(c.opts, iou=0.7))[1].tolist() == [4, 4, 4]
    assert ref.detpost_obb(c.preds[0], c.geos[0], **dict(c.opts, iou=0.3))[1].tolist() == [4, 4, 2]
