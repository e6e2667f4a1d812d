"""tests/detpost_ref.py -- the NumPy restatement the detection post-processing kernels are compared with -- against tables worked
out by hand from the definition (boxmot_amd/csrc/det_post.hpp), and the properties the cases of its table were built to have."""
import numpy as np
import pytest

import detpost_ref as ref

F = np.float32
NAMES = [c.name for c in ref.CASES]


def case(name):
    k = NAMES.index(name)
    return ref.CASES[k], ref.want(k)


def test_iou_of_exactly_one_half_is_kept_by_the_strict_comparison():
    """(0, 0, 2, 2) and (0, 0, 2, 1): inter 2, union 4 + 2 - 2 = 4, IoU = 0.5 exactly"""
    a, b = np.array([[0, 0, 2, 2]], F), np.array([0, 0, 2, 1], F)
    below = np.nextafter(F(0.5), F(0))
    assert not ref.suppresses(a, b, 0.5)[0] and ref.suppresses(a, b, below)[0] and ref.suppresses(a, b, 0.5, ge=True)[0]
    c, w = case("iou_exactly_half_kept")
    assert w[0][0][:, :4].tolist() == [[0, 0, 2, 2], [0, 0, 2, 1]] and w[0][1].tolist() == [2, 2, 2]
    c, w = case("iou_exactly_half_suppressed")
    assert c.opts["iou"] == float(below) < 0.5
    assert w[0][0][:, :4].tolist() == [[0, 0, 2, 2]] and w[0][1].tolist() == [2, 2, 1]
    assert not ref.suppresses(np.array([[0, 0, 0, 0]], F), np.array([0, 0, 0, 0], F), 0.0)[0]          # 0 / 0 does not suppress


def test_argmax_ties_go_to_the_lowest_class_and_conf_ties_to_the_lowest_anchor():
    """six boxes of conf 0.5 at anchors 40, 3, 63, 0, 17, 5 (x centres 100, 150, .. 350), class 2; anchors 3 and 17 have class 1 at
    0.5 too.  max_det 4: anchors 0, 3, 5, 17 in that order"""
    c, w = case("argmax_and_conf_ties")
    rows, counters = w[0]
    assert counters.tolist() == [6, 6, 6]
    assert rows[:, 0].tolist() == [240, 140, 340, 290] and rows[:, 2].tolist() == [260, 160, 360, 310]
    assert rows[:, 4].tolist() == [0.5] * 4 and rows[:, 5].tolist() == [2, 1, 2, 1]
    wrong = ref.want(NAMES.index("argmax_and_conf_ties"), ties_high_first=True)[0][0]
    assert wrong[:, 0].tolist() == [190, 90, 290, 340]                                                 # anchors 63, 40, 17, 5


def test_threshold_is_strict_and_obj_multiplies():
    c, w = case("one_anchor_below_obj_f16")                  # 0.5 * 0.5 = 0.25, not > 0.25
    assert len(w[0][0]) == 0 and w[0][1].tolist() == [0, 0, 0]
    c, w = case("one_anchor_cn_f32")
    assert w[0][1].tolist() == [1, 1, 1] and w[0][0][0, 4] == 0.5
    c, w = case("chain_in_obj_layout")                       # obj 0.75: confs 0.9 * 0.75, ...
    assert w[0][0][:, 4].tolist() == [F(0.75) * F(0.9), F(0.75) * F(0.7)]


def test_chain_duplicates_and_classes():
    c, w = case("chain_frees_the_third")                     # a kept, b suppressed by a, c kept (b is gone), d suppressed by c
    assert w[0][0][:, 0].tolist() == [100, 106] and w[0][1].tolist() == [4, 4, 2]
    c, w = case("exact_duplicates")
    assert [len(r) for r, _ in w] == [2, 2] and w[0][1].tolist() == [5, 5, 2]
    c, w = case("classes_kept_apart")
    assert w[0][0][:, 4:].tolist() == [[F(np.float16(0.9)), 0], [F(np.float16(0.8)), 2], [F(np.float16(0.6)), 1]]
    c, w = case("classes_agnostic")
    assert w[0][0][:, 5].tolist() == [0, 1] and w[0][1].tolist() == [4, 4, 2]


def test_nan_scores_never_pass_and_are_never_the_maximum():
    c, w = case("nan_scores")                                # anchor 1: every score NaN; anchor 2: class 0 NaN beside 0.8 in class 1
    assert w[0][0][:, 4:].tolist() == [[F(0.8), 1], [F(0.7), 2]] and w[0][1].tolist() == [2, 2, 2]
    c, w = case("nan_obj")
    assert w[0][0][:, 5].tolist() == [1] and w[0][1].tolist() == [1, 1, 1]


def test_to_frame_is_letterbox_geometrys():
    from boxmot_amd.ingest import letterbox_geometry
    rng = np.random.default_rng(3)
    xyxy = (rng.random((200, 4)) * 900 - 130).astype(F)
    for (rows, cols), size, mode in [((1080, 1920), (640, 640), "center"), ((1080, 1920), (640, 640), "topleft"), ((700, 300), (64, 64), "center"),
                                     ((97, 211), (640, 512), "center")]:
        g = letterbox_geometry(rows, cols, size, mode)
        got = ref.to_frame(xyxy, ref.geo_of(rows, cols, size, mode))
        assert np.array_equal(got.view(np.uint32), g.to_frame(xyxy).view(np.uint32))
    # by hand: 1080 x 1920 into 640 x 640, centred: gain 1 / 3, 140 rows of padding above
    assert ref.GEO_CENTER[:3] == (1 / 3, 140, 0)
    got = ref.to_frame(np.array([[270, 110, 370, 150], [-15, 130, 25, 600]], F), ref.GEO_CENTER)
    assert got.tolist() == [[F(270) / F(1 / 3), 0, F(370) / F(1 / 3), F(10) / F(1 / 3)], [0, 0, F(25) / F(1 / 3), 1080]]
    c, w = case("clip_to_the_frame")
    assert all((r[:, :4] >= 0).all() and (r[:, [0, 2]] <= g[4]).all() and (r[:, [1, 3]] <= g[3]).all() for (r, _), g in zip(w, c.geos))
    assert any((r[:, :4] == 0).any() for r, _ in w) and (w[0][0][:, 2] == 1920).any() and (w[2][0][:, :4] > 0).any()


def test_the_cases_reach_what_they_were_built_for():
    c, w = case("random_A8400_nc80_cn_f16_topk")
    assert w[0][1][0] > 2000 and w[0][1][1] == 1024 and 20 < w[0][1][2] < 1024
    for name in ("all_pass_A300_K64_ties_at_K", "all_pass_A300_K64_nc_obj"):
        c, w = case(name)
        assert w[0][1][:2].tolist() == [300, 64]
        _, cf, passed = ref.score(c.preds[0], c.layout, c.opts["conf"])
        top = np.sort(cf[passed])[::-1]
        assert top[63] == top[64]                            # a conf tie across the K boundary: the anchor index decides who is in
    c, w = case("nothing_passes")
    assert all(len(r) == 0 and k.tolist() == [0, 0, 0] for r, k in w)
    c, w = case("more_survivors_than_max_det")
    assert len(w[0][0]) == 10 and w[0][1][2] > 10
    for n in (63, 64, 65, 129):
        c, w = case(f"seam_{n}_candidates")
        assert w[0][1][:2].tolist() == [n, n] and (w[0][1][2] < n) == (n == 129)      # from the 66th on, suppressions across a seam
    c, w = case("allow_list")
    assert all(set(r[:, 5].astype(int)) <= {0, 2, 17, 79} and len(r) for r, _ in w)
    assert w[1][0][:, 5].tolist() == [0, 2]                  # class 1's box is gone; the list is applied after the argmax
    assert {c.layout for c in ref.CASES} == {"cn", "nc_obj"} and {c.preds.dtype for c in ref.CASES} == {np.dtype(np.float16), np.dtype(np.float32)}
    assert {c.dims[1] for c in ref.CASES} >= {1, 63, 64, 65, 257, 1000, 8400} and {c.dims[2] for c in ref.CASES} == {1, 3, 80}


def test_references_are_float32_and_prefixes():
    for k, c in enumerate(ref.CASES):
        for rows, counters in ref.want(k):
            assert rows.dtype == np.float32 and rows.shape[1] == 6 and counters.dtype == np.int32
            assert len(rows) == min(counters[2], c.opts["max_det"]) and counters[1] == min(counters[0], c.opts["max_candidates"])
            assert (np.diff(rows[:, 4]) <= 0).all()
