"""GPU tests of the detection post-processing of heads with per-anchor extras (include/boxmot_hip.h boxmot_hip_detpost_create_extra /
_run_extra, boxmot_amd/detpost.py DetPost(extra=...), csrc/det_post_extra.hpp).  Every step is defined in float32 without fused
operations, so every comparison is EXACT (bit for bit against tests/detpost_extra_ref.py): a differing byte is a failure."""
import ctypes

import numpy as np
import pytest

import detpost_extra_ref as ref
import detpost_ref
import detpost_tiled_ref

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
SRC_SENTINEL = -99


def _post(c, **over):
    from boxmot_amd.detpost import DetPost
    S, A = c.dims
    o = dict(c.opts, **over)
    return DetPost(S, A, c.nc, layout=c.layout, extra=c.E, extra_kind=c.kind, tiles=c.tiles or None, **o)


def _outputs(torch, S, stride, E):
    return (torch.full((S, stride, 6), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((S,), -77, dtype=torch.int32, device="cuda"),
            torch.full((S, stride, E), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((S, stride), SRC_SENTINEL, dtype=torch.int32, device="cuda"))


def _assert_stream(name, s, dets, rows, counters, extra, src, want, with_src=True):
    w_rows, w_cnt, w_extra, w_src = want
    k = len(w_rows)
    assert rows[s] == k, (name, s, int(rows[s]), k)
    assert counters[s].tolist() == w_cnt.tolist(), (name, s)
    assert np.array_equal(dets[s, :k].view(np.uint32), w_rows.view(np.uint32)), (name, s)
    assert np.array_equal(extra[s, :k].view(np.uint32), w_extra.view(np.uint32)), (name, s, "extras")
    assert (dets[s, k:] == np.float32(SENTINEL)).all() and (extra[s, k:] == np.float32(SENTINEL)).all(), (name, s, "rows beyond the count were written")
    if with_src:
        assert np.array_equal(src[s, :k], w_src) and (src[s, k:] == SRC_SENTINEL).all(), (name, s, "src")
    else:
        assert (src[s] == SRC_SENTINEL).all(), (name, s)


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_each_case_equals_the_reference_twice(k):
    """rows, extras and source anchors as bytes, counts, counters, untouched sentinel rows in all four blocks -- and the same bytes
    from a second run of the same handle into fresh blocks, on a side stream, this time without a src block"""
    import torch
    c = ref.CASES[k]
    S = c.dims[0]
    pred = torch.from_numpy(c.preds).cuda()
    post = _post(c)
    st = torch.cuda.Stream()
    try:
        first = None
        for rep in range(2):
            with torch.cuda.stream(st):
                d_dets, d_rows, d_extra, d_src = _outputs(torch, S, c.stride, c.E)
                post.run(pred, c.geos, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_extra, d_src=d_src if rep == 0 else None)
                out = (d_dets.clone(), d_rows.clone(), d_extra.clone(), d_src.clone())      # queued behind the kernels
            counters = post.counters()                                                      # waits for the run
            st.synchronize()
            dets, rows, extra, src = (t.cpu().numpy() for t in out)
            for s in range(S):
                _assert_stream(c.name, s, dets, rows, counters, extra, src, ref.want(k)[s], with_src=rep == 0)
            if first is not None:
                assert first[0].tobytes() == dets.tobytes() and first[1].tobytes() == rows.tobytes() and first[2].tobytes() == extra.tobytes() and \
                    first[3].tobytes() == counters.tobytes()
            first = (dets, rows, extra, counters)
    finally:
        torch.cuda.synchronize()
        post.close()


@pytest.mark.parametrize("name", ["table_A96_nc1_cn_float32_E34_kpt2", "tiled_ios_cn_float32"])
def test_fewer_streams_and_then_other_geometry(name):
    """a call over fewer streams than the handle's leaves the last stream alone in all four blocks; a second run of the same handle
    with the streams' geometries swapped maps the keypoints with the new ones"""
    import torch
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    S = c.dims[0]
    T = c.tiles or 1
    post = _post(c)
    try:
        pred = torch.from_numpy(c.preds).cuda()
        d_dets, d_rows, d_extra, d_src = _outputs(torch, S, c.stride, c.E)
        cur = torch.cuda.current_stream().cuda_stream
        post.run(pred, c.geos[:S - 1], d_dets, d_rows, hip_stream=cur, d_extra=d_extra, d_src=d_src)
        counters = post.counters()
        dets, rows, extra, src = (t.cpu().numpy() for t in (d_dets, d_rows, d_extra, d_src))
        for s in range(S - 1):
            _assert_stream(c.name, s, dets, rows, counters, extra, src, ref.want(k)[s])
        assert (dets[S - 1] == np.float32(SENTINEL)).all() and rows[S - 1] == -77 and (extra[S - 1] == np.float32(SENTINEL)).all() and \
            (src[S - 1] == SRC_SENTINEL).all() and counters[S - 1].tolist() == [0, 0, 0]
        geos = [c.geos[1], c.geos[0]] + list(c.geos[2:])
        d_dets, d_rows, d_extra, d_src = _outputs(torch, S, c.stride, c.E)
        post.run(pred, geos, d_dets, d_rows, hip_stream=cur, d_extra=d_extra, d_src=d_src)
        counters = post.counters()
        dets, rows, extra, src = (t.cpu().numpy() for t in (d_dets, d_rows, d_extra, d_src))
        for s in range(S):
            if c.tiles:
                w = ref.detpost_extra_tiled(c.preds[s * T:(s + 1) * T], geos[s], c.layout, c.nc, c.E, c.kind, **c.opts)
            else:
                w = ref.detpost_extra(c.preds[s], geos[s], c.layout, c.nc, c.E, c.kind, **c.opts)
            _assert_stream(c.name, s, dets, rows, counters, extra, src, w)
    finally:
        torch.cuda.synchronize()
        post.close()


def test_run_host_returns_rows_extras_and_src():
    import torch
    k = ref.NAMES.index("raw_encodes_stream_anchor_channel_nc_obj")
    c = ref.CASES[k]
    post = _post(c)
    try:
        got = post.run_host(c.preds, c.geos)
    finally:
        post.close()
    assert len(got) == 3
    for (rows, extras, src), (w_rows, _, w_extras, w_src) in zip(got, ref.want(k)):
        assert np.array_equal(rows.view(np.uint32), w_rows.view(np.uint32)) and np.array_equal(extras.view(np.uint32), w_extras.view(np.uint32))
        assert src.dtype == np.int32 and np.array_equal(src, w_src)


def test_the_comparison_bites():
    """wrong-reference controls: extras in candidate order, and the visibility as a coordinate, differ from the device"""
    import torch
    k = ref.NAMES.index("survivors_cross_a_chunk")
    c = ref.CASES[k]
    post = _post(c)
    try:
        rows, extras, src = post.run_host(torch.from_numpy(c.preds).cuda(), c.geos)[1]
    finally:
        post.close()
    assert np.array_equal(extras.view(np.uint32), ref.want(k)[1][2].view(np.uint32)) and np.array_equal(src, ref.want(k)[1][3])
    for wrong in (dict(candidate_order=True), dict(visibility_is_a_coordinate=True)):
        assert not np.array_equal(extras, ref.want(k, **wrong)[1][2]), wrong


def test_handles_without_extras_give_the_bytes_they_gave():
    """regression guard: the stride and the select kernels changed under them -- three untiled cases of tests/detpost_ref.py and a
    tiled one of tests/detpost_tiled_ref.py through handles WITHOUT extras equal their references, sentinels included"""
    import torch
    from boxmot_amd.detpost import DetPost
    names = [c.name for c in detpost_ref.CASES]
    jobs = [(detpost_ref, names.index(n)) for n in ("clip_to_the_frame", "seam_129_obj_f16", "all_pass_A300_K64_ties_at_K")]
    jobs.append((detpost_tiled_ref, detpost_tiled_ref.NAMES.index("clip_to_the_tile_ios")))
    for mod, k in jobs:
        c = mod.CASES[k]
        if mod is detpost_ref:
            S, A, nc = c.dims
            post = DetPost(S, A, nc, layout=c.layout, **c.opts)
        else:
            S, T, A, nc = c.dims
            post = DetPost(S, A, nc, layout=c.layout, tiles=T, **c.opts)
        try:
            d_dets = torch.full((S, c.stride, 6), SENTINEL, dtype=torch.float32, device="cuda")
            d_rows = torch.full((S,), -77, dtype=torch.int32, device="cuda")
            post.run(torch.from_numpy(c.preds).cuda(), c.geos, d_dets, d_rows, hip_stream=torch.cuda.current_stream().cuda_stream)
            counters = post.counters()
            dets, rows = d_dets.cpu().numpy(), d_rows.cpu().numpy()
            for s in range(S):
                w_rows, w_cnt = mod.want(k)[s]
                assert rows[s] == len(w_rows) and counters[s].tolist() == w_cnt.tolist(), (c.name, s)
                assert np.array_equal(dets[s, :rows[s]].view(np.uint32), w_rows.view(np.uint32)), (c.name, s)
                assert (dets[s, rows[s]:] == np.float32(SENTINEL)).all(), (c.name, s)
        finally:
            torch.cuda.synchronize()
            post.close()


def test_c_abi_refusals():
    import torch
    from boxmot_amd import _lib
    lib = _lib.load()
    base = _lib.DetPostConfig(n_streams=2, n_anchors=64, n_classes=3, layout=0, conf_thres=0.25, iou_thres=0.45, max_candidates=64, max_det=8, agnostic=0,
                              class_allow=None)
    good = dict(base=base, n_tiles=0, merge=0, n_extra=6, extra_kind=2)
    for kw, word in [(dict(n_extra=0), "n_extra"), (dict(n_extra=1025), "n_extra"), (dict(n_extra=-1), "n_extra"), (dict(extra_kind=3), "extra_kind"),
                     (dict(extra_kind=-1), "extra_kind"), (dict(n_extra=5), "n_extra"), (dict(n_extra=7, extra_kind=1), "n_extra"), (dict(n_tiles=65), "n_tiles"),
                     (dict(n_tiles=-1), "n_tiles"), (dict(n_tiles=3, merge=2), "merge")]:
        cfg = _lib.DetPostExtraConfig(**dict(good, **kw))
        assert not lib.boxmot_hip_detpost_create_extra(ctypes.byref(cfg)) and word in _lib.last_error(), (kw, _lib.last_error())
    assert not lib.boxmot_hip_detpost_create_extra(None) and "null" in _lib.last_error()
    cfg = _lib.DetPostExtraConfig(**good)
    h = lib.boxmot_hip_detpost_create_extra(ctypes.byref(cfg))
    assert h, _lib.last_error()
    tcfg = _lib.DetPostExtraConfig(**dict(good, n_tiles=2))
    ht = lib.boxmot_hip_detpost_create_extra(ctypes.byref(tcfg))
    assert ht, _lib.last_error()
    plain = lib.boxmot_hip_detpost_create(ctypes.byref(base))
    assert plain, _lib.last_error()
    try:
        pred = torch.zeros((4, 13, 64), device="cuda")
        d_dets, d_rows, d_extra, d_src = _outputs(torch, 2, 8, 6)
        geom = np.array([[1.0, 0, 0, 64, 64], [0.5, 0, 0, 64, 64]], dtype=np.float64)
        tgeom = np.array([[[1.0, 0, 0, 0, 0, 64, 64]] * 2] * 2, dtype=np.float64)
        P = lambda t: ctypes.c_void_p(t.data_ptr())

        def call(handle=h, n=2, dtype=0, g=geom, stride=8, extra=d_extra.data_ptr(), src=d_src.data_ptr()):
            ok = lib.boxmot_hip_detpost_run_extra(handle, n, P(pred), dtype, g.ctypes.data_as(_lib.c_double_p), P(d_dets), stride, P(d_rows),
                                                  ctypes.c_void_p(extra), ctypes.c_void_p(src), None)
            return ok, _lib.last_error()
        bad_geom = geom.copy()
        bad_geom[1, 0] = 0.0
        for kw, word in [(dict(n=0), "stream count"), (dict(n=3), "stream count"), (dict(dtype=2), "dtype"), (dict(stride=7), "max_det"), (dict(extra=0), "d_extra"),
                         (dict(extra=d_extra.data_ptr() + 2), "aligned"), (dict(src=d_src.data_ptr() + 2), "aligned"), (dict(g=bad_geom), "stream 1"),
                         (dict(handle=plain), "boxmot_hip_detpost_create_extra"), (dict(handle=None), "null")]:
            ok, msg = call(**kw)
            assert not ok and word in msg, (kw, msg)
        # a handle with extras through the two older entry points, tiled or not: refused, naming the right one
        for entry, handle, g in ((lib.boxmot_hip_detpost_run, h, geom), (lib.boxmot_hip_detpost_run_tiled, ht, tgeom), (lib.boxmot_hip_detpost_run, ht, geom),
                                 (lib.boxmot_hip_detpost_run_tiled, h, tgeom)):
            assert not entry(handle, 2, P(pred), 0, g.ctypes.data_as(_lib.c_double_p), P(d_dets), 8, P(d_rows), None)
            assert "boxmot_hip_detpost_run_extra" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        assert (d_dets == SENTINEL).all() and (d_rows == -77).all() and (d_extra == SENTINEL).all() and (d_src == SRC_SENTINEL).all()     # none of them wrote
        for handle, g in ((h, geom), (ht, tgeom)):
            ok, msg = call(handle=handle, g=g)
            assert ok, msg
            ok, msg = call(handle=handle, g=g, src=0)                   # d_src may be null
            assert ok, msg
        torch.cuda.synchronize()
        assert d_rows.tolist() == [0, 0] and (d_extra == SENTINEL).all() and (d_src == SRC_SENTINEL).all()
    finally:
        torch.cuda.synchronize()
        for x in (h, ht, plain):
            lib.boxmot_hip_detpost_destroy(x)


def test_pose_head_detpost_step_device_end_to_end():
    """a synthetic pose head -> DetPost(extra=6, extra_kind="kpt3").run -> MultiStreamBotSort.step_device for three frames of eight
    well-separated, slightly moving boxes per stream whose keypoints encode the box's identity: in every output row,
    d_extra[s, det_ind] is the skeleton of the box that row's track started on"""
    import torch
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.streams import MultiStreamBotSort
    S, A, ND, NB, FRAMES = 2, 128, 16, 8, 3
    post = DetPost(S, A, 1, layout="cn", extra=6, extra_kind="kpt3", conf=0.25, iou=0.45, max_det=ND, max_candidates=64)
    trk = MultiStreamBotSort(S, max_tracks=64, max_dets=ND, emb_dim=1, with_reid=False)
    st = torch.cuda.current_stream()

    def centre(s, b, t):
        return 60.0 + 140 * (b % 4) + 2 * t + s, 100.0 + 250 * (b // 4) + t

    try:
        d_dets = torch.zeros((S, ND, 6), dtype=torch.float32, device="cuda")
        d_rows = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_kpts = torch.zeros((S, ND, 6), dtype=torch.float32, device="cuda")
        d_src = torch.zeros((S, ND), dtype=torch.int32, device="cuda")
        d_out = torch.zeros((S, ND, 8), dtype=torch.float32, device="cuda")
        d_out_n = torch.zeros(S, dtype=torch.int32, device="cuda")
        started_on = {}                                         # (stream, track id) -> the box it started on
        total = 0
        for t in range(FRAMES):
            rng = np.random.default_rng(t)
            pred = np.zeros((S, 4 + 1 + 6, A), dtype=np.float32)
            pred[:, :4] = rng.uniform(8, 48, (S, 4, A))
            pred[:, 4] = rng.uniform(0, 0.2, (S, A))                                            # clutter below the threshold
            pred[:, 5:] = rng.uniform(0, 600, (S, 6, A))
            where = {}
            for s in range(S):
                for b in range(NB):
                    a = (7 + 13 * b + 5 * t + s) % A                                            # another anchor every frame
                    cx, cy = centre(s, b, t)
                    # keypoint 0: the box's centre, visibility (b + 1) / 16; keypoint 1: 10 b + 1, 10 b + 2, visibility s / 4
                    pred[s, :, a] = [cx, cy, 50, 80, 0.9 - 0.03 * b, cx, cy, (b + 1) / 16, 10 * b + 1, 10 * b + 2, s / 4]
                    where[s, a] = b
            post.run(torch.from_numpy(pred).cuda(), [detpost_ref.GEO_UNIT] * S, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_kpts, d_src=d_src)
            st.synchronize()                                    # the tracker's own stream starts after the rows are there
            trk.step_device(d_dets.data_ptr(), d_rows.data_ptr(), None, None, 0, 0, d_out.data_ptr(), d_out_n.data_ptr())
            trk.synchronize()
            rows, kpts, src, out, out_n = (x.cpu().numpy() for x in (d_rows, d_kpts, d_src, d_out, d_out_n))
            assert rows.tolist() == [NB] * S
            for s in range(S):
                assert sorted(where[s, int(a)] for a in src[s, :NB]) == list(range(NB)), (t, s)
                for row in out[s, :out_n[s]]:
                    tid, det_ind = int(row[4]), int(row[7])
                    assert 0 <= det_ind < NB
                    sk = kpts[s, det_ind]
                    b = where[s, int(src[s, det_ind])]
                    cx, cy = centre(s, b, t)
                    assert sk.tolist() == [np.float32(cx), np.float32(cy), (b + 1) / 16, 10 * b + 1, 10 * b + 2, s / 4], (t, s, tid)
                    assert abs((row[0] + row[2]) / 2 - cx) < 20 and abs((row[1] + row[3]) / 2 - cy) < 20, (t, s, tid, row)     # the track's own box
                    assert started_on.setdefault((s, tid), b) == b, (t, s, tid, "the skeleton is another box's than the track started on")
                    total += 1
        assert total >= S * NB and len(started_on) == S * NB and (trk.status() == 0).all()
    finally:
        torch.cuda.synchronize()
        post.close(); trk.close()
