"""GPU tests of the device-side post-processing of oriented detector heads (include/boxmot_hip.h boxmot_hip_detpost_create_obb,
boxmot_amd/detpost.py DetPost(layout="cn_obb"), csrc/det_post_obb.hpp).  The cases of tests/detpost_obb_ref.py keep a margin around
the NMS threshold, so the decisions do not depend on the last bits of the device's cosf / sinf / logf / expf; everything else in a
row is computed exactly in float32, and every comparison is bit for bit: a differing byte is a failure."""
import ctypes

import numpy as np
import pytest

import detpost_obb_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
NAMES = ref.NAMES
SMALL = [k for k, n in enumerate(NAMES) if n != "K4096_A4504"]


def _post(c, **over):
    from boxmot_amd.detpost import DetPost
    S, A, nc = c.dims
    o = dict(c.opts, **over)
    return DetPost(S, A, nc, layout="cn_obb", nms=o.pop("nms_mode"), **o)


def _outputs(torch, S, stride):
    return (torch.full((S, stride, 7), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((S,), -77, dtype=torch.int32, device="cuda"))


def _assert_stream(name, s, dets, rows, counters, want):
    w_rows, w_cnt = want
    assert rows[s] == len(w_rows), (name, s, int(rows[s]), len(w_rows))
    assert counters[s].tolist() == w_cnt.tolist(), (name, s)
    assert np.array_equal(dets[s, :rows[s]].view(np.uint32), w_rows.view(np.uint32)), (name, s)
    assert (dets[s, rows[s]:] == np.float32(SENTINEL)).all(), (name, s, "rows beyond the count were written")


def _twice(k):
    """rows as bytes, counts, counters, untouched sentinel rows -- and the same bytes from a second run of the same handle into a
    fresh block, on a side stream: nothing of a call is left in the handle's scratch"""
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
                d_dets, d_rows = _outputs(torch, S, c.stride)
                post.run(pred, c.geos, d_dets, d_rows, hip_stream=st.cuda_stream)
                out = (d_dets.clone(), d_rows.clone())          # queued behind the kernels: no synchronisation by the caller
            counters = post.counters()                          # waits for the run
            st.synchronize()
            dets, rows = out[0].cpu().numpy(), out[1].cpu().numpy()
            for s in range(S):
                _assert_stream(c.name, s, dets, rows, counters, ref.want(k)[s])
            if first is not None:
                assert first[0].tobytes() == dets.tobytes() and first[1].tobytes() == rows.tobytes() and first[2].tobytes() == counters.tobytes()
            first = (dets, rows, counters)
    finally:
        torch.cuda.synchronize()
        post.close()


@pytest.mark.parametrize("k", SMALL, ids=[NAMES[k] for k in SMALL])
def test_each_case_equals_the_reference_twice(k):
    _twice(k)


def test_the_largest_candidate_table():
    """max_candidates = 4096: 137 KB of the workgroup's LDS, and more anchors passing than candidates"""
    k = NAMES.index("K4096_A4504")
    assert ref.want(k)[0][1][:2].tolist() == [4504, 4096]
    _twice(k)


def test_an_unaligned_tensor_takes_the_narrow_score_kernel():
    """one element past a 16-byte boundary the tensor cannot be read 16 bytes at a time: same rows through the other kernel"""
    import torch
    for name in ("clusters_200_fast_A600_float16", "non_finite_angle_A64_float16"):
        k = NAMES.index(name)
        c = ref.CASES[k]
        buf = torch.zeros(c.preds.size + 16, dtype=torch.float16, device="cuda")
        view = buf[1:1 + c.preds.size].view(c.preds.shape)
        view.copy_(torch.from_numpy(c.preds))
        assert view.data_ptr() % 16 == 2 and view.is_contiguous()
        post = _post(c)
        try:
            got = post.run_host(view, c.geos)
            assert got[0].shape[1] == 7 and np.array_equal(got[0].view(np.uint32), ref.want(k)[0][0].view(np.uint32))
            assert post.counters()[0].tolist() == ref.want(k)[0][1].tolist()
        finally:
            post.close()


def test_fewer_streams_than_the_handle_leave_the_others_alone():
    import torch
    k = NAMES.index("three_geometries_unclipped")
    c = ref.CASES[k]
    S = c.dims[0]
    assert S == 3
    post = _post(c)
    try:
        pred = torch.from_numpy(c.preds).cuda()
        d_dets, d_rows = _outputs(torch, S, c.stride)
        post.run(pred, c.geos[:2], d_dets, d_rows, hip_stream=torch.cuda.current_stream().cuda_stream)
        counters = post.counters()
        dets, rows = d_dets.cpu().numpy(), d_rows.cpu().numpy()
        for s in range(2):
            _assert_stream(c.name, s, dets, rows, counters, ref.want(k)[s])
        assert (dets[2] == np.float32(SENTINEL)).all() and rows[2] == -77 and counters[2].tolist() == [0, 0, 0]
    finally:
        torch.cuda.synchronize()
        post.close()


def test_the_comparison_bites():
    """the mode swap: the chain through a handle of the other mode gives the other mode's reference, not its own; and the
    reference that reads the angle from channel 4 differs from the device on the case built for it"""
    import torch
    kg, kf = NAMES.index("chain_greedy"), NAMES.index("chain_fast")
    for k, other, mode in ((kg, kf, "fast"), (kf, kg, "greedy")):
        c = ref.CASES[k]
        post = _post(c, nms_mode=mode)
        try:
            got = post.run_host(torch.from_numpy(c.preds).cuda(), c.geos)[0]
        finally:
            post.close()
        assert np.array_equal(got.view(np.uint32), ref.want(other)[0][0].view(np.uint32)) and len(got) != len(ref.want(k)[0][0])
    k = NAMES.index("angle_in_the_last_row")
    c = ref.CASES[k]
    post = _post(c)
    try:
        got = post.run_host(torch.from_numpy(c.preds).cuda(), c.geos)[0]
    finally:
        post.close()
    bad = ref.want(k, angle_row=4)[0][0]
    assert np.array_equal(got.view(np.uint32), ref.want(k)[0][0].view(np.uint32)) and (got.shape != bad.shape or not np.array_equal(got, bad))


def test_c_abi_errors():
    import torch
    from boxmot_amd import _lib
    lib = _lib.load()
    good = dict(n_streams=2, n_anchors=64, n_classes=3, layout=0, conf_thres=0.25, iou_thres=0.45, max_candidates=64, max_det=8, agnostic=0,
                class_allow=None)

    def create(nms_mode=0, regularize=0, **kw):
        cfg = _lib.DetPostObbConfig(_lib.DetPostConfig(**dict(good, **kw)), nms_mode, regularize)
        return lib.boxmot_hip_detpost_create_obb(ctypes.byref(cfg))
    for kw, word in [(dict(layout=1), "base.layout 0 (cn), got 1"), (dict(layout=2), "got 2"), (dict(nms_mode=2), "nms_mode 2"), (dict(nms_mode=-1), "nms_mode -1"),
                     (dict(n_streams=0), ">= 1"), (dict(max_candidates=5000), "max_candidates"), (dict(max_det=0), "max_det")]:
        assert not create(**kw) and word in _lib.last_error(), (kw, _lib.last_error())
    assert not lib.boxmot_hip_detpost_create_obb(None) and "null" in _lib.last_error()
    h = create(nms_mode=1, regularize=1)
    assert h, _lib.last_error()
    try:
        pred = torch.zeros((2, 8, 64), device="cuda")
        d_dets, d_rows = _outputs(torch, 2, 8)
        geom = np.array([[1.0, 0, 0, 64, 64], [0.5, 0, 0, 64, 64]], dtype=np.float64)

        def call(n=2, p=None, dtype=0, g=geom, stride=8, d=None, r=None):
            ok = lib.boxmot_hip_detpost_run(h, n, ctypes.c_void_p(pred.data_ptr() if p is None else p), dtype, g.ctypes.data_as(_lib.c_double_p),
                                            ctypes.c_void_p(d_dets.data_ptr() if d is None else d), stride,
                                            ctypes.c_void_p(d_rows.data_ptr() if r is None else r), None)
            return ok, _lib.last_error()
        for kw, word in [(dict(n=3), "stream count"), (dict(p=0), "null"), (dict(d=0), "null"), (dict(r=0), "null"), (dict(dtype=2), "dtype"),
                         (dict(stride=7), "out_stride_rows 7 is below max_det 8")]:
            ok, msg = call(**kw)
            assert not ok and word in msg, (kw, msg)
        assert not lib.boxmot_hip_detpost_run(h, 2, ctypes.c_void_p(pred.data_ptr()), 0, None, ctypes.c_void_p(d_dets.data_ptr()), 8,
                                              ctypes.c_void_p(d_rows.data_ptr()), None) and "null" in _lib.last_error()
        torch.cuda.synchronize()
        assert (d_dets == SENTINEL).all() and (d_rows == -77).all()            # none of them wrote
        ok, msg = call()
        assert ok, msg
        torch.cuda.synchronize()
        assert d_rows.tolist() == [0, 0]
    finally:
        lib.boxmot_hip_detpost_destroy(h)


SIZES = [(48, 64), (40, 40), (30, 56)]
PLANTED = [(16, 20, 14, 6, 0.5, 0.9), (46, 24, 6, 16, -0.25, 0.8), (30, 46, 12, 5, 1.25, 0.7)]     # cx, cy, w, h, angle, conf: letterbox pixels of 64 x 64


def _toy_detector(torch, x, t):
    """a synthetic oriented "detector" on the device: whatever the picture, it plants the fixed boxes (drifting and turning with t)
    plus shifted, slightly rotated near-duplicates of lower confidence and sub-threshold clutter into a (S, 4 + 1 + 1, 128) tensor"""
    S = x.shape[0]
    g = torch.Generator(device="cuda").manual_seed(200 + t)
    pred = torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda")
    pred[:, :4] = torch.rand((S, 4, 128), generator=g, device="cuda") * 40 + 8
    pred[:, 4] = torch.rand((S, 128), generator=g, device="cuda") * 0.2                          # clutter below 0.25
    pred[:, 5] = torch.rand((S, 128), generator=g, device="cuda") * 3 - 1.5
    for s in range(S):
        for k, (cx, cy, w, h, ang, cf) in enumerate(PLANTED):
            for d in range(3):                                                                  # the box and two near-duplicates
                a = 5 + 17 * k + 40 * d + s
                pred[s, :, a] = torch.tensor([cx + 0.5 * t + 0.25 * d + 0.5 * s, cy + 0.25 * t, w, h, cf - 0.05 * d, ang + 0.03125 * t + 0.015625 * d],
                                             device="cuda")
    return pred + 0 * x.float().mean()


def test_ring_letterbox_detector_detpost_step_device_end_to_end():
    """FrameRing -> letterbox -> a synthetic oriented detector -> DetPost.run -> MultiStreamBotSort(is_obb=True).step_device for a
    few frames, three streams of different frame sizes: the tracker's rows equal those of a second handle fed through update_batch
    with the reference's rows for the same tensors"""
    import torch
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.ingest import FrameRing
    from boxmot_amd.streams import MultiStreamBotSort
    import letterbox_ref
    S, T, ND = len(SIZES), 4, 16
    frames = [letterbox_ref.make_frame(r, c, "random", 70 + s) for s, (r, c) in enumerate(SIZES)]
    ring = FrameRing(2, S, sizes=SIZES)
    post = DetPost(S, 128, 1, layout="cn_obb", conf=0.25, iou=0.45, max_det=ND, max_candidates=64)
    kw = dict(max_tracks=64, max_dets=ND, emb_dim=1, with_reid=False, is_obb=True)      # (motion only: the step needs no frames)
    dev, host = MultiStreamBotSort(S, **kw), MultiStreamBotSort(S, **kw)
    st = torch.cuda.current_stream()
    try:
        d_dets = torch.zeros((S, ND, 7), dtype=torch.float32, device="cuda")
        d_rows = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((S, ND, 9), dtype=torch.float32, device="cuda")
        d_out_n = torch.zeros(S, dtype=torch.int32, device="cuda")
        total = 0
        for t in range(T):
            for s, f in enumerate(frames):
                ring.host_view(t % 2, s)[...] = np.roll(f, 2 * t, axis=1)
            ring.submit(t % 2)
            x = torch.empty((S, 3, 64, 64), dtype=torch.float16, device="cuda")
            geo = ring.letterbox(t % 2, x, hip_stream=st.cuda_stream)
            pred = _toy_detector(torch, x, t)
            post.run(pred, geo, d_dets, d_rows, hip_stream=st.cuda_stream)
            st.synchronize()                                    # the tracker's own stream starts after the rows are there
            dev.step_device(d_dets.data_ptr(), d_rows.data_ptr(), None, None, 0, 0, d_out.data_ptr(), d_out_n.data_ptr())
            dev.synchronize()
            ring.host_done(t % 2)
            pred_h = pred.cpu().numpy()
            want_dets = []
            for s, g in enumerate(geo):
                found = ref.pairs(pred_h[s], 0.25, 0.45, 64)
                assert found.margin >= ref.MARGIN and found.err32 <= ref.FP32_ERR, (t, s, found.margin, found.err32)
                want_dets.append(ref.detpost_obb(pred_h[s], (g.gain, g.top, g.left, g.rows, g.cols), 0.25, 0.45, ND, 64, found=found)[0])
            assert all(len(w) == 3 for w in want_dets), [len(w) for w in want_dets]              # the planted boxes, not their duplicates
            got_dets, got_n = d_dets.cpu().numpy(), d_rows.cpu().numpy()
            want_rows = host.update_batch(want_dets)
            out, out_n = d_out.cpu().numpy(), d_out_n.cpu().numpy()
            for s in range(S):
                assert got_n[s] == 3 and np.array_equal(got_dets[s, :3].view(np.uint32), want_dets[s].view(np.uint32)), (t, s)
                w = np.asarray(want_rows[s], dtype=np.float32).reshape(-1, 9)
                assert out_n[s] == len(w) and np.array_equal(out[s, :out_n[s]], w), (t, s)
                total += len(w)
        assert total > 0
        assert (dev.status() == 0).all()
    finally:
        torch.cuda.synchronize()
        ring.close(); post.close(); dev.close(); host.close()
