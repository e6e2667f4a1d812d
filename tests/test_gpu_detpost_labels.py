"""GPU tests of the frame-space label map (include/boxmot_hip.h boxmot_hip_detpost_labels, boxmot_amd/detpost.py DetPost.labels,
csrc/det_post_labels.hpp).  Every step is defined in float32 without fused operations, so every comparison is EXACT (bit for bit
against tests/detpost_labels_ref.py): a differing pixel is a failure."""
import ctypes

import numpy as np
import pytest

import detpost_labels_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -21931


def _post(c, n_streams=None):
    from boxmot_amd.detpost import DetPost
    return DetPost(len(c.geos) if n_streams is None else n_streams, 64, 1, layout="cn", extra=c.E, mask=c.mask, in_shape=c.in_shape, max_det=c.max_det,
                   max_candidates=64)


def _inputs(torch, c, protos=None):
    return (torch.from_numpy(c.protos if protos is None else protos).cuda(), torch.from_numpy(c.dets).cuda(), torch.from_numpy(c.n_rows).cuda(),
            torch.from_numpy(c.coefs).cuda())


def _assert_labels(c, want, labels, n_streams=None):
    S = len(c.geos)
    n = S if n_streams is None else n_streams
    for s in range(n):
        rows, cols = want[s].shape
        got = labels[s, :rows, :cols]
        assert got.tobytes() == want[s].tobytes(), (c.name, s, np.argwhere(got != want[s])[:8].tolist())
        rest = labels[s].copy()
        rest[:rows, :cols] = SENTINEL
        assert (rest == SENTINEL).all(), (c.name, s, "a pixel beyond the frame was written")
    for s in range(n, S):
        assert (labels[s] == SENTINEL).all(), (c.name, s, "a stream beyond the call's was written")


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_each_case_equals_the_reference_twice(k):
    """every frame pixel and the sentinels around the frames -- and the same bytes from a second call of the same handle into a
    fresh block, on a side stream"""
    import torch
    c = ref.CASES[k]
    S = len(c.geos)
    post = _post(c)
    st = torch.cuda.Stream()
    try:
        proto, dets, n_rows, coefs = _inputs(torch, c)
        torch.cuda.synchronize()
        first = None
        for rep in range(2):
            with torch.cuda.stream(st):
                d_labels = torch.full((S,) + c.plane, SENTINEL, dtype=torch.int16, device="cuda")
                post.labels(c.geos, proto, dets, n_rows, coefs, d_labels, hip_stream=st.cuda_stream)
            st.synchronize()
            labels = d_labels.cpu().numpy()
            _assert_labels(c, ref.want(k), labels)
            assert first is None or first.tobytes() == labels.tobytes()
            first = labels
    finally:
        torch.cuda.synchronize()
        post.close()


@pytest.mark.parametrize("name", ["three_streams_float16", "three_streams_float32"])
def test_fewer_streams_and_then_swapped_prototypes(name):
    """a call over fewer streams than the handle's leaves the last plane alone; a second call of the same handle with the prototype
    tensors of streams 0 and 1 swapped labels with the new ones"""
    import torch
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    S = len(c.geos)
    post = _post(c)
    try:
        proto, dets, n_rows, coefs = _inputs(torch, c)
        cur = torch.cuda.current_stream().cuda_stream
        d_labels = torch.full((S,) + c.plane, SENTINEL, dtype=torch.int16, device="cuda")
        post.labels(c.geos[:S - 1], proto, dets, n_rows, coefs, d_labels, hip_stream=cur)
        torch.cuda.synchronize()
        _assert_labels(c, ref.want(k), d_labels.cpu().numpy(), n_streams=S - 1)
        swapped = c.protos.copy()
        swapped[0], swapped[1] = c.protos[1], c.protos[0]
        d_labels = torch.full((S,) + c.plane, SENTINEL, dtype=torch.int16, device="cuda")
        post.labels(c.geos, torch.from_numpy(swapped).cuda(), dets, n_rows, coefs, d_labels, hip_stream=cur)
        torch.cuda.synchronize()
        want = [ref.labels_of(c.geos[s], c.dets[s], c.n_rows[s], c.coefs[s], swapped[s], c.mask, c.in_shape, c.max_det) for s in range(S)]
        _assert_labels(c, want, d_labels.cpu().numpy())
        assert any(w.tobytes() != v.tobytes() for w, v in zip(want, ref.want(k)))
    finally:
        torch.cuda.synchronize()
        post.close()


@pytest.mark.parametrize("name", ["three_streams_float16", "table_7x9_frame_24x40_centre_E32_float32", "patch_beyond_the_budget"])
def test_blocks_off_16_byte_alignment_give_the_same_bytes(name):
    """prototypes and labels that start one element into their allocations, and rows, counts and coefficients one float in; the
    element before the labels stays"""
    import torch
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    S = len(c.geos)
    post = _post(c)
    try:
        def shifted(a):
            t = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
            t[1:] = torch.from_numpy(a).cuda().reshape(-1)
            return t[1:].view(a.shape)
        proto, dets, n_rows, coefs = shifted(c.protos), shifted(c.dets), shifted(c.n_rows), shifted(c.coefs)
        block = torch.full((1 + S * c.plane[0] * c.plane[1],), SENTINEL, dtype=torch.int16, device="cuda")
        d_labels = block[1:].view((S,) + c.plane)
        assert d_labels.data_ptr() % 16 == 2 and proto.data_ptr() % 16 == c.protos.itemsize and dets.data_ptr() % 16 == 4
        post.labels(c.geos, proto, dets, n_rows, coefs, d_labels, hip_stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _assert_labels(c, ref.want(k), d_labels.cpu().numpy())
        assert int(block[0]) == SENTINEL
    finally:
        torch.cuda.synchronize()
        post.close()


def test_the_comparison_bites():
    """a wrong-reference control: the pixel-corner convention (no + 0.5) fails the device output, as do last-wins and <= at the right edge"""
    import torch
    for wrong, name in (("corner", "table_8x8_frame_24x40_centre_E32_float16"), ("last_wins", "first_wins_three"), ("inclusive_edge", "edges_on_integers")):
        k = ref.NAMES.index(name)
        c = ref.CASES[k]
        post = _post(c)
        try:
            d_labels = torch.full((1,) + c.plane, SENTINEL, dtype=torch.int16, device="cuda")
            post.labels(c.geos, *_inputs(torch, c), d_labels, hip_stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = d_labels.cpu().numpy()[0]
        finally:
            post.close()
        assert got.tobytes() == ref.want(k)[0].tobytes()
        assert got.tobytes() != ref.want(k, **{wrong: True})[0].tobytes(), wrong


def test_handles_without_labels_give_the_bytes_they_gave():
    """regression guard: a mask handle's run equals tests/detpost_mask_ref.py in all five blocks before and after a labels call on the
    same handle (which shares its geometry table and its wait chain), and an extras handle's run equals tests/detpost_extra_ref.py"""
    import torch
    import detpost_extra_ref as eref
    import detpost_mask_ref as mref
    from boxmot_amd.detpost import DetPost
    for name in ("table_8x8_cn_E32_pred_float16_proto_float16", "encoding_prototypes_nc_obj"):
        k = mref.NAMES.index(name)
        c = mref.CASES[k]
        S, A = c.dims
        post = DetPost(S, A, c.nc, layout=c.layout, extra=c.E, mask=c.mask, in_shape=c.in_shape, **c.opts)
        try:
            pred, proto = torch.from_numpy(c.preds).cuda(), torch.from_numpy(c.protos).cuda()
            cur = torch.cuda.current_stream().cuda_stream
            for rep in range(2):
                d_dets = torch.full((S, c.stride, 6), -12345.5, dtype=torch.float32, device="cuda")
                d_rows = torch.full((S,), -77, dtype=torch.int32, device="cuda")
                d_extra = torch.full((S, c.stride, c.E), -12345.5, dtype=torch.float32, device="cuda")
                d_src = torch.full((S, c.stride), -99, dtype=torch.int32, device="cuda")
                d_masks = torch.full((S, c.stride) + c.mask, 0xA5, dtype=torch.uint8, device="cuda")
                post.run(pred, c.geos, d_dets, d_rows, hip_stream=cur, d_extra=d_extra, d_src=d_src, d_proto=proto, d_masks=d_masks)
                counters = post.counters()
                dets, rows, extra, src, masks = (t.cpu().numpy() for t in (d_dets, d_rows, d_extra, d_src, d_masks))
                for s in range(S):
                    w_rows, w_cnt, w_extra, w_src, w_masks = mref.want(k)[s]
                    n = len(w_rows)
                    assert rows[s] == n and counters[s].tolist() == w_cnt.tolist(), (name, rep, s)
                    assert dets[s, :n].tobytes() == w_rows.tobytes() and extra[s, :n].tobytes() == w_extra.tobytes() and np.array_equal(src[s, :n], w_src)
                    assert masks[s, :n].tobytes() == w_masks.tobytes() and (masks[s, n:] == 0xA5).all() and (dets[s, n:] == np.float32(-12345.5)).all()
                if rep == 0:        # a labels call in between, with geometries of its own: the next run brings the table back
                    geo = [(0.5, 1.0, 2.0, 20.0, 30.0)] * S
                    d_labels = torch.full((S, 20, 30), SENTINEL, dtype=torch.int16, device="cuda")
                    post.labels(geo, proto, d_dets, d_rows, d_extra, d_labels, hip_stream=cur)
                    torch.cuda.synchronize()
                    lab = d_labels.cpu().numpy()
                    for s in range(S):
                        assert lab[s].tobytes() == ref.labels_of(geo[s], dets[s], rows[s], extra[s], c.protos[s], c.mask, c.in_shape, c.opts["max_det"]).tobytes()
        finally:
            torch.cuda.synchronize()
            post.close()
    k = eref.NAMES.index("raw_encodes_stream_anchor_channel_nc_obj")
    c = eref.CASES[k]
    S, A = c.dims
    post = DetPost(S, A, c.nc, layout=c.layout, extra=c.E, extra_kind=c.kind, **c.opts)
    try:
        got = post.run_host(torch.from_numpy(c.preds).cuda(), c.geos)
        for (g_rows, g_extra, g_src), (w_rows, _, w_extra, w_src) in zip(got, eref.want(k)):
            assert g_rows.tobytes() == w_rows.tobytes() and g_extra.tobytes() == w_extra.tobytes() and np.array_equal(g_src, w_src)
        with pytest.raises(ValueError, match="mask handle"):
            post.labels(c.geos, None, None, None, None, None)
    finally:
        post.close()


def test_c_abi_refusals():
    import torch
    from boxmot_amd import _lib
    lib = _lib.load()

    def base(max_det=8):
        return _lib.DetPostConfig(n_streams=2, n_anchors=64, n_classes=3, layout=0, conf_thres=0.25, iou_thres=0.45, max_candidates=64, max_det=max_det, agnostic=0,
                                  class_allow=None)

    def mask_handle(n_tiles=0, max_det=8):
        cfg = _lib.DetPostMaskConfig(_lib.DetPostExtraConfig(base(max_det), n_tiles, 0, 4, 0), 8, 12, 32, 48)
        h = lib.boxmot_hip_detpost_create_mask(ctypes.byref(cfg))
        assert h, _lib.last_error()
        return h

    h, ht, hbig = mask_handle(), mask_handle(n_tiles=2), mask_handle(max_det=32768)
    ecfg = _lib.DetPostExtraConfig(base(), 0, 0, 4, 0)
    extras = lib.boxmot_hip_detpost_create_extra(ctypes.byref(ecfg))
    assert extras, _lib.last_error()
    bcfg = base()
    plain = lib.boxmot_hip_detpost_create(ctypes.byref(bcfg))
    assert plain, _lib.last_error()
    try:
        proto = torch.ones((2, 4, 8, 12), device="cuda")
        d_dets = torch.zeros((2, 8, 6), device="cuda")
        d_dets[:, 0, :4] = torch.tensor([2.0, 3.0, 20.0, 17.0], device="cuda")
        d_rows = torch.ones(2, dtype=torch.int32, device="cuda")
        d_extra = torch.ones((2, 8, 4), device="cuda")
        d_labels = torch.full((2, 24, 40), SENTINEL, dtype=torch.int16, device="cuda")
        geom = np.array([[1.0, 0, 0, 24, 40], [0.5, 0, 0, 20, 38]], dtype=np.float64)

        def call(handle=h, n=2, g=geom, pro=proto.data_ptr(), pdtype=0, dets=d_dets.data_ptr(), stride=8, rows=d_rows.data_ptr(), extra=d_extra.data_ptr(),
                 labels=d_labels.data_ptr(), lr=24, lc=40):
            ok = lib.boxmot_hip_detpost_labels(handle, n, None if g is None else g.ctypes.data_as(_lib.c_double_p), ctypes.c_void_p(pro), pdtype, ctypes.c_void_p(dets),
                                               stride, ctypes.c_void_p(rows), ctypes.c_void_p(extra), ctypes.c_void_p(labels), lr, lc, None)
            return ok, _lib.last_error()
        swapped = geom[::-1].copy()
        for kw, word in [(dict(handle=plain), "boxmot_hip_detpost_create_mask"), (dict(handle=extras), "boxmot_hip_detpost_create_mask"),
                         (dict(handle=ht), "tiled handles are out of scope"), (dict(handle=hbig, stride=32768), "max_det 32768 exceeds 32767"), (dict(handle=None), "null"),
                         (dict(n=0), "stream count"), (dict(n=3), "stream count"), (dict(g=None), "null detpost geom"), (dict(pro=0), "null detpost d_proto"),
                         (dict(dets=0), "null detpost d_dets"), (dict(rows=0), "null detpost d_det_rows"), (dict(extra=0), "null detpost d_extra"),
                         (dict(labels=0), "null detpost d_labels"), (dict(pdtype=2), "proto_dtype"), (dict(pro=proto.data_ptr() + 2), "aligned"),
                         (dict(labels=d_labels.data_ptr() + 1), "aligned"), (dict(stride=7), "max_det"), (dict(lr=0), "label_rows"),
                         (dict(lr=23), "stream 0: the frame of 24 x 40 does not fit label planes of 23 x 40"), (dict(lc=39), "stream 0: the frame of 24 x 40"),
                         (dict(g=swapped, lr=23), "stream 1: the frame of 24 x 40"), (dict(g=np.array([[0.0, 0, 0, 24, 40]] * 2)), "gain > 0")]:
            ok, msg = call(**kw)
            assert not ok and word in msg, (kw, msg)
        torch.cuda.synchronize()
        assert (d_labels == SENTINEL).all()                             # none of them wrote
        ok, msg = call()
        assert ok, msg
        proto16 = torch.ones((2, 4, 8, 12), dtype=torch.float16, device="cuda")
        ok, msg = call(pdtype=1, pro=proto16.data_ptr())
        assert ok, msg
        torch.cuda.synchronize()
        lab = d_labels.cpu().numpy()
        assert (lab[0, 3:17, 2:20] == 0).all() and (lab[0] == 0).sum() == 14 * 18 and (lab[0] == -1).sum() == 24 * 40 - 14 * 18
        assert (lab[1, 3:17, 2:20] == 0).all() and (lab[1, :20, :38] == 0).sum() == 14 * 18 and (lab[1, 20:] == SENTINEL).all() and (lab[1, :, 38:] == SENTINEL).all()
    finally:
        torch.cuda.synchronize()
        for x in (h, ht, hbig, extras, plain):
            lib.boxmot_hip_detpost_destroy(x)


def test_labels_host_returns_rows_extras_src_and_labels():
    """run + labels through the convenience form on a planted head: the labels equal the reference run on the rows it returned"""
    import torch
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.ingest import letterbox_geometry
    rng = np.random.default_rng(5)
    geo = [letterbox_geometry(45, 80, (32, 48)), letterbox_geometry(30, 40, (32, 48))]
    pred = np.zeros((2, 4 + 1 + 5, 64), dtype=np.float32)
    pred[:, :4] = rng.uniform(4, 12, (2, 4, 64))
    pred[:, 4] = rng.uniform(0, 0.2, (2, 64))
    for s in range(2):
        for b in range(3):
            pred[s, :, 5 + 9 * b + s] = [10 + 12 * b, 14 + 3 * b, 16, 14, 0.9 - 0.1 * b] + ref.vals(rng, (5,)).tolist()
    proto = ref.vals(rng, (2, 5, 8, 12)).astype(np.float16)
    post = DetPost(2, 64, 1, layout="cn", extra=5, mask=(8, 12), in_shape=(32, 48), max_det=8, max_candidates=64)
    try:
        got = post.labels_host(pred, geo, proto)
    finally:
        post.close()
    assert len(got) == 2
    for s, (rows, extras, src, labels) in enumerate(got):
        g = geo[s]
        assert len(rows) == 3 and labels.dtype == np.int16 and labels.shape == (g.rows, g.cols)
        want = ref.labels_of((g.gain, g.top, g.left, g.rows, g.cols), rows, len(rows), extras, proto[s], (8, 12), (32, 48), 8)
        assert labels.tobytes() == want.tobytes() and len(np.unique(labels)) >= 3


def test_seg_head_labels_step_device_end_to_end():
    """a synthetic segmentation head -> DetPost(mask=...).run -> labels -> MultiStreamBotSort.step_device for three frames of six
    overlapping, slightly moving boxes per stream: the per-pixel track-id map built on the device through det_ind -- lut[d_out[:, 7]] =
    d_out[:, 4]; lut[labels] -- equals the map made from the reference's labels of the emitted rows and a host tracker's update_batch rows"""
    import torch
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.ingest import letterbox_geometry
    from boxmot_amd.streams import MultiStreamBotSort
    S, A, ND, NB, E, FRAMES, MASK, IN, FRAME = 2, 128, 16, 6, 8, 3, (16, 24), (64, 96), (90, 120)
    geo = [letterbox_geometry(FRAME[0], FRAME[1], IN)] * S
    g5 = [(g.gain, g.top, g.left, g.rows, g.cols) for g in geo]
    post = DetPost(S, A, 1, layout="cn", extra=E, mask=MASK, in_shape=IN, conf=0.25, iou=0.45, max_det=ND, max_candidates=64)
    dev = MultiStreamBotSort(S, max_tracks=64, max_dets=ND, emb_dim=1, with_reid=False)
    host = MultiStreamBotSort(S, max_tracks=64, max_dets=ND, emb_dim=1, with_reid=False)
    st = torch.cuda.current_stream()
    rng = np.random.default_rng(11)
    proto = ref.vals(rng, (S, E) + MASK).astype(np.float16)
    coef = ref.vals(rng, (S, NB, E))
    try:
        d_dets = torch.zeros((S, ND, 6), dtype=torch.float32, device="cuda")
        d_rows = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_coef = torch.zeros((S, ND, E), dtype=torch.float32, device="cuda")
        d_masks = torch.zeros((S, ND) + MASK, dtype=torch.uint8, device="cuda")
        d_labels = torch.full((S,) + FRAME, SENTINEL, dtype=torch.int16, device="cuda")
        d_out = torch.zeros((S, ND, 8), dtype=torch.float32, device="cuda")
        d_out_n = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_proto = torch.from_numpy(proto).cuda()
        owned = 0
        for t in range(FRAMES):
            pred = np.zeros((S, 4 + 1 + E, A), dtype=np.float32)
            pred[:, :4] = rng.uniform(2, 6, (S, 4, A))
            pred[:, 4] = rng.uniform(0, 0.2, (S, A))                                            # clutter below the threshold
            for s in range(S):
                for b in range(NB):                                                             # a 3 x 2 grid of 34 x 30 boxes 26 / 22 apart: neighbours overlap
                    a = (7 + 13 * b + 5 * t + s) % A
                    pred[s, :, a] = [22 + 26 * (b % 3) + t + s, 20 + 22 * (b // 3) + t, 34, 30, 0.9 - 0.05 * b] + coef[s, b].tolist()
            post.run(torch.from_numpy(pred).cuda(), geo, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_coef, d_proto=d_proto, d_masks=d_masks)
            post.labels(geo, d_proto, d_dets, d_rows, d_coef, d_labels, hip_stream=st.cuda_stream)
            st.synchronize()                                    # the tracker's own stream starts after the rows are there
            dev.step_device(d_dets.data_ptr(), d_rows.data_ptr(), None, None, 0, 0, d_out.data_ptr(), d_out_n.data_ptr())
            dev.synchronize()
            dets, rows, extras = d_dets.cpu().numpy(), d_rows.cpu().numpy(), d_coef.cpu().numpy()
            assert rows.tolist() == [NB] * S
            want_rows = host.update_batch([dets[s, :rows[s]] for s in range(S)])
            for s in range(S):
                n = int(d_out_n[s])
                lut = torch.full((ND + 1,), -1.0, device="cuda")                                 # (index -1, "no row", is the last entry)
                lut[d_out[s, :n, 7].long()] = d_out[s, :n, 4]
                got = lut[d_labels[s].long()].cpu().numpy()
                w = np.asarray(want_rows[s], dtype=np.float32).reshape(-1, 8)
                want_labels = ref.labels_of(g5[s], dets[s], rows[s], extras[s], proto[s], MASK, IN, ND)
                want_lut = np.full(ND + 1, -1.0, dtype=np.float32)
                want_lut[w[:, 7].astype(np.int64)] = w[:, 4]
                assert len(w) == n and np.array_equal(got, want_lut[want_labels]), (t, s)
                assert len(np.unique(want_labels)) >= 4                                          # (several rows own pixels)
                owned += int((got >= 0).sum())
        assert owned > 1000 and (dev.status() == 0).all()
    finally:
        torch.cuda.synchronize()
        post.close(); dev.close(); host.close()
