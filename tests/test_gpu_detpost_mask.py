"""GPU tests of the device mask decoding (include/boxmot_hip.h boxmot_hip_detpost_create_mask / _run_mask, boxmot_amd/detpost.py
DetPost(mask=...), csrc/det_post_mask.hpp).  Every step is defined in float32 without fused operations, so every comparison is EXACT
(bit for bit against tests/detpost_mask_ref.py): a differing byte is a failure."""
import ctypes

import numpy as np
import pytest

import detpost_extra_ref
import detpost_mask_ref as ref
import detpost_ref

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
SRC_SENTINEL = -99
MASK_SENTINEL = 0xA5


def _post(c, **over):
    from boxmot_amd.detpost import DetPost
    S, A = c.dims
    o = dict(c.opts, **over)
    return DetPost(S, A, c.nc, layout=c.layout, extra=c.E, mask=c.mask, in_shape=c.in_shape, tiles=c.tiles or None, **o)


def _outputs(torch, S, stride, E, mask):
    return (torch.full((S, stride, 6), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((S,), -77, dtype=torch.int32, device="cuda"),
            torch.full((S, stride, E), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((S, stride), SRC_SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((S, stride) + tuple(mask), MASK_SENTINEL, dtype=torch.uint8, device="cuda"))


def _assert_stream(name, s, dets, rows, counters, extra, src, masks, want, with_src=True):
    w_rows, w_cnt, w_extra, w_src, w_masks = want
    k = len(w_rows)
    assert rows[s] == k, (name, s, int(rows[s]), k)
    assert counters[s].tolist() == w_cnt.tolist(), (name, s)
    assert np.array_equal(dets[s, :k].view(np.uint32), w_rows.view(np.uint32)), (name, s)
    assert np.array_equal(extra[s, :k].view(np.uint32), w_extra.view(np.uint32)), (name, s, "extras")
    assert masks[s, :k].tobytes() == w_masks.tobytes(), (name, s, "masks", np.argwhere(masks[s, :k] != w_masks)[:8].tolist())
    assert (dets[s, k:] == np.float32(SENTINEL)).all() and (extra[s, k:] == np.float32(SENTINEL)).all() and (masks[s, k:] == MASK_SENTINEL).all(), \
        (name, s, "rows beyond the count were written")
    if with_src:
        assert np.array_equal(src[s, :k], w_src) and (src[s, k:] == SRC_SENTINEL).all(), (name, s, "src")
    else:
        assert (src[s] == SRC_SENTINEL).all(), (name, s)


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.NAMES)
def test_each_case_equals_the_reference_twice(k):
    """rows, extras, source anchors and masks as bytes, counts, counters, untouched sentinel rows in all five blocks -- and the same
    bytes from a second run of the same handle into fresh blocks, on a side stream, this time without a src block"""
    import torch
    c = ref.CASES[k]
    S = c.dims[0]
    pred, proto = torch.from_numpy(c.preds).cuda(), torch.from_numpy(c.protos).cuda()
    post = _post(c)
    st = torch.cuda.Stream()
    try:
        first = None
        for rep in range(2):
            with torch.cuda.stream(st):
                d_dets, d_rows, d_extra, d_src, d_masks = _outputs(torch, S, c.stride, c.E, c.mask)
                post.run(pred, c.geos, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_extra, d_src=d_src if rep == 0 else None, d_proto=proto, d_masks=d_masks)
                out = (d_dets.clone(), d_rows.clone(), d_extra.clone(), d_src.clone(), d_masks.clone())        # queued behind the kernels
            counters = post.counters()                                                                          # waits for the run
            st.synchronize()
            dets, rows, extra, src, masks = (t.cpu().numpy() for t in out)
            for s in range(S):
                _assert_stream(c.name, s, dets, rows, counters, extra, src, masks, ref.want(k)[s], with_src=rep == 0)
            if first is not None:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(first, (dets, rows, extra, masks, counters)))
            first = (dets, rows, extra, masks, counters)
    finally:
        torch.cuda.synchronize()
        post.close()


@pytest.mark.parametrize("name", ["table_12x20_cn_E32_pred_float32_proto_float16", "tiled_T2_ios"])
def test_fewer_streams_and_then_swapped_prototypes(name):
    """a call over fewer streams than the handle's leaves the last stream alone in all five blocks; a second run of the same handle
    with the prototype tensors of streams 0 and 1 swapped decodes with the new ones"""
    import torch
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    (S, A), T = c.dims, c.tiles or 1
    post = _post(c)
    try:
        pred, proto = torch.from_numpy(c.preds).cuda(), torch.from_numpy(c.protos).cuda()
        d_dets, d_rows, d_extra, d_src, d_masks = _outputs(torch, S, c.stride, c.E, c.mask)
        cur = torch.cuda.current_stream().cuda_stream
        post.run(pred, c.geos[:S - 1], d_dets, d_rows, hip_stream=cur, d_extra=d_extra, d_src=d_src, d_proto=proto, d_masks=d_masks)
        counters = post.counters()
        dets, rows, extra, src, masks = (t.cpu().numpy() for t in (d_dets, d_rows, d_extra, d_src, d_masks))
        for s in range(S - 1):
            _assert_stream(c.name, s, dets, rows, counters, extra, src, masks, ref.want(k)[s])
        assert (dets[S - 1] == np.float32(SENTINEL)).all() and rows[S - 1] == -77 and (extra[S - 1] == np.float32(SENTINEL)).all() and \
            (src[S - 1] == SRC_SENTINEL).all() and (masks[S - 1] == MASK_SENTINEL).all() and counters[S - 1].tolist() == [0, 0, 0]
        swapped = c.protos.copy()
        swapped[:T], swapped[T:2 * T] = c.protos[T:2 * T], c.protos[:T]
        d_dets, d_rows, d_extra, d_src, d_masks = _outputs(torch, S, c.stride, c.E, c.mask)
        post.run(pred, c.geos, d_dets, d_rows, hip_stream=cur, d_extra=d_extra, d_src=d_src, d_proto=torch.from_numpy(swapped).cuda(), d_masks=d_masks)
        counters = post.counters()
        dets, rows, extra, src, masks = (t.cpu().numpy() for t in (d_dets, d_rows, d_extra, d_src, d_masks))
        changed = False
        for s in range(S):
            w = ref.want(k)[s]
            w_masks = ref.step9(c.preds[s * T:(s + 1) * T], swapped[s * T:(s + 1) * T], c.layout, A, w[0], w[2], w[3], c.mask, c.in_shape, bool(c.tiles))
            _assert_stream(c.name, s, dets, rows, counters, extra, src, masks, w[:4] + (w_masks,))
            changed = changed or w_masks.tobytes() != w[4].tobytes()
        assert changed
    finally:
        torch.cuda.synchronize()
        post.close()


@pytest.mark.parametrize("name", ["table_8x8_cn_E32_pred_float16_proto_float16", "table_40x72_nc_obj_E32_pred_float32_proto_float32", "tiled_T2_iou"])
def test_blocks_off_the_wide_alignment_give_the_same_bytes(name):
    """prototypes that start one element, and masks that start one byte, into their allocations: the launch takes the byte path for
    a width that is a multiple of 4, and the byte before the masks stays"""
    import torch
    k = ref.NAMES.index(name)
    c = ref.CASES[k]
    S = c.dims[0]
    post = _post(c)
    try:
        pred = torch.from_numpy(c.preds).cuda()
        proto = torch.zeros(c.protos.size + 1, dtype=torch.from_numpy(c.protos).dtype, device="cuda")
        proto[1:] = torch.from_numpy(c.protos).cuda().reshape(-1)
        d_dets, d_rows, d_extra, d_src, _ = _outputs(torch, S, c.stride, c.E, c.mask)
        block = torch.full((1 + S * c.stride * c.mask[0] * c.mask[1],), MASK_SENTINEL, dtype=torch.uint8, device="cuda")
        d_masks = block[1:].view((S, c.stride) + c.mask)
        assert d_masks.data_ptr() % 4 == 1 and proto[1:].data_ptr() % (4 * c.protos.itemsize) != 0
        post.run(pred, c.geos, d_dets, d_rows, hip_stream=torch.cuda.current_stream().cuda_stream, d_extra=d_extra, d_src=d_src,
                 d_proto=proto[1:].view(c.protos.shape), d_masks=d_masks)
        counters = post.counters()
        dets, rows, extra, src, masks = (t.cpu().numpy() for t in (d_dets, d_rows, d_extra, d_src, d_masks))
        for s in range(S):
            _assert_stream(c.name, s, dets, rows, counters, extra, src, masks, ref.want(k)[s])
        assert int(block[0]) == MASK_SENTINEL
    finally:
        torch.cuda.synchronize()
        post.close()


def test_run_host_returns_rows_extras_src_and_masks():
    k = ref.NAMES.index("encoding_prototypes_nc_obj")
    c = ref.CASES[k]
    post = _post(c)
    try:
        got = post.run_host(c.preds, c.geos, c.protos)
        with pytest.raises(ValueError, match="needs proto"):
            post.run_host(c.preds, c.geos)
    finally:
        post.close()
    assert len(got) == 3
    for (rows, extras, src, masks), (w_rows, _, w_extras, w_src, w_masks) in zip(got, ref.want(k)):
        assert np.array_equal(rows.view(np.uint32), w_rows.view(np.uint32)) and np.array_equal(extras.view(np.uint32), w_extras.view(np.uint32))
        assert src.dtype == np.int32 and np.array_equal(src, w_src)
        assert masks.dtype == np.uint8 and masks.shape == w_masks.shape and masks.tobytes() == w_masks.tobytes()


WRONG_ON = {"descending_k": "order_of_the_chain", "float64_acc": "order_of_the_chain", "inclusive_edge": "window_edges_on_integers",
            "frame_box": "table_8x8_cn_E3_pred_float32_proto_float16", "tile0_protos": "tiled_T2_iou", "ge_zero": "special_logits_proto_float32"}


def test_the_comparison_bites():
    """wrong-reference controls: each differs from the device on the case built for it"""
    import torch
    got = {}
    for wrong, name in WRONG_ON.items():
        k = ref.NAMES.index(name)
        c = ref.CASES[k]
        if name not in got:
            post = _post(c)
            try:
                got[name] = post.run_host(torch.from_numpy(c.preds).cuda(), c.geos, torch.from_numpy(c.protos).cuda())
            finally:
                post.close()
        masks = [g[3] for g in got[name]]
        assert all(m.tobytes() == w[4].tobytes() for m, w in zip(masks, ref.want(k)))
        assert any(m.tobytes() != w[4].tobytes() for m, w in zip(masks, ref.want(k, **{wrong: True}))), wrong


def test_handles_without_masks_give_the_bytes_they_gave():
    """regression guard: three untiled cases and a tiled one of tests/detpost_extra_ref.py through plain extras handles equal their
    references, sentinels included, and run_host still returns 3-tuples"""
    import torch
    from boxmot_amd.detpost import DetPost
    eref = detpost_extra_ref
    for name in ("table_A96_nc1_cn_float16_E1_raw", "raw_encodes_stream_anchor_channel_nc_obj", "survivors_cross_a_chunk", "tiled_ios_nc_obj_float16"):
        k = eref.NAMES.index(name)
        c = eref.CASES[k]
        S, A = c.dims
        post = DetPost(S, A, c.nc, layout=c.layout, extra=c.E, extra_kind=c.kind, tiles=c.tiles or None, **c.opts)
        try:
            assert post.mask is None
            pred = torch.from_numpy(c.preds).cuda()
            d_dets = torch.full((S, c.stride, 6), SENTINEL, dtype=torch.float32, device="cuda")
            d_rows = torch.full((S,), -77, dtype=torch.int32, device="cuda")
            d_extra = torch.full((S, c.stride, c.E), SENTINEL, dtype=torch.float32, device="cuda")
            d_src = torch.full((S, c.stride), SRC_SENTINEL, dtype=torch.int32, device="cuda")
            post.run(pred, c.geos, d_dets, d_rows, hip_stream=torch.cuda.current_stream().cuda_stream, d_extra=d_extra, d_src=d_src)
            counters = post.counters()
            dets, rows, extra, src = (t.cpu().numpy() for t in (d_dets, d_rows, d_extra, d_src))
            for s in range(S):
                w_rows, w_cnt, w_extra, w_src = eref.want(k)[s]
                n = len(w_rows)
                assert rows[s] == n and counters[s].tolist() == w_cnt.tolist(), (name, s)
                assert np.array_equal(dets[s, :n].view(np.uint32), w_rows.view(np.uint32)) and np.array_equal(extra[s, :n].view(np.uint32), w_extra.view(np.uint32))
                assert np.array_equal(src[s, :n], w_src), (name, s)
                assert (dets[s, n:] == np.float32(SENTINEL)).all() and (extra[s, n:] == np.float32(SENTINEL)).all() and (src[s, n:] == SRC_SENTINEL).all()
            got = post.run_host(pred, c.geos)
            assert all(isinstance(g, tuple) and len(g) == 3 for g in got)
            for (g_rows, g_extra, g_src), (w_rows, _, w_extra, w_src) in zip(got, eref.want(k)):
                assert g_rows.tobytes() == w_rows.tobytes() and g_extra.tobytes() == w_extra.tobytes() and np.array_equal(g_src, w_src)
            with pytest.raises(ValueError, match="mask="):
                post.run(pred, c.geos, d_dets, d_rows, d_extra=d_extra, d_masks=torch.zeros((S, c.stride, 8, 8), dtype=torch.uint8, device="cuda"))
        finally:
            torch.cuda.synchronize()
            post.close()


def test_c_abi_refusals():
    import torch
    from boxmot_amd import _lib
    lib = _lib.load()
    base = _lib.DetPostConfig(n_streams=2, n_anchors=64, n_classes=3, layout=0, conf_thres=0.25, iou_thres=0.45, max_candidates=64, max_det=8, agnostic=0,
                              class_allow=None)

    def config(n_tiles=0, merge=0, n_extra=4, extra_kind=0, mask_h=8, mask_w=12, in_h=32, in_w=48):
        return _lib.DetPostMaskConfig(_lib.DetPostExtraConfig(base, n_tiles, merge, n_extra, extra_kind), mask_h, mask_w, in_h, in_w)

    for kw, word in [(dict(extra_kind=1), "extra_kind"), (dict(extra_kind=2, n_extra=6), "extra_kind"), (dict(n_extra=0), "n_extra"), (dict(n_extra=257), "n_extra"),
                     (dict(mask_h=0), "mask_h"), (dict(mask_h=1025), "mask_h"), (dict(mask_w=0), "mask_w"), (dict(mask_w=1025), "mask_w"), (dict(in_h=0), "in_h"),
                     (dict(in_w=-1), "in_w"), (dict(n_tiles=65), "n_tiles")]:
        cfg = config(**kw)
        assert not lib.boxmot_hip_detpost_create_mask(ctypes.byref(cfg)) and word in _lib.last_error(), (kw, _lib.last_error())
    assert not lib.boxmot_hip_detpost_create_mask(None) and "null" in _lib.last_error()
    cfg, tcfg = config(), config(n_tiles=2)
    h = lib.boxmot_hip_detpost_create_mask(ctypes.byref(cfg))
    assert h, _lib.last_error()
    ht = lib.boxmot_hip_detpost_create_mask(ctypes.byref(tcfg))
    assert ht, _lib.last_error()
    ecfg = _lib.DetPostExtraConfig(base, 0, 0, 4, 0)
    extras = lib.boxmot_hip_detpost_create_extra(ctypes.byref(ecfg))
    assert extras, _lib.last_error()
    plain = lib.boxmot_hip_detpost_create(ctypes.byref(base))
    assert plain, _lib.last_error()
    try:
        pred = torch.zeros((4, 11, 64), device="cuda")
        proto = torch.zeros((4, 4, 8, 12), device="cuda")
        d_dets, d_rows, d_extra, d_src, d_masks = _outputs(torch, 2, 8, 4, (8, 12))
        geom = np.array([[1.0, 0, 0, 64, 64], [0.5, 0, 0, 64, 64]], dtype=np.float64)
        tgeom = np.array([[[1.0, 0, 0, 0, 0, 64, 64]] * 2] * 2, dtype=np.float64)
        P = lambda t: ctypes.c_void_p(t.data_ptr())

        def call(handle=h, n=2, dtype=0, g=geom, stride=8, extra=d_extra.data_ptr(), src=d_src.data_ptr(), pro=proto.data_ptr(), pdtype=0, masks=d_masks.data_ptr()):
            ok = lib.boxmot_hip_detpost_run_mask(handle, n, P(pred), dtype, g.ctypes.data_as(_lib.c_double_p), P(d_dets), stride, P(d_rows), ctypes.c_void_p(extra),
                                                 ctypes.c_void_p(src), ctypes.c_void_p(pro), pdtype, ctypes.c_void_p(masks), None)
            return ok, _lib.last_error()
        for kw, word in [(dict(n=0), "stream count"), (dict(n=3), "stream count"), (dict(dtype=2), "dtype"), (dict(stride=7), "max_det"), (dict(extra=0), "d_extra"),
                         (dict(pro=0), "d_proto"), (dict(masks=0), "d_masks"), (dict(pro=proto.data_ptr() + 2), "d_proto"), (dict(pro=proto.data_ptr() + 1, pdtype=1), "d_proto"),
                         (dict(pdtype=2), "proto_dtype"), (dict(pdtype=-1), "proto_dtype"), (dict(handle=plain), "boxmot_hip_detpost_create_mask"),
                         (dict(handle=extras), "boxmot_hip_detpost_create_mask"), (dict(handle=None), "null")]:
            ok, msg = call(**kw)
            assert not ok and word in msg, (kw, msg)
        # a mask handle through the three older entry points, tiled or not: refused, naming the right one
        for entry, handle, g in ((lib.boxmot_hip_detpost_run, h, geom), (lib.boxmot_hip_detpost_run_tiled, ht, tgeom), (lib.boxmot_hip_detpost_run, ht, geom),
                                 (lib.boxmot_hip_detpost_run_tiled, h, tgeom)):
            assert not entry(handle, 2, P(pred), 0, g.ctypes.data_as(_lib.c_double_p), P(d_dets), 8, P(d_rows), None)
            assert "boxmot_hip_detpost_run_mask" in _lib.last_error(), _lib.last_error()
        for handle, g in ((h, geom), (ht, tgeom)):
            assert not lib.boxmot_hip_detpost_run_extra(handle, 2, P(pred), 0, g.ctypes.data_as(_lib.c_double_p), P(d_dets), 8, P(d_rows), P(d_extra), P(d_src), None)
            assert "boxmot_hip_detpost_run_mask" in _lib.last_error(), _lib.last_error()
        torch.cuda.synchronize()
        assert (d_dets == SENTINEL).all() and (d_rows == -77).all() and (d_extra == SENTINEL).all() and (d_src == SRC_SENTINEL).all() and \
            (d_masks == MASK_SENTINEL).all()                            # none of them wrote
        for handle, g in ((h, geom), (ht, tgeom)):
            for kw in (dict(), dict(src=0), dict(pro=proto.data_ptr() + 4), dict(pdtype=1)):           # d_src may be null; fp32 prototypes need 4-byte alignment only
                ok, msg = call(handle=handle, g=g, **kw)
                assert ok, (kw, msg)
        torch.cuda.synchronize()
        assert d_rows.tolist() == [0, 0] and (d_extra == SENTINEL).all() and (d_src == SRC_SENTINEL).all() and (d_masks == MASK_SENTINEL).all()
        counters = np.zeros((2, 3), dtype=np.int32)
        assert lib.boxmot_hip_detpost_counters(h, counters.ctypes.data, 2) and counters.tolist() == [[0, 0, 0]] * 2
    finally:
        torch.cuda.synchronize()
        for x in (h, ht, extras, plain):
            lib.boxmot_hip_detpost_destroy(x)


def test_seg_head_detpost_step_device_end_to_end():
    """a synthetic segmentation head -> DetPost(mask=...).run -> MultiStreamBotSort.step_device for three frames of eight
    well-separated, slightly moving boxes per stream; prototype plane b is 1 everywhere and box b's coefficients are the unit vector
    e_b, so the mask of box b is its window: in every output row, d_masks[s, det_ind] is the window of the box that row's track
    started on (moved with it)"""
    import torch
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.streams import MultiStreamBotSort
    S, A, ND, NB, FRAMES, MASK, IN = 2, 128, 16, 8, 3, (40, 40), (640, 640)
    post = DetPost(S, A, 1, layout="cn", extra=NB, mask=MASK, in_shape=IN, conf=0.25, iou=0.45, max_det=ND, max_candidates=64)
    trk = MultiStreamBotSort(S, max_tracks=64, max_dets=ND, emb_dim=1, with_reid=False)
    st = torch.cuda.current_stream()

    def centre(s, b, t):
        return 60.0 + 140 * (b % 4) + 2 * t + s, 100.0 + 250 * (b // 4) + t

    try:
        d_dets = torch.zeros((S, ND, 6), dtype=torch.float32, device="cuda")
        d_rows = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_coef = torch.zeros((S, ND, NB), dtype=torch.float32, device="cuda")
        d_src = torch.zeros((S, ND), dtype=torch.int32, device="cuda")
        d_masks = torch.zeros((S, ND) + MASK, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((S, ND, 8), dtype=torch.float32, device="cuda")
        d_out_n = torch.zeros(S, dtype=torch.int32, device="cuda")
        # plane b: +1 in stream 0, +2 in stream 1 -- the other stream's prototypes would do as well, the sign is what counts; plane b of
        # stream s is NEGATIVE on row 0 so that a mask is the window minus row 0 and not just "the window"
        proto = np.ones((S, NB) + MASK, dtype=np.float16)
        proto[1] *= 2
        proto[:, :, 0, :] = -1
        d_proto = torch.from_numpy(proto).cuda()
        started_on = {}                                         # (stream, track id) -> the box it started on
        total = 0
        for t in range(FRAMES):
            rng = np.random.default_rng(t)
            pred = np.zeros((S, 4 + 1 + NB, A), dtype=np.float32)
            pred[:, :4] = rng.uniform(8, 48, (S, 4, A))
            pred[:, 4] = rng.uniform(0, 0.2, (S, A))                                            # clutter below the threshold
            pred[:, 5:] = rng.uniform(-1, 1, (S, NB, A))
            where = {}
            for s in range(S):
                for b in range(NB):
                    a = (7 + 13 * b + 5 * t + s) % A                                            # another anchor every frame
                    cx, cy = centre(s, b, t)
                    pred[s, :, a] = [cx, cy, 50, 80, 0.9 - 0.03 * b] + [1.0 if e == b else 0.0 for e in range(NB)]
                    where[s, a] = b
            post.run(torch.from_numpy(pred).cuda(), [detpost_ref.GEO_UNIT] * S, d_dets, d_rows, hip_stream=st.cuda_stream, d_extra=d_coef, d_src=d_src,
                     d_proto=d_proto, d_masks=d_masks)
            st.synchronize()                                    # the tracker's own stream starts after the rows are there
            trk.step_device(d_dets.data_ptr(), d_rows.data_ptr(), None, None, 0, 0, d_out.data_ptr(), d_out_n.data_ptr())
            trk.synchronize()
            rows, src, masks, out, out_n = (x.cpu().numpy() for x in (d_rows, d_src, d_masks, d_out, d_out_n))
            assert rows.tolist() == [NB] * S
            for s in range(S):
                for row in out[s, :out_n[s]]:
                    tid, det_ind = int(row[4]), int(row[7])
                    assert 0 <= det_ind < NB
                    b = where[s, int(src[s, det_ind])]
                    cx, cy = centre(s, b, t)
                    box = tuple(np.float32(v) for v in (cx - 25, cy - 40, cx + 25, cy + 40))
                    win = ref.window_of(box, MASK, IN)
                    win[0, :] = False
                    assert win.sum() >= 8 and np.array_equal(masks[s, det_ind].astype(bool), win), (t, s, tid)
                    assert abs((row[0] + row[2]) / 2 - cx) < 20 and abs((row[1] + row[3]) / 2 - cy) < 20, (t, s, tid, row)     # the track's own box
                    assert started_on.setdefault((s, tid), b) == b, (t, s, tid, "the mask is another box's than the track started on")
                    total += 1
        assert total >= S * NB and len(started_on) == S * NB and (trk.status() == 0).all()
    finally:
        torch.cuda.synchronize()
        post.close(); trk.close()
