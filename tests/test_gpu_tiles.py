"""GPU tests of tiled detection for large frames: FrameRing.letterbox_tiles (include/boxmot_hip.h boxmot_hip_ingest_letterbox_tiles,
csrc/ingest_letterbox_tiles.hpp) and DetPost(tiles=T) (boxmot_hip_detpost_*_tiled, csrc/det_post_tiled.hpp).  The resize is integer
arithmetic, the tensor's values come out of a table and the post-processing is float32 without fused operations, so every
comparison is EXACT (bit for bit against tests/letterbox_tiles_ref.py and tests/detpost_tiled_ref.py): a differing byte is a failure."""
import ctypes

import numpy as np
import pytest

import detpost_ref
import detpost_tiled_ref as dref
import letterbox_tiles_ref as lref

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {np.float16: "float16", np.float32: "float32"}
SENTINEL = -12345.5


def _same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


# ---- letterbox_tiles ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring():
    """the two frames of the reference, of different sizes, as the streams of one ring; slot 0 holds them"""
    from boxmot_amd.ingest import FrameRing
    r = FrameRing(2, len(lref.FRAMES), sizes=lref.SIZES)
    for s, f in enumerate(lref.FRAMES):
        r.host_view(0, s)[...] = f
    r.submit(0)
    yield r
    r.close()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("mode", ["center", "topleft"])
@pytest.mark.parametrize("size", lref.OUT_SIZES, ids=["64x64", "32x64"])
def test_tiles_equal_the_reference_and_leave_the_tensors_beyond_alone(ring, size, mode, dtype):
    import torch
    n = len(lref.FRAMES) * lref.T
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        x = torch.full((n + 2, 3, *size), -3.0, dtype=getattr(torch, TORCH_DTYPE[dtype]), device="cuda")
        geo = ring.letterbox_tiles(0, x, lref.TILES, mode=mode, hip_stream=st.cuda_stream)
        y = x.clone()                                   # queued behind the kernel on the same stream: no synchronisation by the caller
    st.synchronize()
    got, want = y.cpu().numpy(), lref.want(size, mode, dtype=dtype)
    for k in range(n):
        s, t = divmod(k, lref.T)
        assert tuple(geo[s][t]) == lref.geometry(lref.TILES[s][t], size, mode), (s, t)
        assert _same(got[k], want[k]), (size, mode, dtype, "stream", s, "tile", lref.TILES[s][t])
    assert (got[n:] == -3.0).all()


def test_plane_order_scale_pad_and_fewer_streams(ring):
    import torch
    x = torch.full((2 * lref.T, 3, 64, 64), -3.0, dtype=torch.float32, device="cuda")
    geo = ring.letterbox_tiles(0, x, lref.TILES, rgb=False, unit=False, pad=7, n_streams=1, hip_stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert len(geo) == 1 and len(geo[0]) == lref.T
    got = x.cpu().numpy()
    assert _same(got[:lref.T], lref.want((64, 64), "center", False, False, 7, np.float32)[:lref.T]) and (got[lref.T:] == -3.0).all()


def test_the_single_whole_frame_tile_is_letterbox_byte_for_byte(ring):
    import torch
    whole = [[(0, 0, c, r)] for r, c in lref.SIZES]
    st = torch.cuda.current_stream().cuda_stream
    for size in lref.OUT_SIZES:
        for mode, dtype in (("center", torch.float16), ("topleft", torch.float32)):
            a = torch.zeros((2, 3, *size), dtype=dtype, device="cuda")
            b = torch.ones((2, 3, *size), dtype=dtype, device="cuda")
            ga = ring.letterbox(0, a, mode=mode, hip_stream=st)
            gb = ring.letterbox_tiles(0, b, whole, mode=mode, hip_stream=st)
            torch.cuda.synchronize()
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (size, mode)
            for s in range(2):
                assert tuple(gb[s][0])[:7] == tuple(ga[s]) and tuple(gb[s][0])[7:] == (0, 0)


def test_letterbox_tiles_errors(ring):
    import torch
    from boxmot_amd import _lib
    from boxmot_amd.ingest import tile_grid
    lib = _lib.load()
    x = torch.full((2 * lref.T, 3, 64, 64), 5.0, dtype=torch.float32, device="cuda")
    bad = [list(t) for t in lref.TILES]
    bad[1][3] = (150, 100, 60, 28)
    with pytest.raises(ValueError, match="stream 1 tile 3"):                   # outside the frame
        ring.letterbox_tiles(0, x, bad)
    with pytest.raises(ValueError, match="stream 1: 7 tiles where stream 0 has 8"):
        ring.letterbox_tiles(0, x, [lref.TILES[0], lref.TILES[1][:7]])
    bad[1][3] = (0, 0, 200, 1)
    with pytest.raises(ValueError, match="stream 1 tile 3.*no picture"):       # a vanishing picture
        ring.letterbox_tiles(0, x, bad)
    with pytest.raises(ValueError, match="N >= 16"):
        ring.letterbox_tiles(0, x[:15], lref.TILES)
    # the library checks for itself
    cfg = _lib.Letterbox(out_rows=64, out_cols=64, mode=0, dtype=0, rgb=1, unit=1, pad_value=114)

    def call(rects, n=2, T=lref.T, slot=0):
        r = np.ascontiguousarray(np.array(rects, dtype=np.int32))
        ok = lib.boxmot_hip_ingest_letterbox_tiles(ring._handle, slot, n, T, r.ctypes.data, ctypes.byref(cfg), ctypes.c_void_p(x.data_ptr()), None)
        return ok, _lib.last_error()
    good = np.array(lref.TILES, dtype=np.int32)
    for kw, word in [(dict(T=0), "n_tiles"), (dict(T=65), "n_tiles"), (dict(n=3), "stream count"), (dict(slot=2), "slot")]:
        ok, msg = call(good, **kw)
        assert not ok and word in msg, (kw, msg)
    outside = good.copy(); outside[1, 3] = (150, 100, 60, 28)
    ok, msg = call(outside)
    assert not ok and "stream 1 tile 3" in msg and "not inside" in msg, msg
    vanish = good.copy(); vanish[0, 6] = (0, 0, 131, 1)
    ok, msg = call(vanish)
    assert not ok and "stream 0 tile 6" in msg and "no picture" in msg, msg
    assert not lib.boxmot_hip_ingest_letterbox_tiles(ring._handle, 0, 2, lref.T, None, ctypes.byref(cfg), ctypes.c_void_p(x.data_ptr()), None)
    torch.cuda.synchronize()
    assert (x == 5.0).all()                                                     # none of them wrote
    out = np.zeros(9)
    r = np.array((7, 11, 33, 20), dtype=np.int32)
    assert lib.boxmot_hip_letterbox_tile_geometry(97, 131, r.ctypes.data, ctypes.byref(cfg), out.ctypes.data_as(_lib.c_double_p))
    assert tuple(out) == lref.geometry((7, 11, 33, 20), (64, 64))
    r = np.array((100, 0, 32, 10), dtype=np.int32)
    assert not lib.boxmot_hip_letterbox_tile_geometry(97, 131, r.ctypes.data, ctypes.byref(cfg), out.ctypes.data_as(_lib.c_double_p))
    assert "not inside" in _lib.last_error()
    # a grid over both frame sizes: the same count, one call
    grids = [tile_grid(r_, c_, grid=(2, 2), overlap=0.25) for r_, c_ in lref.SIZES]
    y = torch.empty((10, 3, 32, 64), dtype=torch.float16, device="cuda")
    ring.letterbox_tiles(0, y, grids, hip_stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _same(y, lref.letterbox_tiles(lref.FRAMES, grids, (32, 64), dtype=np.float16))


# ---- DetPost(tiles=T) ------------------------------------------------------------------------------------------------------------------
def _post(c, **over):
    from boxmot_amd.detpost import DetPost
    S, T, A, nc = c.dims
    return DetPost(S, A, nc, layout=c.layout, tiles=T, **dict(c.opts, **over))


def _outputs(torch, S, stride):
    return (torch.full((S, stride, 6), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((S,), -77, dtype=torch.int32, device="cuda"))


def _assert_stream(name, s, dets, rows, counters, want):
    w_rows, w_cnt = want
    assert rows[s] == len(w_rows), (name, s, int(rows[s]), len(w_rows))
    assert counters[s].tolist() == w_cnt.tolist(), (name, s)
    assert np.array_equal(dets[s, :rows[s]].view(np.uint32), w_rows.view(np.uint32)), (name, s)
    assert (dets[s, rows[s]:] == np.float32(SENTINEL)).all(), (name, s, "rows beyond the count were written")


@pytest.mark.parametrize("k", range(len(dref.CASES)), ids=dref.NAMES)
def test_each_tiled_case_equals_the_reference_twice(k):
    """rows as bytes, counts, counters, untouched sentinel rows -- and the same bytes from a second run of the same handle into a
    fresh block, on a side stream: nothing of a call is left in the handle's scratch"""
    import torch
    c = dref.CASES[k]
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
                out = (d_dets.clone(), d_rows.clone())
            counters = post.counters()                          # waits for the run
            st.synchronize()
            dets, rows = out[0].cpu().numpy(), out[1].cpu().numpy()
            for s in range(S):
                _assert_stream(c.name, s, dets, rows, counters, dref.want(k)[s])
            if first is not None:
                assert first[0].tobytes() == dets.tobytes() and first[1].tobytes() == rows.tobytes() and first[2].tobytes() == counters.tobytes()
            first = (dets, rows, counters)
    finally:
        torch.cuda.synchronize()
        post.close()


def test_fewer_streams_than_the_handle_leave_the_others_alone():
    import torch
    k = dref.NAMES.index("clip_to_the_tile_ios")
    c = dref.CASES[k]
    post = _post(c)
    try:
        pred = torch.from_numpy(c.preds).cuda()
        d_dets, d_rows = _outputs(torch, 2, c.stride)
        post.run(pred, c.geos[:1], d_dets, d_rows, hip_stream=torch.cuda.current_stream().cuda_stream)
        counters = post.counters()
        dets, rows = d_dets.cpu().numpy(), d_rows.cpu().numpy()
        _assert_stream(c.name, 0, dets, rows, counters, dref.want(k)[0])
        assert (dets[1] == np.float32(SENTINEL)).all() and rows[1] == -77 and counters[1].tolist() == [0, 0, 0]
        # the geometry changes between calls of one handle: the table is uploaded again (stream 0's tensors under stream 1's tiles)
        post.run(pred, [c.geos[1], c.geos[0]], d_dets, d_rows, hip_stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        w = dref.detpost_tiled(c.preds[:3], c.geos[1], c.layout, **c.opts)[0]
        assert d_rows[0].item() == len(w) and np.array_equal(d_dets[0, :len(w)].cpu().numpy().view(np.uint32), w.view(np.uint32))
    finally:
        torch.cuda.synchronize()
        post.close()


def test_one_unit_tile_gives_the_untiled_detposts_bytes():
    """T = 1, unit gain, no padding, boxes inside the frame: the rows of an untiled DetPost run on the same tensor, and the reference's"""
    import torch
    from boxmot_amd.detpost import DetPost
    names = [c.name for c in detpost_ref.CASES]
    for name in dref.IDENTITY:
        k = names.index(name)
        u = detpost_ref.CASES[k]
        S, A, nc = u.dims
        pred = torch.from_numpy(u.preds[:1]).cuda()
        plain, tiled = DetPost(1, A, nc, layout=u.layout, **u.opts), DetPost(1, A, nc, layout=u.layout, tiles=1, **u.opts)
        try:
            a, b = plain.run_host(pred, u.geos[:1])[0], tiled.run_host(pred, [[dref.TILE_UNIT]])[0]
            assert a.tobytes() == b.tobytes() and np.array_equal(b.view(np.uint32), detpost_ref.want(k)[0][0].view(np.uint32)), name
            assert plain.counters().tolist() == tiled.counters().tolist()
        finally:
            plain.close(); tiled.close()


def test_the_comparison_bites():
    """wrong-reference controls: `>=` in the NMS test, and conf ties to the higher tile, differ from the device on their cases"""
    import torch
    for name, wrong in (("cut_box_ios_exactly_at_the_threshold", dict(nms_ge=True)), ("equal_conf_tile_order_decides", dict(tiles_high_first=True))):
        k = dref.NAMES.index(name)
        c = dref.CASES[k]
        post = _post(c)
        try:
            got = post.run_host(torch.from_numpy(c.preds).cuda(), c.geos)[0]
        finally:
            post.close()
        assert np.array_equal(got.view(np.uint32), dref.want(k)[0][0].view(np.uint32))
        bad = dref.want(k, **wrong)[0][0]
        assert got.shape != bad.shape or not np.array_equal(got, bad), name


def test_tiled_c_abi_errors():
    import torch
    from boxmot_amd import _lib
    lib = _lib.load()
    base = dict(n_streams=2, n_anchors=64, n_classes=3, layout=0, conf_thres=0.25, iou_thres=0.45, max_candidates=64, max_det=8, agnostic=0, class_allow=None)
    for kw, word in [(dict(n_tiles=0), "n_tiles"), (dict(n_tiles=65), "n_tiles"), (dict(merge=2), "merge")]:
        cfg = _lib.DetPostTiledConfig(_lib.DetPostConfig(**base), **dict(dict(n_tiles=3, merge=0), **kw))
        assert not lib.boxmot_hip_detpost_create_tiled(ctypes.byref(cfg)) and word in _lib.last_error(), (kw, _lib.last_error())
    cfg = _lib.DetPostTiledConfig(_lib.DetPostConfig(**dict(base, max_candidates=32)), 3, 0)
    assert not lib.boxmot_hip_detpost_create_tiled(ctypes.byref(cfg)) and "max_candidates" in _lib.last_error()
    assert not lib.boxmot_hip_detpost_create_tiled(None) and "null" in _lib.last_error()
    cfg = _lib.DetPostTiledConfig(_lib.DetPostConfig(**base), 3, 1)
    h = lib.boxmot_hip_detpost_create_tiled(ctypes.byref(cfg))
    assert h, _lib.last_error()
    ucfg = _lib.DetPostConfig(**base)
    u = lib.boxmot_hip_detpost_create(ctypes.byref(ucfg))
    assert u, _lib.last_error()
    try:
        pred = torch.zeros((6, 7, 64), device="cuda")
        d_dets, d_rows = _outputs(torch, 2, 8)
        geom = np.tile(np.array([0.5, 0, 0, 10, 20, 64, 64], dtype=np.float64), (2, 3, 1))

        def call(fn=lib.boxmot_hip_detpost_run_tiled, handle=h, n=2, p=None, dtype=0, g=geom, stride=8):
            ok = fn(handle, n, ctypes.c_void_p(pred.data_ptr() if p is None else p), dtype, g.ctypes.data_as(_lib.c_double_p),
                    ctypes.c_void_p(d_dets.data_ptr()), stride, ctypes.c_void_p(d_rows.data_ptr()), None)
            return ok, _lib.last_error()
        bad_gain, bad_w, bad_nan = geom.copy(), geom.copy(), geom.copy()
        bad_gain[1, 2, 0] = 0.0
        bad_w[0, 1, 5] = 0.5
        bad_nan[1, 0, 3] = np.nan
        for kw, word in [(dict(n=0), "stream count"), (dict(n=3), "stream count"), (dict(p=0), "null"), (dict(dtype=2), "dtype"), (dict(stride=7), "max_det"),
                         (dict(p=pred.data_ptr() + 2), "aligned"), (dict(g=bad_gain), "stream 1 tile 2"), (dict(g=bad_w), "stream 0 tile 1"),
                         (dict(g=bad_nan), "stream 1 tile 0"), (dict(handle=u), "create_tiled"), (dict(fn=lib.boxmot_hip_detpost_run), "run_tiled")]:
            ok, msg = call(**kw)
            assert not ok and word in msg, (kw, msg)
        torch.cuda.synchronize()
        assert (d_dets == SENTINEL).all() and (d_rows == -77).all()            # none of them wrote
        ok, msg = call()
        assert ok, msg
        torch.cuda.synchronize()
        assert d_rows.tolist() == [0, 0]
    finally:
        lib.boxmot_hip_detpost_destroy(h)
        lib.boxmot_hip_detpost_destroy(u)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
E2E_SIZES = [(128, 192), (100, 150)]
E2E_TILES = [[(0, 0, 192, 128), (0, 0, 128, 128), (64, 0, 128, 128)], [(0, 0, 150, 100), (0, 0, 64, 64), (86, 36, 64, 64)]]
E2E_OBJECTS = [[(90, 50, 40, 40, 1), (30, 90, 30, 30, 0), (160, 40, 30, 40, 2)], [(30, 30, 20, 24, 2), (120, 70, 16, 16, 0), (75, 20, 16, 16, 1)]]          # (the last: only the whole frame sees it)


def _toy_detector(torch, x, geo, t):
    """a synthetic "detector": per tile tensor it reports the known frame-space objects (drifting with t) that reach into the tile,
    through the tile's geometry -- surer (0.9 - 0.05 * tile) in a tile than in the whole frame (0.6), and unclipped, so an object cut
    by the tile's edge is reported beyond it -- plus sub-threshold clutter; a (S * T, 4 + 3, 128) "cn" tensor on the device"""
    tensors = []
    for s, tiles in enumerate(geo):
        for k, g in enumerate(tiles):
            row = (g.gain, g.top, g.left, g.x0, g.y0, g.cols, g.rows)
            dets = []
            for cx, cy, w, h, cls in E2E_OBJECTS[s]:
                cx, cy = cx + t, cy + 0.5 * t
                if cx + w / 2 > g.x0 and cx - w / 2 < g.x0 + g.cols and cy + h / 2 > g.y0 and cy - h / 2 < g.y0 + g.rows:
                    dets.append(dref.in_tile((cx, cy, w, h, 0.6 if k == 0 else 0.9 - 0.05 * k, cls), row))
            tensors.append(detpost_ref.pack(dets, 128, 3, "cn", np.float32, 1000 + 100 * t + 10 * s + k))
    return torch.from_numpy(np.ascontiguousarray(np.stack(tensors))).cuda() + 0 * x.float().mean()


def test_ring_letterbox_tiles_detector_tiled_detpost_step_device_end_to_end():
    """FrameRing -> letterbox_tiles -> a synthetic detector on the S * T tile tensors -> DetPost(tiles=T).run -> MultiStreamBotSort
    .step_device for a few frames, two streams of different frame sizes: the merged rows equal the reference's, and the tracker's
    rows equal those of a second handle fed through update_batch with the reference's merged detections"""
    import torch
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.ingest import FrameRing
    from boxmot_amd.streams import MultiStreamBotSort
    import letterbox_ref
    S, T, NF, ND = 2, 3, 4, 16
    frames = [letterbox_ref.make_frame(r, c, "random", 80 + s) for s, (r, c) in enumerate(E2E_SIZES)]
    ring = FrameRing(2, S, sizes=E2E_SIZES)
    opts = dict(conf=0.25, iou=0.45, max_det=ND, max_candidates=64)
    post = DetPost(S, 128, 3, layout="cn", tiles=T, merge="ios", **opts)
    kw = dict(max_tracks=64, max_dets=ND, emb_dim=1, with_reid=False)           # (motion only: the step needs no frames)
    dev, host = MultiStreamBotSort(S, **kw), MultiStreamBotSort(S, **kw)
    st = torch.cuda.current_stream()
    try:
        d_dets = torch.zeros((S, ND, 6), dtype=torch.float32, device="cuda")
        d_rows = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((S, ND, 8), dtype=torch.float32, device="cuda")
        d_out_n = torch.zeros(S, dtype=torch.int32, device="cuda")
        total = 0
        for t in range(NF):
            for s, f in enumerate(frames):
                ring.host_view(t % 2, s)[...] = np.roll(f, 2 * t, axis=1)
            ring.submit(t % 2)
            x = torch.empty((S * T, 3, 64, 64), dtype=torch.float16, device="cuda")
            geo = ring.letterbox_tiles(t % 2, x, E2E_TILES, hip_stream=st.cuda_stream)
            pred = _toy_detector(torch, x, geo, t)
            post.run(pred, geo, d_dets, d_rows, hip_stream=st.cuda_stream)
            st.synchronize()                                    # the tracker's own stream starts after the rows are there
            dev.step_device(d_dets.data_ptr(), d_rows.data_ptr(), None, None, 0, 0, d_out.data_ptr(), d_out_n.data_ptr())
            dev.synchronize()
            ring.host_done(t % 2)
            want_x = lref.letterbox_tiles([np.roll(f, 2 * t, axis=1) for f in frames], E2E_TILES, (64, 64), dtype=np.float16)
            assert _same(x, want_x), t
            pred_h = pred.cpu().numpy()
            rows7 = [[(g.gain, g.top, g.left, g.x0, g.y0, g.cols, g.rows) for g in tiles] for tiles in geo]
            want_dets = [dref.detpost_tiled(pred_h[s * T:(s + 1) * T], rows7[s], "cn", merge="ios", **opts)[0] for s in range(S)]
            assert all(len(w) == 3 for w in want_dets), [len(w) for w in want_dets]              # the objects, once each
            got_dets, got_n = d_dets.cpu().numpy(), d_rows.cpu().numpy()
            want_rows = host.update_batch(want_dets)
            out, out_n = d_out.cpu().numpy(), d_out_n.cpu().numpy()
            for s in range(S):
                assert got_n[s] == 3 and np.array_equal(got_dets[s, :3].view(np.uint32), want_dets[s].view(np.uint32)), (t, s)
                w = np.asarray(want_rows[s], dtype=np.float32).reshape(-1, 8)
                assert out_n[s] == len(w) and np.array_equal(out[s, :out_n[s]], w), (t, s)
                total += len(w)
        assert total > 0
        assert (dev.status() == 0).all()
    finally:
        torch.cuda.synchronize()
        ring.close(); post.close(); dev.close(); host.close()
