"""In-handle ReID for ORIENTED detections on the device: the fp32-grade (mode 2) oriented crop kernels and their features against
oracle.crops / the torch oracle, the crop geometry the device makes for the crop list of an oriented handle against
oracle.crops.obb_crop_geometry, and an oriented MultiStreamBotSort that crops, embeds and tracks by itself (update_batch with host
frames or a FrameRing, step_device with device frames, mixed frame sizes, the DetPost chain) against the same handle fed the
embeddings HipReID computes for the same boxes."""
import ctypes

import numpy as np
import pytest

from common import obb_frames
from obb_reid_common import BLANK_GEOMETRY, FIXED, expected_planes, geometry_pool, non_finite_boxes, oracle_geometry, same_bits

pytestmark = pytest.mark.gpu

# Largest |device - oracle| over the six map entries of the pool, measured on an MI355X (the device's double-precision cos / sin
# against the host's libm; everything else is the same sequence of IEEE operations): see DESIGN.md section 4.13.  The test asserts
# 4 x the measured figure and never more than 1e-9 (a map error of 1e-9 moves a sampling position of a 512-pixel crop by about
# 1e-6 pixel, a thousandth of warpAffine's 2^-10-pixel quantum: anything larger is a bug, not noise).
GEOMETRY_MEASURED = 2.274e-13
GEOMETRY_BOUND = min(4 * GEOMETRY_MEASURED, 1e-9)


@pytest.fixture(scope="module")
def sd():
    from boxmot_amd.reid_weights import reference_init_state_dict
    return reference_init_state_dict("osnet_x0_25", seed=0)


def _boxes_and_image():
    """the 39 boxes and the 480 x 641 image of tests/test_gpu_reid.py's oriented test (same seeds)"""
    rng = np.random.default_rng(21)
    img = rng.integers(0, 255, (480, 641, 3), dtype=np.uint8)
    rand = np.stack([rng.uniform(-20, 660, 30), rng.uniform(-20, 500, 30), rng.uniform(2, 200, 30), rng.uniform(2, 400, 30),
                     rng.uniform(-np.pi, np.pi, 30)], 1).astype(np.float32)
    return np.concatenate([FIXED, rand]), img


# ---- 1. fp32-grade oriented crops and features ----
@pytest.mark.parametrize("pre", ["resize", "resize_pad"])
def test_fp32_grade_oriented_crops_bit_exact_and_features_within_the_reid_bar(sd, pre):
    """HipReID(mode=2) on oriented boxes: features within 1e-3 of the torch oracle (more boxes than one engine chunk), the (hi, lo)
    planes the family reads bit for bit what oracle.crops gives after the table and the (hi, lo) split, an axis-aligned call right
    after an oriented one unharmed, and a batch over two images of different sizes."""
    from boxmot_amd.reid import MODE_FP32_FUSED, HipReID
    from oracle.osnet import OracleReID
    boxes, img = _boxes_and_image()
    orc = OracleReID(sd, preprocess=pre)
    r = HipReID(sd, mode=MODE_FP32_FUSED, preprocess=pre, max_crops=16)
    try:
        err = np.abs(r.get_features(boxes, img) - orc.get_features(boxes, img)).max()
        print(f"{pre}: mode 2 oriented features, max |diff| vs the oracle {err:.3e}")
        assert err < 1e-3, (pre, err)
        want_h, want_l = expected_planes(boxes, img, pre)
        for i0 in range(0, len(boxes), 16):
            hi, lo = r.debug_crop_planes(boxes[i0:i0 + 16], img)
            assert same_bits(hi, want_h[i0:i0 + 16]) and same_bits(lo, want_l[i0:i0 + 16]), (pre, i0)
        # an axis-aligned call right after an oriented one does not see stale geometry
        aabb = np.array([[136, 72, 264, 328]], dtype=np.float32)
        assert np.abs(r.get_features(aabb, img) - orc.get_features(aabb, img)).max() < 1e-3
        # two images of different sizes in one pass (the table-form kernel)
        img2 = np.random.default_rng(22).integers(0, 255, (160, 200, 3), dtype=np.uint8)
        b2 = np.array([[100, 80, 40, 90, 0.3], [10, 12, 30, 50, -1.2], [190, 150, 50, 60, 2.0], [96.5, 70.5, 33.4, 71.6, 0.77]], dtype=np.float32)
        got = r.get_features_batch([boxes[:9], b2], [img, img2])
        assert np.abs(got[0] - orc.get_features(boxes[:9], img)).max() < 1e-3
        assert np.abs(got[1] - orc.get_features(b2, img2)).max() < 1e-3
        assert np.abs(r.get_features(aabb, img) - orc.get_features(aabb, img)).max() < 1e-3
    finally:
        r.close()


def test_wide_fp32_grade_family_takes_oriented_boxes():
    """osnet_x1_0 in mode 2 (the wide fp32-grade family reads the same (hi, lo) planes): 4 oriented boxes within 1e-3"""
    from boxmot_amd.reid import MODE_FP32_FUSED, HipReID
    from boxmot_amd.reid_weights import reference_init_state_dict
    from oracle.osnet import OracleReID
    sd1 = reference_init_state_dict("osnet_x1_0", seed=0)
    img = np.random.default_rng(23).integers(0, 255, (160, 200, 3), dtype=np.uint8)
    boxes = np.array([[100, 80, 40, 90, 0.3], [10, 12, 30, 50, -1.2], [190, 150, 50, 60, 2.0], [96.5, 70.5, 33.4, 71.6, 0.77]], dtype=np.float32)
    r = HipReID(sd1, mode=MODE_FP32_FUSED, max_crops=8)
    try:
        err = np.abs(r.get_features(boxes, img) - OracleReID(sd1).get_features(boxes, img)).max()
        print(f"osnet_x1_0 mode 2 oriented features, max |diff| vs the oracle {err:.3e}")
        assert err < 1e-3, err
        hi, lo = r.debug_crop_planes(boxes, img)
        wh, wl = expected_planes(boxes, img, "resize")
        assert same_bits(hi, wh) and same_bits(lo, wl)
    finally:
        r.close()


# ---- 2. geometry on the device ----
def test_device_crop_geometry_against_the_oracle(sd):
    """obb_crop_geometry as the device computes it (the function the oriented crop-list kernel calls): sizes exact, the six map
    entries within the measured band (and never beyond 1e-9); non-finite boxes give the blank geometry and a finite embedding."""
    from boxmot_amd.reid import MODE_FP32_FUSED, HipReID
    pool = geometry_pool()
    want = oracle_geometry(pool)
    r = HipReID(sd, mode=MODE_FP32_FUSED, max_crops=16)
    try:
        got = r.debug_obb_geometry(pool)
        assert np.array_equal(got[:, :2], want[:, :2])
        diff = np.abs(got[:, 2:] - want[:, 2:])
        worst = np.unravel_index(diff.argmax(), diff.shape)
        print(f"device crop geometry: max |map - oracle| = {diff.max():.3e} at box {worst[0]} entry {worst[1]} "
              f"(2x2 part {diff[:, [0, 1, 3, 4]].max():.3e}, offsets {diff[:, [2, 5]].max():.3e}); bound {GEOMETRY_BOUND:.1e}")
        assert diff.max() <= GEOMETRY_BOUND, (diff.max(), pool[worst[0]])
        bad = non_finite_boxes()
        assert np.array_equal(r.debug_obb_geometry(bad), np.tile(BLANK_GEOMETRY, (len(bad), 1)))
        img = np.random.default_rng(24).integers(0, 255, (160, 200, 3), dtype=np.uint8)
        f = r.get_features(np.concatenate([bad[:4], pool[:1]]), img)
        assert np.isfinite(f).all() and np.allclose(np.linalg.norm(f, axis=1), 1.0, atol=1e-4)
        assert np.array_equal(f[0], f[1]) and np.array_equal(f[0], f[3])         # every blank crop is the same crop
        # ... the all-zero crop, which is what an empty axis-aligned box is (the oracle's, at the ReID bar: the axis-aligned call
        # itself goes through the fused stem, another route of the same precision grade, so it is not bit-identical)
        from oracle.osnet import OracleReID
        empty = np.array([[50, 50, 50, 50]], dtype=np.float32)
        want0 = OracleReID(sd).get_features(empty, img)
        assert np.abs(f[:1] - want0).max() < 1e-3 and np.abs(r.get_features(empty, img) - want0).max() < 1e-3
    finally:
        r.close()


# ---- 3. in-handle ReID equals caller-supplied embeddings ----
ROWS, COLS, ND, HIGH = 144, 192, 16, 0.5


def _scene(n_frames, seed, scale=0.3, max_rows=12):
    """the oriented stress scene of the other oriented tests, shrunk into a small frame, at most 12 detections per frame"""
    out = []
    for d in obb_frames(n_frames, seed=seed):
        d = np.array(d[:max_rows], dtype=np.float32)
        d[:, :4] *= np.float32(scale)
        out.append(np.ascontiguousarray(d))
    return out


def _frame(rows, cols, seed, t):
    base = np.random.default_rng(seed).integers(0, 255, (rows, cols, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.roll(base, (t % 3, 2 * (t % 4)), axis=(0, 1)))


def _caller_embs(reid, dets, img):
    """embeddings of the rows above track_high_thresh (the rows the handle itself embeds), zeros elsewhere (never read)"""
    e = np.zeros((len(dets), 512), dtype=np.float32)
    m = dets[:, 5].astype(np.float64) > HIGH
    if m.any():
        e[m] = reid.get_features(dets[m, :5], img)
    return e


def _same_tracks(a, b, n_streams, tol=1e-5):
    for s in range(n_streams):
        for which in (0, 1):
            da, db = a.state_dump(s, which), b.state_dump(s, which)
            assert da["n"] == db["n"] and np.array_equal(da["ints"], db["ints"]), (s, which)
            if da["n"]:
                assert np.abs(da["smooth"] - db["smooth"]).max() <= tol, (s, which, np.abs(da["smooth"] - db["smooth"]).max())


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("path", ["update_batch", "ring", "step_device"])
def test_in_handle_oriented_reid_equals_caller_supplied_embeddings(sd, mode, path):
    """One oriented handle with ReID weights crops and embeds by itself -- host frames, a FrameRing slot, or the device-resident step
    on the ring's frames (two-stage pipeline) --; a second handle of the same configuration gets HipReID's embeddings of the same
    boxes.  Rows (ids, boxes, det indices) equal frame by frame, smoothed features within 1e-5.  (The BoT-SORT handle has no
    set_crop_bound -- that is DeepOCSORT's / StrongSORT's -- so there is no bounded variant to repeat this with.)"""
    import torch
    from boxmot_amd.ingest import FrameRing
    from boxmot_amd.reid import HipReID
    from boxmot_amd.streams import MultiStreamBotSort
    S, T = 2, 12
    scenes = [_scene(T, seed=4 + s) for s in range(S)]
    kw = dict(max_tracks=64, max_dets=ND, emb_dim=512, is_obb=True)
    own, fed = MultiStreamBotSort(S, reid_weights=sd, **kw), MultiStreamBotSort(S, **kw)
    own.set_reid_mode(mode)
    reid = HipReID(sd, mode=mode, max_crops=ND)
    ring = FrameRing(2, S, rows=ROWS, cols=COLS) if path != "update_batch" else None
    total = embedded = 0
    try:
        if path == "step_device":
            d_dets = torch.zeros((S, ND, 7), dtype=torch.float32, device="cuda")
            d_rows = torch.zeros(S, dtype=torch.int32, device="cuda")
            d_out = torch.zeros((S, ND, 9), dtype=torch.float32, device="cuda")
            d_out_n = torch.zeros(S, dtype=torch.int32, device="cuda")
            stream = own._lib.boxmot_hip_botsort_stream(own._handle)
        for t in range(T):
            dets = [scenes[s][t] for s in range(S)]
            imgs = [_frame(ROWS, COLS, 30 + s, t) for s in range(S)]
            want = fed.update_batch(dets, embs_list=[_caller_embs(reid, d, im) for d, im in zip(dets, imgs)])
            if path == "update_batch":
                got = [np.asarray(g) for g in own.update_batch(dets, imgs=imgs)]
            else:
                slot = t % 2
                ring.host_done(slot)
                for s in range(S):
                    ring.host_view(slot)[s] = imgs[s]
                ring.submit(slot)
                if path == "ring":
                    got = [np.asarray(g) for g in own.update_batch(dets, ring=ring, slot=slot)]
                else:
                    h = np.zeros((S, ND, 7), dtype=np.float32)
                    for s, d in enumerate(dets):
                        h[s, :len(d)] = d
                    d_dets.copy_(torch.from_numpy(h))
                    d_rows.copy_(torch.tensor([len(d) for d in dets], dtype=torch.int32))
                    torch.cuda.synchronize()
                    ring.wait(slot, stream)
                    own.step_device(d_dets.data_ptr(), d_rows.data_ptr(), None, ring.device_frames(slot), ROWS, COLS, d_out.data_ptr(), d_out_n.data_ptr())
                    ring.release(slot, stream)
                    own.synchronize()
                    out, n = d_out.cpu().numpy(), d_out_n.cpu().numpy()
                    got = [out[s, :n[s]] for s in range(S)]
            for s in range(S):
                w = np.asarray(want[s], dtype=np.float32).reshape(-1, 9)
                assert got[s].shape == w.shape and np.array_equal(got[s], w), (t, s)
                total += len(w)
                embedded += int((dets[s][:, 5] > HIGH).sum())
        assert total > 40 and embedded > 40
        assert (own.status() == 0).all()
        _same_tracks(own, fed, S)
    finally:
        torch.cuda.synchronize()
        own.synchronize()
        if ring is not None:
            ring.close()
        own.close(); fed.close(); reid.close()


def test_botsort_class_with_a_mode_2_reid_model_embeds_oriented_detections(sd):
    """BotSort(reid_model=HipReID(mode=2)).update(dets7, img): the class embeds the oriented rows above track_high_thresh through
    model.get_features, as the reference's update does; its rows equal those of an oriented handle that embeds by itself."""
    from boxmot_amd import BotSort
    from boxmot_amd.reid import HipReID
    from boxmot_amd.streams import MultiStreamBotSort
    reid = HipReID(sd, mode=2, max_crops=ND)
    trk = BotSort(reid_model=reid, use_cmc=False, max_tracks=64, max_dets=ND, emb_dim=512)
    own = MultiStreamBotSort(1, max_tracks=64, max_dets=ND, emb_dim=512, is_obb=True, reid_weights=sd)
    own.set_reid_mode(2)
    total = 0
    try:
        for t, d in enumerate(_scene(8, seed=5)):
            img = _frame(ROWS, COLS, 60, t)
            got = np.asarray(trk.update(d, img), dtype=np.float32).reshape(-1, 9)
            want = np.asarray(own.update_batch([d], imgs=[img])[0], dtype=np.float32).reshape(-1, 9)
            assert got.shape == want.shape and np.array_equal(got, want), t
            total += len(want)
        assert total > 20 and trk.is_obb
    finally:
        trk.close(); own.close(); reid.close()


# ---- 4. mixed frame sizes ----
SIZES = [(96, 128), (160, 200), (120, 96)]


def test_oriented_reid_streams_of_three_frame_sizes_equal_single_stream_handles(sd):
    """streams of 96 x 128, 160 x 200 and 120 x 96 in one oriented ReID handle (the table-form oriented crop kernel) give, per stream,
    the rows of a single-stream handle of that size (the scalar form)"""
    from boxmot_amd.streams import MultiStreamBotSort
    S, T = len(SIZES), 10
    scenes = [_scene(T, seed=7 + s, scale=min(r / 480, c / 640)) for s, (r, c) in enumerate(SIZES)]
    kw = dict(max_tracks=64, max_dets=ND, emb_dim=512, is_obb=True, reid_weights=sd)
    mixed = MultiStreamBotSort(S, frame_sizes=SIZES, **kw)
    singles = [MultiStreamBotSort(1, **kw) for _ in range(S)]
    for trk in [mixed] + singles:
        trk.set_reid_mode(2)
    total = 0
    try:
        for t in range(T):
            dets = [scenes[s][t] for s in range(S)]
            imgs = [_frame(r, c, 40 + s, t) for s, (r, c) in enumerate(SIZES)]
            got = mixed.update_batch(dets, imgs=imgs)
            for s in range(S):
                want = singles[s].update_batch([dets[s]], imgs=[imgs[s]])[0]
                assert np.array_equal(np.asarray(got[s]), np.asarray(want)), (t, s)
                total += len(want)
        assert total > 40
        for s in range(S):
            for which in (0, 1):
                a, b = mixed.state_dump(s, which), singles[s].state_dump(0, which)
                assert a["n"] == b["n"] and np.array_equal(a["ints"], b["ints"]) and np.abs(a["smooth"] - b["smooth"]).max(initial=0) <= 1e-5
    finally:
        for trk in [mixed] + singles:
            trk.close()


# ---- 5. end to end ----
E2E_SIZES = [(120, 160), (160, 200)]
PLANTED = [(16, 24, 12, 6, 0.4, 0.9, 0), (44, 22, 6, 14, -0.3, 0.85, 1), (28, 42, 10, 5, 1.2, 0.8, 0), (50, 46, 8, 8, 0.1, 0.75, 1)]   # letterbox pixels of 64 x 64


def _toy_obb_detector(torch, x, t):
    """a synthetic cn_obb head (S, 4 + 2 + 1, 64): four well-separated boxes that drift and turn with t, everything else silent"""
    S = x.shape[0]
    pred = torch.zeros((S, 7, 64), dtype=torch.float32, device="cuda")
    pred[:, 0:2] = 32.0
    pred[:, 2:4] = 4.0
    for s in range(S):
        for k, (cx, cy, w, h, ang, cf, cls) in enumerate(PLANTED):
            a = 3 + 13 * k + s
            pred[s, :, a] = torch.tensor([cx + 0.5 * t + 0.25 * s, cy + 0.25 * t, w, h, cf if cls == 0 else 0.0, cf if cls == 1 else 0.0,
                                          ang + 0.03125 * t], device="cuda")
    return pred + 0 * x.float().mean()


def test_ring_letterbox_detpost_step_device_with_in_handle_oriented_reid(sd):
    """FrameRing.letterbox -> a synthetic cn_obb tensor -> DetPost(layout="cn_obb") -> step_device of an oriented ReID handle on the
    ring's frames: nothing leaves the device between the frame and the rows.  Row counts, ids and det indices equal those of a
    second handle given the same detections through update_batch with the host frames."""
    import torch
    from boxmot_amd.detpost import DetPost
    from boxmot_amd.ingest import FrameRing
    from boxmot_amd.streams import MultiStreamBotSort
    S, T = len(E2E_SIZES), 6
    ring = FrameRing(2, S, sizes=E2E_SIZES)
    post = DetPost(S, 64, 2, layout="cn_obb", conf=0.25, iou=0.45, max_det=ND, max_candidates=64)
    kw = dict(max_tracks=64, max_dets=ND, emb_dim=512, is_obb=True, reid_weights=sd, frame_sizes=E2E_SIZES)
    dev, host = MultiStreamBotSort(S, **kw), MultiStreamBotSort(S, **kw)
    dev.set_reid_mode(2); host.set_reid_mode(2)
    st = torch.cuda.current_stream()
    total = 0
    try:
        d_dets = torch.zeros((S, ND, 7), dtype=torch.float32, device="cuda")
        d_rows = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((S, ND, 9), dtype=torch.float32, device="cuda")
        d_out_n = torch.zeros(S, dtype=torch.int32, device="cuda")
        for t in range(T):
            slot = t % 2
            imgs = [_frame(r, c, 50 + s, t) for s, (r, c) in enumerate(E2E_SIZES)]
            ring.host_done(slot)
            for s in range(S):
                ring.host_view(slot, s)[...] = imgs[s]
            ring.submit(slot)
            x = torch.empty((S, 3, 64, 64), dtype=torch.float16, device="cuda")
            geo = ring.letterbox(slot, x, hip_stream=st.cuda_stream)
            post.run(_toy_obb_detector(torch, x, t), geo, d_dets, d_rows, hip_stream=st.cuda_stream)
            st.synchronize()
            dev.step_device(d_dets.data_ptr(), d_rows.data_ptr(), None, ring.device_frames(slot), 0, 0, d_out.data_ptr(), d_out_n.data_ptr())
            dev.synchronize()
            dets_h, n_h = d_dets.cpu().numpy(), d_rows.cpu().numpy()
            assert n_h.tolist() == [len(PLANTED)] * S, (t, n_h)
            want = host.update_batch([dets_h[s, :n_h[s]] for s in range(S)], imgs=imgs)
            out, out_n = d_out.cpu().numpy(), d_out_n.cpu().numpy()
            for s in range(S):
                w = np.asarray(want[s], dtype=np.float32).reshape(-1, 9)
                assert out_n[s] == len(w), (t, s, out_n[s], len(w))
                assert np.array_equal(out[s, :out_n[s], 5], w[:, 5]) and np.array_equal(out[s, :out_n[s], 8], w[:, 8]), (t, s)
                total += len(w)
        assert total >= S * len(PLANTED) * (T - 2)
        assert (dev.status() == 0).all()
    finally:
        torch.cuda.synchronize()
        dev.synchronize()
        ring.close(); post.close(); dev.close(); host.close()


# ---- 6. guards ----
def test_guards_of_an_oriented_reid_handle_are_the_axis_aligned_handles():
    """an oriented with_reid handle with neither weights nor embeddings fails with the axis-aligned handle's words (host update and
    device-resident step); reid_model_path at the creation of an oriented handle is still refused"""
    import torch
    from boxmot_amd import _lib
    from boxmot_amd.streams import MultiStreamBotSort
    img = np.zeros((64, 64, 3), np.uint8)
    msgs = {}
    for obb in (False, True):
        trk = MultiStreamBotSort(1, max_tracks=64, max_dets=8, emb_dim=512, is_obb=obb)
        d = np.array([[32, 32, 20, 10, 0.15, 0.95, 0]] if obb else [[22, 27, 42, 37, 0.95, 0]], dtype=np.float32)
        try:
            with pytest.raises(RuntimeError) as e1:
                trk.update_batch([d], imgs=[img])
            z = torch.zeros(8 * 9, dtype=torch.float32, device="cuda")
            n = torch.ones(1, dtype=torch.int32, device="cuda")
            with pytest.raises(RuntimeError) as e2:
                trk.step_device(z.data_ptr(), n.data_ptr(), None, None, 64, 64, z.data_ptr(), n.data_ptr())
            frames = torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda")
            ptrs = torch.tensor([frames.data_ptr()], dtype=torch.int64, device="cuda")
            with pytest.raises(RuntimeError) as e3:
                trk.step_device(z.data_ptr(), n.data_ptr(), None, ptrs.data_ptr(), 64, 64, z.data_ptr(), n.data_ptr())
            msgs[obb] = (str(e1.value), str(e2.value), str(e3.value))
        finally:
            torch.cuda.synchronize()
            trk.close()
    assert msgs[True] == msgs[False]
    assert "no ReID weights" in msgs[True][0] and "d_embs or d_frames" in msgs[True][1] and "no ReID weights" in msgs[True][2]
    lib = _lib.load()
    cfg = _lib.BotSortConfig()
    lib.boxmot_hip_botsort_default_config(ctypes.byref(cfg))
    cfg.max_tracks, cfg.max_dets, cfg.emb_dim, cfg.is_obb, cfg.with_reid = 64, 32, 512, 1, 1
    cfg.reid_model_path = b"/nonexistent/weights.bin"
    assert not lib.boxmot_hip_botsort_create(ctypes.byref(cfg)) and "oriented" in _lib.last_error()
