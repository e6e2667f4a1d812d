"""Frames of different sizes in one ReID pass (HipReID.get_features_batch, the `_sized` table-form kernels) against the same boxes
run per image (get_features, the scalar-form kernels).  Every comparison between the two is EXACT: the mixed pass and the uniform
pass run the same instructions on the same operands per crop, so there is no tolerance to choose.  Frames are seeded noise on a
smooth gradient; every box and every size is valid."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(480, 640), (487, 651), (720, 1280), (1080, 1920), (2160, 3840)]       # (rows, cols); 651: rows at every dword offset
TOL = 1e-3          # tests/test_gpu_reid.py: embeddings within 1e-3 of the fp32 oracle (BASELINE.json north_star)


def _frame(rows, cols, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    g = np.stack([x * 200.0 / cols, y * 200.0 / rows, (x + y) * 200.0 / (rows + cols)], axis=2)
    return np.ascontiguousarray(np.clip(g + rng.integers(0, 56, (rows, cols, 3)), 0, 255).astype(np.uint8))


def _boxes(rows, cols):
    """interior, clipped by each of the frame's own four borders, the resampler's special cases, the whole frame, and a box that is
    interior in a larger frame but clipped (or outside) in the smaller ones"""
    W, H = float(cols), float(rows)
    b = [[0.1 * W + 0.2, 0.2 * H + 0.7, 0.3 * W + 0.1, 0.7 * H + 0.3],
         [-20.0, 0.3 * H, 50.4, 0.6 * H],
         [0.4 * W, -15.5, 0.5 * W, 100.2],
         [W - 60.4, 0.2 * H, W + 30.0, 0.5 * H],
         [0.5 * W, H - 80.7, 0.6 * W, H + 25.0],
         [10, 10, 138, 266],
         [20, 8, 276, 520],
         [0, 0, W, H],
         [0.6 * W, 0.1 * H, 0.7 * W, 0.4 * H]]
    if rows <= 487:
        b.append([600.3, 300.2, 900.6, 700.1])               # interior in 1080 x 1920, clipped right and bottom here
    elif rows == 720:
        b.append([1100.3, 500.2, 1500.6, 900.1])
    elif rows == 1080:
        b.append([1800.2, 900.4, 2400.1, 1500.3])            # interior in 2160 x 3840
    else:
        b.append([3000.2, 1500.4, 3300.1, 2100.3])
    return np.array(b, dtype=np.float32)


def _obb_boxes(rows, cols):
    W, H = float(cols), float(rows)
    return np.array([[0.3 * W, 0.4 * H, 80.3, 190.2, 0.3], [0.5 * W, 0.5 * H, 120.0, 260.5, -0.8], [10.0, 20.0, 90.0, 150.0, 1.2],
                     [W - 15.0, H - 30.0, 100.0, 220.0, 0.1], [0.7 * W, 0.2 * H, 60.0, 60.0, 0.0], [0.2 * W, 0.8 * H, 45.5, 130.0, 2.0],
                     [0.5 * W, 5.0, 70.0, 140.0, -0.2], [5.0, 0.5 * H, 64.0, 128.0, 0.6]], dtype=np.float32)


@pytest.fixture(scope="module")
def frames():
    return [_frame(r, c, 21 + k) for k, (r, c) in enumerate(SIZES)]


def _compare(reid, boxes_list, frames, what):
    got = reid.get_features_batch(boxes_list, frames)
    assert len(got) == len(frames)
    for k, (b, im) in enumerate(zip(boxes_list, frames)):
        want = reid.get_features(b, im)
        assert got[k].shape == (len(b), reid.feature_dim) and got[k].dtype == np.float32
        bad = np.flatnonzero((got[k] != want).any(axis=1))
        print(f"{what}: frame {im.shape[0]}x{im.shape[1]}: {len(b)} boxes, {len(bad)} rows differ"
              + (f", max|diff| {np.abs(got[k] - want).max():.3e}" if len(bad) else ""))
        assert np.array_equal(got[k], want), (what, k, bad)
    return got


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_osnet_x025_batch_of_five_frame_sizes_equals_per_image_features(frames, mode):
    from boxmot_amd.reid import HipReID
    from boxmot_amd.reid_weights import random_osnet_state_dict, reference_init_state_dict
    from oracle.osnet import OracleReID

    sd = reference_init_state_dict("osnet_x0_25", seed=0) if mode == 1 else random_osnet_state_dict("osnet_x0_25", seed=0)
    reid = HipReID(sd, max_crops=64, mode=mode)
    boxes_list = [_boxes(r, c) for r, c in SIZES]
    try:
        got = _compare(reid, boxes_list, frames, f"osnet_x0_25 mode {mode}")
        # an image without boxes in the middle of the batch, and frames given in another order
        boxes2 = [boxes_list[4], np.zeros((0, 4), np.float32), boxes_list[0], boxes_list[3]]
        frames2 = [frames[4], frames[2], frames[0], frames[3]]
        got2 = reid.get_features_batch(boxes2, frames2)
        assert got2[1].shape == (0, reid.feature_dim)
        assert np.array_equal(got2[0], got[4]) and np.array_equal(got2[2], got[0]) and np.array_equal(got2[3], got[3])
        # frames of ONE size take the scalar-form kernels: the same answer again
        same = reid.get_features_batch([boxes_list[2], boxes_list[2][::-1]], [frames[2], frames[2]])
        assert np.array_equal(same[0], got[2]) and np.array_equal(same[1], got[2][::-1])
        if mode == 2:
            orc = OracleReID(sd)
            for k, (b, im) in enumerate(zip(boxes_list, frames)):
                err = float(np.abs(got[k] - orc.get_features(b, im)).max())
                print(f"mode 2 vs the fp32 oracle, frame {im.shape[0]}x{im.shape[1]}: max|diff| {err:.2e}")
                assert err < TOL, (k, err)
    finally:
        reid.close()


def test_batch_crops_equal_per_image_crops_and_the_oracle(frames):
    """crop level, so that a crop error is told apart from a backbone one: both preprocess modes"""
    from boxmot_amd.reid import HipReID
    from boxmot_amd.reid_weights import random_osnet_state_dict
    from oracle.crops import get_crops

    boxes_list = [_boxes(r, c) for r, c in SIZES]
    for pre in ("resize", "resize_pad"):
        reid = HipReID(random_osnet_state_dict("osnet_x0_25", seed=0), max_crops=64, preprocess=pre)
        try:
            got = reid.get_crops_batch(boxes_list, frames)
            for k, (b, im) in enumerate(zip(boxes_list, frames)):
                assert np.array_equal(got[k], reid.get_crops(b, im)), (pre, k)
                assert np.array_equal(got[k], get_crops(b, im, preprocess=pre)), (pre, k)
        finally:
            reid.close()


def test_batch_larger_than_the_engine_runs_in_passes(frames):
    """50 boxes through a 16-crop engine: four passes, each with crops of several frames"""
    from boxmot_amd.reid import HipReID
    from boxmot_amd.reid_weights import random_osnet_state_dict

    reid = HipReID(random_osnet_state_dict("osnet_x0_25", seed=1), max_crops=16, mode=2)
    try:
        _compare(reid, [_boxes(r, c) for r, c in SIZES], frames, "mode 2, 16-crop engine")
    finally:
        reid.close()


def test_resize_pad_batch_equals_per_image_features(frames):
    from boxmot_amd.reid import HipReID
    from boxmot_amd.reid_weights import random_osnet_state_dict

    for mode in (1, 2):         # the separate crop kernels in the stem's RGBX and (hi, lo) layouts
        reid = HipReID(random_osnet_state_dict("osnet_x0_25", seed=2), max_crops=64, mode=mode, preprocess="resize_pad")
        try:
            _compare(reid, [_boxes(r, c) for r, c in SIZES], frames, f"resize_pad mode {mode}")
        finally:
            reid.close()


def test_oriented_boxes_batch_equals_per_image_features(frames):
    from boxmot_amd.reid import HipReID
    from boxmot_amd.reid_weights import reference_init_state_dict

    for mode in (0, 1):         # (mode 2 takes axis-aligned boxes only)
        reid = HipReID(reference_init_state_dict("osnet_x0_25", seed=0), max_crops=64, mode=mode)
        try:
            _compare(reid, [_obb_boxes(r, c) for r, c in SIZES], frames, f"oriented, mode {mode}")
        finally:
            reid.close()


def test_osnet_x1_0_fp32_grade_batch_equals_per_image_features(frames):
    from boxmot_amd.reid import HipReID
    from boxmot_amd.reid_weights import random_osnet_state_dict

    reid = HipReID(random_osnet_state_dict("osnet_x1_0", seed=0), max_crops=64, mode=2)
    try:
        _compare(reid, [_boxes(r, c) for r, c in SIZES], frames, "osnet_x1_0 mode 2")
    finally:
        reid.close()


def test_clipreid_batch_equals_per_image_features(frames):
    from boxmot_amd.clip_weights import pack_clipreid, random_clipreid_state_dict
    from boxmot_amd.reid import HipReID

    reid = HipReID(pack_clipreid(random_clipreid_state_dict(0)), max_crops=16)
    try:
        _compare(reid, [_boxes(r, c)[:8] for r, c in SIZES], frames, "CLIP-ReID")
    finally:
        reid.close()


# ---- tracker handles: streams of different frame sizes in ONE MultiStreamBotSort against one uniform handle per size ----
N_FRAMES = 40


def _scenes():
    from boxmot_amd.scenario import Scenario
    return [Scenario(n_dets=16, n_tracks=32, width=SIZES[s // 2][1], height=SIZES[s // 2][0], stream=s) for s in range(10)]


def _image(sc, t):
    """the scene's frame, moved a little from frame to frame (so that camera-motion estimation has something to find)"""
    return np.ascontiguousarray(np.roll(sc.image, (t % 3, 2 * (t % 2)), axis=(0, 1)))


def _trackers(cmc_method=None, frame_sizes=None):
    from boxmot_amd.reid_weights import random_osnet_state_dict
    from boxmot_amd.streams import MultiStreamBotSort
    sd = random_osnet_state_dict("osnet_x0_25", seed=0)
    kw = dict(max_tracks=64, max_dets=32, emb_dim=512, reid_weights=sd, cmc_method=cmc_method)
    mixed = MultiStreamBotSort(10, frame_sizes=frame_sizes, **kw)
    uniform = [MultiStreamBotSort(2, **kw) for _ in range(5)]
    for t in [mixed] + uniform:
        t.set_reid_mode(2)          # the uniform path crops inside the fused stem: the table-form stem is what is compared
    return mixed, uniform


def _same_state(mixed, uniform, streams=range(10)):
    for s in streams:
        a, b = mixed.state_dump(s), uniform[s // 2].state_dump(s % 2)
        assert a["n"] == b["n"] and a["frame_count"] == b["frame_count"] and a["id_count"] == b["id_count"], s
        for key in ("ints", "kf", "smooth", "misc"):
            assert np.array_equal(a[key], b[key]), (s, key)


def _close(mixed, uniform):
    for t in [mixed] + uniform:
        t.close()


@pytest.mark.parametrize("cmc_method", [None, "ecc", "sof"])
def test_ten_mixed_streams_in_one_handle_equal_five_uniform_handles_host_frames(cmc_method):
    """host update_batch(imgs=...): rows, state_dump ints, Kalman state and smoothed features of every stream, exactly; with
    cmc_method the handle estimates the warps itself (one estimator per distinct size), so equal rows and Kalman state are equal warps"""
    import time
    scenes = _scenes()
    mixed, uniform = _trackers(cmc_method)
    try:
        t_mixed = t_uniform = 0.0
        for t in range(N_FRAMES):
            dets = [sc.frame(t)[0] for sc in scenes]
            imgs = [_image(sc, t) for sc in scenes]
            t0 = time.perf_counter()
            got = mixed.update_batch(dets, imgs=imgs)
            t1 = time.perf_counter()
            want = []
            for k, u in enumerate(uniform):
                want += u.update_batch(dets[2 * k:2 * k + 2], imgs=imgs[2 * k:2 * k + 2])
            t2 = time.perf_counter()
            if t >= 5:
                t_mixed += t1 - t0; t_uniform += t2 - t1
            for s in range(10):
                assert np.array_equal(np.asarray(got[s]), np.asarray(want[s])), (t, s)
        _same_state(mixed, uniform)
        print(f"cmc={cmc_method}: frames 5..{N_FRAMES - 1}, 10 streams: one mixed handle {t_mixed * 1e3:.1f} ms, five uniform handles {t_uniform * 1e3:.1f} ms (host wall time, a measurement)")
    finally:
        _close(mixed, uniform)


def test_ten_mixed_streams_through_a_mixed_frame_ring_equal_five_uniform_handles():
    from boxmot_amd.ingest import FrameRing
    scenes = _scenes()
    sizes = [SIZES[s // 2] for s in range(10)]
    mixed, uniform = _trackers()
    ring = FrameRing(2, 10, sizes=sizes)
    try:
        with pytest.raises(ValueError):
            ring.host_view(0)
        for t in range(N_FRAMES):
            dets = [sc.frame(t)[0] for sc in scenes]
            imgs = [_image(sc, t) for sc in scenes]
            slot = t % 2
            ring.host_done(slot)
            for s in range(10):
                v = ring.host_view(slot, s)
                assert v.shape == sizes[s] + (3,)
                v[...] = imgs[s]
            del v
            ring.submit(slot)
            got = mixed.update_batch(dets, ring=ring, slot=slot)
            want = []
            for k, u in enumerate(uniform):
                want += u.update_batch(dets[2 * k:2 * k + 2], imgs=imgs[2 * k:2 * k + 2])
            for s in range(10):
                assert np.array_equal(np.asarray(got[s]), np.asarray(want[s])), (t, s)
        _same_state(mixed, uniform)
    finally:
        mixed.synchronize()
        ring.close()
        _close(mixed, uniform)


def test_declared_frame_sizes_and_a_stream_that_changes_size():
    """frame_sizes= up front gives the same tracks; a stream whose frame changes size at frame 3 gets a ValueError naming it before
    anything is stepped (the call is atomic by design: every frame is checked before any pointer goes down); the frame is then
    sent with the right image and every stream still matches its uniform handle"""
    scenes = _scenes()
    mixed, uniform = _trackers(frame_sizes=[SIZES[s // 2] for s in range(10)])
    try:
        with pytest.raises(RuntimeError, match="stream 3: frame size changed"):
            r = np.array([sz[0] for sz in [SIZES[s // 2] for s in range(10)]], np.int32)
            c = np.array([sz[1] for sz in [SIZES[s // 2] for s in range(10)]], np.int32)
            r[3] += 1
            from boxmot_amd import _lib
            _lib.check(mixed._lib.boxmot_hip_botsort_set_frame_sizes(mixed._handle, r.ctypes.data, c.ctypes.data, 10))
        for t in range(12):
            dets = [sc.frame(t)[0] for sc in scenes]
            imgs = [_image(sc, t) for sc in scenes]
            if t == 3:
                bad = list(imgs)
                bad[4] = np.zeros((100, 200, 3), np.uint8)
                with pytest.raises(ValueError, match="stream 4"):
                    mixed.update_batch(dets, imgs=bad)
            got = mixed.update_batch(dets, imgs=imgs)
            want = []
            for k, u in enumerate(uniform):
                want += u.update_batch(dets[2 * k:2 * k + 2], imgs=imgs[2 * k:2 * k + 2])
            for s in range(10):
                assert np.array_equal(np.asarray(got[s]), np.asarray(want[s])), (t, s)
        _same_state(mixed, uniform)
    finally:
        _close(mixed, uniform)


def test_ten_mixed_streams_step_device_with_frames_equal_five_uniform_handles():
    """the device-resident step (no host image in the call: sizes declared with frame_sizes=, the scalar rows / cols unused) against
    uniform handles stepped the same way with their one size"""
    import torch
    scenes = _scenes()
    sizes = [SIZES[s // 2] for s in range(10)]
    mixed, uniform = _trackers(frame_sizes=sizes)
    dev = torch.device("cuda:0")
    nd, T = 32, N_FRAMES
    dets_h, cnt_h = np.zeros((T, 10, nd, 6), np.float32), np.zeros((T, 10), np.int32)
    for s, sc in enumerate(scenes):
        for t in range(T):
            d = sc.frame(t)[0]
            dets_h[t, s, : len(d)] = d
            cnt_h[t, s] = len(d)
    d_dets, d_cnt = torch.from_numpy(dets_h).to(dev), torch.from_numpy(cnt_h).to(dev)
    frames = [torch.from_numpy(sc.image).to(dev) for sc in scenes]
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
    out_m, n_m = torch.zeros((T, 10, nd, 8), device=dev), torch.zeros((T, 10), dtype=torch.int32, device=dev)
    out_u, n_u = torch.zeros((T, 10, nd, 8), device=dev), torch.zeros((T, 10), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    try:
        for t in range(T):
            mixed.step_device(d_dets[t].data_ptr(), d_cnt[t].data_ptr(), None, ptrs.data_ptr(), 0, 0, out_m[t].data_ptr(), n_m[t].data_ptr())
            for k, u in enumerate(uniform):
                u.step_device(d_dets[t, 2 * k].data_ptr(), d_cnt[t, 2 * k:].data_ptr(), None, ptrs[2 * k:].data_ptr(), SIZES[k][0], SIZES[k][1],
                              out_u[t, 2 * k].data_ptr(), n_u[t, 2 * k:].data_ptr())
        for trk in [mixed] + uniform:
            trk.synchronize()
            assert (trk.status() == 0).all()
        assert np.array_equal(n_m.cpu().numpy(), n_u.cpu().numpy()) and int(n_m.sum()) > 0
        assert np.array_equal(out_m.cpu().numpy(), out_u.cpu().numpy())
        _same_state(mixed, uniform)
    finally:
        _close(mixed, uniform)


def test_oriented_streams_of_three_sizes_with_handle_owned_sof_equal_uniform_handles():
    """is_obb=True: the estimator of each size sees the enclosing boxes of that stream's oriented detections"""
    from boxmot_amd.streams import MultiStreamBotSort
    from common import obb_frames
    sizes3 = [SIZES[0], SIZES[2], SIZES[3]]
    sizes = [sizes3[s // 2] for s in range(6)]
    kw = dict(max_tracks=128, max_dets=64, emb_dim=1, is_obb=True, with_reid=False, cmc_method="sof")
    mixed = MultiStreamBotSort(6, **kw)
    uniform = [MultiStreamBotSort(2, **kw) for _ in range(3)]
    base = [np.random.default_rng(40 + s).integers(0, 255, sizes[s] + (3,), dtype=np.uint8) for s in range(6)]
    seqs = [list(obb_frames(30, seed=6 + s)) for s in range(6)]
    try:
        for t in range(30):
            dets = [seqs[s][t] for s in range(6)]
            imgs = [np.ascontiguousarray(np.roll(base[s], (t % 5, 2 * (t % 3)), axis=(0, 1))) for s in range(6)]
            got = mixed.update_batch(dets, imgs=imgs)
            want = []
            for k, u in enumerate(uniform):
                want += u.update_batch(dets[2 * k:2 * k + 2], imgs=imgs[2 * k:2 * k + 2])
            for s in range(6):
                assert np.asarray(got[s]).shape[1] == 9
                assert np.array_equal(np.asarray(got[s]), np.asarray(want[s])), (t, s)
        for s in range(6):
            a, b = mixed.state_dump(s), uniform[s // 2].state_dump(s % 2)
            assert a["n"] == b["n"] and np.array_equal(a["ints"], b["ints"]) and np.array_equal(a["kf"], b["kf"]), s
    finally:
        _close(mixed, uniform)


# ---- DeepOCSORT and StrongSORT handles through the C ABI: 3 sizes x 2 streams x 20 frames, mixed against uniform ----
class _AbiHandle:
    def __init__(self, kind, n_streams, blob_path, asso_func=None):
        import ctypes

        from boxmot_amd import _lib
        self.kind, self.S, self.lib = kind, n_streams, _lib.load()
        cfg = (_lib.DeepOcSortConfig if kind == "deepocsort" else _lib.StrongSortConfig)()
        getattr(self.lib, f"boxmot_hip_{kind}_default_config")(ctypes.byref(cfg))
        cfg.n_streams, cfg.max_tracks, cfg.max_dets, cfg.emb_dim = n_streams, 64, 32, 512
        cfg.reid_model_path = blob_path.encode()
        if kind == "deepocsort":
            cfg.cmc_off = 1
            if asso_func is not None:
                cfg.asso_func = asso_func
        self.h = getattr(self.lib, f"boxmot_hip_{kind}_create")(ctypes.byref(cfg))
        assert self.h, _lib.last_error()
        _lib.check(getattr(self.lib, f"boxmot_hip_{kind}_set_reid_mode")(self.h, 2))

    def set_sizes(self, sizes):
        r = np.array([sz[0] for sz in sizes], np.int32)
        c = np.array([sz[1] for sz in sizes], np.int32)
        return getattr(self.lib, f"boxmot_hip_{self.kind}_set_frame_sizes")(self.h, r.ctypes.data, c.ctypes.data, len(sizes))

    def update_batch(self, dets, imgs, rows, cols):
        import ctypes

        from boxmot_amd import _lib
        S = len(dets)
        dets = [np.ascontiguousarray(d, np.float32) for d in dets]
        n = np.array([len(d) for d in dets], np.int32)
        dp = (ctypes.c_void_p * S)(*[d.ctypes.data for d in dets])
        ip = (ctypes.c_void_p * S)(*[im.ctypes.data for im in imgs])
        outs = [np.zeros((64, 9), np.float32) for _ in range(S)]
        op = (ctypes.c_void_p * S)(*[o.ctypes.data for o in outs])
        on = np.zeros(S, np.int32)
        _lib.check(getattr(self.lib, f"boxmot_hip_{self.kind}_update_batch")(self.h, S, dp, n.ctypes.data, None, 0, ip, rows, cols, 3, op, 64, on.ctypes.data))
        return [o[:k].copy() for o, k in zip(outs, on)]

    def step_frames(self, d_dets, d_n, ptrs, rows, cols, d_out, d_out_n):
        from boxmot_amd import _lib
        _lib.check(getattr(self.lib, f"boxmot_hip_{self.kind}_step_device_frames")(self.h, d_dets, d_n, ptrs, rows, cols, d_out, d_out_n))

    def sync(self):
        from boxmot_amd import _lib
        _lib.check(getattr(self.lib, f"boxmot_hip_{self.kind}_synchronize")(self.h))

    def close(self):
        getattr(self.lib, f"boxmot_hip_{self.kind}_destroy")(self.h)


@pytest.fixture(scope="module")
def blob_path(tmp_path_factory):
    from boxmot_amd.reid_weights import pack_osnet, random_osnet_state_dict, save_blob
    p = str(tmp_path_factory.mktemp("blob") / "x025.reidblob")
    save_blob(pack_osnet(random_osnet_state_dict("osnet_x0_25", seed=0)), p)
    return p


SIZES3 = [SIZES[0], SIZES[2], SIZES[3]]


@pytest.mark.parametrize("kind", ["deepocsort", "strongsort"])
def test_deepocsort_and_strongsort_mixed_handle_equals_uniform_handles_host_and_device(kind, blob_path):
    import torch

    from boxmot_amd.scenario import Scenario
    sizes = [SIZES3[s // 2] for s in range(6)]
    T, nd = 20, 32
    dev = torch.device("cuda:0")
    for path in ("update_batch", "step_device_frames"):
        scenes = [Scenario(n_dets=16, n_tracks=32, width=sizes[s][1], height=sizes[s][0], stream=s) for s in range(6)]
        mixed = _AbiHandle(kind, 6, blob_path)
        uniform = [_AbiHandle(kind, 2, blob_path) for _ in range(3)]
        try:
            assert mixed.set_sizes(sizes) == 1
            if path == "update_batch":
                for t in range(T):
                    dets = [sc.frame(t)[0] for sc in scenes]
                    imgs = [_image(sc, t) for sc in scenes]
                    got = mixed.update_batch(dets, imgs, 0, 0)
                    for k, u in enumerate(uniform):
                        want = u.update_batch(dets[2 * k:2 * k + 2], imgs[2 * k:2 * k + 2], SIZES3[k][0], SIZES3[k][1])
                        for j in range(2):
                            assert len(got[2 * k + j]) > 0 or t < 3
                            assert np.array_equal(got[2 * k + j], want[j]), (kind, path, t, 2 * k + j)
            else:
                frames = [torch.from_numpy(sc.image).to(dev) for sc in scenes]
                ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
                dets_h, cnt_h = np.zeros((T, 6, nd, 6), np.float32), np.zeros((T, 6), np.int32)
                for s, sc in enumerate(scenes):
                    for t in range(T):
                        d = sc.frame(t)[0]
                        dets_h[t, s, : len(d)] = d
                        cnt_h[t, s] = len(d)
                d_dets, d_cnt = torch.from_numpy(dets_h).to(dev), torch.from_numpy(cnt_h).to(dev)
                out_m, n_m = torch.zeros((T, 6, 64, 8), device=dev), torch.zeros((T, 6), dtype=torch.int32, device=dev)
                out_u, n_u = torch.zeros((T, 6, 64, 8), device=dev), torch.zeros((T, 6), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                for t in range(T):
                    mixed.step_frames(d_dets[t].data_ptr(), d_cnt[t].data_ptr(), ptrs.data_ptr(), 0, 0, out_m[t].data_ptr(), n_m[t].data_ptr())
                    for k, u in enumerate(uniform):
                        u.step_frames(d_dets[t, 2 * k].data_ptr(), d_cnt[t, 2 * k:].data_ptr(), ptrs[2 * k:].data_ptr(), SIZES3[k][0], SIZES3[k][1],
                                      out_u[t, 2 * k].data_ptr(), n_u[t, 2 * k:].data_ptr())
                for hnd in [mixed] + uniform:
                    hnd.sync()
                assert np.array_equal(n_m.cpu().numpy(), n_u.cpu().numpy()) and int(n_m.sum()) > 0
                assert np.array_equal(out_m.cpu().numpy(), out_u.cpu().numpy()), (kind, path)
        finally:
            for hnd in [mixed] + uniform:
                hnd.close()


def test_centroid_is_refused_on_a_mixed_deepocsort_handle_and_streams_are_named(blob_path):
    """asso_func centroid normalises by ONE frame diagonal per handle: sizes that differ are refused with a message that says so;
    one size is accepted; a stream whose declared size changes is named"""
    from boxmot_amd import _lib
    h = _AbiHandle("deepocsort", 4, blob_path, asso_func=5)           # BOXMOT_HIP_ASSO_CENTROID
    try:
        assert h.set_sizes([SIZES[0], SIZES[0], SIZES[2], SIZES[2]]) == 0
        msg = _lib.last_error()
        assert "centroid" in msg and "stream 2" in msg and "one handle per size" in msg
        assert h.set_sizes([SIZES[2]] * 4) == 1
        assert h.set_sizes([SIZES[2], SIZES[2], SIZES[3], SIZES[2]]) == 0
        assert "centroid" in _lib.last_error()
    finally:
        h.close()
    for kind in ("deepocsort", "strongsort"):
        h = _AbiHandle(kind, 3, blob_path)
        try:
            assert h.set_sizes([SIZES[0], SIZES[2]]) == 0 and "per stream of the handle (3)" in _lib.last_error()
            assert h.set_sizes([SIZES[0], SIZES[2], SIZES[3]]) == 1
            assert h.set_sizes([SIZES[0], SIZES[3], SIZES[3]]) == 0 and "stream 1: frame size changed" in _lib.last_error()
        finally:
            h.close()
