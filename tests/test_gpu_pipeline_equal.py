"""The two-stage ReID pipeline of the device-resident steps (HandleCore in csrc/boxmot_hip.hip: the ReID pass of frame t + 1 on its
own HIP stream while the frame step of frame t runs, alternating embedding tables) must not change what a tracker returns.

tests/test_gpu_long_parity.py covers the pipelined path for DeepOCSORT.  Here: BoT-SORT (``MultiStreamBotSort.step_device`` with
``d_embs=None`` and device frames) and StrongSORT (``boxmot_hip_strongsort_step_device_frames``), each built once with
BOXMOT_HIP_PIPELINE=1 and once with =0 (read at create).  2 streams x 12 detections, max_tracks 64, max_dets 32, one 320 x 240
random frame per stream, OSNet-x0.25 (random_osnet_state_dict seed 0) in ReID mode 2, 24 frames queued with no synchronisation and
one synchronise at the end.  After frame 11 ``reserve(max_dets=96)`` re-makes the per-frame tables and the engine while the
pipeline is live (max_dets becomes 128: the detection rows of the later frames are laid out for it).

The comparison is bit equality of the row counts and of every row of all 24 frames.  The crop list's order comes from an atomic and
may vary from run to run, but every crop's embedding is computed from its own frame and box alone and written to the row crop_row
names, so the embedding tables -- and with them the deterministic frame steps -- do not depend on that order
(tests/test_gpu_mixed_sizes.py compares such passes bit for bit as well).  Measured on the parent of the change that introduced
HandleCore: two runs of one setting were bit-equal for both trackers and both settings, and so were the pipelined and the
unpipelined build -- hence bit equality here, not the looser convention of smoke()."""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, N_DETS, CAP, ND0, ND1, T, GROW_AFTER = 2, 12, 64, 32, 128, 24, 11
ROWS, COLS = 240, 320


def _nd(t):
    return ND0 if t <= GROW_AFTER else ND1


@functools.lru_cache(maxsize=None)
def _scene():
    """(frames [S][240][320][3] uint8, per frame t the detections [S][max_dets of that frame][6], counts [T][S]) -- made once."""
    from boxmot_amd.scenario import Scenario
    scs = [Scenario(N_DETS, 24, width=COLS, height=ROWS, emb_dim=8, stream=s, random_image=True) for s in range(S)]
    dets = [np.zeros((S, _nd(t), 6), np.float32) for t in range(T)]
    cnt = np.zeros((T, S), np.int32)
    for s, sc in enumerate(scs):
        for t in range(T):
            d, _ = sc.frame(t, with_embs=False)
            dets[t][s, : len(d)] = d
            cnt[t, s] = len(d)
    return np.stack([sc.image for sc in scs]), dets, cnt


@functools.lru_cache(maxsize=None)
def _weights():
    from boxmot_amd.reid_weights import random_osnet_state_dict
    return random_osnet_state_dict("osnet_x0_25", seed=0)


def _device_inputs(out_rows):
    """Device copies of the scene and one result table per frame: out_rows(t) rows per stream."""
    import torch
    dev = torch.device("cuda:0")
    images, dets, cnt = _scene()
    frames = torch.from_numpy(images).to(dev)
    ptrs = torch.tensor([frames[s].data_ptr() for s in range(S)], dtype=torch.int64, device=dev)
    d_dets = [torch.from_numpy(d).to(dev) for d in dets]
    d_cnt = torch.from_numpy(cnt).to(dev)
    d_out = [torch.zeros((S, out_rows(t), 8), dtype=torch.float32, device=dev) for t in range(T)]
    d_out_n = torch.zeros((T, S), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    return frames, ptrs, d_dets, d_cnt, d_out, d_out_n


def _rows(d_out, d_out_n):
    cnt = d_out_n.cpu().numpy()
    return cnt, [[d_out[t][s, : cnt[t, s]].cpu().numpy() for s in range(S)] for t in range(T)]


def run_botsort():
    from boxmot_amd.streams import MultiStreamBotSort
    from boxmot_amd.tracker_zoo import BOTSORT_YAML_DEFAULTS
    kw = {k: v for k, v in BOTSORT_YAML_DEFAULTS.items() if k not in ("use_cmc", "cmc_method")}
    frames, ptrs, d_dets, d_cnt, d_out, d_out_n = _device_inputs(_nd)       # result rows: [S][max_dets]
    ms = MultiStreamBotSort(S, max_tracks=CAP, max_dets=ND0, emb_dim=512, reid_weights=_weights(), **kw)
    try:
        ms.set_reid_mode(2)
        for t in range(T):
            ms.step_device(d_dets[t].data_ptr(), d_cnt[t].data_ptr(), None, ptrs.data_ptr(), ROWS, COLS, d_out[t].data_ptr(), d_out_n[t].data_ptr())
            if t == GROW_AFTER:
                ms.reserve(max_dets=96)
                assert ms.capacity()[:2] == (CAP, ND1)
        ms.synchronize()
        assert (ms.status() == 0).all()
        return _rows(d_out, d_out_n)
    finally:
        ms.close()


def run_strongsort():
    from boxmot_amd import _lib
    from boxmot_amd.reid_weights import pack_osnet, save_blob
    lib = _lib.load()
    fd, path = tempfile.mkstemp(suffix=".reidblob")
    os.close(fd)
    save_blob(pack_osnet(_weights()), path)
    cfg = _lib.StrongSortConfig()
    lib.boxmot_hip_strongsort_default_config(ctypes.byref(cfg))
    cfg.n_streams, cfg.max_tracks, cfg.max_dets, cfg.emb_dim = S, CAP, ND0, 512
    cfg.reid_model_path = path.encode()
    h = lib.boxmot_hip_strongsort_create(ctypes.byref(cfg))
    os.unlink(path)
    assert h, _lib.last_error()
    try:
        _lib.check(lib.boxmot_hip_strongsort_set_reid_mode(h, 2))
        frames, ptrs, d_dets, d_cnt, d_out, d_out_n = _device_inputs(lambda t: CAP)     # result rows: [S][max_tracks]
        for t in range(T):
            _lib.check(lib.boxmot_hip_strongsort_step_device_frames(h, d_dets[t].data_ptr(), d_cnt[t].data_ptr(), ptrs.data_ptr(), ROWS, COLS,
                                                                    d_out[t].data_ptr(), d_out_n[t].data_ptr()))
            if t == GROW_AFTER:
                _lib.check(lib.boxmot_hip_strongsort_reserve(h, 0, 96))
                cap, nd = ctypes.c_int(0), ctypes.c_int(0)
                _lib.check(lib.boxmot_hip_strongsort_capacity(h, ctypes.byref(cap), ctypes.byref(nd), None))
                assert (cap.value, nd.value) == (CAP, ND1)
        _lib.check(lib.boxmot_hip_strongsort_synchronize(h))      # (reports a step whose crops exceeded a declared bound; none is declared)
        # the library has no entry point for StrongSORT's status words: a track table that never filled (births are clamped at
        # max_tracks, the one overflow this scene could reach) is what can be read
        for s in range(S):
            n_tracks = ctypes.c_int(0)
            _lib.check(lib.boxmot_hip_strongsort_track_count(h, s, ctypes.byref(n_tracks)))
            assert 0 < n_tracks.value < CAP
        return _rows(d_out, d_out_n)
    finally:
        lib.boxmot_hip_strongsort_destroy(h)


RUNNERS = {"botsort": run_botsort, "strongsort": run_strongsort}


def differences(a, b):
    """Frames / streams whose row count or rows differ between two runs: [(t, s, what)]."""
    (cnt_a, rows_a), (cnt_b, rows_b) = a, b
    bad = []
    for t in range(T):
        for s in range(S):
            if cnt_a[t, s] != cnt_b[t, s]:
                bad.append((t, s, f"{cnt_a[t, s]} rows against {cnt_b[t, s]}"))
            elif not np.array_equal(rows_a[t][s], rows_b[t][s]):
                bad.append((t, s, f"rows differ by up to {np.abs(rows_a[t][s] - rows_b[t][s]).max():.3g}"))
    return bad


@pytest.mark.parametrize("kind", ["botsort", "strongsort"])
def test_pipelined_and_unpipelined_builds_return_the_same_rows(kind, monkeypatch):
    monkeypatch.setenv("BOXMOT_HIP_PIPELINE", "1")
    piped = RUNNERS[kind]()
    monkeypatch.setenv("BOXMOT_HIP_PIPELINE", "0")
    plain = RUNNERS[kind]()
    assert piped[0].sum() > 0 and (piped[0][-1] > 0).all(), "the scene must produce tracks for the comparison to mean anything"
    assert differences(piped, plain) == []
