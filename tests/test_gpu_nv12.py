"""GPU tests of the NV12 ingest ring (include/boxmot_hip.h boxmot_hip_ingest_*nv12, boxmot_amd/ingest.py, csrc/ingest_nv12.hpp).
The conversion is integer arithmetic with one definition (tests/nv12_ref.py), so every comparison is EXACT: a differing byte, or a
differing result row, is a failure."""
import numpy as np
import pytest

from nv12_ref import bgr_to_nv12, exhaustive_frame, nv12_to_bgr as ref_nv12_to_bgr, random_frame

pytestmark = pytest.mark.gpu

# rows, cols, pitch_y, pitch_uv, byte offset of the Y / UV base past torch's alignment: the shapes of tests/test_nv12_emu.py
SHAPES = [
    (2, 2, 2, 2, 0, 0),
    (6, 10, 10, 10, 0, 0),
    (18, 34, 48, 40, 0, 0),
    (16, 64, 64, 64, 0, 0),
    (10, 72, 128, 128, 0, 0),
    (4, 520, 520, 520, 0, 0),
    (4, 130, 130, 130, 0, 0),
    (10, 6, 6, 6, 0, 0),
    (10, 1032, 1040, 1032, 0, 0),
    (8, 64, 68, 64, 0, 0),               # pitches that are no multiple of 8, and bases that are not 8-byte aligned: the 2 x 2 path
    (8, 64, 64, 100, 0, 0),
    (12, 136, 136, 136, 4, 0),
    (12, 136, 136, 136, 0, 2),
    (12, 136, 143, 141, 1, 3),
]


def test_every_yuv_triple_is_bit_exact():
    from boxmot_amd.ingest import nv12_to_bgr
    f = exhaustive_frame()
    got = nv12_to_bgr(f, 4096, 4096)
    want = ref_nv12_to_bgr(f, 4096, 4096)
    assert got.shape == want.shape == (4096, 4096, 3) and got.dtype == np.uint8
    bad = int((got != want).sum())
    print(f"exhaustive 4096 x 4096 frame: {bad} differing bytes of {want.size}")
    assert bad == 0


@pytest.mark.parametrize("rows,cols", sorted({(s[0], s[1]) for s in SHAPES}))
def test_small_shapes_through_an_nv12_ring(rows, cols):
    from boxmot_amd.ingest import nv12_to_bgr
    f = random_frame(rows, cols, rows * 1000 + cols)
    assert np.array_equal(nv12_to_bgr(f, rows, cols), ref_nv12_to_bgr(f, rows, cols))
    assert np.array_equal(nv12_to_bgr(f.reshape(-1), rows, cols), ref_nv12_to_bgr(f, rows, cols))       # the bytes flat


def _surface(torch, plane, pitch, offset):
    """a torch device buffer holding ``plane`` (2-D uint8) at row pitch ``pitch``, starting ``offset`` bytes into the allocation"""
    host = np.full(offset + plane.shape[0] * pitch, 0x5A, dtype=np.uint8)
    host[offset:].reshape(plane.shape[0], pitch)[:, :plane.shape[1]] = plane
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + offset


def test_pitched_and_misaligned_surfaces_through_submit_device_nv12():
    """all the shapes as the streams of ONE BGR ring: surfaces allocated through torch, pitches above cols, bases off alignment; one
    launch converts streams that take either path"""
    import torch
    from boxmot_amd.ingest import FrameRing
    frames = [random_frame(r, c, 77 + k) for k, (r, c, *_) in enumerate(SHAPES)]
    ring = FrameRing(2, len(SHAPES), sizes=[(r, c) for r, c, *_ in SHAPES])
    try:
        keep, yp, up = [], [], []
        for f, (r, c, py, pu, oy, ou) in zip(frames, SHAPES):
            ty, ay = _surface(torch, f[:r], py, oy)
            tu, au = _surface(torch, f[r:], pu, ou)
            keep += [ty, tu]; yp.append(ay); up.append(au)
        torch.cuda.synchronize()                                          # the surfaces are complete before the call
        ring.submit_device_nv12(1, yp, up, [s[2] for s in SHAPES], [s[3] for s in SHAPES])
        for k, (f, (r, c, *_)) in enumerate(zip(frames, SHAPES)):
            assert np.array_equal(ring.download(1, k), ref_nv12_to_bgr(f, r, c)), SHAPES[k]
    finally:
        ring.close()


SIZES = [(240, 320), (180, 256), (122, 166)]
T = 6


@pytest.fixture(scope="module")
def sequence():
    """three streams of different even sizes, 6 frames: detections, the NV12 frames (shifted per step, so a slot converted late or
    not at all changes the embeddings and the ids) and the rows of a handle fed host BGR frames = the reference conversion"""
    from boxmot_amd.reid_weights import reference_init_state_dict
    from boxmot_amd.scenario import Scenario
    from boxmot_amd.streams import MultiStreamBotSort
    sd = reference_init_state_dict("osnet_x0_25", seed=0)
    scs = [Scenario(10, 20, width=c, height=r, random_image=True, stream=s) for s, (r, c) in enumerate(SIZES)]
    base = [bgr_to_nv12(sc.image) for sc in scs]
    nv = [[np.roll(b, 8 * t, axis=1) for b in base] for t in range(T)]    # an even shift keeps the (U, V) pairs together
    dets = [[sc.frame(t, with_embs=False)[0] for sc in scs] for t in range(T)]
    a = MultiStreamBotSort(len(SIZES), max_tracks=64, max_dets=32, emb_dim=512, reid_weights=sd)
    a.set_reid_mode(1)
    want = []
    for t in range(T):
        imgs = [ref_nv12_to_bgr(f, r, c) for f, (r, c) in zip(nv[t], SIZES)]
        want.append([np.asarray(x).copy() for x in a.update_batch(dets[t], imgs=imgs)])
    a.close()
    assert sum(len(x) for x in want[-1]) > 0
    return dict(sd=sd, nv=nv, dets=dets, want=want)


def _tracker(sd):
    from boxmot_amd.streams import MultiStreamBotSort
    b = MultiStreamBotSort(len(SIZES), max_tracks=64, max_dets=32, emb_dim=512, reid_weights=sd)
    b.set_reid_mode(1)
    return b


def test_nv12_ring_equals_host_bgr_frames(sequence):
    from boxmot_amd.ingest import FrameRing
    b = _tracker(sequence["sd"])
    ring = FrameRing(3, len(SIZES), sizes=SIZES, fmt="nv12")
    assert ring.sizes == SIZES and ring.mixed

    def fill(slot, t):
        for s, f in enumerate(sequence["nv"][t]):
            v = ring.host_view(slot, s)
            assert v.shape == (SIZES[s][0] * 3 // 2, SIZES[s][1])
            v[...] = f
    try:
        fill(0, 0)
        ring.submit(0)
        for t in range(T):
            k, k1 = t % 3, (t + 1) % 3
            if t + 1 < T:                                   # slot t + 1 is submitted before slot t is tracked
                ring.host_done(k1)
                fill(k1, t + 1)
                ring.submit(k1)
            got = b.update_batch(sequence["dets"][t], ring=ring, slot=k)
            for s in range(len(SIZES)):
                assert np.array_equal(np.asarray(got[s]), sequence["want"][t][s]), (t, s)
    finally:
        b.synchronize()
        ring.close(); b.close()


def test_device_surfaces_on_a_bgr_ring_give_the_same_rows(sequence):
    import torch
    from boxmot_amd.ingest import FrameRing
    b = _tracker(sequence["sd"])
    ring = FrameRing(3, len(SIZES), sizes=SIZES)            # a BGR ring: submit_device_nv12 needs only its device side
    surf = [[torch.empty((r * 3 // 2, c), dtype=torch.uint8, device="cuda") for r, c in SIZES] for _ in range(3)]

    def submit(slot, t):
        for s, f in enumerate(sequence["nv"][t]):
            surf[slot][s].copy_(torch.from_numpy(np.ascontiguousarray(f)))
        torch.cuda.synchronize()
        ring.submit_device_nv12(slot, [x.data_ptr() for x in surf[slot]], [x.data_ptr() + r * c for x, (r, c) in zip(surf[slot], SIZES)],
                                [c for _, c in SIZES], [c for _, c in SIZES])
    try:
        submit(0, 0)
        for t in range(4):
            k, k1 = t % 3, (t + 1) % 3
            submit(k1, t + 1)
            got = b.update_batch(sequence["dets"][t], ring=ring, slot=k)
            for s in range(len(SIZES)):
                assert np.array_equal(np.asarray(got[s]), sequence["want"][t][s]), (t, s)
    finally:
        b.synchronize()
        ring.close(); b.close()


def test_errors():
    import ctypes

    from boxmot_amd import _lib
    from boxmot_amd.ingest import FrameRing
    with pytest.raises(ValueError, match="stream 0"):
        FrameRing(2, 1, 11, 10, fmt="nv12")
    lib = _lib.load()
    r, c = np.array([10, 10], np.int32), np.array([10, 9], np.int32)     # the library checks for itself
    assert not lib.boxmot_hip_ingest_create_nv12(2, 2, r.ctypes.data, c.ctypes.data)
    assert "stream 1" in _lib.last_error()
    ring = FrameRing(3, 2, 10, 16, fmt="nv12")
    assert lib.boxmot_hip_ingest_format(ring._handle) == 1
    with pytest.raises(RuntimeError, match="slot"):
        ring.submit(7)
    t = np.zeros(2, np.int32)
    p = (ctypes.c_void_p * 2)(256, 512)
    assert not lib.boxmot_hip_ingest_submit_device_nv12(ring._handle, 0, 2, ctypes.addressof(p), ctypes.addressof(p), t.ctypes.data, t.ctypes.data)
    assert "stream 0" in _lib.last_error() and "pitch" in _lib.last_error()
    held = ring.host_view(2)[0]                 # a slice keeps the slot's view alive: close() must not free the memory under it
    with pytest.raises(RuntimeError, match="still referenced"):
        ring.close()
    del held
    ring.close()
    bgr = FrameRing(2, 1, 10, 16)
    assert lib.boxmot_hip_ingest_format(bgr._handle) == 0
    bgr.close()
