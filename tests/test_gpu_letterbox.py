"""GPU tests of the letterboxed detector input (include/boxmot_hip.h boxmot_hip_ingest_letterbox, boxmot_amd/ingest.py
FrameRing.letterbox, csrc/ingest_letterbox.hpp).  The resize is integer arithmetic and the float values come out of a table, so every
comparison is EXACT (bit for bit against tests/letterbox_ref.py): a differing element is a failure."""
import ctypes

import numpy as np
import pytest

import letterbox_ref as ref
from nv12_ref import nv12_to_bgr as ref_nv12_to_bgr, random_frame as random_nv12

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {np.float16: "float16", np.float32: "float32"}


def _empty(torch, shape, dtype, fill=None):
    x = torch.empty(shape, dtype=getattr(torch, TORCH_DTYPE[dtype]), device="cuda")
    if fill is not None:
        x.fill_(fill)
    return x


def _same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def _ring_of(frames, fmt="bgr", n_slots=2):
    from boxmot_amd.ingest import FrameRing
    return FrameRing(n_slots, len(frames), sizes=[f.shape[:2] for f in frames]) if fmt == "bgr" else \
        FrameRing(n_slots, len(frames), sizes=[(f.shape[0] * 2 // 3, f.shape[1]) for f in frames], fmt="nv12")


def _fill(ring, slot, frames):
    for s, f in enumerate(frames):
        ring.host_view(slot, s)[...] = f
    ring.submit(slot)


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=[c[0] for c in ref.CASES])
def test_each_case_through_a_bgr_ring(k):
    import torch
    _, frame, size = ref.CASES[k]
    ring = _ring_of([frame])
    try:
        _fill(ring, 1, [frame])
        for mode in ("center", "topleft"):
            for dtype in (np.float16, np.float32):
                x = _empty(torch, (1, 3, *size), dtype)
                geo = ring.letterbox(1, x, mode=mode, hip_stream=torch.cuda.current_stream().cuda_stream)
                assert tuple(geo[0])[:5] == ref.geometry(*frame.shape[:2], size, mode)
                torch.cuda.synchronize()
                assert _same(x[0], ref.want(k, mode, dtype=dtype)), (mode, dtype)
    finally:
        ring.close()


def test_even_shapes_through_an_nv12_ring():
    """the shapes an NV12 ring can hold (even rows and cols), as the streams of one NV12 ring: the kernel reads the BGR frames the
    NV12 conversion wrote on the copy stream, ordered by the slot's upload event only"""
    import torch
    shapes = [(f, s) for f, s, _ in ref.ALL_SHAPES if f[0] % 2 == 0 and f[1] % 2 == 0]
    assert len(shapes) >= 7
    nv = [random_nv12(r, c, 300 + k) for k, ((r, c), _) in enumerate(shapes)]
    bgr = [ref_nv12_to_bgr(f, r, c) for f, ((r, c), _) in zip(nv, shapes)]
    ring = _ring_of(nv, "nv12")
    try:
        _fill(ring, 0, nv)
        for size in ((40, 72), (63, 136)):         # sizes at which the thinnest frame, 10 x 700, keeps a line in both modes
            for mode, dtype in (("center", np.float16), ("topleft", np.float32)):
                x = _empty(torch, (len(nv), 3, *size), dtype)
                ring.letterbox(0, x, mode=mode, hip_stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                for s, f in enumerate(bgr):
                    assert _same(x[s], ref.letterbox(f, size, mode, dtype=dtype)), (shapes[s], size, mode)
    finally:
        ring.close()


@pytest.fixture(scope="module")
def mixed():
    """every frame of the table as the streams of ONE ring"""
    frames = [c[1] for c in ref.CASES[:len(ref.ALL_SHAPES)]]
    ring = _ring_of(frames)
    _fill(ring, 0, frames)
    yield ring, frames
    ring.close()


@pytest.mark.parametrize("mode,dtype,rgb,unit,pad", [
    ("center", np.float16, True, True, 114),            # Ultralytics
    ("topleft", np.float32, False, False, 114),         # YOLOX
    ("center", np.float32, True, True, 0),
    ("topleft", np.float16, False, True, 255),
    ("center", np.float16, True, False, 7),
])
def test_all_shapes_as_the_streams_of_one_call_on_a_side_stream(mixed, mode, dtype, rgb, unit, pad):
    import torch
    ring, frames = mixed
    st = torch.cuda.Stream()
    for size in ((40, 72), (63, 136)):
        with torch.cuda.stream(st):
            x = _empty(torch, (len(frames), 3, *size), dtype)
            geo = ring.letterbox(0, x, mode=mode, rgb=rgb, unit=unit, pad=pad, hip_stream=st.cuda_stream)
            y = x.clone()                               # queued behind the kernel on the same stream: no synchronisation by the caller
        st.synchronize()
        assert len(geo) == len(frames)
        for s, f in enumerate(frames):
            assert _same(y[s], ref.letterbox(f, size, mode, rgb, unit, pad, dtype)), (s, f.shape, size)


def test_fewer_streams_than_the_ring_leave_the_rows_beyond_untouched(mixed):
    import torch
    ring, frames = mixed
    for dtype in (np.float16, np.float32):
        x = _empty(torch, (len(frames), 3, 32, 48), dtype, fill=-3.0)
        geo = ring.letterbox(0, x, n_streams=5, hip_stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert len(geo) == 5
        got = x.cpu().numpy()
        for s in range(5):
            assert _same(got[s], ref.letterbox(frames[s], (32, 48), dtype=dtype)), s
        assert (got[5:] == -3.0).all()


def test_a_submit_right_after_letterbox_does_not_reach_the_tensor():
    """slot k is letterboxed on a side stream that is still busy with earlier work; a new frame is submitted into slot k at once.
    The copy stream must wait for the letterbox launch, so the tensor shows the OLD frame -- and the slot the new one afterwards."""
    import torch
    sizes = [(270, 480), (240, 320)]
    old = [ref.make_frame(r, c, "random", 40 + s) for s, (r, c) in enumerate(sizes)]
    new = [ref.make_frame(r, c, "random", 50 + s) for s, (r, c) in enumerate(sizes)]
    ring = _ring_of(old)
    st = torch.cuda.Stream()
    try:
        a = torch.randn((4096, 4096), device="cuda")
        torch.cuda.synchronize()
        _fill(ring, 0, old)
        with torch.cuda.stream(st):
            x = _empty(torch, (2, 3, 160, 160), np.float16)
            for _ in range(6):                          # a few milliseconds of work in front of the kernel
                a = a @ a * 1e-3
            ring.letterbox(0, x, hip_stream=st.cuda_stream)
        ring.host_done(0)
        _fill(ring, 0, new)                             # no wait of any kind in between
        st.synchronize()
        for s in range(2):
            assert _same(x[s], ref.letterbox(old[s], (160, 160), dtype=np.float16)), s
            assert np.array_equal(ring.download(0, s), new[s])
        ring.letterbox(0, x, hip_stream=st.cuda_stream)
        st.synchronize()
        for s in range(2):
            assert _same(x[s], ref.letterbox(new[s], (160, 160), dtype=np.float16)), s
    finally:
        torch.cuda.synchronize()
        ring.close()


SIZES = [(240, 320), (180, 256), (122, 166)]
T = 4


def test_letterbox_before_update_batch_leaves_the_tracker_rows_unchanged():
    """three small NV12 streams, 4 frames, slot t + 1 submitted before slot t is tracked: a run that letterboxes every slot on the
    detector's stream before update_batch(ring=, slot=) gives the rows of a run that does not, and every tensor is exact"""
    import torch
    from boxmot_amd.ingest import FrameRing
    from boxmot_amd.reid_weights import reference_init_state_dict
    from boxmot_amd.scenario import Scenario
    from boxmot_amd.streams import MultiStreamBotSort
    from nv12_ref import bgr_to_nv12
    sd = reference_init_state_dict("osnet_x0_25", seed=0)
    scs = [Scenario(10, 20, width=c, height=r, random_image=True, stream=s) for s, (r, c) in enumerate(SIZES)]
    base = [bgr_to_nv12(sc.image) for sc in scs]
    nv = [[np.roll(b, 8 * t, axis=1) for b in base] for t in range(T)]
    dets = [[sc.frame(t, with_embs=False)[0] for sc in scs] for t in range(T)]
    st = torch.cuda.Stream()

    def run(with_letterbox):
        trk = MultiStreamBotSort(len(SIZES), max_tracks=64, max_dets=32, emb_dim=512, reid_weights=sd)
        trk.set_reid_mode(1)
        ring = FrameRing(3, len(SIZES), sizes=SIZES, fmt="nv12")
        rows, tensors = [], []
        try:
            _fill(ring, 0, nv[0])
            for t in range(T):
                k, k1 = t % 3, (t + 1) % 3
                if t + 1 < T:
                    ring.host_done(k1)
                    _fill(ring, k1, nv[t + 1])
                if with_letterbox:
                    with torch.cuda.stream(st):
                        x = _empty(torch, (len(SIZES), 3, 96, 128), np.float16)
                        ring.letterbox(k, x, hip_stream=st.cuda_stream)
                    tensors.append(x)
                rows.append([np.asarray(r).copy() for r in trk.update_batch(dets[t], ring=ring, slot=k)])
            trk.synchronize()
            st.synchronize()
        finally:
            torch.cuda.synchronize()
            ring.close(); trk.close()
        return rows, tensors

    want, _ = run(False)
    got, tensors = run(True)
    assert sum(len(r) for r in want[-1]) > 0
    for t in range(T):
        for s, (r, c) in enumerate(SIZES):
            assert np.array_equal(got[t][s], want[t][s]), (t, s)
            assert _same(tensors[t][s], ref.letterbox(ref_nv12_to_bgr(nv[t][s], r, c), (96, 128), dtype=np.float16)), (t, s)


def test_errors():
    import torch
    from boxmot_amd import _lib
    from boxmot_amd.ingest import FrameRing
    lib = _lib.load()
    ring = FrameRing(2, 2, sizes=[(8, 8), (3, 200)])
    x = _empty(torch, (2, 3, 16, 64), np.float32, fill=5.0)
    good = dict(out_rows=16, out_cols=64, mode=0, dtype=0, rgb=1, unit=1, pad_value=114)

    def call(slot=0, n=2, ptr=None, **kw):
        cfg = _lib.Letterbox(**dict(good, **kw))
        ok = lib.boxmot_hip_ingest_letterbox(ring._handle, slot, n, ctypes.byref(cfg), ctypes.c_void_p(x.data_ptr() if ptr is None else ptr), None)
        return ok, _lib.last_error()
    try:
        for kw, word in [(dict(slot=2), "slot"), (dict(slot=-1), "slot"), (dict(n=0), "stream count"), (dict(n=3), "stream count"),
                         (dict(ptr=0), "null"), (dict(ptr=x.data_ptr() + 8), "16-byte"), (dict(out_cols=60), "multiple of 8"),
                         (dict(mode=2), "mode"), (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(pad_value=256), "pad_value"),
                         (dict(pad_value=-1), "pad_value"), (dict(out_rows=0), "positive"), (dict(mode=1), "stream 1")]:
            ok, msg = call(**kw)
            assert not ok and word in msg, (kw, msg)
        ok, msg = call(mode=1)
        assert "3 x 200" in msg and "no picture" in msg                   # the degenerate stream, named
        assert not lib.boxmot_hip_ingest_letterbox(ring._handle, 0, 2, None, ctypes.c_void_p(x.data_ptr()), None)
        assert not lib.boxmot_hip_ingest_letterbox(None, 0, 2, ctypes.byref(_lib.Letterbox(**good)), ctypes.c_void_p(x.data_ptr()), None)
        torch.cuda.synchronize()
        assert (x == 5.0).all()                                           # none of them wrote
        with pytest.raises(ValueError, match="stream 1"):
            ring.letterbox(0, x, mode="topleft")
        assert call(mode=1, n=1)[0] and call(mode=0)[0]                   # without the degenerate stream / where it keeps one line
        with pytest.raises(RuntimeError, match="slot"):
            ring.letterbox(5, x)
    finally:
        torch.cuda.synchronize()
        ring.close()
