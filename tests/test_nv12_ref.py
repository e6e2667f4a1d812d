"""tests/nv12_ref.py (the NumPy reference of the ingest ring's NV12 -> BGR conversion) on hand-computed pixels: the formula of
COLOR_YUV2BGR_NV12 (BT.601 limited range, 20-bit fixed point) worked with Python integers, the 2 x 2 chroma sharing, and the
order of U and V in the interleaved plane."""
import numpy as np

from nv12_ref import bgr_to_nv12, exhaustive_frame, nv12_to_bgr, nv12_to_bgr_planes


def _pixel(Y, U, V):
    """one pixel with unbounded Python integers, written from the definition"""
    yy = max(Y - 16, 0) * 1220542
    u, v, h = U - 128, V - 128, 1 << 19
    sat = lambda x: min(max(x >> 20, 0), 255)
    return sat(yy + h + 2116026 * u), sat(yy + h - 852492 * v - 409993 * u), sat(yy + h + 1673527 * v)


def _frame(y, uv):
    return np.concatenate([np.asarray(y, np.uint8), np.asarray(uv, np.uint8)], axis=0)


def test_hand_computed_pixels():
    # white, black, and BT.601 red: (81 - 16) * 1220542 + 2^19 = 79859518; + 1673527 * 112 = 267294542 -> >> 20 = 254;
    # 79859518 - 2116026 * 38 = -549470 -> 0; 79859518 - 852492 * 112 + 409993 * 38 = -39852 -> 0
    for (Y, U, V), want in (((235, 128, 128), (255, 255, 255)), ((16, 128, 128), (0, 0, 0)), ((81, 90, 240), (0, 0, 254))):
        assert _pixel(Y, U, V) == want
        got = nv12_to_bgr(_frame(np.full((2, 2), Y), [[U, V]]), 2, 2)
        assert got.shape == (2, 2, 3) and got.dtype == np.uint8
        assert (got.reshape(-1, 3) == np.array(want)).all(), (Y, U, V, got)
    # luma below 16 clamps before the multiply; mid grey
    assert _pixel(0, 128, 128) == (0, 0, 0) and _pixel(126, 128, 128) == (128, 128, 128)
    assert (nv12_to_bgr(_frame(np.full((2, 2), 126), [[128, 128]]), 2, 2) == 128).all()


def test_each_2x2_block_takes_its_own_chroma_pair():
    y = np.array([[60, 70, 80, 90], [100, 110, 120, 130], [140, 150, 160, 170], [180, 190, 200, 210]])
    uv = np.array([[100, 150, 160, 90], [128, 200, 40, 128]])           # (U, V) of the blocks: top-left, top-right, bottom-left, bottom-right
    got = nv12_to_bgr(_frame(y, uv), 4, 4)
    for r in range(4):
        for c in range(4):
            U, V = uv[r // 2, 2 * (c // 2)], uv[r // 2, 2 * (c // 2) + 1]
            assert tuple(got[r, c]) == _pixel(int(y[r, c]), int(U), int(V)), (r, c)
    # with one luma everywhere the four blocks are four different colours, each constant inside its block
    flat = nv12_to_bgr(_frame(np.full((4, 4), 128), uv), 4, 4)
    blocks = [flat[r:r + 2, c:c + 2].reshape(-1, 3) for r in (0, 2) for c in (0, 2)]
    assert all((b == b[0]).all() for b in blocks)
    assert len({tuple(b[0]) for b in blocks}) == 4


def test_u_and_v_are_not_interchangeable():
    rng = np.random.default_rng(3)
    y = rng.integers(16, 236, (4, 6))
    uv = np.array([[60, 200, 90, 170, 128, 30], [220, 40, 100, 140, 10, 250]])
    a = nv12_to_bgr(_frame(y, uv), 4, 6)
    swapped = uv.reshape(2, 3, 2)[:, :, ::-1].reshape(2, 6)
    b = nv12_to_bgr(_frame(y, swapped), 4, 6)
    assert not np.array_equal(a, b)
    for r in range(4):
        for c in range(6):
            assert tuple(a[r, c]) == _pixel(int(y[r, c]), int(uv[r // 2, 2 * (c // 2)]), int(uv[r // 2, 2 * (c // 2) + 1]))
            assert tuple(b[r, c]) == _pixel(int(y[r, c]), int(uv[r // 2, 2 * (c // 2) + 1]), int(uv[r // 2, 2 * (c // 2)]))


def test_pitched_planes_and_the_exhaustive_frame():
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (9, 10), dtype=np.uint8)                    # 6 x 10 picture
    yp = np.zeros((6, 16), np.uint8); yp[:, :10] = f[:6]
    up = np.zeros((3, 12), np.uint8); up[:, :10] = f[6:]
    assert np.array_equal(nv12_to_bgr_planes(yp[:, :10], up[:, :10]), nv12_to_bgr(f, 6, 10))
    e = exhaustive_frame()
    assert e.shape == (6144, 4096)
    # every (Y, U, V) triple exactly once
    yv = e[:4096].astype(np.int64)
    u = np.repeat(np.repeat(e[4096:, 0::2], 2, 0), 2, 1).astype(np.int64)
    v = np.repeat(np.repeat(e[4096:, 1::2], 2, 0), 2, 1).astype(np.int64)
    counts = np.bincount((yv << 16 | u << 8 | v).ravel(), minlength=1 << 24)
    assert counts.min() == 1 and counts.max() == 1
    assert bgr_to_nv12(np.zeros((5, 7, 3), np.uint8)).shape == (6, 6)
