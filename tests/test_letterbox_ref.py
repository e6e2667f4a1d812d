"""Pins tests/letterbox_ref.py -- the NumPy reference the letterbox kernel is compared with -- on the geometry table of the
definition, on the placement of the padding, on the copy and exact-2x cases against hand-written code, and on the value tables;
and ``LetterboxGeometry.to_frame`` as a round trip of frame-space boxes.  No device, no library."""
from fractions import Fraction

import numpy as np
import pytest

import letterbox_ref as ref


@pytest.mark.parametrize("frame,size,center", ref.ALL_SHAPES)
def test_geometry_table(frame, size, center):
    from boxmot_amd.ingest import letterbox_geometry
    rows, cols = frame
    g = ref.geometry(rows, cols, size, "center")
    assert g[1:] == center
    assert g[0] == min(size[0] / rows, size[1] / cols)
    t = ref.geometry(rows, cols, size, "topleft")
    assert t[3:] == (0, 0) and t[2] == center[1]
    assert t[1] == ref.TOPLEFT_NEW_W.get(frame, center[0])
    for mode, want in (("center", g), ("topleft", t)):
        got = letterbox_geometry(rows, cols, size, mode)
        assert tuple(got)[:5] == want and (got.rows, got.cols) == frame
        assert all(type(v) is int for v in tuple(got)[1:])


def test_box_filter_case_of_a_720p_frame_and_the_degenerate_case():
    from boxmot_amd.ingest import letterbox_geometry
    assert ref.geometry(720, 1280, (640, 640))[1:] == (640, 360, 140, 0)          # both axes shrink by exactly 2
    assert ref.geometry(1080, 1920, (640, 640))[1:] == (640, 360, 140, 0)
    assert ref.geometry(3, 200, (16, 64), "topleft") is None                      # new_h = int(3 * 0.32) = 0
    assert ref.geometry(3, 200, (16, 64), "center")[1:] == (64, 1, 7, 0)
    with pytest.raises(ValueError, match="no picture"):
        letterbox_geometry(3, 200, (16, 64), "topleft")
    with pytest.raises(ValueError, match="mode"):
        letterbox_geometry(3, 200, (16, 64), "middle")
    assert letterbox_geometry(8, 8, 16)[1:5] == (16, 16, 0, 0)                    # an int is a square size


def test_pad_placement_and_odd_padding():
    f = ref.make_frame(50, 131, "random", 5)
    u = ref.letterbox_u8(f, (40, 72), "center", pad=7)
    assert (u[:6] == 7).all() and (u[33:] == 7).all() and u[33:].shape[0] == 7     # 6 lines above, 7 below
    assert np.array_equal(u[6:33], ref.cv2_resize_linear_u8(f, (72, 27)))
    t = ref.letterbox_u8(f, (40, 72), "topleft", pad=7)
    assert np.array_equal(t[:27], u[6:33]) and (t[27:] == 7).all()
    n = ref.letterbox_u8(ref.make_frame(9, 7, "random", 6), (32, 48), "center")
    assert (n[:, :11] == 114).all() and (n[:, 36:] == 114).all() and n[:, 36:].shape[1] == 12      # 11 columns left, 12 right


def test_copy_case_is_the_frame_itself():
    f = ref.make_frame(24, 32, "random", 1)
    out = ref.letterbox(f, (32, 32), rgb=False, unit=False)
    assert out.dtype == np.float32 and out.shape == (3, 32, 32)
    assert np.array_equal(out[:, 4:28], f.transpose(2, 0, 1).astype(np.float32))
    assert (out[:, :4] == 114).all() and (out[:, 28:] == 114).all()
    rgb = ref.letterbox(f, (32, 32), rgb=True, unit=False)
    assert np.array_equal(rgb, out[::-1])


@pytest.mark.parametrize("kind", ["random", "checker", "ramp"])
def test_exact_2x_is_the_box_filter(kind):
    f = ref.make_frame(36, 64, kind, 2)
    u = ref.letterbox_u8(f, (32, 32))
    box = np.empty((18, 32, 3), dtype=np.uint8)
    for y in range(18):                     # hand-written: the rounded mean of each 2 x 2 block
        for x in range(32):
            for c in range(3):
                box[y, x, c] = (int(f[2 * y, 2 * x, c]) + int(f[2 * y, 2 * x + 1, c]) + int(f[2 * y + 1, 2 * x, c]) + int(f[2 * y + 1, 2 * x + 1, c]) + 2) >> 2
    assert np.array_equal(u[7:25], box)
    if kind == "checker":
        assert (box == 128).all()           # (0 + 255 + 255 + 0 + 2) >> 2


def test_value_tables():
    t32, t16 = ref.table(True, np.float32), ref.table(True, np.float16)
    assert t32.dtype == np.float32 and t16.dtype == np.float16
    for v in range(256):
        q = Fraction(v, 255)
        assert abs(Fraction(float(t32[v])) - q) <= abs(Fraction(float(np.nextafter(t32[v], np.float32(2)))) - q)
        assert abs(Fraction(float(t32[v])) - q) <= abs(Fraction(float(np.nextafter(t32[v], np.float32(-1)))) - q)
        # the fp16 entry is the correctly rounded quotient too, not only the rounded fp32 entry
        assert abs(Fraction(float(t16[v])) - q) <= abs(Fraction(float(np.nextafter(t16[v], np.float16(2)))) - q)
        assert abs(Fraction(float(t16[v])) - q) <= abs(Fraction(float(np.nextafter(t16[v], np.float16(-1)))) - q)
    assert np.array_equal(ref.table(False, np.float16), np.arange(256).astype(np.float16))
    assert t32[255] == 1 and t16[255] == 1 and t32[0] == 0


def test_the_shared_frames():
    names = [c[0] for c in ref.CASES]
    assert len(set(names)) == len(names) == len(ref.ALL_SHAPES) + 8
    ramp = next(f for n, f, _ in ref.CASES if n.startswith("ramp 10x700"))
    assert len(np.unique(ramp)) == 256                                    # every byte value
    chk = next(f for n, f, _ in ref.CASES if n.startswith("checker 37x53"))
    assert set(np.unique(chk)) == {0, 255} and chk[0, 0, 0] != chk[0, 1, 0] and chk[0, 0, 0] != chk[1, 0, 0]
    a = ref.want(0)
    assert ref.want(0) is a and not a.flags.writeable                     # computed once, shared, read-only


@pytest.mark.parametrize("frame,size,_", ref.ALL_SHAPES)
@pytest.mark.parametrize("mode", ["center", "topleft"])
def test_to_frame_round_trip(frame, size, _, mode):
    from boxmot_amd.ingest import letterbox_geometry
    rows, cols = frame
    g = letterbox_geometry(rows, cols, size, mode)
    rng = np.random.default_rng(rows * 1000 + cols)
    x = np.sort(rng.uniform(0, cols, (20, 2)), axis=1)
    y = np.sort(rng.uniform(0, rows, (20, 2)), axis=1)
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1], rng.uniform(0, 1, 20), rng.integers(0, 80, 20)], axis=1).astype(np.float32)
    det = boxes.copy()                      # frame space -> detector space, as the letterbox maps the picture
    det[:, [0, 2]] = boxes[:, [0, 2]] * np.float32(g.gain) + g.left
    det[:, [1, 3]] = boxes[:, [1, 3]] * np.float32(g.gain) + g.top
    keep = det.copy()
    back = g.to_frame(det)
    assert back.dtype == np.float32 and back.shape == boxes.shape
    assert np.array_equal(det, keep)                                       # the input is not modified
    assert np.array_equal(back[:, 4:], boxes[:, 4:])                       # other columns untouched
    # float32: a coordinate up to max(H, W) carries an error of a few ulp through the two operations and the division by gain
    tol = 8 * np.finfo(np.float32).eps * max(size) / g.gain
    assert np.abs(back[:, :4] - boxes[:, :4]).max() <= tol
    # the definition, and the clip: boxes in the padding land on the frame's border
    want = np.array([[(5.0 - g.left) / g.gain, (3.0 - g.top) / g.gain]], dtype=np.float64)
    one = g.to_frame(np.array([[5, 3, 1e6, 1e6]], dtype=np.float32))
    assert np.allclose(one[0, :2], np.clip(want[0], 0, [cols, rows]), rtol=1e-6, atol=1e-6)
    assert one[0, 2] == cols and one[0, 3] == rows
    assert (g.to_frame(np.array([[-50, -50, -40, -40]], dtype=np.float32)) == 0).all()
