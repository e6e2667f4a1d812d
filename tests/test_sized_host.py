"""Host side of the per-frame-size ReID batch: every image and box table is validated in Python before the library is called (a
stub library that fails on any call stands in for it), the new C symbols are declared, bound and -- where the library is built --
exported."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("boxmot_hip_reid_compute_features_batch", "boxmot_hip_reid_preprocess_batch", "boxmot_hip_botsort_set_frame_sizes",
               "boxmot_hip_deepocsort_set_frame_sizes", "boxmot_hip_strongsort_set_frame_sizes",
               "boxmot_hip_ingest_create_sized")


class _NoLib:
    """stands in for the loaded library: reaching it is the failure"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the inputs were validated")


def _reid(monkeypatch):
    from boxmot_amd import _lib
    from boxmot_amd.reid import HipReID
    monkeypatch.setattr(_lib, "load", lambda: _NoLib())
    r = HipReID.__new__(HipReID)
    r._lib, r._handle, r.feature_dim, r.max_crops = _lib.load(), None, 512, 64
    return r


def _streams(monkeypatch):
    from boxmot_amd import _lib
    from boxmot_amd.streams import MultiStreamBotSort
    monkeypatch.setattr(_lib, "load", lambda: _NoLib())
    t = MultiStreamBotSort.__new__(MultiStreamBotSort)
    t._lib, t._handle, t._det_cols, t._out_cols, t.emb_dim, t.n_streams = _lib.load(), None, 6, 8, 512, 2
    t._sizes, t._declared = [None, None], False
    t._own_cmc, t._had_frames = False, False
    return t


BOX = np.array([[10, 10, 60, 120]], np.float32)
IMG = np.zeros((480, 640, 3), np.uint8)


@pytest.mark.parametrize("imgs,boxes,word", [
    ([IMG, IMG.astype(np.float32)], [BOX, BOX], "image 1"),                  # wrong dtype
    ([IMG[:, :, 0], IMG], [BOX, BOX], "image 0"),                            # a 2-D image
    ([IMG, np.zeros((720, 1280, 4), np.uint8)], [BOX, BOX], "image 1"),      # four channels
    ([IMG, None], [BOX, BOX], "image 1"),                                    # a missing image
    ([IMG, IMG], [BOX], "box tables"),                                       # lists of different lengths
    ([], [], "at least one image"),
    ([IMG, IMG], [BOX, np.zeros((2, 3), np.float32)], "image 1"),            # boxes with fewer than 4 columns
    ([IMG, IMG], [BOX, np.zeros((2, 5), np.float32)], "oriented"),           # axis-aligned and oriented rows in one call
])
def test_get_features_batch_validates_before_the_library_is_called(monkeypatch, imgs, boxes, word):
    r = _reid(monkeypatch)
    with pytest.raises(ValueError, match=word):
        r.get_features_batch(boxes, imgs)
    with pytest.raises(ValueError, match=word):
        r.get_crops_batch(boxes, imgs)


def test_get_features_batch_without_boxes_returns_empty_tables_per_image(monkeypatch):
    r = _reid(monkeypatch)
    out = r.get_features_batch([np.zeros((0, 4), np.float32), None], [IMG, np.zeros((720, 1280, 3), np.uint8)])
    assert [o.shape for o in out] == [(0, 512), (0, 512)] and all(o.dtype == np.float32 for o in out)


def test_batch_tables_stack_boxes_in_image_order_and_index_their_image(monkeypatch):
    r = _reid(monkeypatch)
    b0 = np.arange(8, dtype=np.float32).reshape(2, 4)
    b2 = np.arange(12, dtype=np.float32).reshape(3, 4) + 100
    arrs, counts, boxes, box_image = r._batch([b0, None, b2], [IMG, np.zeros((487, 651, 3), np.uint8), np.zeros((1080, 1920, 3), np.uint8)])
    assert counts == [2, 0, 3] and box_image.tolist() == [0, 0, 2, 2, 2] and box_image.dtype == np.int32
    assert np.array_equal(boxes, np.concatenate([b0, b2])) and boxes.flags.c_contiguous
    assert [a.shape for a in arrs] == [(480, 640, 3), (487, 651, 3), (1080, 1920, 3)]


BIG = np.zeros((720, 1280, 3), np.uint8)


@pytest.mark.parametrize("imgs,word", [
    ([IMG, IMG.astype(np.float32)], "stream 1"),                             # wrong dtype
    ([None, IMG[:, :, 0]], "stream 1"),                                      # a 2-D image
    ([IMG, np.zeros((480, 640, 4), np.uint8)], "stream 1"),
    ([IMG, None, IMG], "stream 2"),                                          # more frames than the handle has streams
])
def test_multistream_update_batch_checks_every_frame_before_pointers_go_down(monkeypatch, imgs, word):
    t = _streams(monkeypatch)
    dets = [np.zeros((0, 6), np.float32)] * len(imgs)
    with pytest.raises(ValueError, match=word):
        t.update_batch(dets, imgs=imgs)


@pytest.mark.parametrize("second", [[IMG, IMG], [None, IMG], [BIG, BIG]])
def test_a_stream_whose_later_frame_has_another_shape_is_named_before_the_library_is_called(monkeypatch, second):
    """each stream keeps the size of its first frame: also when the other entries are None, and when every stream changes at once"""
    t = _streams(monkeypatch)
    t._sizes = [(480, 640), (720, 1280)]                                     # as after a first frame of (IMG, BIG)
    t._declared = True
    dets = [np.zeros((0, 6), np.float32)] * 2
    with pytest.raises(ValueError, match="stream [01]: frame is .* this stream's frames are"):
        t.update_batch(dets, imgs=second)
    assert t._sizes == [(480, 640), (720, 1280)]


def test_first_frames_record_each_stream_s_size_and_mixed_sizes_need_every_stream(monkeypatch):
    t = _streams(monkeypatch)
    assert t._check_frames([IMG, None]) == [(480, 640), None]
    assert t._check_frames([IMG, BIG]) == [(480, 640), (720, 1280)]
    t._sizes = [(480, 640), None]
    t2 = _streams(monkeypatch)
    t2.n_streams, t2._sizes = 3, [None, None, None]
    with pytest.raises(ValueError, match="stream 2: no frame yet"):          # sizes differ and stream 2 has none: it cannot be declared
        t2.update_batch([np.zeros((0, 6), np.float32)] * 2, imgs=[IMG, BIG])


def test_a_new_size_after_the_first_frames_of_a_handle_with_its_own_cmc_names_the_stream(monkeypatch):
    """the handle made its estimator for the size it had seen: the later stream is refused by name, before the library is called"""
    t = _streams(monkeypatch)
    t._own_cmc, t._had_frames, t._sizes = True, True, [(480, 640), None]
    with pytest.raises(ValueError, match="stream 1: frame is 720 x 1280.*declared up front"):
        t.update_batch([np.zeros((0, 6), np.float32)] * 2, imgs=[None, BIG])
    assert t._sizes == [(480, 640), None]


@pytest.mark.parametrize("sizes,word", [
    ([(480, 640)], "1 entries for 2 streams"),                               # wrong length
    ([(480, 640), (720, 1280), (1080, 1920)], "3 entries for 2 streams"),
    ([(480, 640), (0, 1280)], "stream 1"),
    ([(480, 640), (720, 1280, 3)], "stream 1"),
])
def test_sizes_of_the_wrong_length_or_shape_raise_before_the_library_is_called(monkeypatch, sizes, word):
    from boxmot_amd import _lib
    from boxmot_amd.ingest import FrameRing
    from boxmot_amd.streams import MultiStreamBotSort
    monkeypatch.setattr(_lib, "load", lambda: _NoLib())
    with pytest.raises(ValueError, match=word):
        FrameRing(2, 2, sizes=sizes)
    with pytest.raises(ValueError, match=word):
        MultiStreamBotSort(2, frame_sizes=sizes)
    with pytest.raises(ValueError):
        FrameRing(2, 2)                                                      # neither rows / cols nor sizes
    with pytest.raises(ValueError):
        FrameRing(2, 2, rows=480, cols=640, sizes=[(480, 640)] * 2)


def test_new_symbols_are_declared_bound_and_exported():
    from boxmot_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "boxmot_hip.h").read_text(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b(?:int|BoxMOTHipIngest\*)\s+%s\s*\(" % n, text), f"{n} is not declared in include/boxmot_hip.h"
        assert n in _lib.SIGNATURES
    m = re.search(r"boxmot_hip_reid_compute_features_batch\s*\((.*?)\)\s*;", text, re.S)
    args = " ".join(m.group(1).split())
    assert args == ("BoxMOTHipReID* handle, const uint8_t* const* images, const int* image_rows, const int* image_cols, int n_images, "
                    "const float* boxes, const int* box_image, int n_boxes, int box_cols, float* out_features, int out_capacity_rows")
    assert len(_lib.SIGNATURES["boxmot_hip_reid_compute_features_batch"][1]) == 11
    so = ROOT / "boxmot_amd" / "libboxmot_hip.so"
    if so.exists() and shutil.which("nm"):
        exported = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
        for n in NEW_SYMBOLS:
            assert re.search(r"\bT %s\b" % n, exported), f"{n} is not exported by the built library"
