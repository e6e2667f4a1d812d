// TEST-ONLY harness: the table forms of the frame-addressing ReID kernels (per-stream frame sizes: k_crop_resize_sized<float>,
// k_crop_resize_rgbx_hl_sized, k_stem_sized_fused_hp) beside their scalar forms, device source unchanged, on CPU threads.  One
// launch takes crops of several frames of different sizes; the scalar form is launched with one frame's W, H.  The launch harness
// is emu_reid.cpp's (included as it is, so the two cannot drift apart).
#include "emu_reid.cpp"

namespace {

void sized_lut(float* lut) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            volatile float a = (float)v / 255.0f;
            volatile float b = a - mean[c];
            lut[c * 256 + v] = b / stdv[c];
        }
}

}  // namespace

extern "C" {

// In all three: frames[s] is frame s ((H_s, W_s, 3) uint8 BGR), crop_stream[i] the frame of box i, boxes (n, 4).
// dims != nullptr: the table form, dims[2 s] = W_s, dims[2 s + 1] = H_s (W, H unused).  dims == nullptr: the scalar form with W, H.

// k_crop_resize<float> / k_crop_resize_sized<float>: out (n, 256, 128, 3) fp32
int emu_sized_crop_f32(const uint8_t* const* frames, const int* crop_stream, const float* boxes, int n, const int* dims, int W, int H,
                       int pad, float* out) {
    using namespace bm;
    float lut[768];
    sized_lut(lut);
    const float* lp = lut;
    if (dims) launch(n, REID_IN_H / 16, REID_IN_W, [=]() { k_crop_resize_sized<float>(frames, crop_stream, boxes, 4, dims, lp, out, 16, pad); });
    else launch(n, REID_IN_H / 16, REID_IN_W, [=]() { k_crop_resize<float>(frames, crop_stream, boxes, 4, W, H, lp, out, 16, pad); });
    return 0;
}

// k_crop_resize_rgbx_hl / _sized: out_hi, out_lo (n, 262, 136, 4) fp16 bit patterns (the caller zeroes them: only the interior is written)
int emu_sized_crop_hl(const uint8_t* const* frames, const int* crop_stream, const float* boxes, int n, const int* dims, int W, int H,
                      int pad, uint16_t* out_hi, uint16_t* out_lo) {
    using namespace bm;
    float lut[768];
    sized_lut(lut);
    const float* lp = lut;
    _Float16 *oh = reinterpret_cast<_Float16*>(out_hi), *ol = reinterpret_cast<_Float16*>(out_lo);
    if (dims) launch(n, REID_IN_H / 16, REID_IN_W, [=]() { k_crop_resize_rgbx_hl_sized(frames, crop_stream, boxes, 4, dims, lp, oh, ol, 16, nullptr, pad); });
    else launch(n, REID_IN_H / 16, REID_IN_W, [=]() { k_crop_resize_rgbx_hl(frames, crop_stream, boxes, 4, W, H, lp, oh, ol, 16, nullptr, pad); });
    return 0;
}

// k_stem_resize_fused_hp / k_stem_sized_fused_hp on an OSN1 x0.25 blob: out_hi, out_lo (n, 2048, 16) fp16 bit patterns in the kernels'
// own channel order (compared between the two forms as they are), out_f32 (may be null) hi + lo as fp32 natural NHWC
int emu_sized_stem_hp(const float* blob, long n_floats, const uint8_t* const* frames, const int* crop_stream, const float* boxes, int n,
                      const int* dims, int W, int H, uint16_t* out_hi, uint16_t* out_lo, float* out_f32) {
    using namespace bm;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(blob);
    if (hdr[0] != REID_MAGIC || hdr[1] != 16) return -1;
    const int ch[4] = {hdr[1], hdr[2], hdr[3], hdr[4]};
    const OsnetLayout L = make_osnet_layout(ch, hdr[5]);
    if (n_floats != REID_HEADER_INTS + L.total) return -2;
    const float* w = blob + REID_HEADER_INTS;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    std::vector<uint8_t> wst;
    pack_stem_hp_fused(w + L.stem_w, w + L.stem_b, mean, stdv, wst);
    const unsigned char* wp = wst.data();
    _Float16 *oh = reinterpret_cast<_Float16*>(out_hi), *ol = reinterpret_cast<_Float16*>(out_lo);
    if (dims) launch(n, 1, 512, [=]() { k_stem_sized_fused_hp(frames, crop_stream, boxes, 4, dims, oh, ol, wp, nullptr); });
    else launch(n, 1, 512, [=]() { k_stem_resize_fused_hp(frames, crop_stream, boxes, 4, W, H, oh, ol, wp, nullptr); });
    if (out_f32) {
        std::vector<float> a((size_t)n * 2048 * 16), b(a.size());
        unpack_act(oh, a.data(), (long)n * 2048, 16);
        unpack_act(ol, b.data(), (long)n * 2048, 16);
        for (size_t k = 0; k < a.size(); ++k) out_f32[k] = a[k] + b[k];
    }
    return 0;
}

}  // extern "C"
