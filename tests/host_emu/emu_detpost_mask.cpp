// TEST-ONLY harness: runs the detection post-processing of a mask handle (boxmot_amd/csrc/det_post_mask.hpp with det_post.hpp,
// det_post_tiled.hpp and det_post_extra.hpp, the device source unchanged, through the library's own kernel sequences
// detpost_launch_with_mask / detpost_launch_tiled_with_mask: score, the select kernel's SRC variant, k_detpost_extra, k_detpost_mask)
// on CPU threads, on emu_detpost.cpp's launcher, included as emu_detpost_extra.cpp includes it.  The scratch -- the handle-owned source
// block that stands in when the caller gives no src included -- and the dynamic LDS are poisoned before every call.
#include "emu_detpost.cpp"

#include "../../boxmot_amd/csrc/det_post_mask.hpp"

// As emu_detpost_extra_run (extra_kind 0), plus: proto (S [* T], E, mask_h, mask_w) of 2- (proto_fp16) or 4-byte elements, masks
// [S][out_stride][mask_h][mask_w], and the two ratios as the library computes them at creation.  Returns the LDS bytes of the
// select launch.
extern "C" long emu_detpost_mask_run(int n_streams, int T, int A, int nc, int layout, int fp16, const void* pred, const float* geom, const uint8_t* allow,
                                     int K, int max_det, int agnostic, int merge, float conf_thres, float iou_thres, float* dets, int out_stride,
                                     int* det_rows, int* counters, int n_extra, float* extra, int* src, const void* proto, int proto_fp16, uint8_t* masks,
                                     int mask_h, int mask_w, int in_h, int in_w) {
    const int NT = T ? T : 1;
    std::vector<uint32_t> keys((size_t)n_streams * NT * A, 0xCDCDCDCDu);
    std::vector<int> cls((size_t)n_streams * NT * A, (int)0xCDCDCDCD);
    std::vector<int> own_src((size_t)n_streams * max_det, (int)0xCDCDCDCD);
    bm::DetPostArgs g{pred, T ? nullptr : reinterpret_cast<const bm::DetPostGeom*>(geom), allow, keys.data(), cls.data(), dets, det_rows, counters,
                      A, nc, layout, K, max_det, agnostic, out_stride, conf_thres, iou_thres, 0, 0, 0,
                      src ? src : own_src.data(), extra, src ? out_stride : max_det, n_extra, 0};
    const int plane = mask_h * mask_w;
    const bm::DetPostMaskArgs m{proto, masks, (long)n_extra * plane, plane, mask_h, mask_w, (float)mask_w / (float)in_w, (float)mask_h / (float)in_h, 0};
    Launcher L;
    size_t lds = 0;
    if (T) {
        bm::DetPostTiledArgs ta{g, reinterpret_cast<const bm::DetPostTileGeom*>(geom), T, merge};
        bm::detpost_launch_tiled_with_mask(L, ta, m, n_streams, fp16, proto_fp16, &lds);
    } else {
        bm::detpost_launch_with_mask(L, g, m, n_streams, fp16, proto_fp16, &lds);
    }
    return (long)lds;
}
