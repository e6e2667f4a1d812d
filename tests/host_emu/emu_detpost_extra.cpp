// TEST-ONLY harness: runs the detection post-processing of a head with per-anchor extras (boxmot_amd/csrc/det_post_extra.hpp with
// det_post.hpp and det_post_tiled.hpp, the device source unchanged, through the library's own kernel sequences detpost_launch /
// detpost_launch_tiled: score, the select kernel's SRC variant, k_detpost_extra) on CPU threads, on emu_detpost.cpp's launcher,
// included as emu_detpost_obb.cpp and emu_tiles.cpp include it.  The scratch -- the handle-owned source block that stands in when
// the caller gives no src included -- and the dynamic LDS are poisoned before every call.
#include "emu_detpost.cpp"

#include "../../boxmot_amd/csrc/det_post_tiled.hpp"

// T = 0: untiled, pred (S, 4 + nc + E, A) or (S, A, 5 + nc + E) and geom [S][5]; T >= 1: tiled, pred (S * T, ...) and geom [S][T][7].
// dets [S][out_stride][6], det_rows [S], counters [S][3], extra [S][out_stride][E], src [S][out_stride] or null (then the anchors go
// to a scratch [S][max_det], as in the library).  Returns the LDS bytes of the select launch.
extern "C" long emu_detpost_extra_run(int n_streams, int T, int A, int nc, int layout, int fp16, const void* pred, const float* geom, const uint8_t* allow,
                                      int K, int max_det, int agnostic, int merge, float conf_thres, float iou_thres, float* dets, int out_stride,
                                      int* det_rows, int* counters, int n_extra, int extra_kind, float* extra, int* src) {
    const int NT = T ? T : 1;
    std::vector<uint32_t> keys((size_t)n_streams * NT * A, 0xCDCDCDCDu);
    std::vector<int> cls((size_t)n_streams * NT * A, (int)0xCDCDCDCD);
    std::vector<int> own_src((size_t)n_streams * max_det, (int)0xCDCDCDCD);
    bm::DetPostArgs g{pred, T ? nullptr : reinterpret_cast<const bm::DetPostGeom*>(geom), allow, keys.data(), cls.data(), dets, det_rows, counters,
                      A, nc, layout, K, max_det, agnostic, out_stride, conf_thres, iou_thres, 0, 0, 0,
                      src ? src : own_src.data(), extra, src ? out_stride : max_det, n_extra, extra_kind};
    Launcher L;
    size_t lds = 0;
    if (T) {
        bm::DetPostTiledArgs ta{g, reinterpret_cast<const bm::DetPostTileGeom*>(geom), T, merge};
        bm::detpost_launch_tiled(L, ta, n_streams, fp16, &lds);
    } else {
        bm::detpost_launch(L, g, n_streams, fp16, &lds);
    }
    return (long)lds;
}
