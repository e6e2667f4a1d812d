// TEST-ONLY harness: runs the ORIENTED detection post-processing kernels (boxmot_amd/csrc/det_post.hpp + det_post_obb.hpp, the device
// source unchanged, including its kernel sequence detpost_launch) on CPU threads with the grids the library launches.  It is
// emu_detpost.cpp -- the barrier-capable launcher that poisons the dynamic LDS before every workgroup -- plus an entry point that
// fills the oriented fields of DetPostArgs; the scratch is poisoned before every call.
#include "emu_detpost.cpp"

// pred: (S, 4 + nc + 1, A) of 2- (fp16) or 4-byte elements; geom: [S][5] float32 gain, top, left, rows, cols; allow: nc bytes or
// null; dets: [S][out_stride][7]; det_rows: [S]; counters: [S][3].  Returns the LDS bytes of the launch.
extern "C" long emu_detpost_obb_run(int n_streams, int A, int nc, int fp16, const void* pred, const float* geom, const uint8_t* allow, int K,
                                    int max_det, int agnostic, int nms_mode, int regularize, float conf_thres, float iou_thres, float* dets,
                                    int out_stride, int* det_rows, int* counters) {
    std::vector<uint32_t> keys((size_t)n_streams * A, 0xCDCDCDCDu);
    std::vector<int> cls((size_t)n_streams * A, (int)0xCDCDCDCD);
    bm::DetPostArgs g{pred, reinterpret_cast<const bm::DetPostGeom*>(geom), allow, keys.data(), cls.data(), dets, det_rows, counters,
                      A, nc, 0, K, max_det, agnostic, out_stride, conf_thres, iou_thres, 1, nms_mode, regularize};
    Launcher L;
    size_t lds = 0;
    bm::detpost_launch(L, g, n_streams, fp16, &lds);
    return (long)lds;
}
