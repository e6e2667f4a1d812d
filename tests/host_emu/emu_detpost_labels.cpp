// TEST-ONLY harness: runs the label-map kernel of a mask handle (boxmot_amd/csrc/det_post_labels.hpp, the device source unchanged,
// through the library's own launch detpost_launch_labels with the library's grid) on CPU threads, on emu_detpost.cpp's launcher.
// The kernel has workgroup barriers and static LDS (function statics here, one workgroup at a time).
#include "emu_detpost.cpp"

#include "../../boxmot_amd/csrc/det_post_labels.hpp"

// geom: [S][5] float32 gain, top, left, rows, cols; proto (S, E, mask_h, mask_w) of 2- (proto_fp16) or 4-byte elements; dets
// [S][det_stride][6]; det_rows [S]; extra [S][det_stride][E]; labels [S][label_rows][label_cols]; the two ratios as the library
// computes them at creation.  fallback 1: the global-memory path on every tile.  The grid covers the call's largest frame, as the
// library's does.  Returns the workgroups launched.
extern "C" long emu_detpost_labels_run(int n_streams, const float* geom, const void* proto, int proto_fp16, const float* dets, int det_stride,
                                       const int* det_rows, const float* extra, int16_t* labels, int label_rows, int label_cols, int max_det, int E,
                                       int mask_h, int mask_w, int in_h, int in_w, int fallback) {
    const bm::DetPostGeom* g = reinterpret_cast<const bm::DetPostGeom*>(geom);
    int frame_rows = 1, frame_cols = 1;
    for (int s = 0; s < n_streams; ++s) {
        if ((int)g[s].rows > frame_rows) frame_rows = (int)g[s].rows;
        if ((int)g[s].cols > frame_cols) frame_cols = (int)g[s].cols;
    }
    const int plane = mask_h * mask_w;
    const bm::DetPostLabelArgs a{g, proto, dets, det_rows, extra, labels, (long)E * plane, (long)label_rows * label_cols, label_cols, det_stride, max_det, E,
                                 mask_h, mask_w, plane, (float)mask_w / (float)in_w, (float)mask_h / (float)in_h, 0, fallback};
    Launcher L;
    bm::detpost_launch_labels(L, a, n_streams, frame_rows, frame_cols, proto_fp16);
    return (long)bm::detpost_label_tiles(frame_cols, bm::DP_LABEL_TW) * bm::detpost_label_tiles(frame_rows, bm::DP_LABEL_TH) * n_streams;
}
