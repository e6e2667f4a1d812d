// Tiled detection post-processing (include/boxmot_hip.h, boxmot_hip_detpost_run_tiled): the detector ran on T tiles per stream
// (ingest_letterbox_tiles.hpp) and the per-tile detections are merged in FRAME coordinates with ONE NMS per stream, on the device.
//
// Definition, extending steps 1-6 at the top of det_post.hpp.  Layouts "cn" and "nc_obj", fp16 / fp32 (the oriented layout has no
// tiled form).  pred is (S * T, ...): tile t of stream s is tensor s * T + t.  geom[s][t] = gain, top, left, x0, y0, w, h as float32:
// the tile's letterbox (gain, top, left) and its rectangle in the frame.
// 1.  Score.  Unchanged, per tile tensor: the score kernels of det_post.hpp run with grid.y = S * T, the keys then lie as
//     [S][T * A].
// 2.  Select.  Of the passing anchors of ALL T tiles of the stream the K largest by (conf descending, tile ascending, anchor
//     ascending), exactly: dp_select_sort on a copy of the arguments with A' = T * A; the candidate word's index is t * A + a.
// 3.  Box.  As step 3 of det_post.hpp, from the tile's tensor, in the tile's letterbox pixels.
// 3b. Frame.  BEFORE the NMS: fx = fminf(fmaxf((x - left) / gain, 0), w) + x0, fy = fminf(fmaxf((y - top) / gain, 0), h) + y0 --
//     one subtraction, one correctly rounded division, a clip to the TILE, one addition.
// 4.  NMS.  Greedy, in the order of step 2, on the frame-space boxes, class-aware by comparing classes or agnostic; the metric is
//     fixed at creation:
//         merge 0 "iou": inter / (area_i + area_j - inter) > iou_thres          (dp_suppresses)
//         merge 1 "ios": inter / fminf(area_i, area_j) > iou_thres              intersection over the SMALLER box, what sliced
//                        inference uses so that a box cut by a tile's edge is absorbed by the whole one a neighbouring tile saw
//     0 / 0 compares false in both.
// 5.  Emit.  The first max_det kept rows as they are: [x1, y1, x2, y2, conf, cls], already in frame coordinates.
// 6.  Counters.  As step 6, per stream: over all its tiles.
// (tests/detpost_tiled_ref.py restates this in NumPy and the kernels are compared with that, bit for bit; parity with SAHI or
// Ultralytics is not pinned by any test.)
//
// k_detpost_select_tiled<T>: one workgroup of DP_THREADS per stream.  Stages a-c are dp_select_sort, stage d decodes and maps to the
// frame, stage e is the chunked 64 x 64 ballot NMS explained in det_post.hpp, written out here with the metric selected inside
// this kernel's predicate (a wave-uniform branch); the LDS layout and the K <= 4096 budget are k_detpost_select's.  The handle's
// key and class scratch is sized [S * T][A].
#pragma once

#include "det_post.hpp"

namespace bm {

constexpr int DP_TILES_MAX = 64;

struct DetPostTiledArgs {
    DetPostArgs base;               // A: the anchors of ONE tile tensor; keys / cls: [S * T][A]; geom unused (null)
    const DetPostTileGeom* tgeom;   // [S][T] (DetPostTileGeom and dp_tile_to_frame are in det_post.hpp: det_post_extra.hpp shares them)
    int T, merge;                   // merge: 0 iou, 1 ios
};

__device__ inline bool dp_suppresses_ios(const DpBox& j, const DpBox& i, float thres) {
    const float area_i = (i.x2 - i.x1) * (i.y2 - i.y1), area_j = (j.x2 - j.x1) * (j.y2 - j.y1);
    const float iw = fmaxf(fminf(i.x2, j.x2) - fmaxf(i.x1, j.x1), 0.0f), ih = fmaxf(fminf(i.y2, j.y2) - fmaxf(i.y1, j.y1), 0.0f);
    const float inter = iw * ih;
    return inter / fminf(area_i, area_j) > thres;
}
__device__ inline bool dp_merge_suppresses(const DpBox& j, const DpBox& i, float thres, int merge) {
    return merge ? dp_suppresses_ios(j, i, thres) : dp_suppresses(j, i, thres);
}

// k_detpost_select_tiled and k_detpost_select_tiled_src are one text, det_post_tiled_select_body.hpp
#define DP_SELECT_KERNEL k_detpost_select_tiled
#define DP_SELECT_SRC false
#include "det_post_tiled_select_body.hpp"
#undef DP_SELECT_KERNEL
#undef DP_SELECT_SRC
#define DP_SELECT_KERNEL k_detpost_select_tiled_src
#define DP_SELECT_SRC true
#include "det_post_tiled_select_body.hpp"
#undef DP_SELECT_KERNEL
#undef DP_SELECT_SRC

// The kernel sequence of one tiled call (L as detpost_launch's): the score kernel over the S * T tile tensors, then one select
// workgroup per stream.
template <class L>
inline void detpost_launch_tiled(L& launch, const DetPostTiledArgs& ta, int n_streams, int fp16, size_t* lds_bytes = nullptr) {
    const size_t lds = detpost_lds_bytes(ta.base.K);
    if (lds_bytes) *lds_bytes = lds;
    detpost_launch_score(launch, ta.base, n_streams * ta.T, fp16);
    if (fp16) {
        if (ta.base.n_extra > 0) launch(k_detpost_select_tiled_src<_Float16>, n_streams, 1, DP_THREADS, lds, ta);
        else launch(k_detpost_select_tiled<_Float16>, n_streams, 1, DP_THREADS, lds, ta);
    } else {
        if (ta.base.n_extra > 0) launch(k_detpost_select_tiled_src<float>, n_streams, 1, DP_THREADS, lds, ta);
        else launch(k_detpost_select_tiled<float>, n_streams, 1, DP_THREADS, lds, ta);
    }
    if (ta.base.n_extra > 0) detpost_launch_extra(launch, ta.base, ta.tgeom, ta.T, n_streams, fp16);
}

}  // namespace bm
