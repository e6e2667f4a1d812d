// Per-anchor extras through the detection post-processing (include/boxmot_hip.h, boxmot_hip_detpost_create_extra / _run_extra): pose
// heads (Ultralytics *-pose: 17 keypoints x, y, visibility after the class scores, decoded to letterbox pixels) and segmentation
// heads (*-seg: 32 mask coefficients; det_post_mask.hpp decodes the masks from them, step 9) carry E more values per anchor.  The
// rows of d_dets say nothing about the anchor they came from, so this writes, beside them and in the same row order, the source
// anchor and the extras of every emitted row -- d_extra[s][det_ind] is then the skeleton or the coefficients of the detection a
// track was matched to.  Included by det_post.hpp.
//
// Definition, extending steps 1-6 at the top of det_post.hpp (and of det_post_tiled.hpp on a tiled handle).  1 <= E <= 1024.
//     layout 0 "cn"      (S, 4 + nc + E, A): the extra channel rows are 4 + nc .. 4 + nc + E - 1
//     layout 1 "nc_obj"  (S, A, 5 + nc + E): the extra columns follow the scores
//     The oriented layout "cn_obb" has no extras (its angle row sits where they would begin; the library refuses the combination).
//     fp16 and fp32; fp16 widens exactly.
// 1-6. Unchanged: they read none of the extra values, only the per-stream / per-anchor stride grows by E.
// 7. Source.  For every emitted row r < d_det_rows[s]: src[s][r] = the anchor index a of the row; on a tiled handle t * A + a, the
//    index of the candidate word (tile t, anchor a of that tile's tensor).
// 8. Extras.  extra[s][r][e], with v the widened value of extra channel e of that anchor, by the kind fixed at creation:
//        kind 0 "raw"   v
//        kind 1 "kpt2"  (E % 2 == 0) values in groups of 2: x, y
//        kind 2 "kpt3"  (E % 3 == 0) values in groups of 3: x, y, visibility
//            component 0, an x:   fminf(fmaxf((v - left) / gain, 0), cols)
//            component 1, a y:    fminf(fmaxf((v - top) / gain, 0), rows)
//            component 2:         v, copied
//    That is dp_to_frame, the arithmetic of the boxes (step 5): one fp32 subtraction, one correctly rounded division, the clip.  It
//    is a reading of Ultralytics' scale_coords + clip_coords; it is pinned against this repository's NumPy restatement
//    (tests/detpost_extra_ref.py) only, not against Ultralytics.  On a tiled handle the geometry of the row's OWN tile is used,
//    dp_tile_to_frame: fminf(fmaxf((v - left) / gain, 0), w) + x0, likewise y with top, h, y0 -- a keypoint is clipped to the tile
//    that reported it, then shifted.
//    A NaN coordinate comes out as 0 (tiled: x0 / y0): fmaxf returns its non-NaN operand.  +-inf are clipped like any value.
// Rows at and beyond the count, and streams beyond n_streams, are not touched in either block; the counters are unchanged.
//
// Kernels.  The select kernels' SRC variants (k_detpost_select_src<T>, k_detpost_select_tiled_src<T>: the same bodies compiled with
// SRC = true) store the index in wavefront 0's emit, where the candidate word is at hand.  k_detpost_extra<T> runs third on the same stream: grid
// (ceil(max_det * E / 256), S), one thread per (row, channel), consecutive lanes on consecutive channels of a row.  It reads
// det_rows[s] and src from device memory -- no host sync -- and writes nothing for row >= det_rows[s].  "cn": the loads of a
// wavefront are A elements apart (inherent to the layout: a row's extras are one column of the tensor); "nc_obj": one contiguous
// run.  The stores of a wavefront are one contiguous run in both.  No LDS, no atomics.
#pragma once

namespace bm {

constexpr int DP_EXTRA_THREADS = 256, DP_EXTRA_MAX = 1024, DP_EXTRA_KINDS = 3;

__host__ __device__ inline int detpost_extra_group(int kind) { return kind == 0 ? 1 : kind + 1; }      // values per keypoint; raw: 1
inline int detpost_extra_grid_x(int max_det, int E) { return (int)(((long)max_det * E + DP_EXTRA_THREADS - 1) / DP_EXTRA_THREADS); }

// tgeom / n_tiles: a tiled call's [S][n_tiles] geometry, else null / 0 and g.geom is read
template <class T>
__global__ void __launch_bounds__(DP_EXTRA_THREADS) k_detpost_extra(DetPostArgs g, const DetPostTileGeom* tgeom, int n_tiles) {
    const int s = (int)blockIdx.y, E = g.n_extra;
    const int idx = (int)blockIdx.x * DP_EXTRA_THREADS + (int)threadIdx.x;      // (max_det * E <= 2^30: the library checks)
    const int row = idx / E, e = idx - row * E;
    if (row >= g.det_rows[s]) return;                           // (det_rows[s] <= max_det <= src_stride, out_stride)
    const T* pred = static_cast<const T*>(g.pred);
    const int src = g.src[(long)s * g.src_stride + row];
    const int first = (g.layout == 0 ? 4 : 5) + g.nc;
    const int comp = e % detpost_extra_group(g.extra_kind);     // 0 for "raw": copied, as component 2 is
    float out;
    if (n_tiles) {
        const int tile = src / g.A, a = src - tile * g.A, ps = s * n_tiles + tile;
        const float v = dp_load(pred, dp_at<true>(g, ps, a, first + e));
        const DetPostTileGeom q = tgeom[ps];
        out = g.extra_kind == 0 || comp == 2 ? v : comp == 0 ? dp_tile_to_frame(v, q.left, q.gain, q.w, q.x0) : dp_tile_to_frame(v, q.top, q.gain, q.h, q.y0);
    } else {
        const float v = dp_load(pred, dp_at<true>(g, s, src, first + e));
        const DetPostGeom q = g.geom[s];
        out = g.extra_kind == 0 || comp == 2 ? v : comp == 0 ? dp_to_frame(v, q.left, q.gain, q.cols) : dp_to_frame(v, q.top, q.gain, q.rows);
    }
    g.extra[((long)s * g.out_stride + row) * E + e] = out;
}

}  // namespace bm
