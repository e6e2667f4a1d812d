// Frame-space instance label map from a mask handle's rows (include/boxmot_hip.h, boxmot_hip_detpost_labels): one int16 plane per
// stream at FRAME resolution, every pixel holding the row of d_dets that owns it -- the det_ind a tracker hands back -- or -1.
// With lut[d_out[s, :n, 7]] = d_out[s, :n, 4] the map becomes a per-pixel track-id map in one gather.  It is made from the float
// logits, upsampled BEFORE thresholding (process_mask_native's order), not from the thresholded bytes of d_masks.  Includes
// det_post_mask.hpp.
//
// Definition, step 10 after step 9 at the top of det_post_mask.hpp.  Everything is float32 and every operation is rounded separately
// (-ffp-contract=off: no fused multiply-add, no fast intrinsics).  Inputs, for stream s of an UNTILED mask handle, after a run on the
// same stream:
//     gain, top, left, rows, cols     the call's geometry row, as the float32 values the device table holds
//     wr, hr                          as det_post_mask.hpp defines them: (float)mask_w / (float)in_w, (float)mask_h / (float)in_h
//     n = min(d_det_rows[s], max_det)
//     d_dets[s][r] = [x1, y1, x2, y2, ...]   the rows in FRAME coordinates, as the run wrote them
//     c_r[k] = d_extra[s][r][k]       the raw coefficients
//     proto[s]                        (E, mask_h, mask_w), fp16 or fp32 (fp16 widens exactly)
// 10. Labels.
//      logit_r(i, j) is exactly step 9's chain: acc = 0.0f; for k = 0 .. E - 1 ascending: acc = acc + c_r[k] * proto[s][k][i][j].
//      For frame pixel (y, x), 0 <= y < rows, 0 <= x < cols:
//          pu = (((float)x + 0.5f) * gain + left) * wr - 0.5f
//          pu = fminf(fmaxf(pu, 0.0f), (float)(mask_w - 1))
//          j0 = (int)pu          j1 = min(j0 + 1, mask_w - 1)          lx = pu - (float)j0
//          pv, i0, i1, ly the same way from y, top, hr and mask_h
//      L_r(y, x) = (1 - ly) * ((1 - lx) * g00 + lx * g01) + ly * ((1 - lx) * g10 + lx * g11)       with g_ab = logit_r(i_a, j_b);
//          every 1 - l, every product and every sum rounded on its own, in that association.
//      Row r COVERS (y, x) when ALL of
//          (float)x >= x1     (float)x < x2     (float)y >= y1     (float)y < y2     L_r(y, x) > 0.0f
//      hold: the window test is Ultralytics crop_mask's >= / <; a NaN anywhere compares false.
//      labels[s][y][x], an int16, is the smallest r < n that covers the pixel -- the highest confidence wins -- or -1 if none does.
//    Every pixel of [0, rows) x [0, cols) of the streams in the call is written.  The rest of a (label_rows, label_cols) plane larger
//    than the frame, streams beyond the call's and every other block are left alone.
// Stated plainly: the pixel mapping is the exact inverse of the handle's letterbox map with half-pixel centres, composed with
// align_corners=False sampling of the prototype plane.  It is NOT Ultralytics scale_masks' integer-cropped interpolation, which
// shifts by a fraction of a prototype pixel, and it is pinned against this repository's NumPy restatement
// (tests/detpost_labels_ref.py) only.  Out of scope: tiled handles, "cn_obb", dense per-row frame masks, polygons.
//
// Kernel.  k_detpost_labels<P> (P: proto's type) is a launch of its own on the caller's stream, after the run: grid (frame tiles of
// DP_LABEL_TW x DP_LABEL_TH pixels, S), one workgroup of DP_LABEL_THREADS per (tile, stream), four pixels of one column per thread,
// their labels in registers until the one store at the end.  A tile outside the stream's frame leaves at once.  The workgroup walks
// the stream's rows in ascending order, DP_LABEL_CHUNK boxes at a time staged in LDS; a row whose box misses the tile is skipped --
// the test reads the box at one LDS address for the whole wavefront, so it is wavefront-uniform.  For a row that hits, the workgroup
// computes the logits of the PROTOTYPE PATCH the tile maps to once, into LDS: x -> j0 and y -> i0 are monotone (every rounded
// operation is), so the patch is [j0(first column), j1(last column)] x [i0(first line), i1(last line)], the image of the tile's
// corners plus one tap.  Every still-unlabelled pixel inside the box then takes its four taps from LDS.  First-wins comes from the
// loop order: no atomics, nothing depends on arrival order.  The workgroup leaves early when no pixel of the tile is unlabelled
// (a flag in LDS, two slots used in turn, between the two barriers a hit row costs).
// When gain * wr > 1 (a frame smaller than the detector's input) or on a degenerate tile the patch would pass DP_LABEL_PATCH floats:
// the FALLBACK path then computes the four logits of a pixel straight from global memory -- the same bits, for it is the same chain
// per logit (dp_label_logit).  At 1080p into 640 x 640 with 160 x 160 prototypes gain * wr = 1 / 12: a tile maps to a 7 x 3 patch.
// LDS: 4 KB of boxes + 8 KB of patch + 8 bytes, static; plain vector stores, no inline assembly.  The kernel has an argument struct
// of its own, DetPostLabelArgs: nothing is added to DetPostArgs, DetPostTiledArgs or DetPostMaskArgs, so every other kernel stays
// what it was instruction for instruction.
#pragma once

#include "det_post_mask.hpp"

namespace bm {

constexpr int DP_LABEL_THREADS = 256, DP_LABEL_TW = 64, DP_LABEL_TH = 16, DP_LABEL_PER = DP_LABEL_TW * DP_LABEL_TH / DP_LABEL_THREADS,
              DP_LABEL_CHUNK = 256, DP_LABEL_PATCH = 2048, DP_LABEL_MAX_DET = 32767, DP_LABEL_DET_COLS = 6;
static_assert(DP_LABEL_TW == 64 && DP_LABEL_PER * DP_LABEL_THREADS == DP_LABEL_TW * DP_LABEL_TH, "a wavefront per line of the tile");

struct DetPostLabelArgs {
    const DetPostGeom* geom;        // [S]: the handle's table
    const void* proto;              // (S, E, mask_h, mask_w), fp16 or fp32
    const float* dets;              // [S][det_stride][6], frame coordinates
    const int* det_rows;            // [S]
    const float* extra;             // [S][det_stride][E]
    int16_t* labels;                // [S][label_rows][label_cols]
    long proto_stride;              // elements per tensor: E * mask_h * mask_w
    long label_stride;              // elements per plane: label_rows * label_cols
    int label_cols, det_stride, max_det, E, mask_h, mask_w, plane;
    float wr, hr;
    int tiles_x;                    // tiles per line of tiles: the grid's x is tiles_x * tiles_y
    int fallback;                   // 1: the global-memory path whatever the patch (tests and tools/detpost_prof; the library passes 0)
};

inline int detpost_label_tiles(int n, int tile) { return (n + tile - 1) / tile; }

// the definition's map of a frame coordinate to the two taps and the weight along one axis
__device__ inline void dp_label_tap(int x, float gain, float off, float ratio, int size, int& t0, int& t1, float& l) {
    float p = (((float)x + 0.5f) * gain + off) * ratio - 0.5f;
    p = fminf(fmaxf(p, 0.0f), (float)(size - 1));
    t0 = (int)p;
    t1 = t0 + 1 < size - 1 ? t0 + 1 : size - 1;
    l = p - (float)t0;
}

// logit_r at one prototype pixel: `at` is proto[s][0][i][j]; the chain is sequential, the loads of DP_MASK_UNROLL planes are issued
// before the first is used
template <class P>
__device__ inline float dp_label_logit(const float* __restrict__ c, int E, const P* __restrict__ at, int plane) {
    float acc = 0.0f;
    int k = 0;
    for (; k + DP_MASK_UNROLL <= E; k += DP_MASK_UNROLL) {
        float v[DP_MASK_UNROLL];
#pragma unroll
        for (int q = 0; q < DP_MASK_UNROLL; ++q) v[q] = (float)at[(long)(k + q) * plane];
#pragma unroll
        for (int q = 0; q < DP_MASK_UNROLL; ++q) acc = acc + c[k + q] * v[q];
    }
    for (; k < E; ++k) acc = acc + c[k] * (float)at[(long)k * plane];
    return acc;
}

__device__ inline float dp_label_blend(float g00, float g01, float g10, float g11, float lx, float ly) {
    const float wx = 1.0f - lx, wy = 1.0f - ly;
    const float upper = wx * g00 + lx * g01, lower = wx * g10 + lx * g11;
    return wy * upper + ly * lower;
}

template <class P>
__global__ void __launch_bounds__(DP_LABEL_THREADS) k_detpost_labels(DetPostLabelArgs a) {
    __shared__ float s_box[DP_LABEL_CHUNK][4];
    __shared__ float s_patch[DP_LABEL_PATCH];
    __shared__ int s_open[2];
    const int s = (int)blockIdx.y, tile_y = (int)blockIdx.x / a.tiles_x, tile_x = (int)blockIdx.x - tile_y * a.tiles_x;
    const DetPostGeom geo = a.geom[s];
    const int rows = (int)geo.rows, cols = (int)geo.cols;          // (the host checked them against the plane)
    const int x0 = tile_x * DP_LABEL_TW, y0 = tile_y * DP_LABEL_TH;
    if (x0 >= cols || y0 >= rows) return;
    const int tid = (int)threadIdx.x, x = x0 + (tid & (DP_LABEL_TW - 1)), yq = y0 + (tid / DP_LABEL_TW) * DP_LABEL_PER;
    const int x_last = (x0 + DP_LABEL_TW < cols ? x0 + DP_LABEL_TW : cols) - 1, y_last = (y0 + DP_LABEL_TH < rows ? y0 + DP_LABEL_TH : rows) - 1;
    int n = a.det_rows[s];
    n = n < a.max_det ? n : a.max_det;

    // the patch of the tile: the image of its corners plus one tap
    int j_lo, j_hi, i_lo, i_hi, unused;
    float unused_l;
    dp_label_tap(x0, geo.gain, geo.left, a.wr, a.mask_w, j_lo, unused, unused_l);
    dp_label_tap(x_last, geo.gain, geo.left, a.wr, a.mask_w, unused, j_hi, unused_l);
    dp_label_tap(y0, geo.gain, geo.top, a.hr, a.mask_h, i_lo, unused, unused_l);
    dp_label_tap(y_last, geo.gain, geo.top, a.hr, a.mask_h, unused, i_hi, unused_l);
    const int pw = j_hi - j_lo + 1, ph = i_hi - i_lo + 1;
    const bool from_lds = !a.fallback && pw * ph <= DP_LABEL_PATCH;

    // this thread's pixels: column x, lines yq .. yq + DP_LABEL_PER - 1
    int j0, j1, i0[DP_LABEL_PER], i1[DP_LABEL_PER], label[DP_LABEL_PER];
    float lx, ly[DP_LABEL_PER];
    dp_label_tap(x, geo.gain, geo.left, a.wr, a.mask_w, j0, j1, lx);
    bool open = false;                                              // a pixel of this thread is in the frame and unlabelled
#pragma unroll
    for (int q = 0; q < DP_LABEL_PER; ++q) {
        dp_label_tap(yq + q, geo.gain, geo.top, a.hr, a.mask_h, i0[q], i1[q], ly[q]);
        label[q] = -1;
        open = open || (x < cols && yq + q < rows);
    }
    const bool mine = open;
    const float fx = (float)x;
    const P* proto = static_cast<const P*>(a.proto) + (long)s * a.proto_stride;
    const float* dets = a.dets + (long)s * a.det_stride * DP_LABEL_DET_COLS;
    const float* extra = a.extra + (long)s * a.det_stride * a.E;

    bool live = true;
    int turn = 0;
    for (int base = 0; base < n && live; base += DP_LABEL_CHUNK) {
        __syncthreads();                                            // (the previous chunk's boxes have been read)
        if (base + tid < n) {
            const float* row = dets + (long)(base + tid) * DP_LABEL_DET_COLS;
#pragma unroll
            for (int q = 0; q < 4; ++q) s_box[tid][q] = row[q];
        }
        __syncthreads();
        const int m = n - base < DP_LABEL_CHUNK ? n - base : DP_LABEL_CHUNK;
        for (int b = 0; b < m && live; ++b) {
            const float x1 = s_box[b][0], y1 = s_box[b][1], x2 = s_box[b][2], y2 = s_box[b][3];
            // no pixel of the tile passes the window test unless its last column / line reaches x1 / y1 and its first lies below x2 / y2
            if (!((float)x_last >= x1 && (float)x0 < x2 && (float)y_last >= y1 && (float)y0 < y2)) continue;
            const int r = base + b;
            const float* c = extra + (long)r * a.E;
            if (tid == 0) s_open[turn] = 0;                         // (last read two hit rows ago, a barrier since)
            if (from_lds) {
                for (int e = tid; e < pw * ph; e += DP_LABEL_THREADS) {
                    const int pi = e / pw, pj = e - pi * pw;
                    s_patch[e] = dp_label_logit(c, a.E, proto + (long)(i_lo + pi) * a.mask_w + (j_lo + pj), a.plane);
                }
            }
            __syncthreads();
            if (open && fx >= x1 && fx < x2) {
                open = false;
#pragma unroll
                for (int q = 0; q < DP_LABEL_PER; ++q) {
                    const float fy = (float)(yq + q);
                    if (label[q] < 0 && fy >= y1 && fy < y2 && yq + q < rows && x < cols) {
                        float g00, g01, g10, g11;
                        if (from_lds) {
                            const int up = (i0[q] - i_lo) * pw - j_lo, lo = (i1[q] - i_lo) * pw - j_lo;
                            g00 = s_patch[up + j0]; g01 = s_patch[up + j1]; g10 = s_patch[lo + j0]; g11 = s_patch[lo + j1];
                        } else {
                            const P* up = proto + (long)i0[q] * a.mask_w, * lo = proto + (long)i1[q] * a.mask_w;
                            g00 = dp_label_logit(c, a.E, up + j0, a.plane); g01 = dp_label_logit(c, a.E, up + j1, a.plane);
                            g10 = dp_label_logit(c, a.E, lo + j0, a.plane); g11 = dp_label_logit(c, a.E, lo + j1, a.plane);
                        }
                        if (dp_label_blend(g00, g01, g10, g11, lx, ly[q]) > 0.0f) label[q] = r;
                    }
                    open = open || (label[q] < 0 && yq + q < rows && x < cols);
                }
            }
            if (open) s_open[turn] = 1;
            __syncthreads();
            live = s_open[turn] != 0;
            turn ^= 1;
        }
    }
    if (mine) {
#pragma unroll
        for (int q = 0; q < DP_LABEL_PER; ++q)
            if (yq + q < rows && x < cols) a.labels[(long)s * a.label_stride + (long)(yq + q) * a.label_cols + x] = (int16_t)label[q];
    }
}

// One launch over the first n_streams streams; frame_rows / frame_cols: the largest frame of the call (the grid covers it, a
// smaller stream's spare tiles leave at once).
template <class L>
inline void detpost_launch_labels(L& launch, const DetPostLabelArgs& args, int n_streams, int frame_rows, int frame_cols, int proto_fp16) {
    DetPostLabelArgs a = args;
    a.tiles_x = detpost_label_tiles(frame_cols, DP_LABEL_TW);
    const int gx = a.tiles_x * detpost_label_tiles(frame_rows, DP_LABEL_TH);
    if (proto_fp16) launch(k_detpost_labels<_Float16>, gx, n_streams, DP_LABEL_THREADS, (size_t)0, a);
    else launch(k_detpost_labels<float>, gx, n_streams, DP_LABEL_THREADS, (size_t)0, a);
}

}  // namespace bm
