// Letterboxed detector input tensors of RECTANGLES of the ring's frames (include/boxmot_hip.h, boxmot_hip_ingest_letterbox_tiles):
// sliced inference on large frames.  A 4K frame letterboxed into 640 x 640 is shrunk 6 times and a 20-pixel pedestrian reaches the
// detector as 3 pixels; the usual answer is to letterbox overlapping tiles of the frame (and, optionally, the whole frame as one
// more tile), run the detector on all of them as one batch and merge the detections in frame coordinates (det_post_tiled.hpp).
// k_letterbox_tiles writes that batch for all streams and tiles of a slot with one launch.
//
// Definition.  Per call: T rectangles per stream, (x0, y0, w, h) in frame pixels, inside the frame, w, h >= 1; 1 <= T <= 64 and the
// same T for every stream (the rectangles themselves may differ per stream, as the frame sizes may).  With F the slot's BGR frame
// of stream s,
//     O[s * T + t] = what k_letterbox (ingest_letterbox.hpp, the definition at its top) writes for a stand-alone frame equal to
//                    F[y0 : y0 + h, x0 : x0 + w]
// -- the same geometry formulas with rows = h and cols = w, both modes; the same resize (resize_axis_x / resize_axis_y /
// resize_sample_f, reused, not restated) with its three paths, copy, exact 2 x box filter and bilinear, chosen by the RECTANGLE's
// size; taps clamp at the rectangle's edge and never read the frame's pixels beyond it; the same 256-entry table, rgb, unit, pad,
// fp16 / fp32.  A rectangle whose picture would vanish (new_w < 1 or new_h < 1) is an error naming the stream and tile.
// letterbox_tiles with the single rectangle (0, 0, cols, rows) is letterbox, byte for byte.
//
// What differs from k_letterbox: the source pointer is the frame's plus (y0 * cols_frame + x0) * 3, the row stride is the FRAME's
// (cols_frame * 3), not the rectangle's; blockIdx.y = s * T + t picks the output tensor and the entry of a per-(stream, tile)
// geometry table, blockIdx.y / T the frame pointer.  The access rules are k_letterbox's: the two x taps of a sample are the 6
// contiguous bytes of two neighbouring pixels of the rectangle's row (letterbox_row_taps with cols = w: the pair starts one pixel
// earlier where the tap is the rectangle's last column, so nothing right of the rectangle is read), a one-column rectangle takes the
// 3-byte path; rectangles with odd x0 put the source rows at any byte alignment, which those loads allow.  No LDS, no barrier, no
// cross-lane operation.  Both kernels are letterbox_item (ingest_letterbox.hpp), one body, called with their own source pointer,
// row stride, geometry and output tensor index.
#pragma once

#include "ingest_letterbox.hpp"

namespace bm {

constexpr int LB_TILES_MAX = 64;

struct LetterboxTileGeom {              // per (stream, tile)
    LetterboxGeom g;                    // rows, cols: the rectangle's h, w
    int stride, reserved;               // bytes between two rows of the frame
    long off;                           // (y0 * cols_frame + x0) * 3
};

// The geometry of one rectangle of a frame of frame_cols columns; false where the picture would vanish.
inline bool letterbox_tile_geometry(int frame_cols, int x0, int y0, int w, int h, int H, int W, int mode, double* gain, LetterboxTileGeom* t) {
    const bool ok = letterbox_geometry(h, w, H, W, mode, gain, &t->g);
    t->stride = frame_cols * 3;
    t->reserved = 0;
    t->off = ((long)y0 * frame_cols + x0) * 3;
    return ok;
}
inline bool letterbox_tile_inside(int frame_rows, int frame_cols, int x0, int y0, int w, int h) {
    return x0 >= 0 && y0 >= 0 && w >= 1 && h >= 1 && (long)x0 + w <= frame_cols && (long)y0 + h <= frame_rows;
}

// frames: the slot's [n_streams] frame pointers; geom: [gridDim.y] with gridDim.y = n_streams * n_tiles; lut, out, H, W, fp16, rgb,
// pad as k_letterbox: out is (gridDim.y, 3, H, W), 16-byte aligned, W % 8 == 0.
__global__ void __launch_bounds__(LB_THREADS) k_letterbox_tiles(const uint8_t* const* __restrict__ frames, const LetterboxTileGeom* __restrict__ geom,
                                                                const uint32_t* __restrict__ lut, void* __restrict__ out, int n_tiles, int H,
                                                                int W, int fp16, int rgb, int pad) {
    const int st = (int)blockIdx.y;
    const LetterboxTileGeom tg = geom[st];
    letterbox_item((const BM_GLOBAL uint8_t*)frames[st / n_tiles] + tg.off, (long)tg.stride, tg.g, st, lut, out, H, W, fp16, rgb, pad);
}

}  // namespace bm
