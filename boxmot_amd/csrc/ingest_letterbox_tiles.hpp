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
// cross-lane operation.
// letterbox_tile_row8 is letterbox_row8 with the row stride as an argument; k_letterbox itself is left exactly as it is.
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

// letterbox_row8 (ingest_letterbox.hpp) for a picture whose rows lie `stride` bytes apart: g.cols bounds the taps, not the stride
template <int PATH, bool WIDE>
__device__ inline void letterbox_tile_row8(const BM_GLOBAL uint8_t* src, long stride, const LetterboxGeom& g, int yy, int x0, uint32_t pad3,
                                           uint32_t (&u)[LB_PX]) {
    ResizeAxis ay{0, 0, 0, 0};
    if (PATH == 2) ay = resize_axis_y(yy, g.new_h, g.rows);
    const int ya = PATH == 0 ? yy : (PATH == 1 ? 2 * yy : ay.s0), yb = PATH == 0 ? yy : (PATH == 1 ? 2 * yy + 1 : ay.s1);
    const BM_GLOBAL uint8_t* row_a = src + (long)ya * stride;
    const BM_GLOBAL uint8_t* row_b = src + (long)yb * stride;
    const CropRect r{0, 0, PATH == 0 ? 1 : 2, PATH == 0 ? 1 : 2};
    const int out_n = PATH == 2 ? 3 : 1;
#pragma unroll
    for (int k = 0; k < LB_PX; ++k) {
        const int xx = x0 + k - g.left;
        const int xc = xx < 0 ? 0 : (xx < g.new_w ? xx : g.new_w - 1);         // a column of the picture in any case: the loads are valid
        ResizeAxis ax{0, 0, 0, 0};
        if (PATH == 2) ax = resize_axis_x(xc, g.new_w, g.cols);
        const int xa = PATH == 0 ? xc : (PATH == 1 ? 2 * xc : ax.s0), xb = PATH == 0 ? xc : (PATH == 1 ? 2 * xc + 1 : ax.s1);
        LetterboxTaps t;
        letterbox_row_taps<WIDE>(row_a, xa, xb, g.cols, t.a0, t.a1);
        letterbox_row_taps<WIDE>(row_b, xa, xb, g.cols, t.b0, t.b1);
        const ResizeAxis tx{0, 1, ax.a0, ax.a1}, ty{0, 1, ay.a0, ay.a1};
        const uint32_t p = (uint32_t)resize_sample_f(t, r, tx, ty, 0, 0, 0, out_n, out_n) | ((uint32_t)resize_sample_f(t, r, tx, ty, 0, 0, 1, out_n, out_n) << 8) |
                           ((uint32_t)resize_sample_f(t, r, tx, ty, 0, 0, 2, out_n, out_n) << 16);
        u[k] = xx == xc ? p : pad3;
    }
}

// frames: the slot's [n_streams] frame pointers; geom: [gridDim.y] with gridDim.y = n_streams * n_tiles; lut, out, H, W, fp16, rgb,
// pad as k_letterbox: out is (gridDim.y, 3, H, W), 16-byte aligned, W % 8 == 0.
__global__ void __launch_bounds__(LB_THREADS) k_letterbox_tiles(const uint8_t* const* __restrict__ frames, const LetterboxTileGeom* __restrict__ geom,
                                                                const uint32_t* __restrict__ lut, void* __restrict__ out, int n_tiles, int H,
                                                                int W, int fp16, int rgb, int pad) {
    const int st = (int)blockIdx.y, s = st / n_tiles;
    const int tcols = W / LB_PX;
    const long item = (long)blockIdx.x * LB_THREADS + (long)threadIdx.x;       // 8 columns of one row each, row-major
    if (item >= (long)H * tcols) return;
    const int y = (int)(item / tcols), x0 = (int)(item - (long)y * tcols) * LB_PX;
    const LetterboxTileGeom tg = geom[st];
    const LetterboxGeom g = tg.g;
    const long stride = (long)tg.stride;
    const BM_GLOBAL uint8_t* src = (const BM_GLOBAL uint8_t*)frames[s] + tg.off;
    const bool same = g.cols == g.new_w && g.rows == g.new_h, half = g.cols == 2 * g.new_w && g.rows == 2 * g.new_h;     // (per tile)
    const uint32_t pad3 = (uint32_t)pad * 0x010101u;

    uint32_t u[LB_PX];                  // B | G << 8 | R << 16 of this thread's 8 columns of the letterboxed picture
    const int yy = y - g.top;
    if (yy < 0 || yy >= g.new_h) {
#pragma unroll
        for (int k = 0; k < LB_PX; ++k) u[k] = pad3;
    } else if (g.cols >= 2) {
        if (same) letterbox_tile_row8<0, true>(src, stride, g, yy, x0, pad3, u);
        else if (half) letterbox_tile_row8<1, true>(src, stride, g, yy, x0, pad3, u);
        else letterbox_tile_row8<2, true>(src, stride, g, yy, x0, pad3, u);
    } else {                            // a one-column rectangle (never an exact 2 x: that needs an even width)
        if (same) letterbox_tile_row8<0, false>(src, stride, g, yy, x0, pad3, u);
        else letterbox_tile_row8<2, false>(src, stride, g, yy, x0, pad3, u);
    }
    uint32_t v[3][LB_PX];               // the table entries per output plane
#pragma unroll
    for (int k = 0; k < LB_PX; ++k) {
        const uint32_t b = u[k] & 255u, gr = (u[k] >> 8) & 255u, rd = u[k] >> 16;
        v[0][k] = lut[rgb ? rd : b];
        v[1][k] = lut[gr];
        v[2][k] = lut[rgb ? b : rd];
    }

    const long plane = (long)H * W, at = (long)y * W + x0;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const long e = ((long)st * 3 + p) * plane + at;                // element index: a multiple of 8
        if (fp16) {
            lb_u32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = v[p][2 * j] | (v[p][2 * j + 1] << 16);
            *(lb_u32x4*)((uint16_t*)out + e) = w;
        } else {
            lb_u32x4 w0, w1;
#pragma unroll
            for (int j = 0; j < 4; ++j) { w0[j] = v[p][j]; w1[j] = v[p][4 + j]; }
            lb_u32x4* o = (lb_u32x4*)((uint32_t*)out + e);
            o[0] = w0; o[1] = w1;
        }
    }
}

}  // namespace bm
