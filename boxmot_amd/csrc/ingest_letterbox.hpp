// Letterboxed detector input tensors from the frame ingest ring (include/boxmot_hip.h, boxmot_hip_ingest_letterbox): the one consumer
// that runs before the tracker is the caller's detector, and every YOLO-family detector takes a letterboxed, planar, normalised
// fp16 / fp32 tensor.  k_letterbox writes that tensor for all streams of a slot straight from the slot's BGR device frames.
//
// Definition.  For stream s let F be the slot's BGR frame, (rows, cols, 3) uint8; the output size (H, W) is common to the call.
// round() is round-half-to-even on a double (Python's round), int() truncates.
//     gain = min(H / rows, W / cols)                                              (double)
//     mode 0 "center"   (Ultralytics LetterBox, auto=False, scaleup=True, center=True):
//         new_w = round(cols * gain), new_h = round(rows * gain)
//         top = round((H - new_h) / 2 - 0.1), left = round((W - new_w) / 2 - 0.1)   = floor of half the padding: an odd padding
//                                                                                     puts the extra line at the bottom / right
//     mode 1 "topleft"  (YOLOX preproc): new_w = int(cols * gain), new_h = int(rows * gain), top = left = 0
//     new_w < 1 or new_h < 1 is an error (e.g. a 3 x 200 frame into 16 x 64, topleft: new_h = 0)
//     R = cv2.resize(F, (new_w, new_h), interpolation=INTER_LINEAR) as the crop kernels restate it (reid_kernels_v1.hpp
//         resize_axis_x / resize_axis_y / resize_sample_f, reused here, not restated): coordinate scales cols / new_w and
//         rows / new_h as doubles, 11-bit coefficients, x clamps and y clips, a plain copy when the size is unchanged and the 2 x 2
//         box filter when both axes shrink by exactly 2 (1280 x 720 into 640 x 640 takes it)
//     u(y, x, c) = R[y - top, x - left, c] inside the picture, the pad byte (default 114) elsewhere
//     O[s, p, y, x] = T[u(y, x, c)], planar (n, 3, H, W), contiguous; c = 2 - p for rgb (Ultralytics), c = p otherwise (YOLOX)
//     T: 256 entries built on the host, so the float result is exact by construction (as the crop kernels' lut):
//         unit, fp32: float32(v) / float32(255);  unit, fp16: that value rounded to fp16 (nearest even);  not unit: v itself
// (Parity with real OpenCV is as unpinned as the crops': DESIGN.md section 3.)
//
// One launch serves all streams: blockIdx.y is the stream, blockIdx.x a tile of LB_THREADS x 8 consecutive elements of the
// stream's (H, W) plane in row-major order.  A thread produces 8 neighbouring columns of one row (W % 8 == 0, so its 8 columns never
// wrap) for all three planes: one 16-byte store per plane for fp16, two for fp32; a wavefront writes 512 consecutive elements of each
// plane.  The tiling is over the flattened plane, not over (rows of threads) x (columns of threads), so that every lane has work at
// widths such as 640 (80 thread columns).  The frame pointer comes from the slot's table of frame pointers, the geometry from a
// per-stream table, and because the output size is common, streams of different frame sizes share the launch with one grid.
// Padding is written by the same threads: the whole (n, 3, H, W) block is defined after the launch.
//
// Taps are read straight from global memory: the two x taps of a sample are the 6 contiguous bytes of two neighbouring BGR pixels,
// one 4-byte and one 2-byte load per source row, never a byte beyond the row (letterbox_row_taps), so nothing past the frame is
// touched.  No LDS, no barrier, no cross-lane operation.  The path of the resize (copy, box filter, bilinear) is a property of the
// stream, so it is picked once per thread and the 8 pixels of a thread are straight-line code (letterbox_row8): the 32 tap loads of
// a thread are in flight together.  Measured: written with the path test and the inside-the-picture test
// around every pixel, each pixel waited for its own loads and the kernel took 215 us where this form takes less; wider 8-byte tap
// loads and a copy of the table in LDS both made it slower -- the kernel is bound by instruction issue, not by bytes.
// The resized value is within 0 .. 255 when the arithmetic is right and indexes T as it is: no clamp (ingest_nv12.hpp records how a
// shift followed by a clamp of two channels was miscompiled into v_ashr_pk_u8_i32 on gfx950).
#pragma once

#include <stdint.h>

#include <cmath>

#include "kernel_macros.hpp"
#include "reid_kernels_v1.hpp"

namespace bm {

constexpr int LB_THREADS = 256, LB_PX = 8;

struct LetterboxGeom { int rows, cols, new_w, new_h, top, left; };      // per stream

#ifndef BM_GLOBAL
// the frames' addresses come out of a table in memory, which makes them generic pointers to the compiler: this says they are
// global memory (global_load); the test harness defines it away
#define BM_GLOBAL __attribute__((address_space(1)))
#endif

typedef uint32_t lb_u32x4 __attribute__((vector_size(16), may_alias));
typedef uint32_t lb_u32_any __attribute__((aligned(1), may_alias));      // a BGR pixel starts at any byte address
typedef uint16_t lb_u16_any __attribute__((aligned(1), may_alias));

// The geometry of one frame size (the definition above); false where the picture would vanish.  mode: 0 center, 1 topleft.
inline bool letterbox_geometry(int rows, int cols, int H, int W, int mode, double* gain, LetterboxGeom* g) {
    const double gy = (double)H / (double)rows, gx = (double)W / (double)cols;
    const double k = gy < gx ? gy : gx;
    g->rows = rows; g->cols = cols;
    if (mode == 0) {
        g->new_w = (int)std::nearbyint((double)cols * k);               // (round-half-to-even: the default rounding mode)
        g->new_h = (int)std::nearbyint((double)rows * k);
        g->top = (int)std::nearbyint((double)(H - g->new_h) / 2.0 - 0.1);
        g->left = (int)std::nearbyint((double)(W - g->new_w) / 2.0 - 0.1);
    } else {
        g->new_w = (int)((double)cols * k);
        g->new_h = (int)((double)rows * k);
        g->top = g->left = 0;
    }
    if (gain) *gain = k;
    return g->new_w >= 1 && g->new_h >= 1;
}
// grid.x of the launch (grid.y = the stream count): the same for every stream, the output size being common
inline int letterbox_grid_x(int H, int W) { return (int)(((long)H * (W / LB_PX) + LB_THREADS - 1) / LB_THREADS); }

// The 2 x 2 neighbourhood a sample reads -- source rows (ya, yb), columns (xa, xb) with xb == xa + 1 or xb == xa -- as four 24-bit
// BGR pixels in registers.  It is handed to resize_sample_f as a picture of its own, 2 x 2 pixels: the sample is asked for at
// position (0, 0) with the tap indices (0, 1) in place of the source coordinates on both axes (the coefficients are the real
// ones), so every path of resize_sample_f -- the copy's (dy, dx), the box filter's (2 dy + 0 | 1, 2 dx + 0 | 1), the general
// (s0 | s1, s0 | s1) -- names its taps as (0 | 1, 0 | 1), constants the compiler resolves to a register each.
struct LetterboxTaps {
    uint32_t a0, a1, b0, b1;            // B | G << 8 | R << 16 of (ya, xa), (ya, xb), (yb, xa), (yb, xb)
    __device__ int operator()(int y, int x, int c) const {
        // masks, not ?: on the members: selecting between members becomes a select between their addresses, and that keeps the
        // whole struct in memory (the compiler put it into LDS) instead of in registers
        const uint32_t mx = 0u - (uint32_t)(x != 0), my = 0u - (uint32_t)(y != 0);
        const uint32_t a = a0 ^ ((a0 ^ a1) & mx), b = b0 ^ ((b0 ^ b1) & mx);
        return (int)(((a ^ ((a ^ b) & my)) >> (8 * c)) & 255u);
    }
};
// The pixels xa and xb of one source row.  WIDE (cols >= 2): always the 6 bytes of two neighbouring pixels, one 4-byte and one
// 2-byte load with no branch -- where xa is the row's last pixel (then xb == xa: the x axis clamps) the pair starts one pixel
// earlier, so nothing beyond the row is read.  Otherwise (a one-column frame) the pixel's 3 bytes.
template <bool WIDE>
__device__ inline void letterbox_row_taps(const BM_GLOBAL uint8_t* row, int xa, int xb, int cols, uint32_t& p0, uint32_t& p1) {
    if (WIDE) {
        const int at = xa < cols - 1 ? xa : cols - 2;
        const BM_GLOBAL uint8_t* px = row + (long)at * 3;
        const uint32_t lo = *(const BM_GLOBAL lb_u32_any*)px, hi = *(const BM_GLOBAL lb_u16_any*)(px + 4);
        const uint32_t first = lo & 0xffffffu, second = (lo >> 24) | (hi << 8);
        p0 = at == xa ? first : second;
        p1 = xb != xa ? second : p0;
    } else {
        p0 = p1 = (uint32_t)*(const BM_GLOBAL lb_u16_any*)row | ((uint32_t)row[2] << 16);
    }
}

// 8 neighbouring columns, from x0, of the picture row yy (0 <= yy < new_h) as B | G << 8 | R << 16 each; columns outside the
// picture are pad3.  PATH is the path of the resize, picked once per stream by the caller -- 0 copy, 1 exact 2 x box filter,
// 2 bilinear -- so that the 8 pixels are straight-line code: all tap loads are issued before the first is needed.  The picture's
// rows lie `stride` bytes apart (a rectangle of a larger frame: ingest_letterbox_tiles.hpp); g.cols bounds the taps, not the stride.
// resize_sample_f picks its path by comparing the picture's size with the output's; it is told the path with the smallest sizes
// that select it: 1 -> 1 (copy), 2 -> 1 (box filter), 2 -> 3 (bilinear).
template <int PATH, bool WIDE>
__device__ inline void letterbox_row8(const BM_GLOBAL uint8_t* src, long stride, const LetterboxGeom& g, int yy, int x0, uint32_t pad3,
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

// What one thread of the two letterbox kernels does: its 8 columns of one row of output tensor `tensor`, all three planes, from the
// picture at src with rows `stride` bytes apart and the geometry g.  blockIdx.x and threadIdx.x name the item (8 columns of one
// row each, row-major).  lut: the 256 entries of T as bit patterns, one 32-bit word each (fp32: the float's bits; fp16: the half's
// bits in the low 16).  out: (tensors, 3, H, W) of 2-byte (fp16 != 0) or 4-byte elements, 16-byte aligned; W % 8 == 0.
__device__ inline void letterbox_item(const BM_GLOBAL uint8_t* src, long stride, const LetterboxGeom& g, int tensor, const uint32_t* __restrict__ lut,
                                      void* __restrict__ out, int H, int W, int fp16, int rgb, int pad) {
    const int tcols = W / LB_PX;
    const long item = (long)blockIdx.x * LB_THREADS + (long)threadIdx.x;
    if (item >= (long)H * tcols) return;
    const int y = (int)(item / tcols), x0 = (int)(item - (long)y * tcols) * LB_PX;
    const bool same = g.cols == g.new_w && g.rows == g.new_h, half = g.cols == 2 * g.new_w && g.rows == 2 * g.new_h;     // (per picture)
    const uint32_t pad3 = (uint32_t)pad * 0x010101u;

    uint32_t u[LB_PX];                  // B | G << 8 | R << 16 of this thread's 8 columns of the letterboxed picture
    const int yy = y - g.top;
    if (yy < 0 || yy >= g.new_h) {
#pragma unroll
        for (int k = 0; k < LB_PX; ++k) u[k] = pad3;
    } else if (g.cols >= 2) {
        if (same) letterbox_row8<0, true>(src, stride, g, yy, x0, pad3, u);
        else if (half) letterbox_row8<1, true>(src, stride, g, yy, x0, pad3, u);
        else letterbox_row8<2, true>(src, stride, g, yy, x0, pad3, u);
    } else {                            // a one-column picture (never an exact 2 x: that needs an even width)
        if (same) letterbox_row8<0, false>(src, stride, g, yy, x0, pad3, u);
        else letterbox_row8<2, false>(src, stride, g, yy, x0, pad3, u);
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
        const long e = ((long)tensor * 3 + p) * plane + at;            // element index: a multiple of 8
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

// frames: the slot's [gridDim.y] frame pointers, geom: [gridDim.y]; lut, out, H, W, fp16, rgb, pad as letterbox_item's, out being
// (gridDim.y, 3, H, W).
__global__ void __launch_bounds__(LB_THREADS) k_letterbox(const uint8_t* const* __restrict__ frames, const LetterboxGeom* __restrict__ geom,
                                                          const uint32_t* __restrict__ lut, void* __restrict__ out, int H, int W, int fp16,
                                                          int rgb, int pad) {
    const int s = (int)blockIdx.y;
    const LetterboxGeom g = geom[s];
    letterbox_item((const BM_GLOBAL uint8_t*)frames[s], (long)g.cols * 3, g, s, lut, out, H, W, fp16, rgb, pad);
}

}  // namespace bm
