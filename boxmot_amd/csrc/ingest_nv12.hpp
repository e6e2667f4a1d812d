// NV12 -> BGR on the device for the frame ingest ring (include/boxmot_hip.h, boxmot_hip_ingest_*_nv12): decoders hand out NV12 -- a
// full-resolution Y plane followed by a half-resolution plane of interleaved (U, V) pairs, 1.5 bytes per pixel -- and every kernel
// downstream of the ring reads packed (rows, cols, 3) uint8 BGR.  k_nv12_to_bgr writes exactly those frames.
//
// The conversion is cv2.cvtColor(..., COLOR_YUV2BGR_NV12) restated: BT.601 limited range in 20-bit fixed point (OpenCV's
// color_yuv.simd.hpp, ITUR_BT_601_*).  For the pixel (r, c) with Y = y[r][c], U = uv[r / 2][2 (c / 2)], V = uv[r / 2][2 (c / 2) + 1]:
//     yy = max(Y - 16, 0) * CY + (1 << 19) ;  u = U - 128 ;  v = V - 128
//     B = sat_u8((yy + CUB u) >> 20)   G = sat_u8((yy + CVG v + CUG u) >> 20)   R = sat_u8((yy + CVR v) >> 20)
// Every intermediate fits int32 (|yy + CUB u| < 2^30), so the kernel is 32-bit integer arithmetic throughout; a negative sum
// saturates to 0, so how the shift rounds negatives cannot matter.  (OpenCV itself is absent offline: DESIGN.md section 3.)
//
// One launch converts all streams of a slot: blockIdx.y is the stream, blockIdx.x a tile of NV12_TILE_X x NV12_TILE_Y threads; the
// grid is as wide as the stream with the most tiles and the workgroups beyond a stream's own tile count exit, which is how streams of
// different sizes share the launch.  A thread owns a block of 2 rows, so the chroma bytes are loaded once and serve both rows:
//   wide    2 rows x 8 columns per thread: two 8-byte Y loads, one 8-byte UV load, 2 x 24 bytes of BGR as three 8-byte stores per row.
//           The 64 lanes of a wavefront cover 512 contiguous bytes of each Y row and of the UV row and 1536 contiguous bytes of each
//           BGR row.  Taken only when cols % 8 == 0, both pitches are multiples of 8 and the three base addresses are 8-byte aligned:
//           a BGR row starts at r * cols * 3, which is a multiple of 8 exactly when cols is.
//   narrow  2 rows x 2 columns per thread, byte accesses: every other (even) size, pitch and alignment.
// Both paths compute a pixel with the same function, so they give identical bytes.  No LDS.
#pragma once

#include <stdint.h>

#include "kernel_macros.hpp"

namespace bm {

constexpr int NV12_THREADS = 256, NV12_TILE_X = 64, NV12_TILE_Y = NV12_THREADS / NV12_TILE_X;
constexpr int NV12_CY = 1220542, NV12_CUB = 2116026, NV12_CUG = -409993, NV12_CVG = -852492, NV12_CVR = 1673527, NV12_SHIFT = 20;

struct Nv12Desc {                       // per stream: the NV12 surface (pitch >= cols, in bytes) and the packed BGR frame it becomes
    const uint8_t* y;
    const uint8_t* uv;
    int pitch_y, pitch_uv, rows, cols;  // rows and cols even
    uint8_t* dst;
};

typedef uint32_t nv12_u32x2 __attribute__((vector_size(8), may_alias));
#ifndef BM_GLOBAL
// the planes' addresses come out of a table in memory, which makes them generic pointers (flat_load / flat_store) to the compiler:
// this says they are global memory (global_load / global_store); the test harness defines it away
#define BM_GLOBAL __attribute__((address_space(1)))
#endif

__host__ __device__ inline bool nv12_wide(const Nv12Desc& d) {
    return d.cols % 8 == 0 && d.pitch_y % 8 == 0 && d.pitch_uv % 8 == 0 && (((uintptr_t)d.y | (uintptr_t)d.uv | (uintptr_t)d.dst) & 7) == 0;
}
// thread columns of a stream (one per 8 / 2 pixel columns), and its tile count
__host__ __device__ inline int nv12_thread_cols(const Nv12Desc& d) { return nv12_wide(d) ? d.cols / 8 : d.cols / 2; }
__host__ __device__ inline int nv12_tiles_x(const Nv12Desc& d) { return (nv12_thread_cols(d) + NV12_TILE_X - 1) / NV12_TILE_X; }
__host__ __device__ inline int nv12_tiles(const Nv12Desc& d) { return nv12_tiles_x(d) * ((d.rows / 2 + NV12_TILE_Y - 1) / NV12_TILE_Y); }
// grid.x of the launch that converts these streams (grid.y = n)
inline int nv12_grid_x(const Nv12Desc* d, int n) {
    int g = 1;
    for (int s = 0; s < n; ++s) g = nv12_tiles(d[s]) > g ? nv12_tiles(d[s]) : g;
    return g;
}

// sat_u8(v >> 20) with the clamp BEFORE the shift (the same value: a negative sum gives 0, a sum of 256 << 20 or more gives 255).
// Written as shift-then-clamp, two channels are matched into one v_ashr_pk_u8_i32 by hipcc (ROCm 7), and that instruction's result
// reached the byte packing below with stale upper 16 bits on gfx950: a quarter of the bytes of a frame came out wrong on the device
// while the same source was exact on CPU threads.  tests/test_gpu_nv12.py runs all 2^24 triples on the device for this reason.
__device__ inline uint32_t nv12_sat(int v) {
    const int top = (256 << NV12_SHIFT) - 1;
    v = v < 0 ? 0 : (v > top ? top : v);
    return (uint32_t)v >> NV12_SHIFT;
}
struct Nv12Chroma { int b, g, r; };     // the chroma terms a 2 x 2 block shares
__device__ inline Nv12Chroma nv12_chroma(int U, int V) {
    const int u = U - 128, v = V - 128;
    return Nv12Chroma{NV12_CUB * u, NV12_CVG * v + NV12_CUG * u, NV12_CVR * v};
}
// the pixel as its three bytes in memory order: B | G << 8 | R << 16
__device__ inline uint32_t nv12_pixel(int Y, const Nv12Chroma& c) {
    const int yy = (Y > 16 ? Y - 16 : 0) * NV12_CY + (1 << (NV12_SHIFT - 1));
    return nv12_sat(yy + c.b) | (nv12_sat(yy + c.g) << 8) | (nv12_sat(yy + c.r) << 16);
}
// 8 pixels of one row -> the 24 bytes of their BGR triples as six little-endian words
__device__ inline void nv12_row8(nv12_u32x2 yv, const Nv12Chroma* c, BM_GLOBAL uint8_t* out) {
    uint32_t p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = nv12_pixel((int)((yv[k >> 2] >> (8 * (k & 3))) & 255u), c[k >> 1]);
    nv12_u32x2 w0, w1, w2;              // every 4 pixels (12 bytes) fill 3 words: p0 | p1 << 24, p1 >> 8 | p2 << 16, p2 >> 16 | p3 << 8
    w0[0] = p[0] | (p[1] << 24); w0[1] = (p[1] >> 8) | (p[2] << 16);
    w1[0] = (p[2] >> 16) | (p[3] << 8); w1[1] = p[4] | (p[5] << 24);
    w2[0] = (p[5] >> 8) | (p[6] << 16); w2[1] = (p[6] >> 16) | (p[7] << 8);
    BM_GLOBAL nv12_u32x2* o = (BM_GLOBAL nv12_u32x2*)out;
    o[0] = w0; o[1] = w1; o[2] = w2;
}

__global__ void __launch_bounds__(NV12_THREADS) k_nv12_to_bgr(const Nv12Desc* __restrict__ descs) {
    const Nv12Desc d = descs[blockIdx.y];
    const int tile = (int)blockIdx.x;
    if (tile >= nv12_tiles(d)) return;                    // (workgroup-uniform) a smaller stream of a mixed launch
    const bool wide = nv12_wide(d);
    const int tiles_x = nv12_tiles_x(d);
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int tc = tile_x * NV12_TILE_X + (int)(threadIdx.x % NV12_TILE_X);       // a wavefront = 64 neighbouring columns of one row pair
    const int tr = tile_y * NV12_TILE_Y + (int)(threadIdx.x / NV12_TILE_X);
    if (tc >= nv12_thread_cols(d) || tr >= d.rows / 2) return;
    const BM_GLOBAL uint8_t* y0 = (const BM_GLOBAL uint8_t*)d.y + (long)(2 * tr) * d.pitch_y;
    const BM_GLOBAL uint8_t* y1 = y0 + d.pitch_y;
    const BM_GLOBAL uint8_t* uv = (const BM_GLOBAL uint8_t*)d.uv + (long)tr * d.pitch_uv;
    BM_GLOBAL uint8_t* o0 = (BM_GLOBAL uint8_t*)d.dst + (long)(2 * tr) * d.cols * 3;
    BM_GLOBAL uint8_t* o1 = o0 + (long)d.cols * 3;
    if (wide) {
        const nv12_u32x2 ya = *(const BM_GLOBAL nv12_u32x2*)(y0 + 8 * tc);
        const nv12_u32x2 yb = *(const BM_GLOBAL nv12_u32x2*)(y1 + 8 * tc);
        const nv12_u32x2 cv = *(const BM_GLOBAL nv12_u32x2*)(uv + 8 * tc);
        Nv12Chroma c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pair = cv[k >> 1] >> (16 * (k & 1));
            c[k] = nv12_chroma((int)(pair & 255u), (int)((pair >> 8) & 255u));
        }
        nv12_row8(ya, c, o0 + 24 * tc);
        nv12_row8(yb, c, o1 + 24 * tc);
    } else {
        const Nv12Chroma c = nv12_chroma(uv[2 * tc], uv[2 * tc + 1]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t p = nv12_pixel(y0[2 * tc + k], c), q = nv12_pixel(y1[2 * tc + k], c);
            BM_GLOBAL uint8_t* a = o0 + 6 * tc + 3 * k;
            BM_GLOBAL uint8_t* b = o1 + 6 * tc + 3 * k;
            a[0] = (uint8_t)p; a[1] = (uint8_t)(p >> 8); a[2] = (uint8_t)(p >> 16);
            b[0] = (uint8_t)q; b[1] = (uint8_t)(q >> 8); b[2] = (uint8_t)(q >> 16);
        }
    }
}

}  // namespace bm
