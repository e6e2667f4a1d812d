// Segmentation masks of the emitted rows, decoded on the device (include/boxmot_hip.h, boxmot_hip_detpost_create_mask / _run_mask):
// a *-seg head's 32 mask coefficients per anchor reach d_extra through det_post_extra.hpp; this multiplies them with the model's
// prototype tensor, crops to the row's box and thresholds, so that d_masks[s][det_ind] is the mask of the detection a track was
// matched to.  Includes det_post_tiled.hpp (and so det_post.hpp, det_post_extra.hpp).
//
// Definition, step 9 after steps 7-8 at the top of det_post_extra.hpp.  A MASK HANDLE is an extras handle with extra_kind 0 "raw",
// n_extra = E (1 <= E <= 256; Ultralytics: 32) and four more creation-time integers: mask_h, mask_w (1..1024 each), the prototypes'
// size, and in_h, in_w (>= 1), the detector's input size.  The host computes two float32 ratios once, at creation, each with one
// IEEE float32 division:
//     wr = (float)mask_w / (float)in_w            hr = (float)mask_h / (float)in_h
// Per call there is one more input, proto: a contiguous tensor (N, E, mask_h, mask_w), fp16 or fp32 independently of pred's dtype
// (fp16 widens exactly); untiled one tensor per stream, tiled one per (stream, tile) at index s * T + t, like pred.
// 9. Masks.  For every emitted row r < d_det_rows[s]:
//      a = src[s][r]; on a tiled handle t = a / A, a -= t * A.  The tensor index is ps = s untiled, ps = s * T + t tiled.
//      c[k] = extra[s][r][k], the raw coefficient, as step 8 wrote it: it is read back from d_extra.
//      x1, y1, x2, y2 = step 3's letterbox-space box of that anchor, recomputed from pred[ps]: cx - w * 0.5f and so on.  The box is
//          neither clipped nor mapped to the frame: masks live in the letterbox space of the tensor that produced them (a tile's
//          letterbox on a tiled handle; the tile of a tiled row is d_src / n_anchors).
//      logit(i, j): acc = 0.0f; for k = 0 .. E - 1 ascending: acc = acc + c[k] * proto[ps][k][i][j] -- every multiply and every add
//          rounded separately to fp32 (-ffp-contract=off), in that order.
//      masks[s][r][i][j], a uint8, is 1 when ALL of
//          (float)j >= x1 * wr     (float)j < x2 * wr     (float)i >= y1 * hr     (float)i < y2 * hr     logit(i, j) > 0.0f
//      hold, else 0.  The window test is Ultralytics crop_mask's >= / <, the logit test is masks.gt_(0.0); the whole is a reading of
//      process_mask(..., upsample=False).  A NaN logit, a NaN box edge, a logit of exactly +-0, an empty window and a window wholly
//      off the tensor all give 0 without special cases: every comparison with a NaN is false.
//    Every byte of an emitted row's mask_h * mask_w plane is written, zeros outside the window.  Rows at and beyond the count,
//    streams beyond n_streams, all other blocks and the counters are not touched.
// Stated plainly: this is pinned against this repository's NumPy restatement (tests/detpost_mask_ref.py) only, not against
// Ultralytics.  The mask is at PROTOTYPE resolution in letterbox (or tile-letterbox) space; bilinear upsampling to the input or
// the frame size (upsample=True, scale_masks) stays the caller's.  There are no masks for the oriented layout "cn_obb".
//
// Kernel.  k_detpost_mask<T, P> (T: pred's type, P: proto's) runs fourth on the caller's stream, after k_detpost_extra: grid
// (max_det, S), one workgroup of DP_MASK_THREADS per (row, stream), which leaves at once for row >= det_rows[s] -- det_rows, src
// and extra are read from device memory, no host sync.  The coefficients' address and the four window edges are the same in every
// lane (wavefront-uniform).  The workgroup walks the plane, which is contiguous, in groups of G pixels of one mask row, consecutive
// lanes on consecutive groups, so the stores of a wavefront are one contiguous run and so are its prototype loads within a plane:
//     wide path, G = 4   mask_w a multiple of 4, d_masks 4-byte aligned, d_proto aligned to 4 of its elements (detpost_launch_mask
//                        checks): one 8- (fp16) or 16-byte (fp32) prototype load per plane and one dword of four mask bytes per lane
//     byte path, G = 1   any other width or alignment (mask_w = 9: rows start at every byte phase): one element, one byte per lane
// A group wholly outside the window stores zeros and loads nothing -- that is where nearly all the arithmetic is saved; a group
// of the wide path that the window cuts loads its whole 8 / 16 bytes (inside the plane; up to three pixels beside the window's left
// and right edge) and the window test then zeroes the pixels outside.  The window test is the definition's own float comparisons,
// per pixel, not integer bounds derived from them.  The chain over k is kept sequential per pixel; the loads of DP_MASK_UNROLL
// planes are issued before the first is used.  No LDS, no atomics, no inline assembly, plain vector stores.
// The kernel has an argument struct of its own, DetPostMaskArgs, beside a DetPostArgs by value: nothing is added to DetPostArgs or
// DetPostTiledArgs, so every other kernel stays what it was instruction for instruction (det_post.hpp's dp_at explains why).
#pragma once

#include "det_post_tiled.hpp"

namespace bm {

constexpr int DP_MASK_THREADS = 256, DP_MASK_E_MAX = 256, DP_MASK_DIM_MAX = 1024, DP_MASK_UNROLL = 8;

struct DetPostMaskArgs {
    const void* proto;              // (S [* T], E, mask_h, mask_w), fp16 or fp32
    uint8_t* masks;                 // [S][out_stride][mask_h][mask_w], out_stride: DetPostArgs'
    long proto_stride;              // elements per tensor: E * mask_h * mask_w
    int plane;                      // mask_h * mask_w: elements per prototype plane, bytes per mask
    int mask_h, mask_w;
    float wr, hr;                   // (float)mask_w / (float)in_w, (float)mask_h / (float)in_h
    int wide;                       // 1: the G = 4 path (detpost_launch_mask sets it)
};

template <class P, int G> struct DpMaskVec;
template <> struct DpMaskVec<float, 4> { typedef float type __attribute__((vector_size(16), may_alias)); };
template <> struct DpMaskVec<_Float16, 4> { typedef _Float16 type __attribute__((vector_size(8), may_alias)); };
typedef uint32_t dp_mask_word __attribute__((may_alias));

// G neighbouring prototype values, widened
template <int G, class P>
__device__ inline void dp_mask_load(const P* p, float (&v)[G]) {
    if constexpr (G == 1) {
        v[0] = (float)p[0];
    } else {
        const typename DpMaskVec<P, G>::type x = *reinterpret_cast<const typename DpMaskVec<P, G>::type*>(p);
#pragma unroll
        for (int u = 0; u < G; ++u) v[u] = (float)x[u];
    }
}

// one (row, stream): the plane of `masks` from the coefficients c[0..E), the prototype planes `proto` and the window's edges
template <int G, class P>
__device__ inline void dp_mask_plane(const DetPostMaskArgs& m, const float* __restrict__ c, int E, const P* __restrict__ proto, uint8_t* __restrict__ masks,
                                     float wx1, float wx2, float wy1, float wy2) {
    const int per_row = m.mask_w / G, groups = m.mask_h * per_row;
    for (int p = (int)threadIdx.x; p < groups; p += DP_MASK_THREADS) {
        const int i = p / per_row, j0 = (p - i * per_row) * G;
        const float fi = (float)i;
        const bool in_y = fi >= wy1 && fi < wy2;
        bool in[G], any = false;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const float fj = (float)(j0 + u);
            in[u] = in_y && fj >= wx1 && fj < wx2;
            any = any || in[u];
        }
        uint32_t word = 0u;
        if (any) {
            const P* at = proto + (long)i * m.mask_w + j0;
            float acc[G];
#pragma unroll
            for (int u = 0; u < G; ++u) acc[u] = 0.0f;
            int k = 0;
            for (; k + DP_MASK_UNROLL <= E; k += DP_MASK_UNROLL) {
                float v[DP_MASK_UNROLL][G];
#pragma unroll
                for (int q = 0; q < DP_MASK_UNROLL; ++q) dp_mask_load<G>(at + (long)(k + q) * m.plane, v[q]);
#pragma unroll
                for (int q = 0; q < DP_MASK_UNROLL; ++q) {
                    const float ck = c[k + q];
#pragma unroll
                    for (int u = 0; u < G; ++u) acc[u] = acc[u] + ck * v[q][u];
                }
            }
            for (; k < E; ++k) {
                float v[G];
                dp_mask_load<G>(at + (long)k * m.plane, v);
                const float ck = c[k];
#pragma unroll
                for (int u = 0; u < G; ++u) acc[u] = acc[u] + ck * v[u];
            }
#pragma unroll
            for (int u = 0; u < G; ++u) word |= (in[u] && acc[u] > 0.0f ? 1u : 0u) << (8 * u);
        }
        if constexpr (G == 1) masks[p] = (uint8_t)word;
        else *reinterpret_cast<dp_mask_word*>(masks + (long)p * G) = word;      // (little-endian: byte u is pixel j0 + u)
    }
}

// n_tiles: a tiled call's T, else 0
template <class T, class P>
__global__ void __launch_bounds__(DP_MASK_THREADS) k_detpost_mask(DetPostArgs g, DetPostMaskArgs m, int n_tiles) {
    const int s = (int)blockIdx.y, row = (int)blockIdx.x;
    if (row >= g.det_rows[s]) return;                           // (det_rows[s] <= max_det = gridDim.x <= src_stride, out_stride)
    const T* pred = static_cast<const T*>(g.pred);
    int a = g.src[(long)s * g.src_stride + row], ps = s;
    if (n_tiles) {
        const int tile = a / g.A;
        a -= tile * g.A;
        ps = s * n_tiles + tile;
    }
    const float cx = dp_load(pred, dp_at<true>(g, ps, a, 0)), cy = dp_load(pred, dp_at<true>(g, ps, a, 1));
    const float w = dp_load(pred, dp_at<true>(g, ps, a, 2)), h = dp_load(pred, dp_at<true>(g, ps, a, 3));
    const float x1 = cx - w * 0.5f, y1 = cy - h * 0.5f, x2 = cx + w * 0.5f, y2 = cy + h * 0.5f;
    const float wx1 = x1 * m.wr, wx2 = x2 * m.wr, wy1 = y1 * m.hr, wy2 = y2 * m.hr;
    const long at = (long)s * g.out_stride + row;
    const float* c = g.extra + at * g.n_extra;
    const P* proto = static_cast<const P*>(m.proto) + (long)ps * m.proto_stride;
    uint8_t* masks = m.masks + at * m.plane;
    if (m.wide) dp_mask_plane<4>(m, c, g.n_extra, proto, masks, wx1, wx2, wy1, wy2);
    else dp_mask_plane<1>(m, c, g.n_extra, proto, masks, wx1, wx2, wy1, wy2);
}

// The fourth kernel of a call on a mask handle (g as detpost_launch_extra's; n_tiles of a tiled call, else 0).  Chooses the wide path.
template <class L>
inline void detpost_launch_mask(L& launch, const DetPostArgs& g, const DetPostMaskArgs& args, int n_tiles, int n_streams, int fp16, int proto_fp16) {
    DetPostMaskArgs m = args;
    m.wide = m.mask_w % 4 == 0 && (uintptr_t)m.masks % 4 == 0 && (uintptr_t)m.proto % (proto_fp16 ? 8 : 16) == 0;
    if (fp16) {
        if (proto_fp16) launch(k_detpost_mask<_Float16, _Float16>, g.max_det, n_streams, DP_MASK_THREADS, (size_t)0, g, m, n_tiles);
        else launch(k_detpost_mask<_Float16, float>, g.max_det, n_streams, DP_MASK_THREADS, (size_t)0, g, m, n_tiles);
    } else {
        if (proto_fp16) launch(k_detpost_mask<float, _Float16>, g.max_det, n_streams, DP_MASK_THREADS, (size_t)0, g, m, n_tiles);
        else launch(k_detpost_mask<float, float>, g.max_det, n_streams, DP_MASK_THREADS, (size_t)0, g, m, n_tiles);
    }
}

// The kernel sequences of one call on a mask handle: detpost_launch / detpost_launch_tiled as they are, then the masks.
template <class L>
inline void detpost_launch_with_mask(L& launch, const DetPostArgs& g, const DetPostMaskArgs& m, int n_streams, int fp16, int proto_fp16, size_t* lds_bytes = nullptr) {
    detpost_launch(launch, g, n_streams, fp16, lds_bytes);
    detpost_launch_mask(launch, g, m, 0, n_streams, fp16, proto_fp16);
}
template <class L>
inline void detpost_launch_tiled_with_mask(L& launch, const DetPostTiledArgs& ta, const DetPostMaskArgs& m, int n_streams, int fp16, int proto_fp16,
                                           size_t* lds_bytes = nullptr) {
    detpost_launch_tiled(launch, ta, n_streams, fp16, lds_bytes);
    detpost_launch_mask(launch, ta.base, m, ta.T, n_streams, fp16, proto_fp16);
}

}  // namespace bm
