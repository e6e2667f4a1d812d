// Device-side detection post-processing (include/boxmot_hip.h, boxmot_hip_detpost_*): from a YOLO-family detector's raw prediction
// tensor on the device to the d_dets [S][stride][6] / d_det_rows [S] block the device-resident tracker steps read, in frame
// coordinates, with no host round trip.  The detector itself stays the caller's.
//
// Definition.  All arithmetic is fp32 (the library is built with -ffp-contract=off: no fused multiply-add); fp16 inputs are widened
// exactly.  Per call, for the streams s < n_streams:
//     pred      one contiguous tensor, fp16 or fp32, in one of two layouts (A anchors, nc >= 1 classes):
//         layout 0 "cn"      (Ultralytics v8 / 11 raw head)   (S, 4 + nc, A): channel rows 0..3 are cx, cy, w, h in letterbox pixels,
//                            rows 4.. the class scores; conf = max_c score[c]
//         layout 1 "nc_obj"  (YOLOX / YOLOv5 decoded head)    (S, A, 5 + nc): a row is cx, cy, w, h, obj, score[0..nc);
//                            conf = obj * max_c score[c], one fp32 multiply
//     geom[s]   gain, top, left, rows, cols of the stream's letterbox (boxmot_hip_letterbox_geometry), as float32 each
//     options   fixed at creation: conf_thres (0 <= . < 1), iou_thres, max_candidates K (64..4096), max_det, agnostic, and an
//               optional class allow-list, an nc-entry 0 / 1 table
// 1. Score.  cls = the index of the largest score, the lowest index on a tie: the scan starts from (-inf, class 0) and a class
//    replaces the best so far when its score is strictly greater -- so a NaN score is never the maximum (as fmaxf ignores it), and
//    an anchor whose scores are all NaN has conf = -inf.  The anchor passes iff conf > conf_thres, STRICTLY -- Ultralytics' rule;
//    YOLOX's own `>=` is deliberately not reproduced -- and, where an allow-list is given, allow[cls] != 0 (the list is applied after
//    the argmax, as Ultralytics applies `classes`).  A NaN conf (a NaN obj) never passes: the comparison is false.
// 2. Select.  Of the passing anchors the K largest by (conf descending, anchor index ascending); all of them, in that order, when
//    no more than K pass.  The selection is exact when more pass: ties at the K boundary go to the lowest anchor indices.
// 3. Box.  x1 = cx - w * 0.5f, y1 = cy - h * 0.5f, x2 = cx + w * 0.5f, y2 = cy + h * 0.5f, in letterbox pixels.
// 4. NMS.  Greedy, in that order, on the letterbox-space boxes: candidate i is kept unless an earlier KEPT candidate j suppresses
//    it; class-aware NMS lets only a j with cls_j == cls_i suppress, agnostic any j.  j suppresses i when
//        inter / (area_i + area_j - inter) > iou_thres                                     (torchvision's nms arithmetic)
//        area = (x2 - x1) * (y2 - y1)
//        inter = max(min(x2_i, x2_j) - max(x1_i, x1_j), 0) * max(min(y2_i, y2_j) - max(y1_i, y1_j), 0)      (fmaxf / fminf)
//    0 / 0 compares false and does not suppress.  Class awareness is BY COMPARING CLASSES, not by Ultralytics' `cls * max_wh`
//    coordinate offset: the offset moves every box by up to nc * 7680 pixels before the arithmetic above and so rounds differently.
// 5. Emit.  The first max_det kept candidates, in order, become the rows [x1, y1, x2, y2, conf, cls] of d_dets[s], the coordinates
//    through LetterboxGeometry.to_frame's arithmetic: clip((x - left) / gain, 0, cols), clip((y - top) / gain, 0, rows) -- one fp32
//    subtraction, one correctly rounded fp32 division, clip(v, lo, hi) = min(max(v, lo), hi).  d_det_rows[s] = the number of rows
//    written; rows at and beyond it are not touched.
// 6. Counters.  counters[s] = {anchors that passed step 1, candidates after step 2, candidates kept by NMS before the max_det cut}.
// The oriented layout "cn_obb" (layout 0 with obb = 1: one more channel row, the angle, after the classes; 7-column rows; rotated NMS)
// is defined at the top of det_post_obb.hpp; it shares the score kernels, stages a-c and the kernel sequence below.
// Heads with E more values per anchor after the class scores (pose keypoints, mask coefficients) are defined at the top of
// det_post_extra.hpp: steps 1-6 read none of them, steps 7-8 write the source anchor and the extras of every emitted row.  Step 9,
// the segmentation masks of the emitted rows from raw coefficients and the model's prototypes, is at the top of det_post_mask.hpp.
// (Parity with torchvision / Ultralytics on real detector output is not pinned by any test: tests/detpost_ref.py restates this
// definition in NumPy, and the kernels are compared with that, bit for bit.)
//
// Kernels.
//   k_detpost_score<T>   grid (ceil(A / 256), S), one thread per anchor: the scan over the nc scores and one 32-bit key per anchor
//       into the handle's scratch -- the conf's bit pattern, or 0 for "did not pass" (for conf > conf_thres >= 0 fp32 bit patterns
//       order like unsigned integers, and are not 0) -- plus the class.  "cn": channel rows are contiguous over anchors, every load
//       of a wavefront is one coalesced run; a 16-byte aligned "cn" tensor with A a multiple of 8 (fp16) / 4 (fp32) goes through
//       k_detpost_score_cn_vec instead, 8 / 4 neighbouring anchors per thread and one 16-byte load per channel row (measured: 74 ->
//       35 us for 64 streams of 8400 x 84 fp16).  "nc_obj": a thread walks its own row; the 64 rows of a wavefront are one contiguous
//       run of memory that the wavefront consumes completely, line by line out of the cache, but a single load instruction is
//       strided -- there is no LDS transpose here.
//   k_detpost_select<T>  one workgroup of DP_THREADS per stream does the rest out of dynamic LDS (a-c are dp_select_sort, which the
//       oriented kernel of det_post_obb.hpp shares):
//       a. the passing count, and when more than K pass an exact radix select of the K-th largest key: four passes of an 8-bit
//          histogram (integer LDS atomics: order-independent) over the keys that match the prefix found so far (the counting sweep
//          fills the first pass's histogram); every sweep over the anchors loads DP_SWEEP keys per thread before it uses one;
//       b. compaction into (key << 32 | ~anchor) words: the keys above the K-th take slots from an integer LDS counter (their order
//          does not matter, they are sorted next); the keys EQUAL to it are ranked by an ordered ballot scan over ascending
//          anchors and the lowest ranks fill what is left -- so nothing depends on arrival order;
//       c. a bitonic sort, descending, of the next power of two >= the candidate count (padding words are 0, below every key);
//       d. box decode from pred into LDS;
//       e. NMS in chunks of 64 and the rows: the chunk's 64 x 64 matrix, a ballot per row; the greedy pass on bit masks; the rows;
//          the carry-over to the later chunks.  The stage is explained once, above dp_finish; the oriented kernel and the tiled
//          one of det_post_tiled.hpp have the same stage written out with their record, their "j suppresses i" and their row.
//          dp_finish then writes d_det_rows and the counters (all three kernels).
//   k_detpost_extra<T>   only on a head with extras (det_post_extra.hpp): third on the same stream, the extras of the emitted rows.
//   k_detpost_mask<T, P> only on a mask handle (det_post_mask.hpp, which includes this file): fourth, the masks of the emitted rows.
//   No floating-point atomic anywhere.  LDS: 8 + 16 + 4 + 1 bytes per candidate slot (K rounded up to a power of two) + 1.6 KB:
//   31 KB at the default K = 1024, 118 KB at K = 4096, of the 160 KB of a CU.
#pragma once

#include <stdint.h>

#include <cmath>

#include "kernel_macros.hpp"

namespace bm {

constexpr int DP_SCORE_THREADS = 256, DP_SCORE_VEC_THREADS = 64, DP_THREADS = 512, DP_CHUNK = 64, DP_K_MIN = 64, DP_K_MAX = 4096, DP_COUNTERS = 3,
              DP_SWEEP = 4;           // keys a thread loads per round of a sweep over the anchors: the loads of a round are in flight together

constexpr int DP_LDS_FIXED = (256 + 16 + 8) * 4 + (DP_CHUNK + 1) * 8 + 8;      // histogram, wave sums, scalars, matrix rows + live mask (bytes)

struct DetPostGeom { float gain, top, left, rows, cols; };         // per stream: LetterboxGeometry as to_frame uses it
struct DetPostTileGeom { float gain, top, left, x0, y0, w, h; };   // per (stream, tile) of a tiled call (det_post_tiled.hpp)

struct DetPostArgs {
    const void* pred;               // (S, 4 + nc, A) or (S, A, 5 + nc)
    const DetPostGeom* geom;        // [S]
    const uint8_t* allow;           // [nc] 0 / 1, or null
    uint32_t* keys;                 // scratch [S][A]
    int* cls;                       // scratch [S][A]
    float* dets;                    // [S][out_stride][6]
    int* det_rows;                  // [S]
    int* counters;                  // [S][DP_COUNTERS]
    int A, nc, layout, K, max_det, agnostic, out_stride;
    float conf_thres, iou_thres;
    int obb, nms_mode, regularize;  // the oriented layout "cn_obb" (det_post_obb.hpp): one angle row after the classes; 0 greedy / 1 fast
    // per-anchor extras (det_post_extra.hpp); all zero / null: a head without them, every address what it is without these fields
    int* src;                       // [S][src_stride] the anchor of every emitted row; set whenever n_extra > 0 (the caller's block or a scratch)
    float* extra;                   // [S][out_stride][n_extra]
    int src_stride, n_extra, extra_kind;                        // n_extra: values per anchor after the class scores; 0 raw / 1 kpt2 / 2 kpt3
};

__host__ __device__ inline int detpost_slots(int K) { int p = DP_CHUNK; while (p < K) p <<= 1; return p; }
inline size_t detpost_lds_bytes(int K) { return (size_t)detpost_slots(K) * (8 + 16 + 4 + 1) + DP_LDS_FIXED; }
inline size_t detpost_obb_lds_bytes(int K) { return (size_t)detpost_slots(K) * (8 + 20 + 4 + 1) + DP_LDS_FIXED; }
inline int detpost_score_grid_x(int A) { return (A + DP_SCORE_THREADS - 1) / DP_SCORE_THREADS; }

__device__ inline float dp_load(const float* p, long i) { return p[i]; }
__device__ inline float dp_load(const _Float16* p, long i) { return (float)p[i]; }

// element index of channel c (0..3 box, then the layout's own columns) of anchor a of stream s; the channel-major layout has
// 4 + nc channels, and one more, the angle, when oriented.  EXTRA: n_extra more per anchor in both layouts (det_post_extra.hpp) --
// a compile-time switch, so that the select kernels of a head without extras keep, instruction for instruction, the code they had
// before there were any (measured: with the sum read at run time, two more scalar instructions, k_detpost_select ran 2.6 - 3.2 %
// longer, far outside its run-to-run spread: profiles/detpost_extra_timing.txt)
template <bool EXTRA = false>
__device__ inline long dp_at(const DetPostArgs& g, int s, int a, int c) {
    const int x = EXTRA ? g.n_extra : 0;
    return g.layout == 0 ? ((long)s * (4 + g.nc + g.obb + x) + c) * g.A + a : ((long)s * g.A + a) * (5 + g.nc + x) + c;
}
__device__ inline bool dp_finite(float v) { return fabsf(v) < INFINITY; }       // false for a NaN and for +-inf

template <class T>
__global__ void __launch_bounds__(DP_SCORE_THREADS) k_detpost_score(DetPostArgs g) {
    const int s = (int)blockIdx.y, a = (int)blockIdx.x * DP_SCORE_THREADS + (int)threadIdx.x;
    if (a >= g.A) return;
    const T* pred = static_cast<const T*>(g.pred);
    const int first = g.layout == 0 ? 4 : 5;
    const long base = dp_at<true>(g, s, a, first), step = g.layout == 0 ? (long)g.A : 1L;
    float best = -INFINITY;
    int cls = 0;
    for (int c = 0; c < g.nc; ++c) {
        const float v = dp_load(pred, base + c * step);
        if (v > best) { best = v; cls = c; }
    }
    float conf = best;
    if (g.layout == 1) conf = dp_load(pred, base - 1) * best;
    bool pass = conf > g.conf_thres;
    if (g.allow && !g.allow[cls]) pass = false;
    if (g.obb && !dp_finite(dp_load(pred, base + g.nc * step))) pass = false;                   // the angle row follows the classes
    g.keys[(long)s * g.A + a] = pass ? __float_as_uint(conf) : 0u;
    g.cls[(long)s * g.A + a] = cls;
}

// "cn" with 16 bytes per load: a thread takes 8 fp16 / 4 fp32 NEIGHBOURING anchors of every channel row (the rows are contiguous over the
// anchors), so a wavefront reads 1 KB per instruction where k_detpost_score reads 128 or 256 bytes.  Needs A a multiple of that
// count and a 16-byte aligned tensor (detpost_launch checks; anything else takes k_detpost_score).  The same scan, the same values.
template <class T> struct DpVec;
template <> struct DpVec<float> { static constexpr int N = 4; typedef float type __attribute__((vector_size(16), may_alias)); };
template <> struct DpVec<_Float16> { static constexpr int N = 8; typedef _Float16 type __attribute__((vector_size(16), may_alias)); };

template <class T>
__global__ void __launch_bounds__(DP_SCORE_VEC_THREADS) k_detpost_score_cn_vec(DetPostArgs g) {
    constexpr int N = DpVec<T>::N;
    typedef typename DpVec<T>::type V;
    const int s = (int)blockIdx.y, a0 = ((int)blockIdx.x * DP_SCORE_VEC_THREADS + (int)threadIdx.x) * N;
    if (a0 >= g.A) return;
    const T* row = static_cast<const T*>(g.pred) + ((long)s * (4 + g.nc + g.obb + g.n_extra) + 4) * g.A + a0;
    float best[N];
    int cls[N];
#pragma unroll
    for (int u = 0; u < N; ++u) { best[u] = -INFINITY; cls[u] = 0; }
#pragma unroll 4
    for (int c = 0; c < g.nc; ++c) {
        const V v = *reinterpret_cast<const V*>(row + (long)c * g.A);
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const float f = (float)v[u];
            if (f > best[u]) { best[u] = f; cls[u] = c; }
        }
    }
    const long at = (long)s * g.A + a0;
    bool finite[N];
#pragma unroll
    for (int u = 0; u < N; ++u) finite[u] = true;
    if (g.obb) {
        const V v = *reinterpret_cast<const V*>(row + (long)g.nc * g.A);
#pragma unroll
        for (int u = 0; u < N; ++u) finite[u] = dp_finite((float)v[u]);
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        bool pass = best[u] > g.conf_thres && finite[u];
        if (g.allow && !g.allow[cls[u]]) pass = false;
        g.keys[at + u] = pass ? __float_as_uint(best[u]) : 0u;
        g.cls[at + u] = cls[u];
    }
}

struct DpBox { float x1, y1, x2, y2; };

__device__ inline bool dp_suppresses(const DpBox& j, const DpBox& i, float thres) {
    const float area_i = (i.x2 - i.x1) * (i.y2 - i.y1), area_j = (j.x2 - j.x1) * (j.y2 - j.y1);
    const float iw = fmaxf(fminf(i.x2, j.x2) - fmaxf(i.x1, j.x1), 0.0f), ih = fmaxf(fminf(i.y2, j.y2) - fmaxf(i.y1, j.y1), 0.0f);
    const float inter = iw * ih;
    return inter / (area_i + area_j - inter) > thres;
}
__device__ inline float dp_to_frame(float v, float off, float gain, float hi) { return fminf(fmaxf((v - off) / gain, 0.0f), hi); }
// ... and of a tiled call: clipped to the tile, then shifted by the tile's origin in the frame (det_post_tiled.hpp step 3b)
__device__ inline float dp_tile_to_frame(float v, float off, float gain, float hi, float origin) { return fminf(fmaxf((v - off) / gain, 0.0f), hi) + origin; }

// The workgroup's dynamic LDS: the candidate words, a per-candidate table of `tab_bytes` each (the box, or the oriented path's
// Gaussian), the classes, the fixed part and the suppression flags.
struct DpLds {
    unsigned long long* cand;       // [slots] key << 32 | ~anchor
    unsigned char* tab;             // [slots][tab_bytes]
    int* ccls;                      // [slots]
    int* hist;                      // [256]
    int* wsum;                      // [16]
    int* misc;                      // [8]: 0 passing, 1 prefix, 2 k_rem, 3 slot counter
    unsigned long long* rowm;       // [64] the chunk's matrix rows
    unsigned char* sup;             // [slots]
};
__device__ inline DpLds dp_lds(unsigned char* lds, int slots, int tab_bytes) {
    DpLds m;
    m.cand = reinterpret_cast<unsigned long long*>(lds);
    m.tab = lds + (size_t)slots * 8;
    m.ccls = reinterpret_cast<int*>(lds + (size_t)slots * (8 + tab_bytes));
    m.hist = reinterpret_cast<int*>(lds + (size_t)slots * (12 + tab_bytes));
    m.wsum = m.hist + 256;
    m.misc = m.wsum + 16;
    m.rowm = reinterpret_cast<unsigned long long*>(m.misc + 8);
    m.sup = lds + (size_t)slots * (12 + tab_bytes) + DP_LDS_FIXED;
    return m;
}

struct DpCount { int n_pass, n_cand; };

// Stages a-c of the select kernels, for the whole workgroup of DP_THREADS: leaves the candidates of stream s sorted in m.cand
// (conf descending, anchor ascending; the words beyond n_cand are 0) and m.sup cleared.  Ends with a barrier.
__device__ inline DpCount dp_select_sort(const DetPostArgs& g, int s, const DpLds& m, int slots) {
    unsigned long long* cand = m.cand;
    int *hist = m.hist, *wsum = m.wsum, *misc = m.misc;
    unsigned char* sup = m.sup;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int A = g.A, K = g.K;
    const uint32_t* keys = g.keys + (long)s * A;
    const unsigned long long below = (1ull << lane) - 1ull;

    // a. how many pass; the K-th largest key when more than K do
    if (t < 8) misc[t] = 0;
    if (t < 256) hist[t] = 0;
    __syncthreads();
    {
        int mine = 0;               // (the first sweep also fills the top byte's histogram: the select's pass 0, should it be needed)
        for (int a0 = t; a0 < A; a0 += DP_THREADS * DP_SWEEP) {
            uint32_t k[DP_SWEEP];
#pragma unroll
            for (int u = 0; u < DP_SWEEP; ++u) { const int a = a0 + u * DP_THREADS; k[u] = a < A ? keys[a] : 0u; }
#pragma unroll
            for (int u = 0; u < DP_SWEEP; ++u)
                if (k[u] != 0u) { mine += 1; atomicAdd(&hist[k[u] >> 24], 1); }
        }
        if (mine) atomicAdd(&misc[0], mine);
    }
    __syncthreads();
    const int n_pass = misc[0];
    const int n_cand = n_pass < K ? n_pass : K;
    uint32_t kth = 0u;              // the keys above it are all taken
    int need_eq = 0;                // and this many of the keys equal to it
    if (n_pass > K) {
        if (t == 0) { misc[1] = 0; misc[2] = K; }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            __syncthreads();
            const uint32_t prefix = (uint32_t)misc[1];
            if (pass > 0) {
                for (int a0 = t; a0 < A; a0 += DP_THREADS * DP_SWEEP) {
                    uint32_t k[DP_SWEEP];
#pragma unroll
                    for (int u = 0; u < DP_SWEEP; ++u) { const int a = a0 + u * DP_THREADS; k[u] = a < A ? keys[a] : 0u; }
#pragma unroll
                    for (int u = 0; u < DP_SWEEP; ++u)
                        if (k[u] != 0u && (k[u] >> (shift + 8)) == prefix) atomicAdd(&hist[(k[u] >> shift) & 255u], 1);
                }
                __syncthreads();
            }
            if (wave == 0) {
                // the bin that holds the rem-th largest of the keys counted: lane l has bins 4 l .. 4 l + 3; a suffix sum over the
                // lanes (six shuffles) tells how many keys lie in the bins of the lanes above (255 dependent steps as a loop of one thread)
                const int rem = misc[2];
                int h[4], tot = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) { h[q] = hist[4 * lane + q]; tot += h[q]; }
                int suf = tot;
                for (int d = 1; d < 64; d <<= 1) {
                    const int v = __shfl(suf, (lane + d) & 63, 64);
                    suf += lane + d < 64 ? v : 0;
                }
                int cum = suf - tot;                            // keys in higher bins than this lane's
                if (cum < rem && rem <= suf) {                  // (one lane: the K-th key exists)
                    int b = 0;
#pragma unroll
                    for (int q = 3; q >= 0; --q) {
                        if (cum + h[q] >= rem) { b = 4 * lane + q; break; }
                        cum += h[q];
                    }
                    misc[1] = (int)((prefix << 8) | (uint32_t)b);
                    misc[2] = rem - cum;
                }
            }
            __syncthreads();
            if (t < 256) hist[t] = 0;                           // (for the next pass; its sweep starts after the loop's first barrier)
        }
        __syncthreads();
        kth = (uint32_t)misc[1];
        need_eq = misc[2];
    }
    const int n_gt = n_cand - need_eq;

    // b. compaction
    for (int i = t; i < slots; i += DP_THREADS) { cand[i] = 0ull; sup[i] = 0; }
    __syncthreads();
    for (int a0 = t; a0 < A; a0 += DP_THREADS * DP_SWEEP) {
        uint32_t k[DP_SWEEP];
#pragma unroll
        for (int u = 0; u < DP_SWEEP; ++u) { const int a = a0 + u * DP_THREADS; k[u] = a < A ? keys[a] : 0u; }
#pragma unroll
        for (int u = 0; u < DP_SWEEP; ++u)
            if (k[u] > kth) {
                const int at = atomicAdd(&misc[3], 1);
                if (at < n_gt) cand[at] = ((unsigned long long)k[u] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)(a0 + u * DP_THREADS));
            }
    }
    if (need_eq > 0) {
        int done = 0;               // keys equal to kth seen in the tiles before this one (the same in every thread)
        for (int a0 = 0; a0 < A && done < need_eq; a0 += DP_THREADS * DP_SWEEP) {
            uint32_t k[DP_SWEEP];
#pragma unroll
            for (int u = 0; u < DP_SWEEP; ++u) { const int a = a0 + u * DP_THREADS + t; k[u] = a < A ? keys[a] : 0u; }
#pragma unroll
            for (int u = 0; u < DP_SWEEP; ++u) {                 // tiles of DP_THREADS anchors, in ascending order
                const int a = a0 + u * DP_THREADS + t;
                const bool eq = k[u] == kth;                    // (kth is a passing key, not 0)
                const unsigned long long m = __ballot(eq);
                if (lane == 0) wsum[wave] = __popcll(m);
                __syncthreads();
                int before = 0, total = 0;
                for (int w = 0; w < DP_THREADS / 64; ++w) { const int c = wsum[w]; before += w < wave ? c : 0; total += c; }
                const int r = done + before + __popcll(m & below);
                if (eq && r < need_eq) cand[n_gt + r] = ((unsigned long long)kth << 32) | (unsigned long long)(0xffffffffu - (uint32_t)a);
                done += total;
                __syncthreads();
            }
        }
    }
    __syncthreads();

    // c. bitonic sort, descending, of the first `n` words (a power of two >= n_cand; the words beyond n_cand are 0)
    int n = DP_CHUNK;
    while (n < n_cand) n <<= 1;
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < n; i += DP_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long u = cand[i], v = cand[p];
                    if ((i & k) == 0 ? u < v : u > v) { cand[i] = v; cand[p] = u; }
                }
            }
            __syncthreads();
        }
    }

    return DpCount{n_pass, n_cand};
}

__device__ inline float dp_readlane_f32(float v, int l) { return __uint_as_float(BM_READLANE_U32(__float_as_uint(v), l)); }
// a candidate's record out of lane l's registers (v_readlane with a wave-uniform lane)
__device__ inline DpBox dp_readlane(const DpBox& b, int l) {
    return DpBox{dp_readlane_f32(b.x1, l), dp_readlane_f32(b.y1, l), dp_readlane_f32(b.x2, l), dp_readlane_f32(b.y2, l)};
}

// Stage e of the three select kernels (this one, k_detpost_select_obb, k_detpost_select_tiled) is the NMS over the sorted
// candidates, in chunks of 64, and the rows of the kept ones.  It is explained here once; each kernel has it WRITTEN OUT with its
// own record (DpBox, or the oriented kernel's DpGauss), its own "j suppresses i" and its own row, so a fix to the stage has to be
// made in all three.  (Tried: one function template for the whole stage, and one for everything after the matrix rows.  Any
// function boundary inside the chunk loop changes the code the compiler makes of it, and the kernels measured 0.3 - 5 % slower,
// outside the parent's run-to-run spread: profiles/frontend_refactor_ab.txt.)  Per chunk:
//   1. the chunk's 64 x 64 matrix, with all eight wavefronts at once: lane l of every wavefront holds candidate c0 + l (`mine`,
//      `mcls`), wavefront w makes the rows j = 8 w .. 8 w + 7 -- bit l of row j: "j, if kept, suppresses l" (l > j only, and only
//      for the l the earlier chunks left alive, `live0`: the others are dropped whatever the row says) -- one ballot per row into
//      rowm, so every division of the chunk runs in parallel; a workgroup barrier follows.  (Measured: resolving a chunk with one
//      wavefront, 64 dependent steps of ballot + IoU, took 12 us per chunk.)
//   2. every wavefront works out the chunk's survivors `km` for itself, so no barrier stands between that and what follows.
//      greedy: one step on 64-bit masks per KEPT candidate, lane l holding row l (the rows of candidates the earlier chunks
//      dropped are empty).  fast (the oriented kernel in nms_mode 1 only): rowm[w] is the OR of wavefront w's eight rows and the
//      survivors are the live lanes outside the OR of all of them.
//   3. wavefront 0 emits: row `rank` = kept so far + the kept lanes below, for the first max_det kept.
//   4. all wavefronts apply the chunk's kept candidates -- fast: ALL its candidates (the chunk is full when there is a later
//      one) -- to the candidates of the later chunks, classes compared here; a second barrier closes the chunk.
// Two workgroup barriers per chunk, none per candidate.  The loop does not stop at max_det kept: counter 2 is the count BEFORE
// the cut and needs every chunk.

// the row count and the counters of stream s (steps 5 and 6)
__device__ inline void dp_finish(const DetPostArgs& g, int s, const DpCount& cnt, int kept) {
    if (threadIdx.x != 0) return;
    g.det_rows[s] = kept < g.max_det ? kept : g.max_det;
    g.counters[s * DP_COUNTERS + 0] = cnt.n_pass;
    g.counters[s * DP_COUNTERS + 1] = cnt.n_cand;
    g.counters[s * DP_COUNTERS + 2] = kept;
}

// k_detpost_select (heads without extras) and k_detpost_select_src (with: det_post_extra.hpp) are one text, det_post_select_body.hpp
#define DP_SELECT_KERNEL k_detpost_select
#define DP_SELECT_SRC false
#include "det_post_select_body.hpp"
#undef DP_SELECT_KERNEL
#undef DP_SELECT_SRC
#define DP_SELECT_KERNEL k_detpost_select_src
#define DP_SELECT_SRC true
#include "det_post_select_body.hpp"
#undef DP_SELECT_KERNEL
#undef DP_SELECT_SRC

}  // namespace bm

#include "det_post_obb.hpp"         // the oriented layout: k_detpost_select_obb
#include "det_post_extra.hpp"       // per-anchor extras: k_detpost_extra

namespace bm {

// The score kernel of a call over n_tensors prediction tensors (L: the library's stream launcher, or the test harness's CPU-thread
// launcher): wide where the layout, the anchor count and the tensor's alignment allow it.
template <class L>
inline void detpost_launch_score(L& launch, const DetPostArgs& g, int n_tensors, int fp16) {
    const int vec = fp16 ? DpVec<_Float16>::N : DpVec<float>::N;
    const bool wide = g.layout == 0 && g.A % vec == 0 && (uintptr_t)g.pred % 16 == 0;
    const int wide_grid = (g.A / vec + DP_SCORE_VEC_THREADS - 1) / DP_SCORE_VEC_THREADS;
    if (fp16) {
        if (wide) launch(k_detpost_score_cn_vec<_Float16>, wide_grid, n_tensors, DP_SCORE_VEC_THREADS, (size_t)0, g);
        else launch(k_detpost_score<_Float16>, detpost_score_grid_x(g.A), n_tensors, DP_SCORE_THREADS, (size_t)0, g);
    } else {
        if (wide) launch(k_detpost_score_cn_vec<float>, wide_grid, n_tensors, DP_SCORE_VEC_THREADS, (size_t)0, g);
        else launch(k_detpost_score<float>, detpost_score_grid_x(g.A), n_tensors, DP_SCORE_THREADS, (size_t)0, g);
    }
}

// The third kernel of a call on a head with extras (g.n_extra > 0: g.src and g.extra must be set; tgeom / n_tiles of a tiled call, else
// null / 0).
template <class L>
inline void detpost_launch_extra(L& launch, const DetPostArgs& g, const DetPostTileGeom* tgeom, int n_tiles, int n_streams, int fp16) {
    const int gx = detpost_extra_grid_x(g.max_det, g.n_extra);
    if (fp16) launch(k_detpost_extra<_Float16>, gx, n_streams, DP_EXTRA_THREADS, (size_t)0, g, tgeom, n_tiles);
    else launch(k_detpost_extra<float>, gx, n_streams, DP_EXTRA_THREADS, (size_t)0, g, tgeom, n_tiles);
}

// The kernel sequence of one call.  (The oriented layout has no extras: the library refuses the combination.)
template <class L>
inline void detpost_launch(L& launch, const DetPostArgs& g, int n_streams, int fp16, size_t* lds_bytes = nullptr) {
    const size_t lds = g.obb ? detpost_obb_lds_bytes(g.K) : detpost_lds_bytes(g.K);
    if (lds_bytes) *lds_bytes = lds;
    detpost_launch_score(launch, g, n_streams, fp16);
    if (fp16) {
        if (g.obb) launch(k_detpost_select_obb<_Float16>, n_streams, 1, DP_THREADS, lds, g);
        else if (g.n_extra > 0) launch(k_detpost_select_src<_Float16>, n_streams, 1, DP_THREADS, lds, g);
        else launch(k_detpost_select<_Float16>, n_streams, 1, DP_THREADS, lds, g);
    } else {
        if (g.obb) launch(k_detpost_select_obb<float>, n_streams, 1, DP_THREADS, lds, g);
        else if (g.n_extra > 0) launch(k_detpost_select_src<float>, n_streams, 1, DP_THREADS, lds, g);
        else launch(k_detpost_select<float>, n_streams, 1, DP_THREADS, lds, g);
    }
    if (g.n_extra > 0 && !g.obb) detpost_launch_extra(launch, g, nullptr, 0, n_streams, fp16);
}

}  // namespace bm
