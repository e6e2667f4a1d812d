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

struct DetPostTileGeom { float gain, top, left, x0, y0, w, h; };      // per (stream, tile)

struct DetPostTiledArgs {
    DetPostArgs base;               // A: the anchors of ONE tile tensor; keys / cls: [S * T][A]; geom unused (null)
    const DetPostTileGeom* tgeom;   // [S][T]
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
__device__ inline float dp_tile_to_frame(float v, float off, float gain, float hi, float origin) { return fminf(fmaxf((v - off) / gain, 0.0f), hi) + origin; }

template <class T>
__global__ void __launch_bounds__(DP_THREADS) k_detpost_select_tiled(DetPostTiledArgs ta) {
    BM_DYNAMIC_LDS_T(unsigned char, lds);
    const DetPostArgs& g = ta.base;
    const int slots = detpost_slots(g.K);
    const DpLds m = dp_lds(lds, slots, (int)sizeof(DpBox));
    const unsigned long long* cand = m.cand;
    DpBox* box = reinterpret_cast<DpBox*>(m.tab);

    const int s = (int)blockIdx.x, t = (int)threadIdx.x;
    const int A = g.A, NT = ta.T, merge = ta.merge;
    const T* pred = static_cast<const T*>(g.pred);

    // a-c. over the stream's T * A keys: the passing count, the exact top-K, the sort (conf descending, t * A + a ascending)
    DetPostArgs all = g;
    all.A = NT * A;
    const DpCount cnt = dp_select_sort(all, s, m, slots);

    // d. boxes, in frame coordinates
    for (int i = t; i < cnt.n_cand; i += DP_THREADS) {
        const int idx = (int)(0xffffffffu - (uint32_t)cand[i]);
        const int tile = idx / A, a = idx - tile * A, ps = s * NT + tile;
        const float cx = dp_load(pred, dp_at(g, ps, a, 0)), cy = dp_load(pred, dp_at(g, ps, a, 1)), w = dp_load(pred, dp_at(g, ps, a, 2)),
                    h = dp_load(pred, dp_at(g, ps, a, 3));
        const DetPostTileGeom q = ta.tgeom[ps];
        box[i] = DpBox{dp_tile_to_frame(cx - w * 0.5f, q.left, q.gain, q.w, q.x0), dp_tile_to_frame(cy - h * 0.5f, q.top, q.gain, q.h, q.y0),
                       dp_tile_to_frame(cx + w * 0.5f, q.left, q.gain, q.w, q.x0), dp_tile_to_frame(cy + h * 0.5f, q.top, q.gain, q.h, q.y0)};
        m.ccls[i] = g.cls[(long)s * NT * A + idx];
    }
    __syncthreads();

    // e. NMS with the metric selected, and the rows as they are: the stage that is explained above k_detpost_select (det_post.hpp)
    float* rows = g.dets + (long)s * g.out_stride * 6;
    const int n_cand = cnt.n_cand, lane = t & 63, wave = t >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int* ccls = m.ccls;
    unsigned long long* rowm = m.rowm;
    unsigned char* sup = m.sup;
    int kept = 0;                   // (the same in every thread)
    for (int c0 = 0; c0 < n_cand; c0 += DP_CHUNK) {
        const int i = c0 + lane;
        const bool valid = i < n_cand;
        const DpBox mine = valid ? box[i] : DpBox{0.f, 0.f, 0.f, 0.f};
        const int mcls = valid ? ccls[i] : -1;
        const unsigned long long live0 = __ballot(valid && !sup[i]);         // what the earlier chunks left alive (every wavefront asks)
        for (int r = 0; r < DP_CHUNK / (DP_THREADS / 64); ++r) {
            const int j = wave * (DP_CHUNK / (DP_THREADS / 64)) + r;
            if (!((live0 >> j) & 1ull) || (live0 >> j) == 1ull) {           // j is gone already, or nobody after it is left: an empty row
                if (lane == 0) rowm[j] = 0ull;
                continue;
            }
            const DpBox bj = dp_readlane(mine, j);
            const int cj = (int)BM_READLANE_U32((unsigned)mcls, j);
            const bool hit = ((live0 >> lane) & 1ull) && lane > j && (g.agnostic || cj == mcls) && dp_merge_suppresses(bj, mine, g.iou_thres, merge);
            const unsigned long long hm = __ballot(hit);
            if (lane == 0) rowm[j] = hm;
        }
        __syncthreads();
        const unsigned long long myrow = rowm[lane];
        const unsigned mylo = (unsigned)myrow, myhi = (unsigned)(myrow >> 32);
        unsigned long long km = live0;
        for (unsigned long long rest = km; rest;) {
            const int j = __builtin_ctzll(rest);
            km &= ~(((unsigned long long)BM_READLANE_U32(myhi, j) << 32) | (unsigned long long)BM_READLANE_U32(mylo, j));
            rest = j == 63 ? 0ull : km & ~((2ull << j) - 1ull);
        }
        if (wave == 0) {
            const bool alive = (km >> lane) & 1ull;
            const int rank = kept + __popcll(km & below);
            if (alive && rank < g.max_det) {
                float* r = rows + (long)rank * 6;
                r[0] = mine.x1; r[1] = mine.y1; r[2] = mine.x2; r[3] = mine.y2;
                r[4] = __uint_as_float((uint32_t)(cand[i] >> 32));
                r[5] = (float)mcls;
            }
        }
        kept += __popcll(km);
        if (km && c0 + DP_CHUNK < n_cand) {
            for (int q = c0 + DP_CHUNK + t; q < n_cand; q += DP_THREADS) {
                if (sup[q]) continue;
                const DpBox qb = box[q];
                const int qcls = ccls[q];
                for (unsigned long long mm = km; mm; mm &= mm - 1ull) {
                    const int j = c0 + __builtin_ctzll(mm);
                    if ((g.agnostic || ccls[j] == qcls) && dp_merge_suppresses(box[j], qb, g.iou_thres, merge)) { sup[q] = 1; break; }
                }
            }
        }
        __syncthreads();
    }
    dp_finish(g, s, cnt, kept);
}

// The kernel sequence of one tiled call (L as detpost_launch's): the score kernel over the S * T tile tensors, then one select
// workgroup per stream.
template <class L>
inline void detpost_launch_tiled(L& launch, const DetPostTiledArgs& ta, int n_streams, int fp16, size_t* lds_bytes = nullptr) {
    const size_t lds = detpost_lds_bytes(ta.base.K);
    if (lds_bytes) *lds_bytes = lds;
    detpost_launch_score(launch, ta.base, n_streams * ta.T, fp16);
    if (fp16) launch(k_detpost_select_tiled<_Float16>, n_streams, 1, DP_THREADS, lds, ta);
    else launch(k_detpost_select_tiled<float>, n_streams, 1, DP_THREADS, lds, ta);
}

}  // namespace bm
