// The text of k_detpost_select_tiled and k_detpost_select_tiled_src (det_post_tiled.hpp includes this file once for each, inside
// namespace bm, with DP_SELECT_KERNEL the kernel's name and DP_SELECT_SRC false / true), as det_post_select_body.hpp is the text of the
// untiled pair, and for the same reasons.  DP_SELECT_SRC: the stride with extras, and the candidate word's index t * A + a of every
// emitted row to g.src.
template <class T>
__global__ void __launch_bounds__(DP_THREADS) DP_SELECT_KERNEL(DetPostTiledArgs ta) {
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
        const float cx = dp_load(pred, dp_at<DP_SELECT_SRC>(g, ps, a, 0)), cy = dp_load(pred, dp_at<DP_SELECT_SRC>(g, ps, a, 1)), w = dp_load(pred, dp_at<DP_SELECT_SRC>(g, ps, a, 2)),
                    h = dp_load(pred, dp_at<DP_SELECT_SRC>(g, ps, a, 3));
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
                if (DP_SELECT_SRC) g.src[(long)s * g.src_stride + rank] = (int)(0xffffffffu - (uint32_t)cand[i]);
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
