// The text of k_detpost_select and k_detpost_select_src (det_post.hpp includes this file once for each, inside namespace bm, with
// DP_SELECT_KERNEL the kernel's name and DP_SELECT_SRC false / true).  DP_SELECT_SRC: the kernel of a head with extras (g.n_extra > 0,
// g.src set): the tensor's stride includes them, and the anchor of every emitted row is stored to g.src (det_post_extra.hpp step 7).
// Two kernels from one text, and not one function template that both call: the kernel of a head without extras has to stay, instruction
// for instruction, what it was before there were any.  With the stride's sum read at run time it was two scalar instructions longer
// and ran 2.6 - 3.2 % longer (profiles/detpost_extra_timing.txt); with this text in an always-inlined function the compiler made 80
// more instructions of it.  And two NAMES, not one template with a bool: tests/test_isa_budget.py counts the kernels of each name.
template <class T>
__global__ void __launch_bounds__(DP_THREADS) DP_SELECT_KERNEL(DetPostArgs g) {
    BM_DYNAMIC_LDS_T(unsigned char, lds);
    const int slots = detpost_slots(g.K);
    const DpLds m = dp_lds(lds, slots, (int)sizeof(DpBox));
    const unsigned long long* cand = m.cand;
    DpBox* box = reinterpret_cast<DpBox*>(m.tab);

    const int s = (int)blockIdx.x, t = (int)threadIdx.x;
    const T* pred = static_cast<const T*>(g.pred);

    // a-c. the passing count, the exact top-K, the sort
    const DpCount cnt = dp_select_sort(g, s, m, slots);

    // d. boxes
    for (int i = t; i < cnt.n_cand; i += DP_THREADS) {
        const int a = (int)(0xffffffffu - (uint32_t)cand[i]);
        const float cx = dp_load(pred, dp_at<DP_SELECT_SRC>(g, s, a, 0)), cy = dp_load(pred, dp_at<DP_SELECT_SRC>(g, s, a, 1)), w = dp_load(pred, dp_at<DP_SELECT_SRC>(g, s, a, 2)),
                    h = dp_load(pred, dp_at<DP_SELECT_SRC>(g, s, a, 3));
        box[i] = DpBox{cx - w * 0.5f, cy - h * 0.5f, cx + w * 0.5f, cy + h * 0.5f};
        m.ccls[i] = g.cls[(long)s * g.A + a];
    }
    __syncthreads();

    // e. NMS and the rows, through to_frame's arithmetic (the stage is explained above dp_finish)
    const DetPostGeom geo = g.geom[s];
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
            const DpBox bj = dp_readlane(mine, j);                          // candidate j's box and class out of lane j's registers
            const int cj = (int)BM_READLANE_U32((unsigned)mcls, j);
            const bool hit = ((live0 >> lane) & 1ull) && lane > j && (g.agnostic || cj == mcls) && dp_suppresses(bj, mine, g.iou_thres);
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
                r[0] = dp_to_frame(mine.x1, geo.left, geo.gain, geo.cols);
                r[1] = dp_to_frame(mine.y1, geo.top, geo.gain, geo.rows);
                r[2] = dp_to_frame(mine.x2, geo.left, geo.gain, geo.cols);
                r[3] = dp_to_frame(mine.y2, geo.top, geo.gain, geo.rows);
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
                    if ((g.agnostic || ccls[j] == qcls) && dp_suppresses(box[j], qb, g.iou_thres)) { sup[q] = 1; break; }
                }
            }
        }
        __syncthreads();
    }
    dp_finish(g, s, cnt, kept);
}
