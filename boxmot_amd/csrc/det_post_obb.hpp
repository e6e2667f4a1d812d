// Device-side post-processing of ORIENTED detector heads (include/boxmot_hip.h, boxmot_hip_detpost_create_obb): from the raw
// tensor of an Ultralytics OBB head on the device to the d_dets [S][stride][7] / d_det_rows [S] block an is_obb tracker handle's
// step_device reads, in frame coordinates, with no host round trip.  Included by det_post.hpp (which has the axis-aligned
// definition, the score kernels, stages a-c and the kernel sequence); it is not meant to be included on its own.
//
// Definition.  All arithmetic is fp32 (the library is built with -ffp-contract=off and without fast-math); fp16 inputs are widened
// exactly.  The functions used are cosf, sinf, logf, expf, sqrtf and fmodf; every division is the correctly rounded one.
// 1. Score.  Layout "cn_obb": (S, 4 + nc + 1, A), channel-major like "cn": rows 0..3 are cx, cy, w, h in letterbox pixels, rows
//    4..4 + nc - 1 the class scores, the LAST row the angle in radians.  Score and argmax exactly as in "cn" (det_post.hpp step 1: the
//    lowest index wins a tie, a NaN is never the maximum).  An anchor passes iff conf > conf_thres, STRICTLY, the allow-list admits
//    its class, and its angle is finite: a NaN or +-inf angle never passes.
// 2. Select.  Unchanged: the K best by (conf descending, anchor ascending), exactly.
// 3. Gaussian of a candidate (Ultralytics _get_covariance_matrix, in this order of operations):
//        a = w*w/12;  b = h*h/12
//        c = cosf(angle);  s = sinf(angle)
//        c2 = c*c;  s2 = s*s
//        A = a*c2 + b*s2
//        B = a*s2 + b*c2
//        C = ((a - b)*c)*s
// 4. ProbIoU of an earlier candidate 1 and a later candidate 2 (Ultralytics batch_probiou), eps = 1e-7f:
//        den = (A1+A2)*(B1+B2) - (C1+C2)*(C1+C2)
//        t1  = (((A1+A2)*((y1-y2)*(y1-y2)) + (B1+B2)*((x1-x2)*(x1-x2))) / (den + eps)) * 0.25f
//        t2  = ((((C1+C2)*(x2-x1))*(y1-y2)) / (den + eps)) * 0.5f
//        t3  = logf(den / (4*sqrtf(fmaxf(A1*B1 - C1*C1, 0) * fmaxf(A2*B2 - C2*C2, 0)) + eps) + eps) * 0.5f
//        bd  = fminf(fmaxf(t1 + t2 + t3, eps), 100.0f)
//        iou = 1 - sqrtf(1 - expf(-bd) + eps)
//    Candidate 1 SUPPRESSES candidate 2 iff iou >= iou_thres: `>=`, the rule of Ultralytics nms_rotated, deliberately not the `>` of
//    the axis-aligned path; a NaN compares false.  Classes are kept apart by comparing them unless agnostic, as in the axis-aligned path.
// 5. NMS, two modes fixed at creation:
//        greedy (0, default)  candidate i is dropped iff an earlier KEPT candidate suppresses it (the rule of the axis-aligned path);
//        fast   (1)           candidate i is dropped iff ANY earlier candidate suppresses it, kept or not: the upper-triangular
//                             formulation Ultralytics nms_rotated computes.
// 6. Emit.  The first max_det kept candidates become rows [cx, cy, w, h, angle, conf, cls]:
//        cx = (cx - left) / gain;  cy = (cy - top) / gain;  w = w / gain;  h = h / gain
//    There is NO clipping: Ultralytics scale_boxes(xywh=True) does not clip, and an oriented box cannot be clipped to a rectangle.
//    With `regularize` (default off) the emitted row only -- ProbIoU is invariant under it -- is regularised before the division:
//        if h > w: swap w and h, and angle = angle + (float)(pi/2)
//        angle = fmodf(angle, (float)pi);  if angle < 0: angle += (float)pi
//    so that w >= h and angle is within [0, pi].  d_det_rows, the counters and "rows at and beyond the count are not touched" are
//    as in det_post.hpp.
// (Not claimed: parity with Ultralytics.  The formulas are a reading of its source; tests/detpost_obb_ref.py restates this
// definition in NumPy.  cosf / sinf / logf / expf differ by units in the last place between NumPy, the CPU-thread emulation and the
// device, so the tests compare DECISIONS -- on cases where no comparable pair lies within 2e-3 of the threshold -- and the exactly
// computed row values, bit for bit.)
//
// Kernel.
//   k_detpost_select_obb<T>  one workgroup of DP_THREADS per stream; stages a-c are dp_select_sort of det_post.hpp, shared with the
//       axis-aligned kernel.
//       d. per candidate (cx, cy, A, B, C), 20 bytes, and its class into LDS: cosf / sinf run once per candidate, not per pair;
//       e. the chunked 64 x 64 ballot NMS explained in det_post.hpp, written out here with DpGauss as the record,
//          dp_suppresses_obb as the predicate and both modes (fast: no row is skipped for being dropped, every wavefront ORs its
//          eight rows, and all of a chunk's candidates go on to the later chunks).  Wavefront 0 emits; it reloads w, h and the
//          angle of the kept anchors from pred.
//   No floating-point atomic.  LDS: 8 + 20 + 4 + 1 bytes per candidate slot + 1.6 KB: 35 KB at K = 1024, 137 KB at K = 4096.
#pragma once

namespace bm {

struct DpGauss { float x, y, a, b, c; };

__device__ inline DpGauss dp_gauss(float cx, float cy, float w, float h, float angle) {
    const float a = w * w / 12.0f, b = h * h / 12.0f;
    const float c = cosf(angle), s = sinf(angle);
    const float c2 = c * c, s2 = s * s;
    return DpGauss{cx, cy, a * c2 + b * s2, a * s2 + b * c2, ((a - b) * c) * s};
}

// does the earlier candidate p suppress the later candidate q
__device__ inline bool dp_suppresses_obb(const DpGauss& p, const DpGauss& q, float thres) {
    const float eps = 1e-7f;
    const float sa = p.a + q.a, sb = p.b + q.b, sc = p.c + q.c;
    const float den = sa * sb - sc * sc;
    const float dy = p.y - q.y, dx = p.x - q.x;
    const float t1 = ((sa * (dy * dy) + sb * (dx * dx)) / (den + eps)) * 0.25f;
    const float t2 = (((sc * (q.x - p.x)) * dy) / (den + eps)) * 0.5f;
    const float t3 = logf(den / (4.0f * sqrtf(fmaxf(p.a * p.b - p.c * p.c, 0.0f) * fmaxf(q.a * q.b - q.c * q.c, 0.0f)) + eps) + eps) * 0.5f;
    const float bd = fminf(fmaxf(t1 + t2 + t3, eps), 100.0f);
    const float iou = 1.0f - sqrtf(1.0f - expf(-bd) + eps);
    return iou >= thres;
}

__device__ inline DpGauss dp_readlane(const DpGauss& g, int l) {
    return DpGauss{dp_readlane_f32(g.x, l), dp_readlane_f32(g.y, l), dp_readlane_f32(g.a, l), dp_readlane_f32(g.b, l), dp_readlane_f32(g.c, l)};
}

template <class T>
__global__ void __launch_bounds__(DP_THREADS) k_detpost_select_obb(DetPostArgs g) {
    BM_DYNAMIC_LDS_T(unsigned char, lds);
    const int slots = detpost_slots(g.K);
    const DpLds m = dp_lds(lds, slots, (int)sizeof(DpGauss));
    unsigned long long* cand = m.cand;
    DpGauss* gauss = reinterpret_cast<DpGauss*>(m.tab);
    int* ccls = m.ccls;
    unsigned long long* rowm = m.rowm;
    unsigned char* sup = m.sup;

    const int s = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int A = g.A, angle_row = 4 + g.nc;
    const bool fast = g.nms_mode == 1;
    const T* pred = static_cast<const T*>(g.pred);
    const unsigned long long below = (1ull << lane) - 1ull;
    constexpr int ROWS = DP_CHUNK / (DP_THREADS / 64);          // matrix rows per wavefront

    // a-c. the passing count, the exact top-K, the sort
    const DpCount cnt = dp_select_sort(g, s, m, slots);
    const int n_cand = cnt.n_cand;

    // d. Gaussians
    for (int i = t; i < n_cand; i += DP_THREADS) {
        const int a = (int)(0xffffffffu - (uint32_t)cand[i]);
        gauss[i] = dp_gauss(dp_load(pred, dp_at(g, s, a, 0)), dp_load(pred, dp_at(g, s, a, 1)), dp_load(pred, dp_at(g, s, a, 2)),
                            dp_load(pred, dp_at(g, s, a, 3)), dp_load(pred, dp_at(g, s, a, angle_row)));
        ccls[i] = g.cls[(long)s * A + a];
    }
    __syncthreads();

    // e. NMS and the rows, in both modes: the stage that is explained above k_detpost_select (det_post.hpp), written out with this
    // kernel's record, predicate and row.  w, h and the angle of a kept anchor are reloaded from pred.
    const DetPostGeom geo = g.geom[s];
    float* rows = g.dets + (long)s * g.out_stride * 7;
    int kept = 0;                   // (the same in every thread)
    for (int c0 = 0; c0 < n_cand; c0 += DP_CHUNK) {
        // lane l of every wavefront holds candidate c0 + l, wavefront w makes the rows j = 8 w .. 8 w + 7 -- bit l of row j: "j
        // suppresses l" (l > j only, and only for the l the earlier chunks left alive: the others are dropped whatever the row says)
        const int i = c0 + lane;
        const bool valid = i < n_cand;
        const DpGauss mine = valid ? gauss[i] : DpGauss{0.f, 0.f, 0.f, 0.f, 0.f};
        const int mcls = valid ? ccls[i] : -1;
        const unsigned long long live0 = __ballot(valid && !sup[i]);         // what the earlier chunks left alive (every wavefront asks)
        unsigned long long acc = 0ull;                                       // fast: the OR of this wavefront's rows
        for (int r = 0; r < ROWS; ++r) {
            const int j = wave * ROWS + r;
            // an empty row: nobody after j is left; greedy: j is gone already; fast: j is beyond the candidates
            const bool row = fast ? c0 + j < n_cand : (bool)((live0 >> j) & 1ull);
            if (!row || ((live0 >> j) >> 1) == 0ull) {
                if (!fast && lane == 0) rowm[j] = 0ull;
                continue;
            }
            const DpGauss gj = dp_readlane(mine, j);
            const int cj = (int)BM_READLANE_U32((unsigned)mcls, j);
            const bool hit = ((live0 >> lane) & 1ull) && lane > j && (g.agnostic || cj == mcls) && dp_suppresses_obb(gj, mine, g.iou_thres);
            const unsigned long long mj = __ballot(hit);
            if (fast) acc |= mj;
            else if (lane == 0) rowm[j] = mj;
        }
        if (fast && lane == 0) rowm[wave] = acc;
        __syncthreads();
        unsigned long long km = live0;                                       // the chunk's survivors; every wavefront works them out
        if (fast) {
            unsigned long long dead = 0ull;
            for (int w = 0; w < DP_THREADS / 64; ++w) dead |= rowm[w];
            km &= ~dead;
        } else {
            // the greedy pass over the chunk, on bit masks: one step per KEPT candidate, lane l holding row l
            const unsigned long long myrow = rowm[lane];
            const unsigned mylo = (unsigned)myrow, myhi = (unsigned)(myrow >> 32);
            for (unsigned long long rest = km; rest;) {
                const int j = __builtin_ctzll(rest);
                km &= ~(((unsigned long long)BM_READLANE_U32(myhi, j) << 32) | (unsigned long long)BM_READLANE_U32(mylo, j));
                rest = j == 63 ? 0ull : km & ~((2ull << j) - 1ull);
            }
        }
        if (wave == 0) {
            const bool alive = (km >> lane) & 1ull;
            const int rank = kept + __popcll(km & below);
            if (alive && rank < g.max_det) {
                const int a = (int)(0xffffffffu - (uint32_t)cand[i]);
                float w = dp_load(pred, dp_at(g, s, a, 2)), h = dp_load(pred, dp_at(g, s, a, 3)), angle = dp_load(pred, dp_at(g, s, a, angle_row));
                if (g.regularize) {
                    const float pi = (float)3.14159265358979323846, half_pi = (float)(3.14159265358979323846 / 2);
                    if (h > w) { const float v = w; w = h; h = v; angle = angle + half_pi; }
                    angle = fmodf(angle, pi);
                    if (angle < 0.0f) angle += pi;
                }
                float* r = rows + (long)rank * 7;
                r[0] = (mine.x - geo.left) / geo.gain;
                r[1] = (mine.y - geo.top) / geo.gain;
                r[2] = w / geo.gain;
                r[3] = h / geo.gain;
                r[4] = angle;
                r[5] = __uint_as_float((uint32_t)(cand[i] >> 32));
                r[6] = (float)mcls;
            }
        }
        kept += __popcll(km);
        // greedy: the chunk's kept candidates go on to the later ones; fast: all of them (the chunk is full when there is a later one)
        const unsigned long long apply = fast ? ~0ull : km;
        if (apply && c0 + DP_CHUNK < n_cand) {
            for (int q = c0 + DP_CHUNK + t; q < n_cand; q += DP_THREADS) {
                if (sup[q]) continue;
                const DpGauss qg = gauss[q];
                const int qcls = ccls[q];
                for (unsigned long long mm = apply; mm; mm &= mm - 1ull) {
                    const int j = c0 + __builtin_ctzll(mm);
                    if ((g.agnostic || ccls[j] == qcls) && dp_suppresses_obb(gauss[j], qg, g.iou_thres)) { sup[q] = 1; break; }
                }
            }
        }
        __syncthreads();
    }
    dp_finish(g, s, cnt, kept);
}

}  // namespace bm
