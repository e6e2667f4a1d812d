// Development tool behind tools/detpost_prof.py: times of the two detection post-processing kernels (boxmot_amd/csrc/det_post.hpp,
// through its own kernel sequence detpost_launch) for S streams of one prediction tensor, beside the first half of what they
// replace: the device-to-host copy of the S-stream tensor (into pinned and into pageable memory).  The other half, the NumPy
// reference on the host, is timed by detpost_prof.py on the same tensor.  Every launch has its own pair of HIP events.  Prints one
// line per kernel -- median, min and max in microseconds -- and a checksum of stream 0's output (the sum of its rows' 6 columns, 7
// on the oriented path, and its counters) that detpost_prof.py compares with the reference's.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o detpost_prof tools/detpost_prof.hip
//     ./detpost_prof pred.bin [streams = 16] [anchors = 8400] [classes = 80] [layout = 0] [fp16 = 1] [K = 1024] [max_det = 256] [repeats = 30]
//                   [obb = 0] [nms_mode = 0] [extra = 0] [extra_kind = 0]
// pred.bin: ONE stream's tensor, (4 + nc, A) or (A, 5 + nc), raw; every stream gets a copy.  obb = 1: the oriented layout
// (det_post_obb.hpp), (4 + nc + 1, A) with layout 0, nms_mode 0 greedy / 1 fast; the host copies are not timed again.  conf 0.25, iou 0.45, class-aware,
// geometry of a 1080 x 1920 frame in a centred 640 x 640 letterbox.  extra = E > 0: a head with E more values per anchor
// (det_post_extra.hpp), (4 + nc + E, A) or (A, 5 + nc + E): the three-kernel sequence -- score, the select kernel's source-storing
// variant, k_detpost_extra -- a line for the third kernel, and the sums of stream 0's extras and source anchors in the checksum.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../boxmot_amd/csrc/det_post.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static void report(const char* name, std::vector<float> ms) {
    std::sort(ms.begin(), ms.end());
    std::printf("%-22s median %.1f us  min %.1f  max %.1f  (%zu samples)\n", name, 1e3 * ms[ms.size() / 2], 1e3 * ms.front(), 1e3 * ms.back(), ms.size());
}

struct TimedLaunch {            // every kernel of the sequence between its own pair of events
    hipStream_t stream;
    hipEvent_t* ev;             // [6]: up to three kernels
    int k = 0;
    template <class K, class... A>
    void operator()(K kernel, int gx, int gy, int threads, size_t lds_bytes, A... args) {
        (void)hipEventRecord(ev[2 * k], stream);
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3((unsigned)threads), lds_bytes, stream, args...);
        (void)hipEventRecord(ev[2 * k + 1], stream);
        ++k;
    }
};

int main(int argc, char** argv) {
    auto arg = [&](int k, int d) { return argc > k ? std::atoi(argv[k]) : d; };
    if (argc < 2) { std::fprintf(stderr, "usage: detpost_prof pred.bin [streams anchors classes layout fp16 K max_det repeats]\n"); return 1; }
    const int S = arg(2, 16), A = arg(3, 8400), nc = arg(4, 80), layout = arg(5, 0), fp16 = arg(6, 1), K = arg(7, 1024), max_det = arg(8, 256), reps = arg(9, 30),
              obb = arg(10, 0), mode = arg(11, 0), cols = obb ? 7 : 6, E = arg(12, 0), kind = arg(13, 0);
    if (E < 0 || E > bm::DP_EXTRA_MAX || kind < 0 || kind >= bm::DP_EXTRA_KINDS || (E && obb) || (E && E % bm::detpost_extra_group(kind))) {
        std::fprintf(stderr, "extra within 0..1024 and a multiple of its kind's group (0 raw, 1 kpt2, 2 kpt3); not with obb\n");
        return 1;
    }
    if (S < 1 || A < 1 || nc < 1 || (layout != 0 && layout != 1) || (obb != 0 && obb != 1) || (obb && layout != 0) || (mode != 0 && mode != 1) || K < bm::DP_K_MIN || K > bm::DP_K_MAX || max_det < 1 || reps < 20) {
        std::fprintf(stderr, "streams, anchors, classes >= 1, layout 0 or 1, K within 64..4096, repeats >= 20\n");
        return 1;
    }
    const size_t per = (size_t)A * ((layout == 0 ? 4 + obb : 5) + nc + E) * (fp16 ? 2 : 4), bytes = per * S;
    std::vector<unsigned char> one(per);
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f || std::fread(one.data(), 1, per, f) != per) { std::fprintf(stderr, "%s: cannot read %zu bytes\n", argv[1], per); return 1; }
        std::fclose(f);
    }
    void *d_pred = nullptr, *h_pinned = nullptr;
    uint32_t* d_keys = nullptr;
    int *d_cls = nullptr, *d_rows = nullptr, *d_counters = nullptr;
    float *d_dets = nullptr, *d_extra = nullptr;
    int* d_src = nullptr;
    bm::DetPostGeom* d_geom = nullptr;
    CHECK(hipMalloc(&d_pred, bytes));
    CHECK(hipMalloc(&d_keys, (size_t)S * A * 4));
    CHECK(hipMalloc(&d_cls, (size_t)S * A * 4));
    CHECK(hipMalloc(&d_rows, (size_t)S * 4));
    CHECK(hipMalloc(&d_counters, (size_t)S * bm::DP_COUNTERS * 4));
    CHECK(hipMalloc(&d_dets, (size_t)S * max_det * cols * 4));
    CHECK(hipMalloc(&d_geom, (size_t)S * sizeof(bm::DetPostGeom)));
    if (E) {
        CHECK(hipMalloc(&d_extra, (size_t)S * max_det * E * 4));
        CHECK(hipMalloc(&d_src, (size_t)S * max_det * 4));
        CHECK(hipMemset(d_extra, 0, (size_t)S * max_det * E * 4));
    }
    CHECK(hipHostMalloc(&h_pinned, bytes, hipHostMallocDefault));
    std::vector<unsigned char> h_pageable(bytes);
    for (int s = 0; s < S; ++s) CHECK(hipMemcpy((unsigned char*)d_pred + per * s, one.data(), per, hipMemcpyHostToDevice));
    std::vector<bm::DetPostGeom> geom(S, bm::DetPostGeom{(float)(1.0 / 3.0), 140.f, 0.f, 1080.f, 1920.f});
    CHECK(hipMemcpy(d_geom, geom.data(), S * sizeof(bm::DetPostGeom), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_dets, 0, (size_t)S * max_det * cols * 4));
    const int lds = (int)(obb ? bm::detpost_obb_lds_bytes(K) : bm::detpost_lds_bytes(K));
    if (obb) {
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bm::k_detpost_select_obb<float>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bm::k_detpost_select_obb<_Float16>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    } else if (E) {
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bm::k_detpost_select_src<float>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bm::k_detpost_select_src<_Float16>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    } else {
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bm::k_detpost_select<float>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bm::k_detpost_select<_Float16>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    hipStream_t st;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    bm::DetPostArgs a{d_pred, d_geom, nullptr, d_keys, d_cls, d_dets, d_rows, d_counters, A, nc, layout, K, max_det, 0, max_det, 0.25f, 0.45f, obb, mode, 0};
    if (E) { a.src = d_src; a.extra = d_extra; a.src_stride = max_det; a.n_extra = E; a.extra_kind = kind; }
    constexpr int EV = 10;          // events per timed call: three kernel pairs, two copy pairs
    std::vector<hipEvent_t> ev(EV * (size_t)reps);
    for (auto& e : ev) CHECK(hipEventCreate(&e));
    for (int k = 0; k < 5; ++k) { TimedLaunch warm{st, ev.data()}; bm::detpost_launch(warm, a, S, fp16); }
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < reps; ++k) {
        hipEvent_t* e = &ev[EV * (size_t)k];
        TimedLaunch tl{st, e};
        bm::detpost_launch(tl, a, S, fp16);
        if (obb) { CHECK(hipStreamSynchronize(st)); continue; }
        CHECK(hipEventRecord(e[6], st)); CHECK(hipMemcpyAsync(h_pinned, d_pred, bytes, hipMemcpyDeviceToHost, st)); CHECK(hipEventRecord(e[7], st));
        CHECK(hipStreamSynchronize(st));
        CHECK(hipEventRecord(e[8], st)); CHECK(hipMemcpyAsync(h_pageable.data(), d_pred, bytes, hipMemcpyDeviceToHost, st)); CHECK(hipEventRecord(e[9], st));
        CHECK(hipStreamSynchronize(st));
    }
    CHECK(hipGetLastError());
    std::vector<float> t_score(reps), t_select(reps), t_both(reps), t_pin(reps), t_page(reps), t_extra(reps), t_three(reps);
    for (int k = 0; k < reps; ++k) {
        hipEvent_t* e = &ev[EV * (size_t)k];
        CHECK(hipEventElapsedTime(&t_score[k], e[0], e[1]));
        CHECK(hipEventElapsedTime(&t_select[k], e[2], e[3]));
        CHECK(hipEventElapsedTime(&t_both[k], e[0], e[3]));
        if (E) { CHECK(hipEventElapsedTime(&t_extra[k], e[4], e[5])); CHECK(hipEventElapsedTime(&t_three[k], e[0], e[5])); }
        if (obb) continue;
        CHECK(hipEventElapsedTime(&t_pin[k], e[6], e[7]));
        CHECK(hipEventElapsedTime(&t_page[k], e[8], e[9]));
    }
    std::vector<float> rows((size_t)max_det * cols);
    int n = 0, counters[bm::DP_COUNTERS];
    CHECK(hipMemcpy(&n, d_rows, 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(rows.data(), d_dets, rows.size() * 4, hipMemcpyDeviceToHost));
    double sum = 0.0;
    for (int k = 0; k < n * cols; ++k) sum += rows[k];
    if (E) std::printf("(a head with %d extra values per anchor, extra_kind %d)\n", E, kind);
    std::printf("%d streams of %d anchors x %d classes, layout %d%s, %s, K %d, max_det %d: tensor %.2f MB, LDS %d bytes per workgroup\n", S, A, nc, layout,
                obb ? (mode ? " oriented, fast NMS" : " oriented, greedy NMS") : "", fp16 ? "fp16" : "fp32", K, max_det, bytes * 1e-6, lds);
    report("k_detpost_score", t_score);
    report(obb ? "k_detpost_select_obb" : E ? "k_detpost_select_src" : "k_detpost_select", t_select);
    report("both kernels", t_both);
    if (E) {
        report("k_detpost_extra", t_extra);
        report("all three kernels", t_three);
    }
    if (!obb) {
        report("D2H of pred, pinned", t_pin);
        report("D2H of pred, pageable", t_page);
    }
    if (E) {                        // stream 0's extras and source anchors beside the rows
        std::vector<float> ex((size_t)max_det * E);
        std::vector<int> src(max_det);
        CHECK(hipMemcpy(ex.data(), d_extra, ex.size() * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(src.data(), d_src, src.size() * 4, hipMemcpyDeviceToHost));
        double esum = 0.0;
        long ssum = 0;
        for (int k = 0; k < n * E; ++k) esum += ex[k];
        for (int k = 0; k < n; ++k) ssum += src[k];
        std::printf("checksum: rows %d counters %d %d %d sum %.6f extra %.6f src %ld\n", n, counters[0], counters[1], counters[2], sum, esum, ssum);
        return 0;
    }
    std::printf("checksum: rows %d counters %d %d %d sum %.6f\n", n, counters[0], counters[1], counters[2], sum);
    return 0;
}
