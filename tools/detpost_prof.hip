// Development tool behind tools/detpost_prof.py: times of the two detection post-processing kernels (boxmot_amd/csrc/det_post.hpp,
// through its own kernel sequence detpost_launch) for S streams of one prediction tensor, beside the first half of what they
// replace: the device-to-host copy of the S-stream tensor (into pinned and into pageable memory).  The other half, the NumPy
// reference on the host, is timed by detpost_prof.py on the same tensor.  Every launch has its own pair of HIP events.  Prints one
// line per kernel -- median, min and max in microseconds -- and a checksum of stream 0's output (the sum of its rows' 6 columns, 7
// on the oriented path, and its counters) that detpost_prof.py compares with the reference's.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o detpost_prof tools/detpost_prof.hip
//     ./detpost_prof pred.bin [streams = 16] [anchors = 8400] [classes = 80] [layout = 0] [fp16 = 1] [K = 1024] [max_det = 256] [repeats = 30]
//                   [obb = 0] [nms_mode = 0] [extra = 0] [extra_kind = 0] [mask_h = 0] [mask_w = 0] [in_h = 0] [in_w = 0] [proto.bin]
// pred.bin: ONE stream's tensor, (4 + nc, A) or (A, 5 + nc), raw; every stream gets a copy.  obb = 1: the oriented layout
// (det_post_obb.hpp), (4 + nc + 1, A) with layout 0, nms_mode 0 greedy / 1 fast; the host copies are not timed again.  conf 0.25, iou 0.45, class-aware,
// geometry of a 1080 x 1920 frame in a centred 640 x 640 letterbox.  extra = E > 0: a head with E more values per anchor
// (det_post_extra.hpp), (4 + nc + E, A) or (A, 5 + nc + E): the three-kernel sequence -- score, the select kernel's source-storing
// variant, k_detpost_extra -- a line for the third kernel, and the sums of stream 0's extras and source anchors in the checksum.
// mask_h > 0 (with extra = E, extra_kind 0): a mask handle's four-kernel sequence (det_post_mask.hpp); proto.bin is ONE stream's
// (E, mask_h, mask_w) fp16 prototypes, every stream gets a copy.  A line for k_detpost_mask, one for a hipMemsetAsync of exactly the
// emitted mask bytes (streams x rows x mask_h x mask_w, into a block of its own) timed in the same calls -- the floor of a kernel
// that must write those bytes -- one for the device-to-host copy of the prototypes, and in the checksum the sum of stream 0's mask
// bytes and a position-weighted sum of them.
//     ./detpost_prof labels dets.bin coef.bin proto.bin n_rows streams E mask_h mask_w in_h in_w rows cols gain top left [repeats = 30]
// the label-map kernel alone (det_post_labels.hpp): ONE stream's rows (n_rows, 6) float32 in frame coordinates, coefficients (n_rows, E)
// float32 and (E, mask_h, mask_w) fp16 prototypes, every stream gets a copy; k_detpost_labels on the path it chooses (the LDS patch)
// and with the fallback forced, in alternating blocks of five launches, each launch between its own pair of events.  The checksum is
// the sum and a position-weighted sum of stream 0's labels; the two paths must give equal blocks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../boxmot_amd/csrc/det_post_labels.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static void report(const char* name, std::vector<float> ms) {
    std::sort(ms.begin(), ms.end());
    std::printf("%-22s median %.1f us  min %.1f  max %.1f  (%zu samples)\n", name, 1e3 * ms[ms.size() / 2], 1e3 * ms.front(), 1e3 * ms.back(), ms.size());
}

struct TimedLaunch {            // every kernel of the sequence between its own pair of events
    hipStream_t stream;
    hipEvent_t* ev;             // [8]: up to four kernels
    int k = 0;
    template <class K, class... A>
    void operator()(K kernel, int gx, int gy, int threads, size_t lds_bytes, A... args) {
        (void)hipEventRecord(ev[2 * k], stream);
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3((unsigned)threads), lds_bytes, stream, args...);
        (void)hipEventRecord(ev[2 * k + 1], stream);
        ++k;
    }
};

struct PlainLaunch {
    hipStream_t stream;
    template <class K, class... A>
    void operator()(K kernel, int gx, int gy, int threads, size_t lds_bytes, A... args) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3((unsigned)threads), lds_bytes, stream, args...);
    }
};

template <class T>
static bool read_file(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) std::fclose(f);
    if (!ok) std::fprintf(stderr, "%s: cannot read %zu bytes\n", path, v.size() * sizeof(T));
    return ok;
}

static int labels_main(int argc, char** argv) {
    if (argc < 18) { std::fprintf(stderr, "usage: detpost_prof labels dets.bin coef.bin proto.bin n_rows streams E mask_h mask_w in_h in_w rows cols gain top left [repeats]\n"); return 1; }
    const int n = std::atoi(argv[5]), S = std::atoi(argv[6]), E = std::atoi(argv[7]), mh = std::atoi(argv[8]), mw = std::atoi(argv[9]), in_h = std::atoi(argv[10]),
              in_w = std::atoi(argv[11]), rows = std::atoi(argv[12]), cols = std::atoi(argv[13]), reps = argc > 17 ? std::atoi(argv[17]) : 30;
    const float gain = (float)std::atof(argv[14]), top = (float)std::atof(argv[15]), left = (float)std::atof(argv[16]);
    if (n < 1 || n > bm::DP_LABEL_MAX_DET || S < 1 || E < 1 || E > bm::DP_MASK_E_MAX || mh < 1 || mh > bm::DP_MASK_DIM_MAX || mw < 1 || mw > bm::DP_MASK_DIM_MAX || in_h < 1 ||
        in_w < 1 || rows < 1 || cols < 1 || !(gain > 0.f) || reps < 10 || reps % 5) {
        std::fprintf(stderr, "labels: n_rows within 1..32767, E within 1..256, mask within 1..1024, a frame of >= 1 x 1, gain > 0, repeats a multiple of 5\n");
        return 1;
    }
    const size_t plane = (size_t)mh * mw, frame = (size_t)rows * cols;
    std::vector<float> dets((size_t)n * 6), coef((size_t)n * E);
    std::vector<_Float16> proto((size_t)E * plane);
    if (!read_file(argv[2], dets) || !read_file(argv[3], coef) || !read_file(argv[4], proto)) return 1;
    float *d_dets = nullptr, *d_coef = nullptr;
    void* d_proto = nullptr;
    int* d_rows = nullptr;
    int16_t* d_labels[2] = {nullptr, nullptr};
    bm::DetPostGeom* d_geom = nullptr;
    CHECK(hipMalloc(&d_dets, (size_t)S * n * 6 * 4));
    CHECK(hipMalloc(&d_coef, (size_t)S * n * E * 4));
    CHECK(hipMalloc(&d_proto, (size_t)S * E * plane * 2));
    CHECK(hipMalloc(&d_rows, (size_t)S * 4));
    CHECK(hipMalloc(&d_geom, (size_t)S * sizeof(bm::DetPostGeom)));
    for (int q = 0; q < 2; ++q) { CHECK(hipMalloc(&d_labels[q], (size_t)S * frame * 2)); CHECK(hipMemset(d_labels[q], 0xA5, (size_t)S * frame * 2)); }
    std::vector<int> n_rows(S, n);
    std::vector<bm::DetPostGeom> geom(S, bm::DetPostGeom{gain, top, left, (float)rows, (float)cols});
    for (int s = 0; s < S; ++s) {
        CHECK(hipMemcpy(d_dets + (size_t)s * n * 6, dets.data(), dets.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_coef + (size_t)s * n * E, coef.data(), coef.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy((_Float16*)d_proto + (size_t)s * E * plane, proto.data(), proto.size() * 2, hipMemcpyHostToDevice));
    }
    CHECK(hipMemcpy(d_rows, n_rows.data(), (size_t)S * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_geom, geom.data(), (size_t)S * sizeof(bm::DetPostGeom), hipMemcpyHostToDevice));
    hipStream_t st;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    PlainLaunch on{st};
    auto launch = [&](int fallback) {
        const bm::DetPostLabelArgs a{d_geom, d_proto, d_dets, d_rows, d_coef, d_labels[fallback], (long)E * (long)plane, (long)frame, cols, n, n, E, mh, mw, (int)plane,
                                     (float)mw / (float)in_w, (float)mh / (float)in_h, 0, fallback};
        bm::detpost_launch_labels(on, a, S, rows, cols, 1);
    };
    for (int k = 0; k < 3; ++k) { launch(0); launch(1); }
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(st));
    std::vector<hipEvent_t> ev(4 * (size_t)reps);
    for (auto& e : ev) CHECK(hipEventCreate(&e));
    for (int block = 0; block < reps / 5; ++block)
        for (int fallback = 0; fallback < 2; ++fallback)
            for (int k = 0; k < 5; ++k) {
                hipEvent_t* e = &ev[4 * (size_t)(block * 5 + k) + 2 * fallback];
                CHECK(hipEventRecord(e[0], st)); launch(fallback); CHECK(hipEventRecord(e[1], st));
                CHECK(hipStreamSynchronize(st));
            }
    CHECK(hipGetLastError());
    std::vector<float> t[2] = {std::vector<float>(reps), std::vector<float>(reps)};
    for (int k = 0; k < reps; ++k)
        for (int q = 0; q < 2; ++q) CHECK(hipEventElapsedTime(&t[q][k], ev[4 * (size_t)k + 2 * q], ev[4 * (size_t)k + 2 * q + 1]));
    std::vector<int16_t> got[2] = {std::vector<int16_t>((size_t)S * frame), std::vector<int16_t>((size_t)S * frame)};
    for (int q = 0; q < 2; ++q) CHECK(hipMemcpy(got[q].data(), d_labels[q], got[q].size() * 2, hipMemcpyDeviceToHost));
    std::printf("%d streams of %d x %d frames, %d rows per stream, E %d, prototypes %d x %d fp16 of a %d x %d input, gain %.6f: %d x %d tiles per stream, labels %.2f MB\n", S, rows,
                cols, n, E, mh, mw, in_h, in_w, gain, bm::detpost_label_tiles(cols, bm::DP_LABEL_TW), bm::detpost_label_tiles(rows, bm::DP_LABEL_TH), S * frame * 2e-6);
    report("labels, LDS patch", t[0]);
    report("labels, forced fallback", t[1]);
    if (got[0] != got[1]) { std::fprintf(stderr, "the LDS path and the fallback path differ\n"); return 1; }
    std::printf("the two paths give equal label blocks\n");
    long sum = 0, wsum = 0, owned = 0;
    for (size_t k = 0; k < frame; ++k) { sum += got[0][k]; wsum += (long)got[0][k] * (long)(k % 251 + 1); owned += got[0][k] >= 0; }
    std::printf("checksum: labels sum %ld weighted %ld owned %ld\n", sum, wsum, owned);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "labels")) return labels_main(argc, argv);
    auto arg = [&](int k, int d) { return argc > k ? std::atoi(argv[k]) : d; };
    if (argc < 2) { std::fprintf(stderr, "usage: detpost_prof pred.bin [streams anchors classes layout fp16 K max_det repeats]\n"); return 1; }
    const int S = arg(2, 16), A = arg(3, 8400), nc = arg(4, 80), layout = arg(5, 0), fp16 = arg(6, 1), K = arg(7, 1024), max_det = arg(8, 256), reps = arg(9, 30),
              obb = arg(10, 0), mode = arg(11, 0), cols = obb ? 7 : 6, E = arg(12, 0), kind = arg(13, 0), mh = arg(14, 0), mw = arg(15, 0), in_h = arg(16, 0),
              in_w = arg(17, 0);
    if (mh && (!E || kind != 0 || E > bm::DP_MASK_E_MAX || mh < 1 || mh > bm::DP_MASK_DIM_MAX || mw < 1 || mw > bm::DP_MASK_DIM_MAX || in_h < 1 || in_w < 1 || argc < 19)) {
        std::fprintf(stderr, "masks: extra within 1..256 of extra_kind 0, mask_h and mask_w within 1..1024, in_h and in_w >= 1, and proto.bin\n");
        return 1;
    }
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
    const size_t plane = (size_t)mh * mw, proto_per = (size_t)E * plane * 2, proto_bytes = proto_per * S, mask_bytes = (size_t)S * max_det * plane;
    void *d_proto = nullptr, *h_proto = nullptr;
    uint8_t *d_masks = nullptr, *d_yard = nullptr;
    if (mh) {
        std::vector<unsigned char> one_proto(proto_per);
        FILE* f = std::fopen(argv[18], "rb");
        if (!f || std::fread(one_proto.data(), 1, proto_per, f) != proto_per) { std::fprintf(stderr, "%s: cannot read %zu bytes\n", argv[18], proto_per); return 1; }
        std::fclose(f);
        CHECK(hipMalloc(&d_proto, proto_bytes));
        CHECK(hipMalloc(&d_masks, mask_bytes));
        CHECK(hipMalloc(&d_yard, mask_bytes));
        CHECK(hipMemset(d_masks, 0xA5, mask_bytes));
        CHECK(hipHostMalloc(&h_proto, proto_bytes, hipHostMallocDefault));
        for (int s = 0; s < S; ++s) CHECK(hipMemcpy((unsigned char*)d_proto + proto_per * s, one_proto.data(), proto_per, hipMemcpyHostToDevice));
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
    const bm::DetPostMaskArgs m{d_proto, d_masks, (long)E * (long)plane, (int)plane, mh, mw, mh ? (float)mw / (float)in_w : 0.f, mh ? (float)mh / (float)in_h : 0.f, 0};
    auto sequence = [&](TimedLaunch& on) { if (mh) bm::detpost_launch_with_mask(on, a, m, S, fp16, 1); else bm::detpost_launch(on, a, S, fp16); };
    constexpr int EV = 16;          // events per timed call: four kernel pairs, two copy pairs, the memset, the prototypes' copy
    std::vector<hipEvent_t> ev(EV * (size_t)reps);
    for (auto& e : ev) CHECK(hipEventCreate(&e));
    for (int k = 0; k < 5; ++k) { TimedLaunch warm{st, ev.data()}; sequence(warm); }
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(st));
    int n = 0;                      // stream 0's rows: every stream holds the same tensor
    CHECK(hipMemcpy(&n, d_rows, 4, hipMemcpyDeviceToHost));
    const size_t emitted = (size_t)S * n * plane;
    for (int k = 0; k < reps; ++k) {
        hipEvent_t* e = &ev[EV * (size_t)k];
        TimedLaunch tl{st, e};
        sequence(tl);
        if (obb) { CHECK(hipStreamSynchronize(st)); continue; }
        CHECK(hipEventRecord(e[8], st)); CHECK(hipMemcpyAsync(h_pinned, d_pred, bytes, hipMemcpyDeviceToHost, st)); CHECK(hipEventRecord(e[9], st));
        CHECK(hipStreamSynchronize(st));
        CHECK(hipEventRecord(e[10], st)); CHECK(hipMemcpyAsync(h_pageable.data(), d_pred, bytes, hipMemcpyDeviceToHost, st)); CHECK(hipEventRecord(e[11], st));
        CHECK(hipStreamSynchronize(st));
        if (mh) {
            CHECK(hipEventRecord(e[12], st)); if (emitted) CHECK(hipMemsetAsync(d_yard, 0, emitted, st)); CHECK(hipEventRecord(e[13], st));
            CHECK(hipStreamSynchronize(st));
            CHECK(hipEventRecord(e[14], st)); CHECK(hipMemcpyAsync(h_proto, d_proto, proto_bytes, hipMemcpyDeviceToHost, st)); CHECK(hipEventRecord(e[15], st));
            CHECK(hipStreamSynchronize(st));
        }
    }
    CHECK(hipGetLastError());
    std::vector<float> t_score(reps), t_select(reps), t_both(reps), t_pin(reps), t_page(reps), t_extra(reps), t_three(reps), t_mask(reps), t_four(reps), t_set(reps),
        t_proto(reps);
    for (int k = 0; k < reps; ++k) {
        hipEvent_t* e = &ev[EV * (size_t)k];
        CHECK(hipEventElapsedTime(&t_score[k], e[0], e[1]));
        CHECK(hipEventElapsedTime(&t_select[k], e[2], e[3]));
        CHECK(hipEventElapsedTime(&t_both[k], e[0], e[3]));
        if (E) { CHECK(hipEventElapsedTime(&t_extra[k], e[4], e[5])); CHECK(hipEventElapsedTime(&t_three[k], e[0], e[5])); }
        if (mh) {
            CHECK(hipEventElapsedTime(&t_mask[k], e[6], e[7])); CHECK(hipEventElapsedTime(&t_four[k], e[0], e[7]));
            CHECK(hipEventElapsedTime(&t_set[k], e[12], e[13])); CHECK(hipEventElapsedTime(&t_proto[k], e[14], e[15]));
        }
        if (obb) continue;
        CHECK(hipEventElapsedTime(&t_pin[k], e[8], e[9]));
        CHECK(hipEventElapsedTime(&t_page[k], e[10], e[11]));
    }
    std::vector<float> rows((size_t)max_det * cols);
    int counters[bm::DP_COUNTERS];
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
    if (mh) {
        std::printf("(masks %d x %d of a %d x %d input, fp16 prototypes %.2f MB; %d rows per stream: %zu mask bytes emitted)\n", mh, mw, in_h, in_w, proto_bytes * 1e-6, n, emitted);
        report("k_detpost_mask", t_mask);
        report("all four kernels", t_four);
        report("memset of those bytes", t_set);
        report("D2H of proto, pinned", t_proto);
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
        if (mh) {                   // ... and stream 0's masks
            std::vector<uint8_t> mk((size_t)n * plane);
            CHECK(hipMemcpy(mk.data(), d_masks, mk.size(), hipMemcpyDeviceToHost));
            long msum = 0, wsum = 0;
            for (size_t k = 0; k < mk.size(); ++k) { msum += mk[k]; wsum += (long)mk[k] * (long)(k % 251 + 1); }
            std::printf("checksum: rows %d counters %d %d %d sum %.6f extra %.6f src %ld mask %ld weighted %ld\n", n, counters[0], counters[1], counters[2], sum, esum,
                        ssum, msum, wsum);
            return 0;
        }
        std::printf("checksum: rows %d counters %d %d %d sum %.6f extra %.6f src %ld\n", n, counters[0], counters[1], counters[2], sum, esum, ssum);
        return 0;
    }
    std::printf("checksum: rows %d counters %d %d %d sum %.6f\n", n, counters[0], counters[1], counters[2], sum);
    return 0;
}
