// Standalone timing of the ORIENTED ReID front end beside the axis-aligned one it mirrors.  Development tool, not part of the library
// (built and run by tools/obb_reid_prof.py):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/obb_reid_prof.hip -o tools/_build/obb_reid_prof
//   tools/_build/obb_reid_prof [streams 64] [crops per stream 64] [rows 1080] [cols 1920] [repeats 30]
// Workload: `streams` random frames, `crops` oriented detections per stream (all above the threshold), OSNet-x0.25 with random weights
// in mode 2 (only the access pattern and the instruction stream matter).  HIP events around every launch (set), 5 warm-up and
// `repeats` timed runs of each, the two sides alternating; median, min and max.  Three pairs:
//   crop list   build_crop_list_kernel on the enclosing boxes      | build_crop_list_obb_kernel (geometry made on the device)
//   crops       k_crop_resize_rgbx_hl on the enclosing boxes       | k_crop_resize_obb_rgbx_hl
//   ReID pass   ReidEngine::run_counted, axis-aligned (crop fused into the stem, as shipped; and with the separate crop kernel)
//                                                                  | run_counted with the oriented geometry (separate crop kernel)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../boxmot_amd/csrc/crop_list.hpp"
#include "../boxmot_amd/csrc/reid_engine.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static unsigned g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return ((g_seed >> 8) & 0xffff) / 65536.0f; }

template <class T> static T* dev(const std::vector<T>& v) {
    T* d; CK(hipMalloc(&d, v.size() * sizeof(T))); CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); return d;
}
template <class T> static T* dev_zero(size_t n) { T* d; CK(hipMalloc(&d, n * sizeof(T))); CK(hipMemset(d, 0, n * sizeof(T))); return d; }

struct Stat { float med, mn, mx; };

// alternate a and b: 5 warm-up and `repeats` timed runs each, every run with its own event pair
static void time_pair(hipStream_t st, int repeats, const std::function<void()>& a, const std::function<void()>& b, Stat& sa, Stat& sb) {
    const int warm = 5, n = warm + repeats;
    std::vector<hipEvent_t> ev((size_t)n * 4);
    for (auto& e : ev) CK(hipEventCreate(&e));
    for (int k = 0; k < n; ++k) {
        CK(hipEventRecord(ev[4 * k], st)); a(); CK(hipEventRecord(ev[4 * k + 1], st));
        CK(hipEventRecord(ev[4 * k + 2], st)); b(); CK(hipEventRecord(ev[4 * k + 3], st));
    }
    CK(hipStreamSynchronize(st));
    CK(hipGetLastError());
    auto stat = [&](int off) {
        std::vector<float> t;
        for (int k = warm; k < n; ++k) { float ms = 0; CK(hipEventElapsedTime(&ms, ev[4 * k + off], ev[4 * k + off + 1])); t.push_back(ms * 1000.f); }
        std::sort(t.begin(), t.end());
        return Stat{(t[t.size() / 2] + t[(t.size() - 1) / 2]) / 2, t.front(), t.back()};
    };
    sa = stat(0); sb = stat(2);
    for (auto& e : ev) CK(hipEventDestroy(e));
}

static void line(const char* what, const Stat& a, const Stat& b) {
    printf("%-58s %9.1f %9.1f %9.1f | %9.1f %9.1f %9.1f | %5.2fx\n", what, a.med, a.mn, a.mx, b.med, b.mn, b.mx, b.med / a.med);
}

int main(int argc, char** argv) {
    const int S = argc > 1 ? atoi(argv[1]) : 64, ND = argc > 2 ? atoi(argv[2]) : 64, H = argc > 3 ? atoi(argv[3]) : 1080,
              W = argc > 4 ? atoi(argv[4]) : 1920, repeats = argc > 5 ? atoi(argv[5]) : 30;
    if (S < 1 || ND < 1 || H < 16 || W < 16 || repeats < 1 || (long)S * ND > 4096) { fprintf(stderr, "bad arguments (streams x crops <= 4096)\n"); return 2; }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { fprintf(stderr, "no HIP device\n"); return 3; }
    const int N = S * ND;
    hipStream_t st;
    CK(hipStreamCreate(&st));

    // frames: one random picture per stream
    std::vector<uint8_t> pic((size_t)H * W * 3);
    std::vector<const uint8_t*> fptr(S);
    for (int s = 0; s < S; ++s) {
        for (auto& v : pic) v = (uint8_t)(rnd() * 255.f);
        fptr[s] = dev(pic);
    }
    const uint8_t** d_frames = dev(fptr);

    // oriented detections [cx, cy, w, h, angle, conf, cls] and their enclosing boxes [x1, y1, x2, y2, conf, cls]
    std::vector<float> obb((size_t)N * 7), box((size_t)N * 6);
    for (int i = 0; i < N; ++i) {
        const float cx = 60.f + rnd() * (W - 120.f), cy = 60.f + rnd() * (H - 120.f), w = 40.f + rnd() * 80.f, h = 80.f + rnd() * 160.f;
        const float a = (rnd() * 2.f - 1.f) * 3.14159265f, c = std::fabs(std::cos(a)), s = std::fabs(std::sin(a));
        const float ex = 0.5f * (w * c + h * s), ey = 0.5f * (w * s + h * c);
        float* o = &obb[(size_t)i * 7];
        o[0] = cx; o[1] = cy; o[2] = w; o[3] = h; o[4] = a; o[5] = 0.9f; o[6] = 0.f;
        float* b = &box[(size_t)i * 6];
        b[0] = cx - ex; b[1] = cy - ey; b[2] = cx + ex; b[3] = cy + ey; b[4] = 0.9f; b[5] = 0.f;
    }
    float *d_obb = dev(obb), *d_box = dev(box);
    std::vector<int> nd(S, ND);
    int* d_nd = dev(nd);
    int *d_count = dev_zero<int>(1), *d_cs = dev_zero<int>(N), *d_row = dev_zero<int>(N);          // axis-aligned list
    int *d_cs_o = dev_zero<int>(N), *d_row_o = dev_zero<int>(N);                                   // oriented list (its own entry order)
    float* d_cb = dev_zero<float>((size_t)N * 4);
    double* d_geo = dev_zero<double>((size_t)N * 8);
    float* d_emb = dev_zero<float>((size_t)N * 512);

    // OSNet-x0.25, random weights
    const int ch[4] = {16, 64, 96, 128};
    const bm::OsnetLayout L = bm::make_osnet_layout(ch, 512);
    std::vector<float> blob((size_t)bm::REID_HEADER_INTS + L.total, 0.f);
    int32_t* hdr = reinterpret_cast<int32_t*>(blob.data());
    hdr[0] = bm::REID_MAGIC; hdr[1] = ch[0]; hdr[2] = ch[1]; hdr[3] = ch[2]; hdr[4] = ch[3]; hdr[5] = 512; hdr[6] = (int32_t)L.total;
    for (long k = 0; k < L.total; ++k) blob[bm::REID_HEADER_INTS + k] = rnd() * 0.2f - 0.1f;
    bm::ReidEngine eng(blob.data(), (long)blob.size(), N, N);
    eng.set_mode(2);

    printf("oriented ReID front end beside the axis-aligned one: %d streams x %d crops, %d x %d frames, OSNet-x0.25 mode 2; HIP events, "
           "%d timed runs after 5 warm-up runs, alternating; microseconds\n", S, ND, H, W, repeats);
    printf("%-58s %9s %9s %9s | %9s %9s %9s | %6s\n", "", "aabb med", "min", "max", "obb med", "min", "max", "ratio");
    Stat a, b;

    auto list_aabb = [&]() {
        CK(hipMemsetAsync(d_count, 0, 4, st));
        hipLaunchKernelGGL(bm::build_crop_list_kernel, dim3(S), dim3(256), 0, st, (const float*)d_box, (const int*)d_nd, ND, 0.5, d_count, d_cs, d_cb, d_row, 0, 0);
    };
    auto list_obb = [&]() {
        CK(hipMemsetAsync(d_count, 0, 4, st));
        hipLaunchKernelGGL(bm::build_crop_list_obb_kernel, dim3(S), dim3(256), 0, st, (const float*)d_obb, (const int*)d_nd, ND, 0.5, d_count, d_cs_o, d_row_o, d_geo, 0, 0);
    };
    time_pair(st, repeats, list_aabb, list_obb, a, b);
    line("crop list (count memset + kernel)", a, b);

    // each side keeps the table its own kernel wrote last (the same (stream, row) set, each in its own order)
    list_aabb(); list_obb();
    CK(hipStreamSynchronize(st));
    int count = 0;
    CK(hipMemcpy(&count, d_count, 4, hipMemcpyDeviceToHost));
    if (count != N) { fprintf(stderr, "crop list holds %d entries, expected %d\n", count, N); return 1; }

    eng.set_fuse_stem(false);
    auto crops_aabb = [&]() { eng.set_obb_geometry(nullptr); eng.preprocess(d_frames, d_cs, d_cb, 4, N, W, H, st); };
    auto crops_obb = [&]() { eng.set_obb_geometry(d_geo); eng.preprocess(d_frames, d_cs_o, d_cb, 4, N, W, H, st); eng.set_obb_geometry(nullptr); };
    time_pair(st, repeats, crops_aabb, crops_obb, a, b);
    line("(hi, lo) crop kernel (enclosing boxes | oriented)", a, b);

    auto pass_aabb = [&]() { eng.set_obb_geometry(nullptr); eng.run_counted(d_frames, d_cs, d_cb, 4, d_count, N, W, H, d_emb, d_row, st); };
    auto pass_obb = [&]() { eng.set_obb_geometry(d_geo); eng.run_counted(d_frames, d_cs_o, d_cb, 4, d_count, N, W, H, d_emb, d_row_o, st); eng.set_obb_geometry(nullptr); };
    time_pair(st, repeats, pass_aabb, pass_obb, a, b);
    line("ReID pass, separate crop kernel on both sides", a, b);
    eng.set_fuse_stem(true);
    time_pair(st, repeats, pass_aabb, pass_obb, a, b);
    line("ReID pass as shipped (aabb: crop fused into the stem)", a, b);

    std::vector<float> e((size_t)N * 512);
    CK(hipMemcpy(e.data(), d_emb, e.size() * 4, hipMemcpyDeviceToHost));
    double sum = 0;
    bool finite = true;
    for (float v : e) { finite = finite && std::isfinite(v); sum += v; }
    printf("embeddings of the last oriented pass (random weights): %s, checksum %.4f\n", finite ? "finite" : "not all finite", sum);
    return 0;
}
