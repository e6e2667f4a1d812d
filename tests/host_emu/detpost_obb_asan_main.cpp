// TEST-ONLY stand-alone program: the ORIENTED detection post-processing kernels on CPU threads (emu_detpost_obb.cpp, i.e.
// det_post.hpp + det_post_obb.hpp unchanged) under -fsanitize=address,undefined.  Every buffer is a heap block of exactly the size
// the library would allocate, so an access past the tensor, the scratch, the output block or the dynamic LDS is reported.
// Arguments: groups of 8 integers
//     S A nc fp16 K max_det nms_mode pass_percent
// (tests/test_detpost_obb_emu.py passes the shapes of detpost_obb_ref.CASES); the data is pseudo-random with quantised scores, a
// few objects and a few non-finite angles, so ties, the radix select and cross-chunk suppressions all occur.  Exit status 0 and a
// checksum line when every run kept its promises.
#include "emu_detpost_obb.cpp"

#include <cstdio>
#include <limits>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

template <class T>
static void fill(std::vector<T>& pred, int S, int A, int nc, int pass_percent) {
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < A; ++a) {
            auto at = [&](int c) -> T& { return pred[((size_t)s * (5 + nc) + c) * A + a]; };
            const int obj = (int)(rnd() % 8);       // a few objects: plenty of overlap
            at(0) = (T)(float)(80 + 60 * obj + (int)(rnd() % 9)); at(1) = (T)(float)(100 + (int)(rnd() % 9));
            at(2) = (T)(float)(40 + (int)(rnd() % 5)); at(3) = (T)(float)(10 + (int)(rnd() % 5));
            const bool active = (int)(rnd() % 100) < pass_percent;
            for (int c = 0; c < nc; ++c) at(4 + c) = (T)((active ? 8 + (int)(rnd() % 25) : (int)(rnd() % 4)) / 32.0f);
            const int kind = (int)(rnd() % 50);
            at(4 + nc) = kind == 0 ? (T)std::numeric_limits<float>::quiet_NaN() : kind == 1 ? (T)std::numeric_limits<float>::infinity()
                                                                                            : (T)(((int)(rnd() % 257) - 128) / 32.0f);
        }
}

int main(int argc, char** argv) {
    if (argc < 9 || (argc - 1) % 8) { std::fprintf(stderr, "usage: groups of S A nc fp16 K max_det nms_mode pass_percent\n"); return 2; }
    double sum = 0.0;
    for (int k = 1; k + 7 < argc; k += 8) {
        const int S = std::atoi(argv[k]), A = std::atoi(argv[k + 1]), nc = std::atoi(argv[k + 2]), fp16 = std::atoi(argv[k + 3]),
                  K = std::atoi(argv[k + 4]), max_det = std::atoi(argv[k + 5]), mode = std::atoi(argv[k + 6]), pct = std::atoi(argv[k + 7]);
        const size_t n = (size_t)S * A * (5 + nc);
        std::vector<_Float16> ph(fp16 ? n : 0);
        std::vector<float> pf(fp16 ? 0 : n);
        if (fp16) fill(ph, S, A, nc, pct); else fill(pf, S, A, nc, pct);
        std::vector<float> geom((size_t)S * 5);
        for (int s = 0; s < S; ++s) { float* g = &geom[5 * s]; g[0] = 1.0f / 3.0f; g[1] = 10.f; g[2] = 0.f; g[3] = 1080.f; g[4] = 1920.f; }
        std::vector<uint8_t> allow(nc, 1);
        if (nc > 1) allow[1] = 0;
        std::vector<float> dets((size_t)S * max_det * 7, -7.0f);
        std::vector<int> rows(S, -1), counters((size_t)S * bm::DP_COUNTERS, -1);
        emu_detpost_obb_run(S, A, nc, fp16, fp16 ? (const void*)ph.data() : (const void*)pf.data(), geom.data(), (k / 8) % 2 ? allow.data() : nullptr, K,
                            max_det, (k / 8) % 3 == 0, mode, (k / 8) % 2, 0.25f, 0.45f, dets.data(), max_det, rows.data(), counters.data());
        for (int s = 0; s < S; ++s) {
            const int* c = &counters[(size_t)s * bm::DP_COUNTERS];
            if (rows[s] < 0 || rows[s] > max_det || c[0] < 0 || c[0] > A || c[1] != (c[0] < K ? c[0] : K) || c[2] > c[1] || rows[s] != (c[2] < max_det ? c[2] : max_det)) {
                std::fprintf(stderr, "run %d stream %d: rows %d counters %d %d %d\n", k / 8, s, rows[s], c[0], c[1], c[2]);
                return 1;
            }
            for (int r = 0; r < max_det; ++r)
                for (int j = 0; j < 7; ++j) {
                    const float v = dets[((size_t)s * max_det + r) * 7 + j];
                    if (r >= rows[s] && v != -7.0f) { std::fprintf(stderr, "run %d stream %d: row %d beyond the count was written\n", k / 8, s, r); return 1; }
                    if (r < rows[s]) {
                        if (!(v == v) || v - v != 0.0f) { std::fprintf(stderr, "run %d stream %d: row %d has a non-finite value\n", k / 8, s, r); return 1; }
                        sum += v;
                    }
                }
        }
    }
    std::printf("detpost_obb_asan_main: %d runs, checksum %.3f\n", (argc - 1) / 8, sum);
    return 0;
}
