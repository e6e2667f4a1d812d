// TEST-ONLY stand-alone program: the detection post-processing of a head with per-anchor extras on CPU threads
// (emu_detpost_extra.cpp, i.e. det_post.hpp, det_post_tiled.hpp and det_post_extra.hpp unchanged) under -fsanitize=address,undefined.
// Every buffer is a heap block of exactly the size the library would allocate, so an access past the tensor, the scratch, one of
// the four output blocks or the dynamic LDS is reported.  Arguments: groups of 11 integers
//     S T A nc layout fp16 K max_det E kind pass_percent                (T = 0: untiled)
// (tests/test_detpost_extra_emu.py passes the shapes of detpost_extra_ref.CASES); the data is pseudo-random with quantised scores, so
// ties, the radix select and cross-chunk suppressions all occur; every other run passes no src block.  Exit status 0 and a checksum
// line when every run kept its promises.
#include "emu_detpost_extra.cpp"

#include <cstdio>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

template <class T>
static void fill(std::vector<T>& pred, int N, int A, int nc, int E, int layout, int pass_percent) {
    for (int s = 0; s < N; ++s)
        for (int a = 0; a < A; ++a) {
            auto at = [&](int c) -> T& { return pred[layout == 0 ? ((size_t)s * (4 + nc + E) + c) * A + a : ((size_t)s * A + a) * (5 + nc + E) + c]; };
            const int obj = (int)(rnd() % 6);       // a few objects: plenty of overlap, within and across the tiles
            at(0) = (T)(float)(8 + 9 * obj + (int)(rnd() % 3)); at(1) = (T)(float)(20 + (int)(rnd() % 3));
            at(2) = (T)(float)(8 + (int)(rnd() % 3)); at(3) = (T)(float)(8 + (int)(rnd() % 3));
            const bool active = (int)(rnd() % 100) < pass_percent;
            if (layout == 1) at(4) = (T)1.0f;
            const int first = layout == 0 ? 4 : 5;
            for (int c = 0; c < nc; ++c) at(first + c) = (T)((active ? 8 + (int)(rnd() % 25) : (int)(rnd() % 4)) / 32.0f);
            for (int e = 0; e < E; ++e) at(first + nc + e) = (T)(float)((int)(rnd() % 440) / 4.0f - 20.0f);
        }
}

int main(int argc, char** argv) {
    if (argc < 12 || (argc - 1) % 11) { std::fprintf(stderr, "usage: groups of S T A nc layout fp16 K max_det E kind pass_percent\n"); return 2; }
    double sum = 0.0;
    for (int k = 1, run = 0; k + 10 < argc; k += 11, ++run) {
        const int S = std::atoi(argv[k]), T = std::atoi(argv[k + 1]), A = std::atoi(argv[k + 2]), nc = std::atoi(argv[k + 3]), layout = std::atoi(argv[k + 4]),
                  fp16 = std::atoi(argv[k + 5]), K = std::atoi(argv[k + 6]), max_det = std::atoi(argv[k + 7]), E = std::atoi(argv[k + 8]),
                  kind = std::atoi(argv[k + 9]), pct = std::atoi(argv[k + 10]);
        const int NT = T ? T : 1;
        const size_t n = (size_t)S * NT * A * ((layout == 0 ? 4 : 5) + nc + E);
        std::vector<_Float16> ph(fp16 ? n : 0);
        std::vector<float> pf(fp16 ? 0 : n);
        if (fp16) fill(ph, S * NT, A, nc, E, layout, pct); else fill(pf, S * NT, A, nc, E, layout, pct);
        std::vector<float> geom((size_t)S * NT * (T ? 7 : 5));
        for (int q = 0; q < S * NT; ++q) {
            float* g = &geom[(size_t)q * (T ? 7 : 5)];
            if (T) { g[0] = q % T ? 0.5f : 1.0f / 3.0f; g[1] = q % T ? 0.f : 10.f; g[2] = 0.f; g[3] = 32.f * (q % T); g[4] = 0.f; g[5] = 128.f; g[6] = 100.f; }
            else { g[0] = 1.0f / 3.0f; g[1] = 10.f; g[2] = 0.f; g[3] = 100.f; g[4] = 192.f; }
        }
        std::vector<uint8_t> allow(nc, 1);
        if (nc > 1) allow[1] = 0;
        std::vector<float> dets((size_t)S * max_det * 6, -7.0f), extra((size_t)S * max_det * E, -7.0f);
        std::vector<int> rows(S, -1), counters((size_t)S * bm::DP_COUNTERS, -1), src((size_t)S * max_det, -7);
        const bool with_src = run % 2 == 0;
        emu_detpost_extra_run(S, T, A, nc, layout, fp16, fp16 ? (const void*)ph.data() : (const void*)pf.data(), geom.data(), run % 2 ? allow.data() : nullptr, K,
                              max_det, run % 3 == 0, run % 2, 0.25f, 0.45f, dets.data(), max_det, rows.data(), counters.data(), E, kind, extra.data(),
                              with_src ? src.data() : nullptr);
        for (int s = 0; s < S; ++s) {
            const int* c = &counters[(size_t)s * bm::DP_COUNTERS];
            if (rows[s] < 0 || rows[s] > max_det || c[0] < 0 || c[0] > NT * A || c[1] != (c[0] < K ? c[0] : K) || c[2] > c[1] || rows[s] != (c[2] < max_det ? c[2] : max_det)) {
                std::fprintf(stderr, "run %d stream %d: rows %d counters %d %d %d\n", run, s, rows[s], c[0], c[1], c[2]);
                return 1;
            }
            for (int r = 0; r < max_det; ++r) {
                const int a = src[(size_t)s * max_det + r];
                if (with_src ? (r < rows[s] ? a < 0 || a >= NT * A : a != -7) : a != -7) {
                    std::fprintf(stderr, "run %d stream %d: src row %d holds %d\n", run, s, r, a);
                    return 1;
                }
                for (int e = 0; e < E; ++e) {
                    const float v = extra[((size_t)s * max_det + r) * E + e];
                    if (r >= rows[s] && v != -7.0f) { std::fprintf(stderr, "run %d stream %d: extras of row %d beyond the count were written\n", run, s, r); return 1; }
                    if (r < rows[s]) sum += v;
                }
            }
        }
    }
    std::printf("detpost_extra_asan_main: %d runs, checksum %.3f\n", (argc - 1) / 11, sum);
    return 0;
}
