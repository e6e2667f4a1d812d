// TEST-ONLY stand-alone program: the two tiled-detection kernels on CPU threads (emu_tiles.cpp, i.e. ingest_letterbox_tiles.hpp and
// det_post_tiled.hpp unchanged) under -fsanitize=address,undefined.  Every buffer is a heap block of exactly the size the library
// would allocate -- a frame is rows * cols * 3 bytes and nothing more -- so a tap read past a rectangle that is flush with the
// frame's last row or column, or an access past the tensor, the scratch, the output block or the dynamic LDS, is reported.
// Arguments: a list of runs, each introduced by a letter,
//     L n T H W mode fp16  then per stream: rows cols  then per (stream, tile): x0 y0 w h
//     D S T A nc layout fp16 K max_det merge pass_percent
// (tests/test_tiles_emu.py passes the shapes of its references).  Exit status 0 and a checksum line when every run kept its promises.
#include "emu_tiles.cpp"

#include <cstdio>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

static int run_letterbox(char** a, int& k, double& sum) {
    const int n = std::atoi(a[k]), T = std::atoi(a[k + 1]), H = std::atoi(a[k + 2]), W = std::atoi(a[k + 3]), mode = std::atoi(a[k + 4]),
              fp16 = std::atoi(a[k + 5]);
    k += 6;
    std::vector<int> rows(n), cols(n), rects((size_t)n * T * 4);
    for (int s = 0; s < n; ++s) { rows[s] = std::atoi(a[k]); cols[s] = std::atoi(a[k + 1]); k += 2; }
    for (size_t q = 0; q < rects.size(); ++q) rects[q] = std::atoi(a[k++]);
    std::vector<std::vector<uint8_t>> frames(n);
    std::vector<const uint8_t*> ptrs(n);
    for (int s = 0; s < n; ++s) {
        frames[s].resize((size_t)rows[s] * cols[s] * 3);
        for (auto& b : frames[s]) b = (uint8_t)rnd();
        ptrs[s] = frames[s].data();
    }
    uint32_t lut[256];
    for (int v = 0; v < 256; ++v) lut[v] = (uint32_t)v;            // (any table: the lookups are what is checked)
    const size_t elems = (size_t)n * T * 3 * H * W;
    void* out = std::aligned_alloc(16, elems * (fp16 ? 2 : 4));     // exactly the block
    const int gx = emu_letterbox_tiles_run(n, T, ptrs.data(), rows.data(), cols.data(), rects.data(), H, W, mode, fp16, 1, 114, lut, out, 2);
    if (gx < 1) { std::fprintf(stderr, "letterbox run refused: %d\n", gx); std::free(out); return 1; }
    for (size_t e = 0; e < elems; ++e) {
        const uint32_t v = fp16 ? static_cast<uint16_t*>(out)[e] : static_cast<uint32_t*>(out)[e];
        if (v > 255u) { std::fprintf(stderr, "letterbox element %zu is no table entry: %u\n", e, v); std::free(out); return 1; }
        sum += v;
    }
    std::free(out);
    return 0;
}

template <class T>
static void fill(std::vector<T>& pred, int N, int A, int nc, int layout, int pass_percent) {
    for (int s = 0; s < N; ++s)
        for (int a = 0; a < A; ++a) {
            auto at = [&](int c) -> T& { return pred[layout == 0 ? ((size_t)s * (4 + nc) + c) * A + a : ((size_t)s * A + a) * (5 + nc) + c]; };
            const int obj = (int)(rnd() % 6);       // a few objects: plenty of overlap, within and across the tiles
            at(0) = (T)(float)(8 + 9 * obj + (int)(rnd() % 3)); at(1) = (T)(float)(20 + (int)(rnd() % 3));
            at(2) = (T)(float)(8 + (int)(rnd() % 3)); at(3) = (T)(float)(8 + (int)(rnd() % 3));
            const bool active = (int)(rnd() % 100) < pass_percent;
            if (layout == 1) at(4) = (T)1.0f;
            for (int c = 0; c < nc; ++c) at((layout == 0 ? 4 : 5) + c) = (T)((active ? 8 + (int)(rnd() % 25) : (int)(rnd() % 4)) / 32.0f);
        }
}

static int run_detpost(char** a, int& k, int run, double& sum) {
    const int S = std::atoi(a[k]), T = std::atoi(a[k + 1]), A = std::atoi(a[k + 2]), nc = std::atoi(a[k + 3]), layout = std::atoi(a[k + 4]),
              fp16 = std::atoi(a[k + 5]), K = std::atoi(a[k + 6]), max_det = std::atoi(a[k + 7]), merge = std::atoi(a[k + 8]), pct = std::atoi(a[k + 9]);
    k += 10;
    const size_t n = (size_t)S * T * A * ((layout == 0 ? 4 : 5) + nc);
    std::vector<_Float16> ph(fp16 ? n : 0);
    std::vector<float> pf(fp16 ? 0 : n);
    if (fp16) fill(ph, S * T, A, nc, layout, pct); else fill(pf, S * T, A, nc, layout, pct);
    std::vector<float> geom((size_t)S * T * 7);
    for (int q = 0; q < S * T; ++q) {
        float* g = &geom[7 * (size_t)q];
        g[0] = q % T ? 0.5f : 1.0f / 3.0f; g[1] = q % T ? 0.f : 10.f; g[2] = 0.f; g[3] = 32.f * (q % T); g[4] = 0.f; g[5] = 128.f; g[6] = 100.f;
    }
    std::vector<uint8_t> allow(nc, 1);
    if (nc > 1) allow[1] = 0;
    std::vector<float> dets((size_t)S * max_det * 6, -7.0f);
    std::vector<int> rows(S, -1), counters((size_t)S * bm::DP_COUNTERS, -1);
    emu_detpost_tiled_run(S, T, A, nc, layout, fp16, fp16 ? (const void*)ph.data() : (const void*)pf.data(), geom.data(), run % 2 ? allow.data() : nullptr, K,
                          max_det, run % 3 == 0, merge, 0.25f, 0.45f, dets.data(), max_det, rows.data(), counters.data());
    for (int s = 0; s < S; ++s) {
        const int* c = &counters[(size_t)s * bm::DP_COUNTERS];
        if (rows[s] < 0 || rows[s] > max_det || c[0] < 0 || c[0] > T * A || c[1] != (c[0] < K ? c[0] : K) || c[2] > c[1] || rows[s] != (c[2] < max_det ? c[2] : max_det)) {
            std::fprintf(stderr, "run %d stream %d: rows %d counters %d %d %d\n", run, s, rows[s], c[0], c[1], c[2]);
            return 1;
        }
        for (int r = 0; r < max_det; ++r)
            for (int j = 0; j < 6; ++j) {
                const float v = dets[((size_t)s * max_det + r) * 6 + j];
                if (r >= rows[s] && v != -7.0f) { std::fprintf(stderr, "run %d stream %d: row %d beyond the count was written\n", run, s, r); return 1; }
                if (r < rows[s]) sum += v;
            }
    }
    return 0;
}

int main(int argc, char** argv) {
    double sum = 0.0;
    int runs = 0;
    for (int k = 1; k < argc;) {
        const char what = argv[k][0];
        ++k;
        int rc = 2;
        if (what == 'L' && k + 6 <= argc) {
            const int n = std::atoi(argv[k]), T = std::atoi(argv[k + 1]);
            if (n >= 1 && T >= 1 && k + 6 + 2 * n + 4 * n * T <= argc) rc = run_letterbox(argv, k, sum);
        } else if (what == 'D' && k + 10 <= argc) {
            rc = run_detpost(argv, k, runs, sum);
        }
        if (rc == 2) std::fprintf(stderr, "usage: L n T H W mode fp16 {rows cols} {x0 y0 w h} | D S T A nc layout fp16 K max_det merge pass_percent\n");
        if (rc) return rc;
        ++runs;
    }
    std::printf("tiles_asan_main: %d runs, checksum %.3f\n", runs, sum);
    return runs ? 0 : 2;
}
