// TEST-ONLY stand-alone program: the detection post-processing of a mask handle on CPU threads (emu_detpost_mask.cpp, i.e.
// det_post.hpp, det_post_tiled.hpp, det_post_extra.hpp and det_post_mask.hpp unchanged) under -fsanitize=address,undefined.  Every
// buffer is a heap block of exactly the size the library would be given, so an access past the tensor, the prototypes, the scratch,
// one of the five output blocks or the dynamic LDS is reported.  Arguments: groups of 15 integers
//     S T A nc layout fp16 K max_det E proto_fp16 mask_h mask_w in_h in_w pass_percent                (T = 0: untiled)
// (tests/test_detpost_mask_emu.py passes the shapes of detpost_mask_ref.CASES); the data is pseudo-random with quantised scores and
// boxes that reach beyond the input on every side; every other run passes no src block, every third one prototypes and masks that
// start one element / one byte into their blocks (the byte path).  Exit status 0 and a checksum line when every run kept its promises.
#include "emu_detpost_mask.cpp"

#include <cstdio>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

template <class T>
static void fill(std::vector<T>& pred, int N, int A, int nc, int E, int layout, int pass_percent, int in_h, int in_w) {
    for (int s = 0; s < N; ++s)
        for (int a = 0; a < A; ++a) {
            auto at = [&](int c) -> T& { return pred[layout == 0 ? ((size_t)s * (4 + nc + E) + c) * A + a : ((size_t)s * A + a) * (5 + nc + E) + c]; };
            at(0) = (T)(float)((int)(rnd() % (unsigned)(in_w + 40)) - 20); at(1) = (T)(float)((int)(rnd() % (unsigned)(in_h + 40)) - 20);
            at(2) = (T)(float)(1 + (int)(rnd() % (unsigned)in_w)); at(3) = (T)(float)(1 + (int)(rnd() % (unsigned)in_h));
            const bool active = (int)(rnd() % 100) < pass_percent;
            if (layout == 1) at(4) = (T)1.0f;
            const int first = layout == 0 ? 4 : 5;
            for (int c = 0; c < nc; ++c) at(first + c) = (T)((active ? 8 + (int)(rnd() % 25) : (int)(rnd() % 4)) / 32.0f);
            for (int e = 0; e < E; ++e) at(first + nc + e) = (T)(float)((int)(rnd() % 33) / 4.0f - 4.0f);
        }
}
template <class P>
static void fill_proto(std::vector<P>& p) { for (auto& v : p) v = (P)(float)((int)(rnd() % 33) / 8.0f - 2.0f); }

int main(int argc, char** argv) {
    if (argc < 16 || (argc - 1) % 15) { std::fprintf(stderr, "usage: groups of S T A nc layout fp16 K max_det E proto_fp16 mask_h mask_w in_h in_w pass_percent\n"); return 2; }
    long sum = 0;
    for (int k = 1, run = 0; k + 14 < argc; k += 15, ++run) {
        int v[15];
        for (int q = 0; q < 15; ++q) v[q] = std::atoi(argv[k + q]);
        const int S = v[0], T = v[1], A = v[2], nc = v[3], layout = v[4], fp16 = v[5], K = v[6], max_det = v[7], E = v[8], pfp16 = v[9], mh = v[10], mw = v[11],
                  in_h = v[12], in_w = v[13], pct = v[14];
        const int NT = T ? T : 1;
        const size_t n = (size_t)S * NT * A * ((layout == 0 ? 4 : 5) + nc + E);
        std::vector<_Float16> ph(fp16 ? n : 0);
        std::vector<float> pf(fp16 ? 0 : n);
        if (fp16) fill(ph, S * NT, A, nc, E, layout, pct, in_h, in_w); else fill(pf, S * NT, A, nc, E, layout, pct, in_h, in_w);
        const bool shifted = run % 3 == 2;              // the blocks start one element / one byte in: no wide path
        const size_t plane = (size_t)mh * mw, np = (size_t)S * NT * E * plane + (shifted ? 1 : 0);
        std::vector<_Float16> qh(pfp16 ? np : 0);
        std::vector<float> qf(pfp16 ? 0 : np);
        if (pfp16) fill_proto(qh); else fill_proto(qf);
        const void* proto = pfp16 ? (const void*)(qh.data() + (shifted ? 1 : 0)) : (const void*)(qf.data() + (shifted ? 1 : 0));
        std::vector<float> geom((size_t)S * NT * (T ? 7 : 5));
        for (int q = 0; q < S * NT; ++q) {
            float* g = &geom[(size_t)q * (T ? 7 : 5)];
            if (T) { g[0] = q % T ? 0.5f : 1.0f / 3.0f; g[1] = q % T ? 0.f : 10.f; g[2] = 0.f; g[3] = 32.f * (q % T); g[4] = 0.f; g[5] = 128.f; g[6] = 100.f; }
            else { g[0] = 1.0f / 3.0f; g[1] = 10.f; g[2] = 0.f; g[3] = 100.f; g[4] = 192.f; }
        }
        std::vector<float> dets((size_t)S * max_det * 6, -7.0f), extra((size_t)S * max_det * E, -7.0f);
        std::vector<int> rows(S, -1), counters((size_t)S * bm::DP_COUNTERS, -1), src((size_t)S * max_det, -7);
        std::vector<uint8_t> masks((size_t)S * max_det * plane + (shifted ? 1 : 0), 0xA5);
        const bool with_src = run % 2 == 0;
        emu_detpost_mask_run(S, T, A, nc, layout, fp16, fp16 ? (const void*)ph.data() : (const void*)pf.data(), geom.data(), nullptr, K, max_det, run % 3 == 0,
                             run % 2, 0.25f, 0.45f, dets.data(), max_det, rows.data(), counters.data(), E, extra.data(), with_src ? src.data() : nullptr, proto,
                             pfp16, masks.data() + (shifted ? 1 : 0), mh, mw, in_h, in_w);
        if (shifted && masks[0] != 0xA5) { std::fprintf(stderr, "run %d: the byte before the masks was written\n", run); return 1; }
        for (int s = 0; s < S; ++s) {
            if (rows[s] < 0 || rows[s] > max_det) { std::fprintf(stderr, "run %d stream %d: rows %d\n", run, s, rows[s]); return 1; }
            for (int r = 0; r < max_det; ++r) {
                const uint8_t* m = masks.data() + (shifted ? 1 : 0) + ((size_t)s * max_det + r) * plane;
                for (size_t q = 0; q < plane; ++q) {
                    if (r < rows[s] ? m[q] > 1 : m[q] != 0xA5) {
                        std::fprintf(stderr, "run %d stream %d row %d: mask byte %zu holds %d\n", run, s, r, q, (int)m[q]);
                        return 1;
                    }
                    if (r < rows[s]) sum += m[q];
                }
            }
        }
    }
    std::printf("detpost_mask_asan_main: %d runs, checksum %ld\n", (argc - 1) / 15, sum);
    return 0;
}
