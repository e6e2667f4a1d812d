// TEST-ONLY stand-alone program: the label-map kernel on CPU threads (emu_detpost_labels.cpp, i.e. det_post_labels.hpp unchanged)
// under -fsanitize=address,undefined.  The prototypes, the rows, the coefficients and the label block are heap blocks of exactly
// their size -- the label planes are exactly the frame -- so a tap past a plane, a read past the rows or a store past a frame is
// reported.  Arguments: groups of 12 integers
//     S E proto_fp16 mask_h mask_w in_h in_w rows cols centre n_rows max_det
// (tests/test_detpost_labels_emu.py passes the shapes of detpost_labels_ref.CASES); the data is pseudo-random, the boxes reach beyond
// the frame on every side, every third run's prototypes and labels start one element into their blocks.  Every run is made twice,
// on the path the kernel chooses and with the fallback forced, and the two label blocks must be equal.  Exit status 0 and a
// checksum line when every run kept its promises.
#include "emu_detpost_labels.cpp"

#include <cstdio>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

template <class P>
static void fill_proto(std::vector<P>& p) { for (auto& v : p) v = (P)(float)((int)(rnd() % 33) / 8.0f - 2.0f); }

int main(int argc, char** argv) {
    if (argc < 13 || (argc - 1) % 12) { std::fprintf(stderr, "usage: groups of S E proto_fp16 mask_h mask_w in_h in_w rows cols centre n_rows max_det\n"); return 2; }
    long sum = 0;
    for (int k = 1, run = 0; k + 11 < argc; k += 12, ++run) {
        int v[12];
        for (int q = 0; q < 12; ++q) v[q] = std::atoi(argv[k + q]);
        const int S = v[0], E = v[1], pfp16 = v[2], mh = v[3], mw = v[4], in_h = v[5], in_w = v[6], rows = v[7], cols = v[8], centre = v[9], n_rows = v[10],
                  max_det = v[11];
        const bool shifted = run % 3 == 2;
        const int off = shifted ? 1 : 0;
        const size_t plane = (size_t)mh * mw, np = (size_t)S * E * plane + off;
        std::vector<_Float16> qh(pfp16 ? np : 0);
        std::vector<float> qf(pfp16 ? 0 : np);
        if (pfp16) fill_proto(qh); else fill_proto(qf);
        const void* proto = pfp16 ? (const void*)(qh.data() + off) : (const void*)(qf.data() + off);
        const float gain = std::fmin((float)in_h / rows, (float)in_w / cols);
        std::vector<float> geom((size_t)S * 5);
        for (int s = 0; s < S; ++s) {
            float* g = &geom[(size_t)s * 5];
            g[0] = gain; g[1] = centre ? std::floor((in_h - rows * gain) / 2) : 0.f; g[2] = centre ? std::floor((in_w - cols * gain) / 2) : 0.f;
            g[3] = (float)rows; g[4] = (float)cols;
        }
        std::vector<float> dets((size_t)S * max_det * 6), extra((size_t)S * max_det * E);
        for (size_t r = 0; r < (size_t)S * max_det; ++r) {
            float* d = &dets[r * 6];
            d[0] = (float)((int)(rnd() % (unsigned)(cols + 8)) - 8); d[1] = (float)((int)(rnd() % (unsigned)(rows + 8)) - 8);
            d[2] = d[0] + (float)(rnd() % (unsigned)(cols + 8)); d[3] = d[1] + (float)(rnd() % (unsigned)(rows + 8));
            d[4] = 0.5f; d[5] = 0.f;
        }
        for (auto& e : extra) e = (float)((int)(rnd() % 33) / 4.0f - 4.0f);
        std::vector<int> det_rows(S, n_rows);
        if (S > 1) det_rows[1] = n_rows + 3;            // (beyond max_det where n_rows == max_det: the kernel clamps)
        std::vector<int16_t> labels[2];
        for (int fallback = 0; fallback < 2; ++fallback) {
            labels[fallback].assign((size_t)S * rows * cols + off, (int16_t)-21931);
            emu_detpost_labels_run(S, geom.data(), proto, pfp16, dets.data(), max_det, det_rows.data(), extra.data(), labels[fallback].data() + off, rows, cols,
                                   max_det, E, mh, mw, in_h, in_w, fallback);
        }
        if (labels[0] != labels[1]) { std::fprintf(stderr, "run %d: the LDS path and the fallback path differ\n", run); return 1; }
        if (shifted && labels[0][0] != -21931) { std::fprintf(stderr, "run %d: the element before the labels was written\n", run); return 1; }
        for (int s = 0; s < S; ++s) {
            const int n = det_rows[s] < max_det ? det_rows[s] : max_det;
            for (size_t q = 0; q < (size_t)rows * cols; ++q) {
                const int l = labels[0][off + (size_t)s * rows * cols + q];
                if (l < -1 || l >= n) { std::fprintf(stderr, "run %d stream %d: pixel %zu holds %d of %d rows\n", run, s, q, l, n); return 1; }
                sum += l;
            }
        }
    }
    std::printf("detpost_labels_asan_main: %d runs, checksum %ld\n", (argc - 1) / 12, sum);
    return 0;
}
