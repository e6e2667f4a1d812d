// TEST-ONLY stand-alone program: the oriented ReID front end on CPU threads (emu_obb_reid.cpp, i.e. crop_list.hpp, obb_crop_geometry.hpp
// and the oriented (hi, lo) crop kernels of reid_hp.hpp unchanged) under -fsanitize=address,undefined.  Every buffer is a heap block of
// exactly the size the library would allocate -- frames of rows x cols x 3 bytes, geometry / crop tables of S x max_dets entries, planes
// of n crops -- so an access past a frame, a table or a plane is reported.  The boxes hang over every frame edge, a few have
// non-finite fields, one stream is empty and one has count -1.  Exit status 0 and a checksum line when every run kept its promises.
#include "emu_obb_reid.cpp"

#include <cstdio>
#include <limits>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }
static float unit() { return (float)(rnd() % 65536) / 65536.0f; }

int main() {
    const int S = 3, ND = 12;
    const int rows[S] = {96, 160, 120}, cols[S] = {128, 200, 96};
    std::vector<std::vector<uint8_t>> frames(S);
    std::vector<const uint8_t*> fptr(S);
    std::vector<int> dims(2 * S);
    for (int s = 0; s < S; ++s) {
        frames[s].resize((size_t)rows[s] * cols[s] * 3);
        for (auto& v : frames[s]) v = (uint8_t)(rnd() & 255);
        fptr[s] = frames[s].data();
        dims[2 * s] = cols[s]; dims[2 * s + 1] = rows[s];
    }
    std::vector<float> dets((size_t)S * ND * 7);
    for (int s = 0; s < S; ++s)
        for (int j = 0; j < ND; ++j) {
            float* d = &dets[((size_t)s * ND + j) * 7];
            d[0] = -30.f + unit() * (cols[s] + 60.f); d[1] = -30.f + unit() * (rows[s] + 60.f);
            d[2] = 0.3f + unit() * 2.f * cols[s]; d[3] = 0.3f + unit() * 2.f * rows[s];
            d[4] = (unit() * 2.f - 1.f) * 3.2f; d[5] = unit(); d[6] = 0.f;
            const int kind = (int)(rnd() % 12);
            if (kind == 0) d[rnd() % 5] = std::numeric_limits<float>::quiet_NaN();
            if (kind == 1) d[rnd() % 5] = std::numeric_limits<float>::infinity();
        }
    const int counts_a[S] = {ND, 0, ND - 5}, counts_b[S] = {-1, ND, 3};
    double sum = 0.0;
    for (int run = 0; run < 2; ++run) {
        const int* counts = run % 2 ? counts_b : counts_a;
        const int inclusive = run;
        std::vector<int> n_dets(counts, counts + S), crop_stream((size_t)S * ND, -7), crop_row((size_t)S * ND, -7), count(1, -5);
        std::vector<double> geo((size_t)S * ND * 8, -77.0);
        emu_build_crop_list_obb(dets.data(), n_dets.data(), S, ND, 0.4, inclusive, 0, count.data(), crop_stream.data(), crop_row.data(), geo.data());
        const int n = count[0];
        int expect = 0;
        for (int s = 0; s < S; ++s)
            for (int j = 0; j < counts[s]; ++j) {
                const double cf = (double)dets[((size_t)s * ND + j) * 7 + 5];
                expect += inclusive ? cf >= 0.4 : cf > 0.4;
            }
        if (n != expect || n < 1) { std::fprintf(stderr, "run %d: count %d, expected %d\n", run, n, expect); return 1; }
        for (int k = 0; k < n; ++k)
            if (crop_stream[k] < 0 || crop_stream[k] >= S || crop_row[k] / ND != crop_stream[k] || !(geo[(size_t)k * 8] >= 1.0)) {
                std::fprintf(stderr, "run %d: entry %d is (%d, %d, out_w %g)\n", run, k, crop_stream[k], crop_row[k], geo[(size_t)k * 8]);
                return 1;
            }
        // planes of exactly n crops; the kernels are launched for n with a count of n - 1: the last crop's planes stay untouched
        const size_t plane = (size_t)262 * 136 * 4;
        std::vector<uint16_t> hi((size_t)n * plane, 0x4700), lo((size_t)n * plane, 0x4700);
        for (int pad = 0; pad < 2; ++pad) {
            emu_crop_resize_obb_hl(fptr.data(), crop_stream.data(), geo.data(), n, 0, 0, dims.data(), n - 1, pad, hi.data(), lo.data());
            for (size_t e = (size_t)(n - 1) * plane; e < (size_t)n * plane; ++e)
                if (hi[e] != 0x4700 || lo[e] != 0x4700) { std::fprintf(stderr, "run %d: a crop beyond the count was written\n", run); return 1; }
            for (size_t e = 0; e < (size_t)(n - 1) * plane; ++e) sum += (hi[e] & 0x7c00) == 0x7c00 ? 1e9 : (double)(hi[e] & 255);
        }
        // the scalar form on the crops of stream 0's frame size only (all addressed to frame 0)
        std::vector<int> zero(n, 0);
        emu_crop_resize_obb_hl(fptr.data(), zero.data(), geo.data(), n, cols[0], rows[0], nullptr, -1, 0, hi.data(), lo.data());
    }
    if (!(sum < 1e9)) { std::fprintf(stderr, "a non-finite value in the planes\n"); return 1; }
    std::printf("obb_reid_asan_main: 2 runs, checksum %.1f\n", sum);
    return 0;
}
