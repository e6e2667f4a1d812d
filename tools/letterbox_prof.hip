// Development tool behind tools/letterbox_prof.py: time of the ingest ring's letterbox kernel (boxmot_amd/csrc/ingest_letterbox.hpp)
// for one slot of S streams of rows x cols frames into (H, W) fp16 / fp32, beside the NV12 -> BGR kernel (ingest_nv12.hpp) that
// fills the same slot -- the comparator: it streams 4.5 bytes per pixel, coalesced.  Every launch has its own pair of HIP events; the
// two kernels alternate, so both see the same state of the machine.  Prints one line per kernel: median, min and max in
// microseconds and the effective bandwidth at the median.
//
// The slot holds pseudo-random pictures (a constant picture would turn the table lookups into one address).  The letterbox kernel
// reads the BGR frames the NV12 kernel wrote.  Bytes of the letterbox kernel: the source rows it touches, whole (at most
// min(rows, 2 new_h) rows of cols x 3 bytes per stream) plus the 3 H W elements it writes.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o letterbox_prof tools/letterbox_prof.hip
//     ./letterbox_prof [streams = 64] [rows = 1080] [cols = 1920] [H = 640] [W = 640] [fp16 = 1] [repeats = 30] [mode = 0]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../boxmot_amd/csrc/ingest_letterbox.hpp"
#include "../boxmot_amd/csrc/ingest_nv12.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static void report(const char* name, std::vector<float> ms, double bytes) {
    std::sort(ms.begin(), ms.end());
    const double med = 1e3 * ms[ms.size() / 2], lo = 1e3 * ms.front(), hi = 1e3 * ms.back();
    std::printf("%-14s median %.1f us  min %.1f  max %.1f  (%zu launches)  %.1f MB  %.0f GB/s at the median\n", name, med, lo, hi, ms.size(),
                bytes * 1e-6, bytes / med * 1e-3);
}

int main(int argc, char** argv) {
    auto arg = [&](int k, int d) { return argc > k ? std::atoi(argv[k]) : d; };
    const int S = arg(1, 64), rows = arg(2, 1080), cols = arg(3, 1920), H = arg(4, 640), W = arg(5, 640), fp16 = arg(6, 1), reps = arg(7, 30),
              mode = arg(8, 0);
    bm::LetterboxGeom g;
    if (S < 1 || rows < 2 || cols < 2 || rows % 2 || cols % 2 || reps < 20 || H < 1 || W < 8 || W % 8 || (mode != 0 && mode != 1) ||
        !bm::letterbox_geometry(rows, cols, H, W, mode, nullptr, &g)) {
        std::fprintf(stderr, "streams >= 1, even rows and cols, W a multiple of 8, repeats >= 20, mode 0 or 1\n");
        return 1;
    }
    const size_t px = (size_t)rows * cols, nv_bytes = (px * 3 / 2 + 255) / 256 * 256, bgr_bytes = (px * 3 + 255) / 256 * 256;
    const size_t elt = fp16 ? 2 : 4, out_bytes = (size_t)S * 3 * H * W * elt;
    uint8_t *d_nv = nullptr, *d_bgr = nullptr;
    void* d_out = nullptr;
    bm::Nv12Desc* d_desc = nullptr;
    bm::LetterboxGeom* d_geom = nullptr;
    const uint8_t** d_frames = nullptr;
    uint32_t* d_lut = nullptr;
    CHECK(hipMalloc(&d_nv, nv_bytes * S));
    CHECK(hipMalloc(&d_bgr, bgr_bytes * S));
    CHECK(hipMalloc(&d_out, out_bytes));
    CHECK(hipMalloc(&d_desc, sizeof(bm::Nv12Desc) * S));
    CHECK(hipMalloc(&d_geom, sizeof(bm::LetterboxGeom) * S));
    CHECK(hipMalloc(&d_frames, sizeof(uint8_t*) * S));
    CHECK(hipMalloc(&d_lut, 256 * sizeof(uint32_t)));
    {
        std::vector<uint8_t> nv(nv_bytes);
        uint32_t x = 12345u;
        for (auto& b : nv) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
        for (int s = 0; s < S; ++s) CHECK(hipMemcpy(d_nv + nv_bytes * s, nv.data(), nv_bytes, hipMemcpyHostToDevice));
    }
    std::vector<bm::Nv12Desc> desc(S);
    std::vector<bm::LetterboxGeom> geom(S, g);
    std::vector<const uint8_t*> frames(S);
    for (int s = 0; s < S; ++s) {
        desc[s] = bm::Nv12Desc{d_nv + nv_bytes * s, d_nv + nv_bytes * s + px, cols, cols, rows, cols, d_bgr + bgr_bytes * s};
        frames[s] = d_bgr + bgr_bytes * s;
    }
    uint32_t lut[256];
    for (int v = 0; v < 256; ++v) {         // the shape of the table is what matters here, not its values: fp32 bits of v / 255, or v
        const float f = (float)v / 255.0f;
        if (fp16) lut[v] = (uint32_t)v; else std::memcpy(&lut[v], &f, 4);
    }
    CHECK(hipMemcpy(d_desc, desc.data(), sizeof(bm::Nv12Desc) * S, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_geom, geom.data(), sizeof(bm::LetterboxGeom) * S, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_frames, frames.data(), sizeof(uint8_t*) * S, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
    hipStream_t st;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const dim3 grid_nv((unsigned)bm::nv12_grid_x(desc.data(), S), (unsigned)S), grid_lb((unsigned)bm::letterbox_grid_x(H, W), (unsigned)S);
    auto nv12 = [&]() { hipLaunchKernelGGL(bm::k_nv12_to_bgr, grid_nv, dim3(bm::NV12_THREADS), 0, st, (const bm::Nv12Desc*)d_desc); };
    auto lb = [&]() {
        hipLaunchKernelGGL(bm::k_letterbox, grid_lb, dim3(bm::LB_THREADS), 0, st, (const uint8_t* const*)d_frames, (const bm::LetterboxGeom*)d_geom,
                           (const uint32_t*)d_lut, d_out, H, W, fp16, 1, 114);
    };
    for (int k = 0; k < 5; ++k) { nv12(); lb(); }
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(st));
    std::vector<hipEvent_t> ev(4 * (size_t)reps);
    for (auto& e : ev) CHECK(hipEventCreate(&e));
    for (int k = 0; k < reps; ++k) {
        CHECK(hipEventRecord(ev[4 * k], st)); nv12(); CHECK(hipEventRecord(ev[4 * k + 1], st));
        CHECK(hipEventRecord(ev[4 * k + 2], st)); lb(); CHECK(hipEventRecord(ev[4 * k + 3], st));
    }
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(st));
    std::vector<float> t_nv(reps), t_lb(reps);
    for (int k = 0; k < reps; ++k) {
        CHECK(hipEventElapsedTime(&t_nv[k], ev[4 * k], ev[4 * k + 1]));
        CHECK(hipEventElapsedTime(&t_lb[k], ev[4 * k + 2], ev[4 * k + 3]));
    }
    const int src_rows = std::min(rows, 2 * g.new_h);
    const double lb_src = (double)S * src_rows * cols * 3, lb_dst = (double)out_bytes;
    std::printf("%d streams of %d x %d -> (%d, %d) %s, mode %d: picture %d x %d at (%d, %d); letterbox grid %u x %u, nv12 grid %u x %u\n", S, rows, cols, H, W,
                fp16 ? "fp16" : "fp32", mode, g.new_h, g.new_w, g.top, g.left, grid_lb.x, grid_lb.y, grid_nv.x, grid_nv.y);
    report("k_nv12_to_bgr", t_nv, 4.5 * px * S);
    report("k_letterbox", t_lb, lb_src + lb_dst);
    std::printf("k_letterbox bytes: %.1f MB of source rows touched (%d of %d rows per stream) + %.1f MB written\n", lb_src * 1e-6, src_rows, rows, lb_dst * 1e-6);
    return 0;
}
