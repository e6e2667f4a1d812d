// Development tool: time of the ingest ring's NV12 -> BGR kernel (boxmot_amd/csrc/ingest_nv12.hpp) for S frames of rows x cols,
// taken with HIP events, beside plain device-to-device hipMemcpyAsync calls that move comparable bytes.  The kernel reads 1.5 and
// writes 3 bytes per pixel: 4.5 bytes of traffic.  A copy of N bytes reads N and writes N, so two copies are timed: one of 2.25
// bytes per pixel (the same 4.5 bytes of traffic) and one of 4.5 bytes per pixel.
//
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -o nv12_kernel_bench tools/nv12_kernel_bench.hip
//     ./nv12_kernel_bench [streams = 16] [rows = 1080] [cols = 1920] [repeats = 50]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../boxmot_amd/csrc/ingest_nv12.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    const int S = argc > 1 ? std::atoi(argv[1]) : 16, rows = argc > 2 ? std::atoi(argv[2]) : 1080, cols = argc > 3 ? std::atoi(argv[3]) : 1920;
    const int reps = argc > 4 ? std::atoi(argv[4]) : 50;
    if (S < 1 || rows < 2 || cols < 2 || rows % 2 || cols % 2 || reps < 1) { std::fprintf(stderr, "streams >= 1, even rows and cols, repeats >= 1\n"); return 1; }
    const size_t px = (size_t)rows * cols, nv_bytes = (px * 3 / 2 + 255) / 256 * 256, bgr_bytes = (px * 3 + 255) / 256 * 256;
    uint8_t *d_nv = nullptr, *d_bgr = nullptr, *d_copy = nullptr;
    bm::Nv12Desc* d_desc = nullptr;
    CHECK(hipMalloc(&d_nv, nv_bytes * S));
    CHECK(hipMalloc(&d_bgr, bgr_bytes * S));
    CHECK(hipMalloc(&d_copy, px * S * 9));
    CHECK(hipMalloc(&d_desc, sizeof(bm::Nv12Desc) * S));
    CHECK(hipMemset(d_nv, 0x80, nv_bytes * S));
    CHECK(hipMemset(d_copy, 0, px * S * 9));
    std::vector<bm::Nv12Desc> desc(S);
    for (int s = 0; s < S; ++s) desc[s] = bm::Nv12Desc{d_nv + nv_bytes * s, d_nv + nv_bytes * s + px, cols, cols, rows, cols, d_bgr + bgr_bytes * s};
    CHECK(hipMemcpy(d_desc, desc.data(), sizeof(bm::Nv12Desc) * S, hipMemcpyHostToDevice));
    hipStream_t st;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    const dim3 grid((unsigned)bm::nv12_grid_x(desc.data(), S), (unsigned)S);
    float ms = 0;
    auto launch = [&]() { hipLaunchKernelGGL(bm::k_nv12_to_bgr, grid, dim3(bm::NV12_THREADS), 0, st, (const bm::Nv12Desc*)d_desc); };
    for (int k = 0; k < 5; ++k) launch();
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(a, st));
    for (int k = 0; k < reps; ++k) launch();
    CHECK(hipEventRecord(b, st));
    CHECK(hipEventSynchronize(b));
    CHECK(hipEventElapsedTime(&ms, a, b));
    const double us_kernel = 1e3 * ms / reps, traffic = 4.5 * px * S;
    std::printf("k_nv12_to_bgr  %d x %d x %d (%s path, grid %u x %u): %.1f us per launch, %.0f GB/s of the 4.5 B/pixel it moves\n", S, rows, cols,
                bm::nv12_wide(desc[0]) ? "wide" : "narrow", grid.x, grid.y, us_kernel, traffic / us_kernel * 1e-3);
    for (int pass = 0; pass < 2; ++pass) {
        const size_t n = pass == 0 ? px * S * 9 / 4 : px * S * 9 / 2;       // from the buffer's first half into its second
        for (int k = 0; k < 5; ++k) CHECK(hipMemcpyAsync(d_copy + px * S * 9 / 2, d_copy, n, hipMemcpyDeviceToDevice, st));
        CHECK(hipEventRecord(a, st));
        for (int k = 0; k < reps; ++k) CHECK(hipMemcpyAsync(d_copy + px * S * 9 / 2, d_copy, n, hipMemcpyDeviceToDevice, st));
        CHECK(hipEventRecord(b, st));
        CHECK(hipEventSynchronize(b));
        CHECK(hipEventElapsedTime(&ms, a, b));
        const double us = 1e3 * ms / reps;
        std::printf("hipMemcpyAsync device-to-device of %.2f B/pixel (%.1f MB, %.1f MB of traffic): %.1f us per copy, %.0f GB/s of traffic\n",
                    (double)n / (px * S), n * 1e-6, 2 * n * 1e-6, us, 2.0 * n / us * 1e-3);
    }
    return 0;
}
