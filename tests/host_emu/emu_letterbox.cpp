// TEST-ONLY harness: runs the ingest ring's letterbox kernel (boxmot_amd/csrc/ingest_letterbox.hpp, the device source unchanged) on
// CPU threads, with the grid the library launches (bm::letterbox_grid_x tiles x n streams, LB_THREADS threads) and the geometry the
// library computes (bm::letterbox_geometry).  The kernel has no barrier and no cross-lane operation, so the emulated threads of a
// workgroup run one after the other; the workgroups are spread over a few OS threads.
#include "hip_shim.hpp"

#include <vector>

#define BM_GLOBAL
#include "../../boxmot_amd/csrc/ingest_letterbox.hpp"

thread_local EmuDim3 threadIdx;
thread_local EmuDim3 blockIdx;
EmuDim3 blockDim;
EmuDim3 gridDim;
EmuBlock* g_emu_block = nullptr;
unsigned char* g_emu_dynamic_lds = nullptr;

namespace {
struct Job {
    const uint8_t* const* frames; const bm::LetterboxGeom* geom; const uint32_t* lut; void* out;
    int H, W, fp16, rgb, pad, gx, gy, first, step;
};
void* worker(void* p) {
    const Job* j = static_cast<const Job*>(p);
    for (int b = j->first; b < j->gx * j->gy; b += j->step) {
        blockIdx.x = b % j->gx; blockIdx.y = b / j->gx;
        for (int t = 0; t < bm::LB_THREADS; ++t) {
            threadIdx.x = t;
            bm::k_letterbox(j->frames, j->geom, j->lut, j->out, j->H, j->W, j->fp16, j->rgb, j->pad);
        }
    }
    return nullptr;
}
}  // namespace

// the library's geometry of one frame size: out5 = gain, new_w, new_h, top, left; returns 0 where the picture would vanish
extern "C" int emu_letterbox_geometry(int rows, int cols, int H, int W, int mode, double* out5) {
    bm::LetterboxGeom g;
    const bool ok = bm::letterbox_geometry(rows, cols, H, W, mode, &out5[0], &g);
    out5[1] = g.new_w; out5[2] = g.new_h; out5[3] = g.top; out5[4] = g.left;
    return ok ? 1 : 0;
}

// n streams in one launch: per stream the (rows, cols, 3) BGR frame; lut: the 256 table entries as 32-bit words; out: (n, 3, H, W)
// elements of 2 (fp16) or 4 bytes.  Returns grid.x, or -1 - s where stream s is degenerate.
extern "C" int emu_letterbox_run(int n, const uint8_t* const* frames, const int* rows, const int* cols, int H, int W, int mode, int fp16,
                                 int rgb, int pad, const uint32_t* lut, void* out, int os_threads) {
    std::vector<bm::LetterboxGeom> g(n);
    for (int s = 0; s < n; ++s)
        if (!bm::letterbox_geometry(rows[s], cols[s], H, W, mode, nullptr, &g[s])) return -1 - s;
    const int gx = bm::letterbox_grid_x(H, W);
    blockDim.x = bm::LB_THREADS; gridDim.x = gx; gridDim.y = n;
    if (os_threads < 1) os_threads = 1;
    std::vector<Job> jobs(os_threads);
    std::vector<pthread_t> th(os_threads);
    for (int k = 0; k < os_threads; ++k) {
        jobs[k] = Job{frames, g.data(), lut, out, H, W, fp16, rgb, pad, gx, n, k, os_threads};
        pthread_create(&th[k], nullptr, worker, &jobs[k]);
    }
    for (int k = 0; k < os_threads; ++k) pthread_join(th[k], nullptr);
    return gx;
}
