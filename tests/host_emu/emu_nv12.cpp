// TEST-ONLY harness: runs the ingest ring's NV12 -> BGR kernel (boxmot_amd/csrc/ingest_nv12.hpp, the device source unchanged) on CPU
// threads, with the grid the library launches (bm::nv12_grid_x tiles x n streams, NV12_THREADS threads).  The kernel has no barrier
// and no cross-lane operation, so the emulated threads of a workgroup run one after the other; the workgroups are spread over a few
// OS threads.
#include "hip_shim.hpp"

#include <vector>

#define BM_GLOBAL
#include "../../boxmot_amd/csrc/ingest_nv12.hpp"

thread_local EmuDim3 threadIdx;
thread_local EmuDim3 blockIdx;
EmuDim3 blockDim;
EmuDim3 gridDim;
EmuBlock* g_emu_block = nullptr;
unsigned char* g_emu_dynamic_lds = nullptr;

namespace {
struct Job { const bm::Nv12Desc* descs; int gx, gy, first, step; };
void* worker(void* p) {
    const Job* j = static_cast<const Job*>(p);
    for (int b = j->first; b < j->gx * j->gy; b += j->step) {
        blockIdx.x = b % j->gx; blockIdx.y = b / j->gx;
        for (int t = 0; t < bm::NV12_THREADS; ++t) {
            threadIdx.x = t;
            bm::k_nv12_to_bgr(j->descs);
        }
    }
    return nullptr;
}
}  // namespace

// n streams in one launch: per stream the Y and UV planes, their pitches, the picture size and the (rows, cols, 3) destination.
// Returns grid.x; out_wide[s] = 1 where the stream takes the 2 x 8 path.
extern "C" int emu_nv12_run(int n, const uint8_t* const* y, const uint8_t* const* uv, const int* pitch_y, const int* pitch_uv, const int* rows,
                            const int* cols, uint8_t* const* dst, int* out_wide, int os_threads) {
    std::vector<bm::Nv12Desc> d(n);
    for (int s = 0; s < n; ++s) {
        d[s] = bm::Nv12Desc{y[s], uv[s], pitch_y[s], pitch_uv[s], rows[s], cols[s], dst[s]};
        if (out_wide) out_wide[s] = bm::nv12_wide(d[s]) ? 1 : 0;
    }
    const int gx = bm::nv12_grid_x(d.data(), n);
    blockDim.x = bm::NV12_THREADS; gridDim.x = gx; gridDim.y = n;
    if (os_threads < 1) os_threads = 1;
    std::vector<Job> jobs(os_threads);
    std::vector<pthread_t> th(os_threads);
    for (int k = 0; k < os_threads; ++k) {
        jobs[k] = Job{d.data(), gx, n, k, os_threads};
        pthread_create(&th[k], nullptr, worker, &jobs[k]);
    }
    for (int k = 0; k < os_threads; ++k) pthread_join(th[k], nullptr);
    return gx;
}
