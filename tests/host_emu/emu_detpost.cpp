// TEST-ONLY harness: runs the detection post-processing kernels (boxmot_amd/csrc/det_post.hpp, the device source unchanged, including
// its kernel sequence detpost_launch) on CPU threads with the grids the library launches.  k_detpost_select has workgroup barriers,
// ballots and LDS atomics, so every workgroup runs on the barrier-capable emulation of hip_shim.hpp (fibers; pthreads under the
// sanitizers).  The scratch and the dynamic LDS are filled with a poison byte before every call: a kernel that relied on what an
// earlier call left there would come out different.
#include "hip_shim.hpp"

#include <cstdlib>
#include <functional>
#include <vector>

#include "../../boxmot_amd/csrc/det_post.hpp"

thread_local EmuDim3 threadIdx;
thread_local EmuDim3 blockIdx;
EmuDim3 blockDim;
EmuDim3 gridDim;
EmuBlock* g_emu_block = nullptr;
unsigned char* g_emu_dynamic_lds = nullptr;

namespace {
struct TA { const std::function<void()>* fn; int tid, bx, by; };
void* tmain(void* p) {
    TA* a = static_cast<TA*>(p);
    threadIdx.x = a->tid; blockIdx.x = a->bx; blockIdx.y = a->by;
    (*a->fn)();
    return nullptr;
}
struct Launcher {
    template <class K, class... A>
    void operator()(K kernel, int gx, int gy, int nthr, size_t lds_bytes, A... args) {
        const std::function<void()> fn = [=]() { kernel(args...); };
        static EmuBlock block;
        g_emu_block = &block;
        blockDim.x = nthr; gridDim.x = gx; gridDim.y = gy;
        std::vector<unsigned char> lds(lds_bytes + 16);         // exactly what the launch asks for: a sanitizer sees an overrun
        g_emu_dynamic_lds = lds.data();
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx) {
                block.block_barrier.init(nthr);
                for (int w = 0; w < EMU_MAX_WAVES; ++w) block.wave_barrier[w].init(EMU_WAVE);
                std::memset(lds.data(), 0xCD, lds_bytes);
                std::vector<TA> ta(nthr);
                for (int t = 0; t < nthr; ++t) ta[t] = TA{&fn, t, bx, by};
                emu_run_threads(nthr, tmain, ta.data(), sizeof(ta[0]), 1 << 18);
            }
        g_emu_dynamic_lds = nullptr;
    }
};
}  // namespace

// pred: (S, 4 + nc, A) or (S, A, 5 + nc) of 2- (fp16) or 4-byte elements; geom: [S][5] float32 gain, top, left, rows, cols;
// allow: nc bytes or null; dets: [S][out_stride][6]; det_rows: [S]; counters: [S][3].  Returns the LDS bytes of the launch.
extern "C" long emu_detpost_run(int n_streams, int A, int nc, int layout, int fp16, const void* pred, const float* geom, const uint8_t* allow,
                                int K, int max_det, int agnostic, float conf_thres, float iou_thres, float* dets, int out_stride, int* det_rows,
                                int* counters) {
    std::vector<uint32_t> keys((size_t)n_streams * A, 0xCDCDCDCDu);
    std::vector<int> cls((size_t)n_streams * A, (int)0xCDCDCDCD);
    bm::DetPostArgs g{pred, reinterpret_cast<const bm::DetPostGeom*>(geom), allow, keys.data(), cls.data(), dets, det_rows, counters,
                      A, nc, layout, K, max_det, agnostic, out_stride, conf_thres, iou_thres};
    Launcher L;
    size_t lds = 0;
    bm::detpost_launch(L, g, n_streams, fp16, &lds);
    return (long)lds;
}
