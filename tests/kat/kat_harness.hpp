// TEST-ONLY plumbing shared by the known-answer harnesses (gemm_kat.hip, clip_kat.hip, reid_hp_kat.hip, wide_kat.hip, wide_hp_kat.hip): the device build's launch / copy helpers and, with
// -DKAT_EMU, their CPU-thread twins over tests/host_emu/hip_shim.hpp (one workgroup after the other, LDS poisoned before each).  Include it
// FIRST and once per harness: it defines the emulation's globals, so every harness is a single translation unit.
//   KAT_LAUNCH(kernel, grid, block, dynamic LDS bytes, args...)    KAT_SET_LDS(kernel, bytes): hipFuncSetAttribute once per instantiation
//   KAT_LAUNCH_XY(kernel, grid x, grid y, block, dynamic LDS bytes, args...): a two-dimensional grid
//   KAT_EMU_STACK (define before including): bytes of stack per emulated thread, 256 KiB unless a harness's kernels need more
//   dev_alloc / dev_free / h2d / d2h / dev_finish: 0, or -2 when a HIP call failed
#pragma once
#ifdef KAT_EMU
#include "../host_emu/hip_shim.hpp"
#else
#include <hip/hip_runtime.h>
#endif

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>


#if defined(KAT_EMU) && !defined(KAT_EMU_STACK)
#define KAT_EMU_STACK (1 << 18)
#endif
#ifdef KAT_EMU
thread_local EmuDim3 threadIdx;
thread_local EmuDim3 blockIdx;
EmuDim3 blockDim;
EmuDim3 gridDim;
EmuBlock* g_emu_block = nullptr;
unsigned char* g_emu_dynamic_lds = nullptr;
EmuMfmaBuf* g_emu_mfma = nullptr;

namespace {
struct TA { const std::function<void()>* fn; int tid, bx, by; };
void* tmain(void* p) {
    TA* a = static_cast<TA*>(p);
    threadIdx.x = a->tid; blockIdx.x = a->bx; blockIdx.y = a->by;
    (*a->fn)();
    return nullptr;
}
// one workgroup after the other; LDS poisoned (0xFF: fp16 NaN) before each
void emu_launch(unsigned grid, int nthr, size_t lds_bytes, const std::function<void()>& fn, unsigned grid_y = 1) {
    static EmuBlock block;
    static EmuMfmaBuf mf;
    static std::vector<unsigned char> lds;
    if (lds.size() < lds_bytes + 64) lds.resize(lds_bytes + 64);
    g_emu_block = &block; g_emu_mfma = &mf;
    g_emu_dynamic_lds = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(lds.data()) + 15) & ~uintptr_t(15));
    blockDim.x = nthr; gridDim.x = grid; gridDim.y = grid_y;
    block.block_barrier.init(nthr);
    for (int w = 0; w < EMU_MAX_WAVES; ++w) block.wave_barrier[w].init(EMU_WAVE);
    for (unsigned by = 0; by < grid_y; ++by)
        for (unsigned bx = 0; bx < grid; ++bx) {
            std::memset(lds.data(), 0xFF, lds.size());
            std::vector<TA> ta(nthr);
            for (int t = 0; t < nthr; ++t) ta[t] = TA{&fn, t, (int)bx, (int)by};
            emu_run_threads(nthr, tmain, ta.data(), sizeof(ta[0]), KAT_EMU_STACK);
        }
}
}  // namespace

#define KAT_LAUNCH(kern, grid, block, lds, ...) emu_launch((unsigned)(grid), (block), (lds), [&]() { kern(__VA_ARGS__); })
#define KAT_LAUNCH_XY(kern, gx, gy, block, lds, ...) emu_launch((unsigned)(gx), (block), (lds), [&]() { kern(__VA_ARGS__); }, (unsigned)(gy))
#define KAT_SET_LDS(kern, bytes) 0
static int dev_alloc(void** p, size_t n) { *p = std::malloc(n ? n : 1); return *p ? 0 : -2; }
static void dev_free(void* p) { std::free(p); }
static int h2d(void* d, const void* h, size_t n) { if (n) std::memcpy(d, h, n); return 0; }
static int d2h(void* h, const void* d, size_t n) { if (n) std::memcpy(h, d, n); return 0; }
static int dev_finish() { return 0; }
#else
#define KAT_LAUNCH(kern, grid, block, lds, ...) hipLaunchKernelGGL(kern, dim3((unsigned)(grid)), dim3(block), (lds), 0, __VA_ARGS__)
#define KAT_LAUNCH_XY(kern, gx, gy, block, lds, ...) hipLaunchKernelGGL(kern, dim3((unsigned)(gx), (unsigned)(gy)), dim3(block), (lds), 0, __VA_ARGS__)
// hipFuncSetAttribute once per instantiation, as the engines' constructors do
#define KAT_SET_LDS(kern, bytes)                                                                                                           \
    ([]() {                                                                                                                                \
        static const int rc = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (bytes)) \
                                      == hipSuccess ? 0 : -2;                                                                              \
        return rc;                                                                                                                         \
    }())
static int dev_alloc(void** p, size_t n) { return hipMalloc(p, n ? n : 1) == hipSuccess ? 0 : -2; }
static void dev_free(void* p) { if (p) (void)hipFree(p); }
static int h2d(void* d, const void* h, size_t n) { return !n || hipMemcpy(d, h, n, hipMemcpyHostToDevice) == hipSuccess ? 0 : -2; }
static int d2h(void* h, const void* d, size_t n) { return !n || hipMemcpy(h, d, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2; }
static int dev_finish() { return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -2; }
#endif
