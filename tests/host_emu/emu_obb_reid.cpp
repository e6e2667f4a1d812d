// TEST-ONLY harness: the device sources of the oriented ReID front end -- obb_crop_geometry / build_crop_list_obb_kernel
// (boxmot_amd/csrc/obb_crop_geometry.hpp, crop_list.hpp) and k_crop_resize_obb_rgbx_hl[_sized] (reid_hp.hpp), unchanged -- on CPU threads, with the
// library's grids.  Built with the ROCm clang in host mode (needs _Float16); not a product path (see hip_shim.hpp).
#include "hip_shim.hpp"

#include <cstdlib>
#include <functional>
#include <vector>

#include "../../boxmot_amd/csrc/crop_list.hpp"
#include "../../boxmot_amd/csrc/reid_hp.hpp"

thread_local EmuDim3 threadIdx;
thread_local EmuDim3 blockIdx;
EmuDim3 blockDim;
EmuDim3 gridDim;
EmuBlock* g_emu_block = nullptr;
unsigned char* g_emu_dynamic_lds = nullptr;
EmuMfmaBuf* g_emu_mfma = nullptr;

namespace {

struct TA { const std::function<void()>* fn; int tid; int bx, by; };

void* tmain(void* p) {
    TA* a = static_cast<TA*>(p);
    threadIdx.x = a->tid; blockIdx.x = a->bx; blockIdx.y = a->by;
    (*a->fn)();
    return nullptr;
}

// run `fn` as a grid of gx x gy workgroups of nthr threads (workgroups sequential)
void launch(int gx, int gy, int nthr, const std::function<void()>& fn) {
    static EmuBlock block;
    g_emu_block = &block;
    blockDim.x = nthr; gridDim.x = (unsigned)gx; gridDim.y = (unsigned)gy;
    block.block_barrier.init(nthr);
    for (int w = 0; w < EMU_MAX_WAVES; ++w) block.wave_barrier[w].init(EMU_WAVE);
    for (int by = 0; by < gy; ++by)
        for (int bx = 0; bx < gx; ++bx) {
            std::vector<TA> ta(nthr);
            for (int t = 0; t < nthr; ++t) ta[t] = TA{&fn, t, bx, by};
            emu_run_threads(nthr, tmain, ta.data(), sizeof(ta[0]), 1 << 20);
        }
}

void make_lut(float* lut) {         // ReidEngine's table: (v / 255 - mean) / std, every step rounded to fp32
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            volatile float a = (float)v / 255.0f;
            volatile float b = a - mean[c];
            lut[c * 256 + v] = b / stdv[c];
        }
}

}  // namespace

extern "C" {

// obb_crop_geometry through obb_geometry_kernel (the library's debug launch: 64 threads per workgroup)
int emu_obb_geometry(const float* boxes, int box_stride, int n, double* geo) {
    launch((n + 63) / 64, 1, 64, [=]() { bm::obb_geometry_kernel(boxes, box_stride, n, geo); });
    return 0;
}

// build_crop_list_obb_kernel as core_reid_pass launches it: one workgroup of 256 threads per stream, the count zeroed before
int emu_build_crop_list_obb(const float* dets, const int* n_dets, int n_streams, int max_dets, double high, int inclusive, int stream_base,
                            int* crop_count, int* crop_stream, int* crop_row, double* crop_geo) {
    *crop_count = 0;
    launch(n_streams, 1, 256, [=]() {
        bm::build_crop_list_obb_kernel(dets, n_dets, max_dets, high, crop_count, crop_stream, crop_row, crop_geo, stream_base, inclusive);
    });
    return 0;
}

// k_crop_resize_obb_rgbx_hl (dims == null: one frame size W x H) or k_crop_resize_obb_rgbx_hl_sized (dims = {W, H} per stream) on the
// engine's grid; `count` < 0: no count pointer.  out_hi / out_lo: [n][262][136][4] halves, written in place (interior only).
int emu_crop_resize_obb_hl(const uint8_t* const* frames, const int* crop_stream, const double* geo, int n, int W, int H, const int* dims,
                           int count, int pad, uint16_t* out_hi, uint16_t* out_lo) {
    using namespace bm;
    static float lut[768];
    make_lut(lut);
    const float* lp = lut;
    const int* cnt = count >= 0 ? &count : nullptr;
    _Float16* oh = reinterpret_cast<_Float16*>(out_hi);
    _Float16* ol = reinterpret_cast<_Float16*>(out_lo);
    if (dims) launch(n, REID_IN_H / 16, REID_IN_W, [=]() { k_crop_resize_obb_rgbx_hl_sized(frames, crop_stream, geo, dims, lp, oh, ol, 16, cnt, pad); });
    else launch(n, REID_IN_H / 16, REID_IN_W, [=]() { k_crop_resize_obb_rgbx_hl(frames, crop_stream, geo, W, H, lp, oh, ol, 16, cnt, pad); });
    return 0;
}

}  // extern "C"
