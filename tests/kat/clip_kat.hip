// TEST-ONLY known-answer harness for the CLIP-ReID kernels around the GEMMs (boxmot_amd/csrc/clip_kernels.hpp, included unchanged):
// k_clip_patches, k_clip_tokens_lnpre, k_clip_layernorm_f16, k_clip_attention, k_clip_attention_t<T> and k_clip_head.
//
// One extern "C" entry point per kernel: each takes host arrays, copies them to the device, launches as ClipNet::forward / ClipNet::ClipNet
// of clip_engine.hpp do (grid formula, block size, dynamic LDS bytes, hipFuncSetAttribute for both attention kernels), copies the WHOLE
// output allocation back (guard rows included) and returns 0, or a negative status (-1: outside the kernel's contract or the caller's
// arrays, nothing launched; -2: a HIP call failed).  Every array comes with its size, and an entry refuses a launch that would read or
// write past one.  kat_expf evaluates BM_EXPF (the attention's exponential: __expf on the device) on a list of arguments.
//
// Built two ways, as gemm_kat.hip: by hipcc for gfx950 (tests/test_gpu_clip_kat.py), and with -DKAT_EMU by a host clang against
// tests/host_emu/hip_shim.hpp, where the same kernels run on CPU threads (tests/test_clip_kat_emu.py).  Nothing in boxmot_amd/ includes it.
#include "kat_harness.hpp"

#include "../../boxmot_amd/csrc/clip_kernels.hpp"

using namespace bm;

namespace {

// device copies of host arrays; freed on scope exit
struct Bufs {
    std::vector<void*> owned;
    ~Bufs() { for (void* p : owned) dev_free(p); }
    template <class T>
    int up(T*& d, const void* h, size_t bytes) {
        d = nullptr;
        if (!h) return 0;
        void* p = nullptr;
        if (dev_alloc(&p, bytes)) return -2;
        owned.push_back(p);
        d = static_cast<T*>(p);
        return h2d(p, h, bytes);
    }
};

int down(void* h, const void* d, size_t bytes) { return dev_finish() ? -2 : d2h(h, d, bytes); }

#ifndef KAT_EMU
__global__ void k_kat_expf(const float* __restrict__ x, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = BM_EXPF(x[i]);
}
#endif

template <int T>
int run_attention_t(const uint16_t* qkv, long qkv_rows, uint16_t* out, long out_bytes, int n, int D, int heads) {
    if (n < 1 || heads < 1 || D != heads * ATT_DH || qkv_rows < (long)n * T || out_bytes < (long)n * T * D * 2 || !qkv || !out) return -1;
    if (KAT_SET_LDS((k_clip_attention_t<T>), clip_attn_t_lds_bytes<T>())) return -2;
    Bufs b;
    _Float16 *dq, *dout;
    if (b.up(dq, qkv, (size_t)qkv_rows * 3 * D * 2) || b.up(dout, out, (size_t)out_bytes)) return -2;
    KAT_LAUNCH((k_clip_attention_t<T>), n * heads, 192, (size_t)clip_attn_t_lds_bytes<T>(), dq, dout, D, heads);
    return down(out, dout, (size_t)out_bytes);
}

}  // namespace

// k_clip_patches: crops fp32 NHWC, crop_floats >= n H W 3 (the rest is the caller's poison); out fp16 rows [n gh gw][patch patch 3] + guard
extern "C" int kat_clip_patches(const float* crops, long crop_floats, uint16_t* out, long out_bytes, int n, int H, int W, int patch, int gh,
                                int gw) {
    if (n < 1 || patch < 1 || gh < 1 || gw < 1 || gh * patch > H || gw * patch > W || !crops || !out) return -1;
    const long total = (long)n * gh * gw * patch * patch * 3;
    if (crop_floats < (long)n * H * W * 3 || out_bytes < total * 2) return -1;
    Bufs b;
    float* dc;
    _Float16* dout;
    if (b.up(dc, crops, (size_t)crop_floats * 4) || b.up(dout, out, (size_t)out_bytes)) return -2;
    const unsigned blocks = (unsigned)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
    KAT_LAUNCH(k_clip_patches, blocks, 256, 0, dc, dout, n, H, W, patch, gh, gw);
    return down(out, dout, (size_t)out_bytes);
}

// k_clip_tokens_lnpre: pe fp32 [pe_rows >= n (T - 1)][D], cls / gamma / beta [D], pos [T][D]; x fp32 rows [n T][D] + guard
extern "C" int kat_clip_tokens_lnpre(const float* pe, long pe_rows, const float* cls, const float* pos, const float* gamma, const float* beta,
                                     float* x, long x_bytes, long rows, int T, int D) {
    if (rows < 1 || T < 2 || D < 1 || rows % T || !pe || !cls || !pos || !gamma || !beta || !x) return -1;
    if (pe_rows < rows / T * (T - 1) || x_bytes < rows * D * 4) return -1;
    Bufs b;
    float *dpe, *dcls, *dpos, *dg, *dbt, *dx;
    if (b.up(dpe, pe, (size_t)pe_rows * D * 4) || b.up(dcls, cls, (size_t)D * 4) || b.up(dpos, pos, (size_t)T * D * 4) ||
        b.up(dg, gamma, (size_t)D * 4) || b.up(dbt, beta, (size_t)D * 4) || b.up(dx, x, (size_t)x_bytes))
        return -2;
    KAT_LAUNCH(k_clip_tokens_lnpre, (rows + 3) / 4, 256, 0, dpe, dcls, dpos, dg, dbt, dx, rows, T, D);
    return down(x, dx, (size_t)x_bytes);
}

// k_clip_layernorm_f16: x fp32 [x_rows >= rows][D] (D % 4 == 0: the kernel reads 16-byte groups); out fp16 rows [rows][D] + guard
extern "C" int kat_clip_layernorm(const float* x, long x_rows, const float* gamma, const float* beta, uint16_t* out, long out_bytes, long rows,
                                  int D) {
    if (rows < 1 || D < 4 || D % 4 || x_rows < rows || out_bytes < rows * D * 2 || !x || !gamma || !beta || !out) return -1;
    Bufs b;
    float *dx, *dg, *dbt;
    _Float16* dout;
    if (b.up(dx, x, (size_t)x_rows * D * 4) || b.up(dg, gamma, (size_t)D * 4) || b.up(dbt, beta, (size_t)D * 4) ||
        b.up(dout, out, (size_t)out_bytes))
        return -2;
    KAT_LAUNCH(k_clip_layernorm_f16, (rows + 3) / 4, 256, 0, dx, dg, dbt, dout, rows, D);
    return down(out, dout, (size_t)out_bytes);
}

// k_clip_attention (run-time T): qkv fp16 [qkv_rows >= n T][3 D], out fp16 rows [n T][D] + guard.  The LDS attribute is set for this T on
// every call, as the constructor of an engine with that token count does.
extern "C" int kat_clip_attention(const uint16_t* qkv, long qkv_rows, uint16_t* out, long out_bytes, int n, int T, int D, int heads) {
    if (n < 1 || T < 1 || T > ATT_MAX_T || heads < 1 || D != heads * ATT_DH || !qkv || !out) return -1;
    if (qkv_rows < (long)n * T || out_bytes < (long)n * T * D * 2) return -1;
#ifndef KAT_EMU
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_clip_attention), hipFuncAttributeMaxDynamicSharedMemorySize,
                            clip_attn_lds_bytes(T)) != hipSuccess)
        return -2;
#endif
    Bufs b;
    _Float16 *dq, *dout;
    if (b.up(dq, qkv, (size_t)qkv_rows * 3 * D * 2) || b.up(dout, out, (size_t)out_bytes)) return -2;
    KAT_LAUNCH(k_clip_attention, n * heads, 256, (size_t)clip_attn_lds_bytes(T), dq, dout, T, D, heads);
    return down(out, dout, (size_t)out_bytes);
}

// k_clip_attention_t<T>: <129> is the product's instantiation (ViT-B/16 on 256 x 128 crops), <33> a small one with the same shape of
// last key tile (one valid key) that keeps the emulated tests fast
extern "C" int kat_clip_attention_t(int T, const uint16_t* qkv, long qkv_rows, uint16_t* out, long out_bytes, int n, int D, int heads) {
    if (T == 129) return run_attention_t<129>(qkv, qkv_rows, out, out_bytes, n, D, heads);
    if (T == 33) return run_attention_t<33>(qkv, qkv_rows, out, out_bytes, n, D, heads);
    return -1;
}

// k_clip_head: x fp32 [x_rows >= n T][D]; out fp32 [out_total_rows][D + E]; out_rows: n row indices below out_total_rows, or null (row = crop)
extern "C" int kat_clip_head(const float* x, long x_rows, const float* gamma, const float* beta, const float* proj, const float* bn_scale,
                             const float* bn_shift, const float* bnp_scale, const float* bnp_shift, float* out, long out_total_rows,
                             const int* out_rows, int n, int T, int D, int E) {
    if (n < 1 || T < 1 || D < 1 || E < 1 || x_rows < (long)n * T || !x || !gamma || !beta || !proj || !bn_scale || !bn_shift || !bnp_scale ||
        !bnp_shift || !out)
        return -1;
    for (int i = 0; i < n; ++i)
        if ((out_rows ? (long)out_rows[i] : (long)i) >= out_total_rows || (out_rows && out_rows[i] < 0)) return -1;
    Bufs b;
    float *dx, *dg, *dbt, *dp, *ds, *dsh, *dps, *dpsh, *dout;
    int* drows;
    const size_t out_bytes = (size_t)out_total_rows * (D + E) * 4;
    if (b.up(dx, x, (size_t)x_rows * D * 4) || b.up(dg, gamma, (size_t)D * 4) || b.up(dbt, beta, (size_t)D * 4) ||
        b.up(dp, proj, (size_t)D * E * 4) || b.up(ds, bn_scale, (size_t)D * 4) || b.up(dsh, bn_shift, (size_t)D * 4) ||
        b.up(dps, bnp_scale, (size_t)E * 4) || b.up(dpsh, bnp_shift, (size_t)E * 4) || b.up(dout, out, out_bytes) ||
        b.up(drows, out_rows, (size_t)n * 4))
        return -2;
    KAT_LAUNCH(k_clip_head, n, 256, (size_t)(D + 8) * 4, dx, dg, dbt, dp, ds, dsh, dps, dpsh, dout, drows, T, D, E);
    return down(out, dout, out_bytes);
}

// y[i] = BM_EXPF(x[i]): the exponential k_clip_attention evaluates (__expf on the device, expf in the emulation)
extern "C" int kat_expf(const float* x, float* y, long n) {
    if (n < 1 || !x || !y) return -1;
    Bufs b;
    float *dx, *dy;
    if (b.up(dx, x, (size_t)n * 4) || b.up(dy, y, (size_t)n * 4)) return -2;
#ifdef KAT_EMU
    for (long i = 0; i < n; ++i) dy[i] = BM_EXPF(dx[i]);
#else
    KAT_LAUNCH(k_kat_expf, (n + 255) / 256, 256, 0, dx, dy, n);
#endif
    return down(y, dy, (size_t)n * 4);
}
