// TEST-ONLY known-answer harness for the fp16 wide-OSNet kernels (ReID mode 1: boxmot_amd/csrc/osnet_wide_kernels.hpp and the stem packer
// of osnet_wide_pack.hpp, both included unchanged): k_wide_stem<32 | 64>, k_light_fused<32 | 64 | 96 | 128>, k_gate_sum4<C>, k_wide_gap,
// k_wide_l2 -- the family's GEMMs are gemm_kat.hip's.
//
// One extern "C" entry point per kernel: each takes host arrays (every one with its length, so that the caller's poison and guard
// elements travel with it), copies them to the device, launches exactly as WideOsnet::forward (osnet_wide.hpp) does -- grid, 256 threads,
// dynamic LDS and hipFuncSetAttribute per instantiation -- copies the WHOLE output allocations back and returns 0, or a negative status
// (-1: outside the kernel's contract, nothing launched; -2: a HIP call failed).
//
// Built two ways, as gemm_kat.hip: by hipcc for gfx950 (tests/test_gpu_wide_kat.py), and with -DKAT_EMU by a host clang against
// tests/host_emu/hip_shim.hpp, where the same kernels run on CPU threads (tests/test_wide_kat_emu.py).  Nothing in boxmot_amd/ includes this
// file.
#define KAT_EMU_STACK (1 << 20)
#include "kat_harness.hpp"

#include "../../boxmot_amd/csrc/osnet_wide_kernels.hpp"
#include "../../boxmot_amd/csrc/osnet_wide_pack.hpp"

using namespace bm;

namespace {

// device copies of host arrays; freed on scope exit
struct Dev {
    std::vector<void*> owned;
    ~Dev() { for (void* p : owned) dev_free(p); }
    // nullptr stays nullptr (status 0); *ok is cleared when an allocation or a copy fails
    template <class T>
    T* up(const void* h, size_t bytes, bool* ok) {
        if (!h) return nullptr;
        void* p = nullptr;
        if (dev_alloc(&p, bytes)) { *ok = false; return nullptr; }
        owned.push_back(p);
        if (h2d(p, h, bytes)) *ok = false;
        return static_cast<T*>(p);
    }
};

int down(void* h, const void* d, size_t bytes) { return d2h(h, d, bytes); }

template <int C0>
int run_stem(const uint16_t* crops, long crops_halves, int n, const float* w, const float* bias, uint16_t* out, long out_halves) {
    // the product packs a whole OSN1 blob: the smallest network the family supports around the stem under test, every other tensor zero
    const int ch[4] = {C0, 128, 128, 128};
    const OsnetLayout L = make_osnet_layout(ch, 128);
    if (!wide_osnet_supports(L)) return -1;
    std::vector<float> blob((size_t)L.total, 0.f);
    std::memcpy(blob.data() + L.stem_w, w, (size_t)C0 * 147 * 4);
    const WideW16 pk = wide_pack_w16(blob.data(), L);
    Dev d;
    bool ok = true;
    _Float16* d_crops = d.up<_Float16>(crops, (size_t)crops_halves * 2, &ok);
    _Float16* d_w16 = d.up<_Float16>(pk.data.data(), pk.data.size() * 2, &ok);
    float* d_bias = d.up<float>(bias, (size_t)C0 * 4, &ok);
    _Float16* d_out = d.up<_Float16>(out, (size_t)out_halves * 2, &ok);
    if (!ok) return -2;
    KAT_LAUNCH_XY(k_wide_stem<C0>, 64 / WSTEM_PBAND, n, 256, 0, d_crops, d_w16 + pk.stem, d_bias, d_out);
    if (dev_finish()) return -2;
    return down(out, d_out, (size_t)out_halves * 2);
}

template <int C>
int run_light(const uint16_t* in, const uint16_t* pw, const float* dw, const float* bias, uint16_t* out, long out_halves, float* gap,
              long gap_floats, int use_gap, int n, int H, int W) {
    const int lds = light_lds_bytes<C>(W);
    if (W > (C <= 64 ? 32 : 16)) return -1;
    if (KAT_SET_LDS(k_light_fused<C>, light_lds_bytes<C>(C <= 64 ? 32 : 16))) return -2;      // the product's widest image row at this width: once per instantiation
    Dev d;
    bool ok = true;
    _Float16* d_in = d.up<_Float16>(in, (size_t)n * H * W * C * 2, &ok);
    _Float16* d_pw = d.up<_Float16>(pw, (size_t)C * C * 2, &ok);
    float* d_dw = d.up<float>(dw, (size_t)C * 9 * 4, &ok);
    float* d_bias = d.up<float>(bias, (size_t)C * 4, &ok);
    _Float16* d_out = d.up<_Float16>(out, (size_t)out_halves * 2, &ok);
    float* d_gap = d.up<float>(gap, (size_t)gap_floats * 4, &ok);
    if (!ok) return -2;
    KAT_LAUNCH_XY(k_light_fused<C>, H / WIDE_BAND, n, 256, lds, d_in, d_pw, d_dw, d_bias, d_out, use_gap ? d_gap : nullptr, H, W);
    if (dev_finish()) return -2;
    if (down(out, d_out, (size_t)out_halves * 2)) return -2;
    return down(gap, d_gap, (size_t)gap_floats * 4);
}

template <int C>
int run_gate(const uint16_t* const* x, const float* gap, const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
             uint16_t* out, long out_halves, int P, int nbands, int n) {
    constexpr int HID = C / 16;
    Dev d;
    bool ok = true;
    _Float16* dx[4];
    for (int b = 0; b < 4; ++b) dx[b] = d.up<_Float16>(x[b], (size_t)n * P * C * 2, &ok);
    float* d_gap = d.up<float>(gap, (size_t)4 * n * nbands * C * 4, &ok);
    float* d_f1w = d.up<float>(fc1_w, (size_t)HID * C * 4, &ok);
    float* d_f1b = d.up<float>(fc1_b, (size_t)HID * 4, &ok);
    float* d_f2w = d.up<float>(fc2_w, (size_t)C * HID * 4, &ok);
    float* d_f2b = d.up<float>(fc2_b, (size_t)C * 4, &ok);
    _Float16* d_out = d.up<_Float16>(out, (size_t)out_halves * 2, &ok);
    if (!ok) return -2;
    const int ppb = 128;
    KAT_LAUNCH_XY(k_gate_sum4<C>, n, (P + ppb - 1) / ppb, 256, 0, dx[0], dx[1], dx[2], dx[3], d_gap, d_f1w, d_f1b, d_f2w, d_f2b, d_out, P,
                  nbands, (long)n, ppb);
    if (dev_finish()) return -2;
    return down(out, d_out, (size_t)out_halves * 2);
}

}  // namespace

// k_wide_stem<c0>: crops fp16 [.][262][136][4] of crops_halves halves in all (>= n crops: what follows the last crop is the caller's
// poison), w fp32 [c0][7][7][3] as in the OSN1 blob (packed here by wide_pack_w16), out fp16 of out_halves >= n * 2048 * c0 halves
extern "C" int kat_wide_stem(int c0, const uint16_t* crops, long crops_halves, int n, const float* w, const float* bias, uint16_t* out,
                             long out_halves) {
    if (n < 1 || !crops || !w || !bias || !out || crops_halves < (long)n * WSTEM_ROWS * WSTEM_COLS * 4 || out_halves < (long)n * 2048 * c0) return -1;
    if (c0 == 32) return run_stem<32>(crops, crops_halves, n, w, bias, out, out_halves);
    if (c0 == 64) return run_stem<64>(crops, crops_halves, n, w, bias, out, out_halves);
    return -1;
}

// k_light_fused<C>: in fp16 [n][H][W][C], pw fp16 [C][C], dw fp32 [C][9], bias fp32 [C], out fp16 of out_halves >= n H W C halves,
// gap fp32 of gap_floats >= n (H / 8) C floats: uploaded and copied back either way, handed to the kernel only with use_gap (else the
// kernel gets nullptr and the caller's poison must come back untouched)
extern "C" int kat_wide_light(int C, const uint16_t* in, const uint16_t* pw, const float* dw, const float* bias, uint16_t* out, long out_halves,
                              float* gap, long gap_floats, int use_gap, int n, int H, int W) {
    if (n < 1 || !in || !pw || !dw || !bias || !out || !gap || H < WIDE_BAND || H % WIDE_BAND || W < 8 || W > 32 || W % 8 || W * (C / 8) > 256) return -1;
    if (out_halves < (long)n * H * W * C || gap_floats < (long)n * (H / WIDE_BAND) * C) return -1;
    switch (C) {
        case 32: return run_light<32>(in, pw, dw, bias, out, out_halves, gap, gap_floats, use_gap, n, H, W);
        case 64: return run_light<64>(in, pw, dw, bias, out, out_halves, gap, gap_floats, use_gap, n, H, W);
        case 96: return run_light<96>(in, pw, dw, bias, out, out_halves, gap, gap_floats, use_gap, n, H, W);
        case 128: return run_light<128>(in, pw, dw, bias, out, out_halves, gap, gap_floats, use_gap, n, H, W);
        default: return -1;
    }
}

// k_gate_sum4<C>: xa .. xd fp16 [n][P][C], gap fp32 [4][n][nbands][C], fc1 [C / 16][C] + [C / 16], fc2 [C][C / 16] + [C], out fp16 of
// out_halves >= n P C halves; pixel blocks of 128
extern "C" int kat_wide_gate(int C, const uint16_t* xa, const uint16_t* xb, const uint16_t* xc, const uint16_t* xd, const float* gap,
                             const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b, uint16_t* out, long out_halves, int P,
                             int nbands, int n) {
    if (n < 1 || P < 1 || nbands < 1 || !xa || !xb || !xc || !xd || !gap || !fc1_w || !fc1_b || !fc2_w || !fc2_b || !out) return -1;
    if (out_halves < (long)n * P * C) return -1;
    const uint16_t* x[4] = {xa, xb, xc, xd};
    switch (C) {
        case 32: return run_gate<32>(x, gap, fc1_w, fc1_b, fc2_w, fc2_b, out, out_halves, P, nbands, n);
        case 64: return run_gate<64>(x, gap, fc1_w, fc1_b, fc2_w, fc2_b, out, out_halves, P, nbands, n);
        case 96: return run_gate<96>(x, gap, fc1_w, fc1_b, fc2_w, fc2_b, out, out_halves, P, nbands, n);
        case 128: return run_gate<128>(x, gap, fc1_w, fc1_b, fc2_w, fc2_b, out, out_halves, P, nbands, n);
        default: return -1;
    }
}

// k_wide_gap: in fp16 [n][P][C], out fp16 of out_halves >= n C halves
extern "C" int kat_wide_gap(const uint16_t* in, uint16_t* out, long out_halves, int n, int P, int C) {
    if (n < 1 || P < 1 || C < 8 || C % 8 || !in || !out || out_halves < (long)n * C) return -1;
    Dev d;
    bool ok = true;
    _Float16* d_in = d.up<_Float16>(in, (size_t)n * P * C * 2, &ok);
    _Float16* d_out = d.up<_Float16>(out, (size_t)out_halves * 2, &ok);
    if (!ok) return -2;
    const long g8 = (long)n * (C / 8);
    KAT_LAUNCH(k_wide_gap, (g8 + 255) / 256, 256, 0, d_in, d_out, P, C, g8);
    if (dev_finish()) return -2;
    return down(out, d_out, (size_t)out_halves * 2);
}

// k_wide_l2: v fp32 [n][F], out fp32 of out_floats floats, rows nullptr (row i -> i) or int32 [n] (row i -> rows[i], every one inside out)
extern "C" int kat_wide_l2(const float* v, float* out, long out_floats, const int* rows, int n, int F) {
    if (n < 1 || F < 1 || !v || !out) return -1;
    for (int i = 0; i < n; ++i) {
        const long r = rows ? rows[i] : i;
        if (r < 0 || (r + 1) * F > out_floats) return -1;
    }
    Dev d;
    bool ok = true;
    float* d_v = d.up<float>(v, (size_t)n * F * 4, &ok);
    float* d_out = d.up<float>(out, (size_t)out_floats * 4, &ok);
    int* d_rows = d.up<int>(rows, (size_t)n * 4, &ok);
    if (!ok) return -2;
    KAT_LAUNCH(k_wide_l2, (n + 3) / 4, 256, 0, d_v, d_out, d_rows, (long)n, F);
    if (dev_finish()) return -2;
    return down(out, d_out, (size_t)out_floats * 4);
}
