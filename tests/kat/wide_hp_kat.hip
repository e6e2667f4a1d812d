// TEST-ONLY known-answer harness for the fp32-grade wide-OSNet kernels (ReID mode 2 at widths that are multiples of 32:
// boxmot_amd/csrc/osnet_wide_hp_kernels.hpp and the packer osnet_wide_hp_pack.hpp, both included unchanged): k_wide_stem_hp<32 | 64>,
// k_gemm_hp<EPI, BN, DB> in every instantiation wide_hp_forward's dispatch can reach, k_chain_hp<C, W, WR, HALO>, k_gate_sum4_hp<C>,
// k_wide_gap_hp, and wide_pack_hp's planes and biases on the host.
//
// One extern "C" entry point per kernel: each takes host arrays (every one with its length, so that the caller's poison and guard
// elements travel with it), copies them to the device, launches exactly as wide_hp_forward (osnet_wide_hp.hpp) does -- grid, threads,
// dynamic LDS and hipFuncSetAttribute per instantiation -- copies the WHOLE output allocations back and returns 0, or a negative status
// (-1: outside the kernel's contract, nothing launched; -2: a HIP call failed).
//
// Built two ways, as wide_kat.hip: by hipcc for gfx950 (tests/test_gpu_wide_hp_kat.py), and with -DKAT_EMU by a host clang against
// tests/host_emu/hip_shim.hpp, where the same kernels run on CPU threads (tests/test_wide_hp_kat_emu.py).  Nothing in boxmot_amd/ includes
// this file.
#define KAT_EMU_STACK (1 << 20)
#include "kat_harness.hpp"

#include "../../boxmot_amd/csrc/osnet_wide_hp_kernels.hpp"
#include "../../boxmot_amd/csrc/osnet_wide_hp_pack.hpp"

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

int down(void* h, const void* d, size_t bytes) { return h ? d2h(h, d, bytes) : 0; }

// the smallest OSN1 layout the family supports whose block `*blk` has the middle width C (stage 0 up to 64, stage 1 up to 96, stage 2 any)
OsnetLayout layout_with_mid(int c0, int C, int* blk) {
    int ch[4] = {c0, 128, 128, 128};
    const int s = C <= 64 ? 0 : (C <= 96 ? 1 : 2);
    ch[s + 1] = 4 * C;
    *blk = 2 * s + 1;                 // the stage's second block: cin == cout, no downsample
    return make_osnet_layout(ch, 128);
}

// the packed bytes of a blob, 16-byte aligned on the device
unsigned char* up_pack(Dev& d, const WideHpPack& pk, bool* ok) { return d.up<unsigned char>(pk.data.data(), pk.data.size(), ok); }

template <int C0>
int run_stem(const uint16_t* ch, const uint16_t* cl, long crops_halves, int n, const float* w, const float* bias, uint16_t* oh, uint16_t* ol,
             long out_halves) {
    const int chn[4] = {C0, 128, 128, 128};
    const OsnetLayout L = make_osnet_layout(chn, 128);
    if (!wide_hp_supports(L)) return -1;
    std::vector<float> blob((size_t)L.total, 0.f);
    std::memcpy(blob.data() + L.stem_w, w, (size_t)C0 * 147 * 4);
    std::memcpy(blob.data() + L.stem_b, bias, (size_t)C0 * 4);
    const WideHpPack pk = wide_pack_hp(blob.data(), L);
    Dev d;
    bool ok = true;
    _Float16* d_ch = d.up<_Float16>(ch, (size_t)crops_halves * 2, &ok);
    _Float16* d_cl = d.up<_Float16>(cl, (size_t)crops_halves * 2, &ok);
    unsigned char* wp = up_pack(d, pk, &ok);
    _Float16* d_oh = d.up<_Float16>(oh, (size_t)out_halves * 2, &ok);
    _Float16* d_ol = d.up<_Float16>(ol, (size_t)out_halves * 2, &ok);
    if (!ok) return -2;
    KAT_LAUNCH_XY(k_wide_stem_hp<C0>, 64 / WSTEM_PBAND, n, 256, 0, (const _Float16*)d_ch, (const _Float16*)d_cl, (const unsigned char*)(wp + pk.stem_a),
                  reinterpret_cast<const float*>(wp + pk.stem_b), d_oh, d_ol);
    if (dev_finish()) return -2;
    if (down(oh, d_oh, (size_t)out_halves * 2)) return -2;
    return down(ol, d_ol, (size_t)out_halves * 2);
}

struct GemmArgs {
    const uint16_t *xh, *xl; long x_halves;
    const uint16_t *wh, *wl;
    const float* bias;
    void *oh, *ol; long out_bytes;
    const uint16_t *rh, *rl; long res_halves;
    int M, N, K, relu;
    const uint16_t *x2h, *x2l; long x2_halves;
    const uint16_t *w2h, *w2l; int K2;
};

template <int EPI, int BN, int DB>
int run_gemm(const GemmArgs& a) {
    constexpr auto kern = &k_gemm_hp<EPI, BN, DB>;
    constexpr int lds = gemm_hp_lds_bytes<BN, DB>();
    if (KAT_SET_LDS(kern, lds)) return -2;
    Dev d;
    bool ok = true;
    _Float16* xh = d.up<_Float16>(a.xh, (size_t)a.x_halves * 2, &ok);
    _Float16* xl = d.up<_Float16>(a.xl, (size_t)a.x_halves * 2, &ok);
    _Float16* wh = d.up<_Float16>(a.wh, (size_t)a.N * a.K * 2, &ok);
    _Float16* wl = d.up<_Float16>(a.wl, (size_t)a.N * a.K * 2, &ok);
    float* bias = d.up<float>(a.bias, (size_t)a.N * 4, &ok);
    unsigned char* oh = d.up<unsigned char>(a.oh, (size_t)a.out_bytes, &ok);
    unsigned char* ol = d.up<unsigned char>(a.ol, (size_t)a.out_bytes, &ok);
    _Float16* rh = d.up<_Float16>(a.rh, (size_t)a.res_halves * 2, &ok);
    _Float16* rl = d.up<_Float16>(a.rl, (size_t)a.res_halves * 2, &ok);
    GemmHpExt ext;
    ext.X2h = d.up<_Float16>(a.x2h, (size_t)a.x2_halves * 2, &ok);
    ext.X2l = d.up<_Float16>(a.x2l, (size_t)a.x2_halves * 2, &ok);
    ext.W2h = d.up<_Float16>(a.w2h, (size_t)a.N * a.K2 * 2, &ok);
    ext.W2l = d.up<_Float16>(a.w2l, (size_t)a.N * a.K2 * 2, &ok);
    ext.K2 = a.K2;
    if (!ok) return -2;
    const long mt = ((long)a.M + GEMM_BM - 1) / GEMM_BM;
    KAT_LAUNCH_XY(kern, (int)(mt * (a.N / BN)), 1, 256, lds, (const _Float16*)xh, (const _Float16*)xl, (const _Float16*)wh, (const _Float16*)wl,
                  (const float*)bias, (void*)oh, (void*)ol, (const _Float16*)rh, (const _Float16*)rl, a.M, a.N, a.K, a.relu, ext);
    if (dev_finish()) return -2;
    if (down(a.oh, oh, (size_t)a.out_bytes)) return -2;
    return down(a.ol, ol, (size_t)a.out_bytes);
}

template <int C, int W, int WR, int HALO>
int run_chain(const uint16_t* x1h, const uint16_t* x1l, long x_halves, int n, int H, const float* recs, uint16_t* yh, uint16_t* yl, long y_halves,
              float* gap, long gap_floats) {
    using G = ChainGeo<C, W, WR, HALO>;
    constexpr auto kern = &k_chain_hp<C, W, WR, HALO>;
    int blk = 0;
    const OsnetLayout L = layout_with_mid(32, C, &blk);
    if (!wide_hp_supports(L) || L.block[blk].mid != C) return -1;
    std::vector<float> blob((size_t)L.total, 0.f);
    const float* src = recs;
    for (int l = 0; l < 10; ++l) {          // blob order per LightConv: pw [C][C], dw [C][9], bias [C]
        std::memcpy(blob.data() + L.block[blk].light[l].pw, src, (size_t)C * C * 4); src += C * C;
        std::memcpy(blob.data() + L.block[blk].light[l].dw, src, (size_t)C * 9 * 4); src += C * 9;
        std::memcpy(blob.data() + L.block[blk].light[l].b, src, (size_t)C * 4); src += C;
    }
    const WideHpPack pk = wide_pack_hp(blob.data(), L);
    if (chain_rec_bytes(C) != G::LREC) return -1;
    if (KAT_SET_LDS(kern, G::LDS_BYTES)) return -2;
    Dev d;
    bool ok = true;
    _Float16* d_xh = d.up<_Float16>(x1h, (size_t)x_halves * 2, &ok);
    _Float16* d_xl = d.up<_Float16>(x1l, (size_t)x_halves * 2, &ok);
    unsigned char* wp = up_pack(d, pk, &ok);
    _Float16* d_yh = d.up<_Float16>(yh, (size_t)y_halves * 2, &ok);
    _Float16* d_yl = d.up<_Float16>(yl, (size_t)y_halves * 2, &ok);
    float* d_gap = d.up<float>(gap, (size_t)gap_floats * 4, &ok);
    if (!ok) return -2;
    KAT_LAUNCH_XY(kern, H / G::R, n, 512, G::LDS_BYTES, (const _Float16*)d_xh, (const _Float16*)d_xl, (const unsigned char*)(wp + pk.block[blk].chain), d_yh,
                  d_yl, d_gap, H, (long)n);
    if (dev_finish()) return -2;
    if (down(yh, d_yh, (size_t)y_halves * 2) || down(yl, d_yl, (size_t)y_halves * 2)) return -2;
    return down(gap, d_gap, (size_t)gap_floats * 4);
}

template <int C>
int run_gate(const uint16_t* yh, const uint16_t* yl, const float* gap, const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
             uint16_t* oh, uint16_t* ol, long out_halves, int P, int nbands, int n) {
    constexpr int HID = C / 16;
    Dev d;
    bool ok = true;
    _Float16* d_yh = d.up<_Float16>(yh, (size_t)4 * n * P * C * 2, &ok);
    _Float16* d_yl = d.up<_Float16>(yl, (size_t)4 * n * P * C * 2, &ok);
    float* d_gap = d.up<float>(gap, (size_t)4 * n * nbands * C * 4, &ok);
    float* d_f1w = d.up<float>(fc1_w, (size_t)HID * C * 4, &ok);
    float* d_f1b = d.up<float>(fc1_b, (size_t)HID * 4, &ok);
    float* d_f2w = d.up<float>(fc2_w, (size_t)C * HID * 4, &ok);
    float* d_f2b = d.up<float>(fc2_b, (size_t)C * 4, &ok);
    _Float16* d_oh = d.up<_Float16>(oh, (size_t)out_halves * 2, &ok);
    _Float16* d_ol = d.up<_Float16>(ol, (size_t)out_halves * 2, &ok);
    if (!ok) return -2;
    const int ppb = 128;
    KAT_LAUNCH_XY(k_gate_sum4_hp<C>, n, (P + ppb - 1) / ppb, 256, 0, (const _Float16*)d_yh, (const _Float16*)d_yl, (const float*)d_gap, (const float*)d_f1w,
                  (const float*)d_f1b, (const float*)d_f2w, (const float*)d_f2b, d_oh, d_ol, P, nbands, (long)n, ppb);
    if (dev_finish()) return -2;
    if (down(oh, d_oh, (size_t)out_halves * 2)) return -2;
    return down(ol, d_ol, (size_t)out_halves * 2);
}

}  // namespace

// k_wide_stem_hp<c0>: (hi, lo) crops fp16 [.][262][136][4] of crops_halves halves each (>= n crops: what follows the last crop is the
// caller's poison), w fp32 [c0][7][7][3] and bias [c0] as in the OSN1 blob (packed here by wide_pack_hp), (hi, lo) out of out_halves >= n *
// 2048 * c0 halves each, channels in the paired order
extern "C" int kat_hp_stem(int c0, const uint16_t* crops_h, const uint16_t* crops_l, long crops_halves, int n, const float* w, const float* bias,
                           uint16_t* out_h, uint16_t* out_l, long out_halves) {
    if (n < 1 || !crops_h || !crops_l || !w || !bias || !out_h || !out_l) return -1;
    if (crops_halves < (long)n * WSTEM_ROWS * WSTEM_COLS * 4 || out_halves < (long)n * 2048 * c0) return -1;
    if (c0 == 32) return run_stem<32>(crops_h, crops_l, crops_halves, n, w, bias, out_h, out_l, out_halves);
    if (c0 == 64) return run_stem<64>(crops_h, crops_l, crops_halves, n, w, bias, out_h, out_l, out_halves);
    return -1;
}

// k_gemm_hp<epi, bn, db>: (hi, lo) X [M][K] of x_halves halves per plane, (hi, lo) W [N][K], bias [N] or null, outputs of out_elems elements
// per plane: fp16 planes (epi 0, 1: >= M N; epi 2, 3: >= M / 4 * N) or ONE fp32 plane (epi 4: out_l null), (hi, lo) residual [M][N] of
// res_halves halves (epi 1), second pair X2 [M][K2] of x2_halves halves and W2 [N][K2] (epi 0; K2 = 0: none).  The instantiations
// wide_hp_forward's dispatch reaches: <0, 32 | 64 | 96 | 128, 1 | 2> and <1 .. 4, 128, 2>.
extern "C" int kat_hp_gemm(int epi, int bn, int db, const uint16_t* xh, const uint16_t* xl, long x_halves, const uint16_t* wh, const uint16_t* wl,
                           const float* bias, void* out_h, void* out_l, long out_elems, const uint16_t* res_h, const uint16_t* res_l, long res_halves,
                           int M, int N, int K, int relu, const uint16_t* x2h, const uint16_t* x2l, long x2_halves, const uint16_t* w2h,
                           const uint16_t* w2l, int K2) {
    if (M < 1 || N < 1 || K < 32 || K % 32 || K2 < 0 || K2 % 32 || !xh || !xl || !wh || !wl || !out_h) return -1;
    if (bn != 32 && bn != 64 && bn != 96 && bn != 128) return -1;
    if (N % bn || x_halves < (long)M * K) return -1;
    if (epi < 0 || epi > 4 || (epi != 0 && (bn != 128 || db != 2)) || (db != 1 && db != 2)) return -1;
    if ((epi == 4) != (out_l == nullptr)) return -1;
    if (epi == 1 ? (!res_h || !res_l || res_halves < (long)M * N) : (res_h || res_l)) return -1;
    if ((epi == 2 || epi == 3) && (M % 128 || !bias)) return -1;               // whole 128-row tiles of whole image-row pairs; the bias is read unconditionally
    if (K2 ? (epi != 0 || !x2h || !x2l || !w2h || !w2l || x2_halves < (long)M * K2) : (x2h || x2l || w2h || w2l)) return -1;
    const long need = (epi == 2 || epi == 3) ? (long)M / 4 * N : (long)M * N;
    if (out_elems < need) return -1;
    GemmArgs a{xh, xl, x_halves, wh, wl, bias, out_h, out_l, out_elems * (epi == 4 ? 4 : 2), res_h, res_l, res_halves, M, N, K, relu,
               x2h, x2l, x2_halves, w2h, w2l, K2};
    if (epi == 0) {
#define KAT_HP_G0(BN) if (bn == BN) return db == 1 ? run_gemm<0, BN, 1>(a) : run_gemm<0, BN, 2>(a)
        KAT_HP_G0(32); KAT_HP_G0(64); KAT_HP_G0(96); KAT_HP_G0(128);
#undef KAT_HP_G0
        return -1;
    }
    switch (epi) {
        case 1: return run_gemm<1, 128, 2>(a);
        case 2: return run_gemm<2, 128, 2>(a);
        case 3: return run_gemm<3, 128, 2>(a);
        default: return run_gemm<4, 128, 2>(a);
    }
}

#define KAT_HP_CHAIN_TABLE(X) \
    X(32, 32, 24, 4) X(64, 32, 24, 4) X(32, 16, 32, 0) X(64, 16, 32, 0) X(96, 16, 32, 0) X(32, 8, 16, 0) X(64, 8, 16, 0) X(96, 8, 16, 0) X(128, 8, 16, 0)

// ChainGeo<C, W, WR, HALO> of an instantiation wide_hp_chain launches: out[0 .. 2] = tiles per wave NT, band rows R, LDS bytes; -1 outside
extern "C" int kat_hp_chain_geo(int C, int W, int WR, int HALO, int* out) {
    if (!out) return -1;
#define KAT_HP_X(c, w, wr, h) if (C == c && W == w && WR == wr && HALO == h) { using G = ChainGeo<c, w, wr, h>; out[0] = G::NT; out[1] = G::R; out[2] = G::LDS_BYTES; return 0; }
    KAT_HP_CHAIN_TABLE(KAT_HP_X)
#undef KAT_HP_X
    return -1;
}

// k_chain_hp<C, W, WR, HALO>: (hi, lo) x1 [n][H W][C] of x_halves halves per plane, recs fp32: ten LightConv records in blob order (pw [C][C],
// dw [C][9], bias [C] each; packed here by wide_pack_hp), (hi, lo) y [4][n][H W][C] of y_halves halves per plane, gap fp32 [4][n][H / R][C]
// of gap_floats floats.  HALO = 4: H a multiple of the 16 band rows; HALO = 0: the window is the image, H == WR.
extern "C" int kat_hp_chain(int C, int W, int WR, int HALO, const uint16_t* x1h, const uint16_t* x1l, long x_halves, int n, int H, const float* recs,
                            uint16_t* yh, uint16_t* yl, long y_halves, float* gap, long gap_floats) {
    if (n < 1 || !x1h || !x1l || !recs || !yh || !yl || !gap || H < 1) return -1;
    const int R = WR - 2 * HALO;
    if (R < 1 || (HALO ? H % R != 0 : H != WR)) return -1;
    if (x_halves < (long)n * H * W * C || y_halves < 4L * n * H * W * C || gap_floats < 4L * n * (H / R) * C) return -1;
#define KAT_HP_X(c, w, wr, h) if (C == c && W == w && WR == wr && HALO == h) return run_chain<c, w, wr, h>(x1h, x1l, x_halves, n, H, recs, yh, yl, y_halves, gap, gap_floats);
    KAT_HP_CHAIN_TABLE(KAT_HP_X)
#undef KAT_HP_X
    return -1;
}

// k_gate_sum4_hp<C>: (hi, lo) y [4][n][P][C], gap fp32 [4][n][nbands][C], fc1 [C / 16][C] + [C / 16], fc2 [C][C / 16] + [C] (logical channel
// order), (hi, lo) out of out_halves >= n P C halves per plane; pixel blocks of 128
extern "C" int kat_hp_gate(int C, const uint16_t* yh, const uint16_t* yl, const float* gap, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                           const float* fc2_b, uint16_t* out_h, uint16_t* out_l, long out_halves, int P, int nbands, int n) {
    if (n < 1 || P < 1 || nbands < 1 || !yh || !yl || !gap || !fc1_w || !fc1_b || !fc2_w || !fc2_b || !out_h || !out_l) return -1;
    if (out_halves < (long)n * P * C) return -1;
    switch (C) {
        case 32: return run_gate<32>(yh, yl, gap, fc1_w, fc1_b, fc2_w, fc2_b, out_h, out_l, out_halves, P, nbands, n);
        case 64: return run_gate<64>(yh, yl, gap, fc1_w, fc1_b, fc2_w, fc2_b, out_h, out_l, out_halves, P, nbands, n);
        case 96: return run_gate<96>(yh, yl, gap, fc1_w, fc1_b, fc2_w, fc2_b, out_h, out_l, out_halves, P, nbands, n);
        case 128: return run_gate<128>(yh, yl, gap, fc1_w, fc1_b, fc2_w, fc2_b, out_h, out_l, out_halves, P, nbands, n);
        default: return -1;
    }
}

// k_wide_gap_hp: (hi, lo) in [n][P][C], (hi, lo) out of out_halves >= n C halves per plane
extern "C" int kat_hp_gap(const uint16_t* in_h, const uint16_t* in_l, uint16_t* out_h, uint16_t* out_l, long out_halves, int n, int P, int C) {
    if (n < 1 || P < 1 || C < 8 || C % 8 || !in_h || !in_l || !out_h || !out_l || out_halves < (long)n * C) return -1;
    Dev d;
    bool ok = true;
    _Float16* d_ih = d.up<_Float16>(in_h, (size_t)n * P * C * 2, &ok);
    _Float16* d_il = d.up<_Float16>(in_l, (size_t)n * P * C * 2, &ok);
    _Float16* d_oh = d.up<_Float16>(out_h, (size_t)out_halves * 2, &ok);
    _Float16* d_ol = d.up<_Float16>(out_l, (size_t)out_halves * 2, &ok);
    if (!ok) return -2;
    const long g8 = (long)n * (C / 8);
    KAT_LAUNCH_XY(k_wide_gap_hp, (int)((g8 + 255) / 256), 1, 256, 0, (const _Float16*)d_ih, (const _Float16*)d_il, d_oh, d_ol, P, C, g8);
    if (dev_finish()) return -2;
    if (down(out_h, d_oh, (size_t)out_halves * 2)) return -2;
    return down(out_l, d_ol, (size_t)out_halves * 2);
}

// HOST ONLY: wide_pack_hp of an OSN1 blob (fp32, blob_floats == the layout's total) for channels ch[4] and feat.  offs (68 longs): per block
// b at 9 b: conv1 wh, wl, bias, conv3 wh, wl, bias, down wh, wl (-1 without a downsample), chain; then at 54: trans[0] wh, wl, bias,
// trans[1] .., conv5 .., fc ..; at 66: stem_a, stem_b.  Returns the packed size in bytes (copied to `out` when out_bytes holds it), -1 when
// the family does not take the layout.
extern "C" long kat_hp_pack(const int* ch, int feat, const float* blob, long blob_floats, unsigned char* out, long out_bytes, long* offs) {
    if (!ch || !blob || !offs) return -1;
    const OsnetLayout L = make_osnet_layout(ch, feat);
    if (!wide_hp_supports(L) || blob_floats != L.total) return -1;
    const WideHpPack pk = wide_pack_hp(blob, L);
    for (int b = 0; b < 6; ++b) {
        const BlockHp& B = pk.block[b];
        const long o[9] = {B.conv1.wh, B.conv1.wl, B.conv1.bias, B.conv3.wh, B.conv3.wl, B.conv3.bias, B.down.wh, B.down.wl, B.chain};
        for (int i = 0; i < 9; ++i) offs[9 * b + i] = o[i];
    }
    const GemmWHp* g[4] = {&pk.trans[0], &pk.trans[1], &pk.conv5, &pk.fc};
    for (int i = 0; i < 4; ++i) { offs[54 + 3 * i] = g[i]->wh; offs[55 + 3 * i] = g[i]->wl; offs[56 + 3 * i] = g[i]->bias; }
    offs[66] = pk.stem_a; offs[67] = pk.stem_b;
    if (out && out_bytes >= (long)pk.data.size()) std::memcpy(out, pk.data.data(), pk.data.size());
    return (long)pk.data.size();
}

// the blob offsets (in floats) of a layout, for the caller that fills a blob: per block b at 8 b: conv1_w, conv1_b, conv3_w, conv3_b, down_w,
// down_b, cin, mid; at 48: trans_w[0], trans_b[0], trans_w[1], trans_b[1], conv5_w, conv5_b, fc_w, fc_b, stem_w, stem_b; returns the total
extern "C" long kat_hp_layout(const int* ch, int feat, long* offs) {
    if (!ch || !offs) return -1;
    const OsnetLayout L = make_osnet_layout(ch, feat);
    for (int b = 0; b < 6; ++b) {
        const BlockW& B = L.block[b];
        const long o[8] = {B.conv1_w, B.conv1_b, B.conv3_w, B.conv3_b, B.down_w, B.down_b, B.cin, B.mid};
        for (int i = 0; i < 8; ++i) offs[8 * b + i] = o[i];
    }
    const long t[10] = {L.trans_w[0], L.trans_b[0], L.trans_w[1], L.trans_b[1], L.conv5_w, L.conv5_b, L.fc_w, L.fc_b, L.stem_w, L.stem_b};
    for (int i = 0; i < 10; ++i) offs[48 + i] = t[i];
    return L.total;
}
