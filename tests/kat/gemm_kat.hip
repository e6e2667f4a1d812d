// TEST-ONLY known-answer harness for the fp16 GEMM family (boxmot_amd/csrc/gemm_f16.hpp, included unchanged).
//
// One extern "C" entry point per kernel kind (k_gemm_f16<EPI, BN>, k_gemm_f16_glds<EPI, BK>, k_gemm_f16_256<EPI>) and one per product
// dispatch (ClipNet::gemm of clip_engine.hpp, WideOsNet::gemm of osnet_wide.hpp): each takes host arrays, copies them to the device,
// launches with the product's grid formula, block size, dynamic-LDS size and hipFuncSetAttribute (once per instantiation), copies
// the WHOLE output allocation back (guard rows included) and returns 0, or a negative status (-1: outside the kernel's contract,
// nothing launched; -2: a HIP call failed).
//
// Built two ways: by hipcc for gfx950 (tests/test_gpu_gemm_kat.py), and with -DKAT_EMU by a host clang against tests/host_emu/hip_shim.hpp,
// where the same kernels run on CPU threads (tests/test_gemm_kat_emu.py).  Nothing in boxmot_amd/ includes this file.
#include "kat_harness.hpp"

#include "../../boxmot_amd/csrc/gemm_f16.hpp"

using namespace bm;

namespace {

// the operands of one launch, host side.  x_rows / res_rows >= M (rows beyond M are the caller's poison), c_bytes = the whole output
// allocation (in-contract rows followed by guard rows), copied in before and out after the launch.
struct KatArgs {
    const uint16_t* X; long x_rows;
    const uint16_t* W;
    const float* bias;
    void* C; long c_bytes;
    const uint16_t* res; long res_rows;
    int M, N, K, relu;
    const uint16_t* X2; long x2_rows;
    const uint16_t* W2;
    int K2, pool_w;
};

// device copies of a KatArgs; freed on scope exit
struct Dev {
    _Float16 *X = nullptr, *W = nullptr, *res = nullptr, *X2 = nullptr, *W2 = nullptr;
    float* bias = nullptr;
    void* C = nullptr;
    std::vector<void*> owned;
    ~Dev() { for (void* p : owned) dev_free(p); }
    template <class T>
    int up(T*& d, const void* h, size_t bytes) {
        if (!h) { d = nullptr; return 0; }
        void* p = nullptr;
        if (dev_alloc(&p, bytes)) return -2;
        owned.push_back(p);
        d = static_cast<T*>(p);
        return h2d(p, h, bytes);
    }
    int upload(const KatArgs& a) {
        if (up(X, a.X, (size_t)a.x_rows * a.K * 2) || up(W, a.W, (size_t)a.N * a.K * 2) || up(bias, a.bias, (size_t)a.N * 4) ||
            up(C, a.C, (size_t)a.c_bytes) || up(res, a.res, (size_t)a.res_rows * a.N * 2))
            return -2;
        if (a.K2 && (up(X2, a.X2, (size_t)a.x2_rows * a.K2 * 2) || up(W2, a.W2, (size_t)a.N * a.K2 * 2))) return -2;
        return 0;
    }
    int download(const KatArgs& a) {
        if (dev_finish()) return -2;
        return d2h(a.C, C, (size_t)a.c_bytes);
    }
};

// the bytes the kernel may touch in C: M rows of N (fp32 for EPI 2 / 3), or M / 4 pooled rows (EPI 5 / 6)
long out_bytes(int epi, long M, int N) {
    if (epi == 5 || epi == 6) return M / 4 * N * 2;
    return M * N * (epi == 2 || epi == 3 ? 4 : 2);
}

// everything a launch reads or writes lies inside the caller's arrays
bool sane(const KatArgs& a, int epi) {
    if (a.M < 1 || a.N < 1 || a.K < 0 || a.x_rows < a.M || a.c_bytes < out_bytes(epi, a.M, a.N)) return false;
    if (!a.X || !a.W || !a.C) return false;
    if (a.res && a.res_rows < a.M) return false;
    if (a.K2 && (!a.X2 || !a.W2 || a.x2_rows < a.M)) return false;
    return true;
}

template <int EPI, int BN>
int run_f16(const KatArgs& a) {
    if (a.N % BN || a.K % GEMM_BK || a.K < GEMM_BK || a.K2 || a.pool_w || !sane(a, EPI)) return -1;
    Dev d;
    if (d.upload(a)) return -2;
    const long mt = (a.M + GEMM_BM - 1) / GEMM_BM;
    KAT_LAUNCH((k_gemm_f16<EPI, BN>), mt * (a.N / BN), 256, 0, d.X, d.W, d.bias, d.C, d.res, a.M, a.N, a.K, a.relu);
    return d.download(a);
}

template <int EPI, int BK>
int run_glds(const KatArgs& a) {
    if (a.N % GEMM_BN || a.K % BK || a.K < BK || a.K2 % BK || !sane(a, EPI)) return -1;
    if ((EPI == 5 || EPI == 6) != (a.pool_w != 0)) return -1;
    if (a.pool_w && (a.pool_w != (EPI == 5 ? 32 : 16) || a.M % (2 * a.pool_w) || a.M % GEMM_BM)) return -1;
    if (KAT_SET_LDS((k_gemm_f16_glds<EPI, BK>), gemm_glds_lds_bytes<BK>())) return -2;
    Dev d;
    if (d.upload(a)) return -2;
    GemmExt ext;
    ext.X2 = d.X2; ext.W2 = d.W2; ext.K2 = a.K2; ext.pool_w = a.pool_w;
    const long mt = (a.M + GEMM_BM - 1) / GEMM_BM;
    KAT_LAUNCH((k_gemm_f16_glds<EPI, BK>), mt * (a.N / GEMM_BN), 256, gemm_glds_lds_bytes<BK>(), d.X, d.W, d.bias, d.C, d.res, a.M, a.N, a.K,
               a.relu, ext);
    return d.download(a);
}

template <int EPI>
int run_256(const KatArgs& a) {
    if (a.N % 256 || a.K % 64 || a.K < 64 || a.K2 || a.pool_w || !sane(a, EPI)) return -1;
    if (KAT_SET_LDS((k_gemm_f16_256<EPI>), GEMM256_LDS_BYTES)) return -2;
    Dev d;
    if (d.upload(a)) return -2;
    KAT_LAUNCH((k_gemm_f16_256<EPI>), ((a.M + 255) / 256) * (a.N / 256), 512, GEMM256_LDS_BYTES, d.X, d.W, d.bias, d.C, d.res, a.M, a.N,
               a.K, a.relu);
    return d.download(a);
}

template <template <int> class F>
int by_epi(int epi, const KatArgs& a) {
    switch (epi) {
        case 0: return F<0>::run(a);
        case 1: return F<1>::run(a);
        case 2: return F<2>::run(a);
        case 3: return F<3>::run(a);
        case 4: return F<4>::run(a);
        default: return -1;
    }
}
template <int EPI> struct F16_128 { static int run(const KatArgs& a) { return run_f16<EPI, 128>(a); } };
template <int EPI> struct Glds64 { static int run(const KatArgs& a) { return run_glds<EPI, 64>(a); } };
template <int EPI> struct G256 { static int run(const KatArgs& a) { return run_256<EPI>(a); } };

KatArgs args(const uint16_t* X, long x_rows, const uint16_t* W, const float* bias, void* C, long c_bytes, const uint16_t* res, long res_rows,
             int M, int N, int K, int relu) {
    return KatArgs{X, x_rows, W, bias, C, c_bytes, res, res_rows, M, N, K, relu, nullptr, 0, nullptr, 0, 0};
}

}  // namespace

#define KAT_COMMON_PARAMS                                                                                                           \
    const uint16_t *X, long x_rows, const uint16_t *W, const float *bias, void *C, long c_bytes, const uint16_t *res, long res_rows, \
        int M, int N, int K, int relu
#define KAT_COMMON_ARGS X, x_rows, W, bias, C, c_bytes, res, res_rows, M, N, K, relu

// k_gemm_f16<EPI, BN>: the instantiations the product launches -- <4, 32 | 64 | 96> (WideOsNet::gemm), <0..3, 128> (ClipNet::gemm, K % 64 != 0)
extern "C" int kat_gemm_f16(int epi, int bn, KAT_COMMON_PARAMS) {
    const KatArgs a = args(KAT_COMMON_ARGS);
    if (bn == 128) return by_epi<F16_128>(epi, a);
    if (epi != 4) return -1;
    if (bn == 32) return run_f16<4, 32>(a);
    if (bn == 64) return run_f16<4, 64>(a);
    if (bn == 96) return run_f16<4, 96>(a);
    return -1;
}

// k_gemm_f16_glds<EPI, BK>: <0..3, 64> (ClipNet::gemm, M < 1024), <3, 32> (the wide head), <4 | 5 | 6, 32> (WideOsNet::gemm; X2 / W2 / K2
// and pool_w are GemmExt)
extern "C" int kat_gemm_glds(int epi, int bk, KAT_COMMON_PARAMS, const uint16_t* X2, long x2_rows, const uint16_t* W2, int K2, int pool_w) {
    KatArgs a = args(KAT_COMMON_ARGS);
    a.X2 = X2; a.x2_rows = x2_rows; a.W2 = W2; a.K2 = K2; a.pool_w = pool_w;
    if (bk == 64) return a.K2 || a.pool_w ? -1 : by_epi<Glds64>(epi, a);
    if (bk != 32) return -1;
    switch (epi) {
        case 3: return run_glds<3, 32>(a);
        case 4: return run_glds<4, 32>(a);
        case 5: return run_glds<5, 32>(a);
        case 6: return run_glds<6, 32>(a);
        default: return -1;
    }
}

// k_gemm_f16_256<EPI>: <0, 1, 2> (ClipNet::gemm, M >= 1024), <3, 4> (promised by the header)
extern "C" int kat_gemm_256(int epi, KAT_COMMON_PARAMS) { return by_epi<G256>(epi, args(KAT_COMMON_ARGS)); }

// ClipNet::gemm's choice of kernel (clip_engine.hpp), restated: which kernel the product runs for (M, N, K).  Returns 256 / 64 / 128
// for k_gemm_f16_256 / k_gemm_f16_glds<EPI, 64> / k_gemm_f16<EPI, 128>, or -1 where the product throws.
extern "C" int kat_clip_route(long M, int N, int K) {
    if (N % GEMM_BN != 0 || K % GEMM_BK != 0) return -1;
    if (N % 256 == 0 && K % 64 == 0 && M >= 1024) return 256;
    return K % 64 == 0 ? 64 : 128;
}
extern "C" int kat_clip_gemm(int epi, KAT_COMMON_PARAMS) {
    const KatArgs a = args(KAT_COMMON_ARGS);
    switch (kat_clip_route(M, N, K)) {
        case 256: return by_epi<G256>(epi, a);
        case 64: return by_epi<Glds64>(epi, a);
        case 128: return by_epi<F16_128>(epi, a);
        default: return -1;
    }
}

// WideOsNet::gemm's choice of kernel (osnet_wide.hpp), restated: k_gemm_f16_glds<5 | 6, 32> (pool_w 32 | 16), <4, 32> (N % 128 == 0),
// else k_gemm_f16<4, 96 | 64 | 32>; -1 where the product throws
extern "C" int kat_wide_route(int N, int K, int K2, int pool_w) {
    if (K % GEMM_BK != 0 || N % 32 != 0) return -1;
    if (pool_w) return N % 128 != 0 || (pool_w != 16 && pool_w != 32) ? -1 : (pool_w == 32 ? 5 : 6);
    if (N % 128 == 0) return 4;
    if (K2) return -1;
    return N % 96 == 0 ? 96 : (N % 64 == 0 ? 64 : 32);
}
extern "C" int kat_wide_gemm(KAT_COMMON_PARAMS, const uint16_t* X2, long x2_rows, const uint16_t* W2, int K2, int pool_w) {
    KatArgs a = args(KAT_COMMON_ARGS);
    a.X2 = X2; a.x2_rows = x2_rows; a.W2 = W2; a.K2 = K2; a.pool_w = pool_w;
    switch (kat_wide_route(N, K, K2, pool_w)) {
        case 5: return run_glds<5, 32>(a);
        case 6: return run_glds<6, 32>(a);
        case 4: return run_glds<4, 32>(a);
        case 96: return run_f16<4, 96>(a);
        case 64: return run_f16<4, 64>(a);
        case 32: return run_f16<4, 32>(a);
        default: return -1;
    }
}
