// TEST-ONLY known-answer harness for the fp32-grade OSNet-x0.25 kernels (ReID mode 2; boxmot_amd/csrc/reid_hp.hpp, included unchanged):
// k_crop_resize_rgbx_hl, k_stem_hp, k_stem_resize_fused_hp, the six k_osblock_hp instantiations and k_head_hp<128, 512>, every one
// launched ALONE on inputs of the caller's choosing.
//
// One extern "C" entry point per unit.  Each takes the packed weight blob of boxmot_amd.reid_weights.pack_osnet and host arrays with
// their sizes, packs the unit's weights with the product's own packers (make_blk_pack_hp, pack_osblock_hp, pack_pointwise_hp,
// pack_stem_hp, pack_stem_hp_fused, pack_fc_hp), copies everything to the device, launches as ReidNet::prepare_hp / forward_hp of
// reid_engine.hpp do (grid, block, dynamic LDS bytes, hipFuncSetAttribute per instantiation), copies the WHOLE output allocations back
// (guard rows included) and returns 0, or a negative status (-1: outside the kernel's contract or the caller's arrays, nothing launched;
// -2: a HIP call failed; -3: not an OSNet-x0.25 blob).  `count` < 0 launches with a null count pointer, otherwise with a device-side int.
//
// Built two ways, as clip_kat.hip: by hipcc for gfx950 (tests/test_gpu_reid_hp_kat.py), and with -DKAT_EMU -DEMU_DEFER_GLDS=1 by a host
// clang against tests/host_emu/hip_shim.hpp (tests/test_reid_hp_kat_emu.py).  -DBM_HP_* switches of reid_hp.hpp may be added to either
// build (reid_hp_kat_common.build_*(extra_flags=...)).  Nothing in boxmot_amd/ includes it.
#define KAT_EMU_STACK (1 << 20)
#include "kat_harness.hpp"

#include "../../boxmot_amd/csrc/reid_hp.hpp"

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
    int up(const unsigned char*& d, const std::vector<uint8_t>& v) {
        unsigned char* p;
        const int rc = up(p, v.data(), v.size());
        d = p;
        return rc;
    }
    // the device-side crop count, or null
    int count(const int*& d, int value) {
        int* p = nullptr;
        const int rc = value < 0 ? 0 : up(p, &value, sizeof(int));
        d = p;
        return rc;
    }
};

int down(void* h, const void* d, size_t bytes) { return dev_finish() ? -2 : d2h(h, d, bytes); }

struct Net { const float* w; OsnetLayout L; };
int parse(const float* blob, long n_floats, Net& net) {
    if (!blob || n_floats < REID_HEADER_INTS) return -3;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(blob);
    if (hdr[0] != REID_MAGIC || hdr[1] != 16 || hdr[2] != 64 || hdr[3] != 96 || hdr[4] != 128) return -3;
    const int ch[4] = {hdr[1], hdr[2], hdr[3], hdr[4]};
    net.L = make_osnet_layout(ch, hdr[5]);
    if (n_floats != REID_HEADER_INTS + net.L.total) return -3;
    net.w = blob + REID_HEADER_INTS;
    return 0;
}

constexpr long CROP_HALVES = (long)STEM_ROWS * STEM_COLS * 4;       // one (hi or lo) RGBX plane of a crop
const float MEAN_RGB[3] = {0.485f, 0.456f, 0.406f}, STD_RGB[3] = {0.229f, 0.224f, 0.225f};       // base_backend.py:189-193

// one frame for every crop: the device-side frame table and crop -> stream map of the crop kernels
struct FrameSrc {
    const uint8_t* const* frames = nullptr;
    const int* streams = nullptr;
    const float* boxes = nullptr;
    int up(Bufs& b, const uint8_t* frame, int W, int H, const float* bx, int n) {
        uint8_t* df;
        if (b.up(df, frame, (size_t)W * H * 3)) return -2;
        const uint8_t* table[1] = {df};
        const uint8_t** dt;
        if (b.up(dt, table, sizeof(table))) return -2;
        std::vector<int> zero(n, 0);
        int* ds;
        float* db;
        if (b.up(ds, zero.data(), (size_t)n * 4) || b.up(db, bx, (size_t)n * 4 * 4)) return -2;
        frames = dt; streams = ds; boxes = db;
        return 0;
    }
};

// block b of the network (0 .. 5): stage, input width, downsample shortcut
const int BLK_STAGE[6] = {0, 0, 1, 1, 2, 2}, BLK_CIN[6] = {16, 64, 64, 96, 96, 128}, BLK_DOWN[6] = {1, 0, 1, 0, 1, 0};

struct PackedBlock {
    BlkPackHP bp;
    std::vector<uint8_t> host;
    const unsigned char* dev = nullptr;
    int pack(Bufs& b, const Net& net, int blk) {
        bp = make_blk_pack_hp(BLK_STAGE[blk], BLK_CIN[blk], BLK_DOWN[blk]);
        pack_osblock_hp(net.w, net.L.block[blk], bp, host);
        return b.up(dev, host);
    }
};

// k_osblock_hp<STAGE, CIN, DOWN, TRANS> alone: in (hi, lo) [n][P][CIN] -> out (hi, lo) [n][P or P / 4][COUT] (+ guard)
template <int STAGE, int CIN, bool DOWN, bool TRANS>
int run_block(const Net& net, int blk, int trans, const uint16_t* in_h, const uint16_t* in_l, long in_halves, uint16_t* out_h,
              uint16_t* out_l, long out_halves, int n, int count) {
    using G = GeoHP<STAGE>;
    const long out_px = TRANS ? G::P / 4 : G::P;
    if (n < 1 || !in_h || !in_l || !out_h || !out_l || in_halves < (long)n * G::P * CIN || out_halves < (long)n * out_px * G::COUT) return -1;
    if (KAT_SET_LDS((k_osblock_hp<STAGE, CIN, DOWN, TRANS>), G::LDS_BYTES)) return -2;
    Bufs b;
    PackedBlock bw;
    if (bw.pack(b, net, blk)) return -2;
    std::vector<uint8_t> wt;
    const unsigned char* dwt = nullptr;
    if (TRANS) {
        pack_pointwise_hp(net.w + net.L.trans_w[trans], net.w + net.L.trans_b[trans], G::COUT, G::COUT, wt, 0.25f);
        if (b.up(dwt, wt)) return -2;
    }
    _Float16 *dih, *dil, *doh, *dol;
    const int* dcount;
    if (b.up(dih, in_h, (size_t)in_halves * 2) || b.up(dil, in_l, (size_t)in_halves * 2) || b.up(doh, out_h, (size_t)out_halves * 2) ||
        b.up(dol, out_l, (size_t)out_halves * 2) || b.count(dcount, count))
        return -2;
    const BlkPackHP bp = bw.bp;
    const unsigned char* dw = bw.dev;
    float* no_scratch = nullptr;            // the hand-over tensors belong to the EMIT / RECON pair only
    const BlkLinkHP link{};
    KAT_LAUNCH((k_osblock_hp<STAGE, CIN, DOWN, TRANS>), n, 64 * G::NWAVES, (size_t)G::LDS_BYTES, dih, dil, doh, dol, dw, bp, dcount,
               no_scratch, dwt, link);
    if (down(out_h, doh, (size_t)out_halves * 2)) return -2;
    return d2h(out_l, dol, (size_t)out_halves * 2);
}

}  // namespace

// k_crop_resize_rgbx_hl ("resize" preprocessing): frame (H, W, 3) uint8 BGR + boxes [n][4] -> (hi, lo) RGBX planes [n][262][136][4] (+ guard);
// the kernel writes the 256 x 128 interior only
extern "C" int kat_hp_crop(const uint8_t* frame, int W, int H, const float* boxes, uint16_t* out_h, uint16_t* out_l, long out_halves, int n,
                           int count) {
    if (n < 1 || W < 1 || H < 1 || !frame || !boxes || !out_h || !out_l || out_halves < (long)n * CROP_HALVES) return -1;
    float lut[768];
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {         // the engine's table: each operation rounded to fp32 (base_backend.py:183-193)
            volatile float a = (float)v / 255.0f;
            volatile float d = a - MEAN_RGB[c];
            lut[c * 256 + v] = d / STD_RGB[c];
        }
    Bufs b;
    FrameSrc fs;
    float* dlut;
    _Float16 *doh, *dol;
    const int* dcount;
    if (fs.up(b, frame, W, H, boxes, n) || b.up(dlut, lut, sizeof(lut)) || b.up(doh, out_h, (size_t)out_halves * 2) ||
        b.up(dol, out_l, (size_t)out_halves * 2) || b.count(dcount, count))
        return -2;
    const float* lp = dlut;
    KAT_LAUNCH_XY(k_crop_resize_rgbx_hl, n, REID_IN_H / 16, REID_IN_W, 0, fs.frames, fs.streams, fs.boxes, 4, W, H, lp, doh, dol, 16, dcount, 0);
    if (down(out_h, doh, (size_t)out_halves * 2)) return -2;
    return d2h(out_l, dol, (size_t)out_halves * 2);
}

// k_stem_hp: (hi, lo) RGBX planes [n][262][136][4] -> (hi, lo) [n][2048][16] (+ guard)
extern "C" int kat_hp_stem(const float* blob, long n_floats, const uint16_t* in_h, const uint16_t* in_l, long in_halves, uint16_t* out_h,
                           uint16_t* out_l, long out_halves, int n, int count) {
    Net net;
    if (parse(blob, n_floats, net)) return -3;
    if (n < 1 || !in_h || !in_l || !out_h || !out_l || in_halves < (long)n * CROP_HALVES || out_halves < (long)n * 2048 * 16) return -1;
    std::vector<uint8_t> wst;
    pack_stem_hp(net.w + net.L.stem_w, net.w + net.L.stem_b, wst);
    Bufs b;
    const unsigned char* dw;
    _Float16 *dih, *dil, *doh, *dol;
    const int* dcount;
    if (b.up(dw, wst) || b.up(dih, in_h, (size_t)in_halves * 2) || b.up(dil, in_l, (size_t)in_halves * 2) ||
        b.up(doh, out_h, (size_t)out_halves * 2) || b.up(dol, out_l, (size_t)out_halves * 2) || b.count(dcount, count))
        return -2;
    KAT_LAUNCH(k_stem_hp, n, 512, 0, dih, dil, doh, dol, dw, dcount);
    if (down(out_h, doh, (size_t)out_halves * 2)) return -2;
    return d2h(out_l, dol, (size_t)out_halves * 2);
}

// k_stem_resize_fused_hp: frame + boxes -> (hi, lo) [n][2048][16] (+ guard), the normalisation folded into the weights
extern "C" int kat_hp_stem_fused(const float* blob, long n_floats, const uint8_t* frame, int W, int H, const float* boxes, uint16_t* out_h,
                                 uint16_t* out_l, long out_halves, int n, int count) {
    Net net;
    if (parse(blob, n_floats, net)) return -3;
    if (n < 1 || W < 1 || H < 1 || !frame || !boxes || !out_h || !out_l || out_halves < (long)n * 2048 * 16) return -1;
    if (KAT_SET_LDS(k_stem_resize_fused_hp, STEM2_LDS_HP)) return -2;
    std::vector<uint8_t> wst;
    pack_stem_hp_fused(net.w + net.L.stem_w, net.w + net.L.stem_b, MEAN_RGB, STD_RGB, wst);
    Bufs b;
    FrameSrc fs;
    const unsigned char* dw;
    _Float16 *doh, *dol;
    const int* dcount;
    if (fs.up(b, frame, W, H, boxes, n) || b.up(dw, wst) || b.up(doh, out_h, (size_t)out_halves * 2) ||
        b.up(dol, out_l, (size_t)out_halves * 2) || b.count(dcount, count))
        return -2;
    KAT_LAUNCH(k_stem_resize_fused_hp, n, 512, (size_t)STEM2_LDS_HP, fs.frames, fs.streams, fs.boxes, 4, W, H, doh, dol, dw, dcount);
    if (down(out_h, doh, (size_t)out_halves * 2)) return -2;
    return d2h(out_l, dol, (size_t)out_halves * 2);
}

// The stage-0 pair as forward_hp runs it: k_osblock_hp<0, 16, true, false, true, false> (EMIT: conv2.0, hands over `x1s` and `x2s`, fp32
// [n][128 tiles][64 lanes][4] (+ guard), copied back right after this launch) and then k_osblock_hp<0, 64, false, true, false, true>
// (RECON: conv2.1 + the stage's transition + 2 x 2 average pool on the SAME input planes and the two hand-over tensors) -> (hi, lo)
// [n][512][64] (+ guard).
extern "C" int kat_hp_stage0_pair(const float* blob, long n_floats, const uint16_t* in_h, const uint16_t* in_l, long in_halves, float* x1s,
                                  float* x2s, long hand_floats, uint16_t* out_h, uint16_t* out_l, long out_halves, int n, int count) {
    using G = GeoHP<0>;
    Net net;
    if (parse(blob, n_floats, net)) return -3;
    if (n < 1 || !in_h || !in_l || !x1s || !x2s || !out_h || !out_l || in_halves < (long)n * G::P * 16 ||
        hand_floats < (long)n * G::P * G::MIDP || out_halves < (long)n * (G::P / 4) * G::COUT)
        return -1;
    if (KAT_SET_LDS((k_osblock_hp<0, 16, true, false, true, false>), G::LDS_BYTES) ||
        KAT_SET_LDS((k_osblock_hp<0, 64, false, true, false, true>), G::LDS_BYTES))
        return -2;
    Bufs b;
    PackedBlock w0, w1;
    std::vector<uint8_t> wt;
    pack_pointwise_hp(net.w + net.L.trans_w[0], net.w + net.L.trans_b[0], 64, 64, wt, 0.25f);
    const unsigned char* dwt;
    _Float16 *dih, *dil, *doh, *dol;
    float *dx1, *dx2;
    const int* dcount;
    if (w0.pack(b, net, 0) || w1.pack(b, net, 1) || b.up(dwt, wt) || b.up(dih, in_h, (size_t)in_halves * 2) ||
        b.up(dil, in_l, (size_t)in_halves * 2) || b.up(dx1, x1s, (size_t)hand_floats * 4) || b.up(dx2, x2s, (size_t)hand_floats * 4) ||
        b.up(doh, out_h, (size_t)out_halves * 2) || b.up(dol, out_l, (size_t)out_halves * 2) || b.count(dcount, count))
        return -2;
    const BlkPackHP bp0 = w0.bp, bp1 = w1.bp;
    const unsigned char *d0 = w0.dev, *d1 = w1.dev, *none = nullptr;
    _Float16* no_out = nullptr;
    const BlkLinkHP emit{d1, bp1.conv1_a, bp1.conv1_b, 0, dx2}, recon{d0, bp0.conv3_a, bp0.conv3_b, bp0.down_a, dx2};
    KAT_LAUNCH((k_osblock_hp<0, 16, true, false, true, false>), n, 64 * G::NWAVES, (size_t)G::LDS_BYTES, dih, dil, no_out, no_out, d0, bp0,
               dcount, dx1, none, emit);
    if (down(x1s, dx1, (size_t)hand_floats * 4) || d2h(x2s, dx2, (size_t)hand_floats * 4)) return -2;
    KAT_LAUNCH((k_osblock_hp<0, 64, false, true, false, true>), n, 64 * G::NWAVES, (size_t)G::LDS_BYTES, dih, dil, doh, dol, d1, bp1, dcount,
               dx1, dwt, recon);
    if (down(out_h, doh, (size_t)out_halves * 2)) return -2;
    return d2h(out_l, dol, (size_t)out_halves * 2);
}

// blocks 2 .. 5 alone: conv3.0 [n][512][64] -> [n][512][96]; conv3.1 + transition + pool [n][512][96] -> [n][128][96];
// conv4.0 [n][128][96] -> [n][128][128]; conv4.1 [n][128][128] -> [n][128][128]
extern "C" int kat_hp_block(int blk, const float* blob, long n_floats, const uint16_t* in_h, const uint16_t* in_l, long in_halves,
                            uint16_t* out_h, uint16_t* out_l, long out_halves, int n, int count) {
    Net net;
    if (parse(blob, n_floats, net)) return -3;
    switch (blk) {
        case 2: return run_block<1, 64, true, false>(net, 2, -1, in_h, in_l, in_halves, out_h, out_l, out_halves, n, count);
        case 3: return run_block<1, 96, false, true>(net, 3, 1, in_h, in_l, in_halves, out_h, out_l, out_halves, n, count);
        case 4: return run_block<2, 96, true, false>(net, 4, -1, in_h, in_l, in_halves, out_h, out_l, out_halves, n, count);
        case 5: return run_block<2, 128, false, false>(net, 5, -1, in_h, in_l, in_halves, out_h, out_l, out_halves, n, count);
    }
    return -1;
}

// k_head_hp<128, 512>: (hi, lo) [n][128][128] -> out fp32 [out_total_rows][512]; out_rows: n row indices below out_total_rows, or null
extern "C" int kat_hp_head(const float* blob, long n_floats, const uint16_t* in_h, const uint16_t* in_l, long in_halves, float* out,
                           long out_total_rows, const int* out_rows, int n, int count) {
    Net net;
    if (parse(blob, n_floats, net)) return -3;
    if (n < 1 || !in_h || !in_l || !out || in_halves < (long)n * 128 * 128) return -1;
    for (int i = 0; i < n; ++i)
        if ((out_rows ? (long)out_rows[i] : (long)i) >= out_total_rows || (out_rows && out_rows[i] < 0)) return -1;
    std::vector<uint8_t> w5, wfc;
    pack_pointwise_hp(net.w + net.L.conv5_w, net.w + net.L.conv5_b, 128, 128, w5);
    pack_fc_hp(net.w + net.L.fc_w, net.w + net.L.fc_b, 512, 128, wfc);
    Bufs b;
    const unsigned char *d5, *dfc;
    _Float16 *dih, *dil;
    float* dout;
    int* drows;
    const int* dcount;
    const size_t out_bytes = (size_t)out_total_rows * 512 * 4;
    if (b.up(d5, w5) || b.up(dfc, wfc) || b.up(dih, in_h, (size_t)in_halves * 2) || b.up(dil, in_l, (size_t)in_halves * 2) ||
        b.up(dout, out, out_bytes) || b.up(drows, out_rows, (size_t)n * 4) || b.count(dcount, count))
        return -2;
    const int* rows = drows;
    KAT_LAUNCH((k_head_hp<128, 512>), (n + HEAD_NB - 1) / HEAD_NB, 256, 0, dih, dil, d5, dfc, dout, rows, dcount, n);
    return down(out, dout, out_bytes);
}

// the geometry the cases are built from: waves per workgroup of stage `stage` (the seams between the waves' row strips)
extern "C" int kat_hp_nwaves(int stage) { return stage == 0 ? GeoHP<0>::NWAVES : (stage == 1 ? GeoHP<1>::NWAVES : GeoHP<2>::NWAVES); }
