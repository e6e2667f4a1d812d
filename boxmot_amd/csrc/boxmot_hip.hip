// C-ABI shared library of the MI355X BoT-SORT update path (include/boxmot_hip.h).
// Host side: opaque handles, buffer staging, kernel sequencing on one HIP stream.
// Device side: botsort_step.hpp (tracker), reid_kernels_v1.hpp / reid_fused.hpp (ReID).
// There is no CPU implementation behind these entry points: without a usable
// HIP device every call fails with an error message.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/boxmot_hip.h"
#include "../../include/boxmot_compat.h"
#include "botsort_alloc.hpp"
#include "botsort_step.hpp"
#include "deepocsort_step.hpp"
#include "strongsort_step.hpp"
#include "reid_engine.hpp"
#include "crop_list.hpp"
#include "cmc_ecc.hpp"
#include "cmc_sof.hpp"
#include "ingest_nv12.hpp"
#include "ingest_letterbox.hpp"
#include "ingest_letterbox_tiles.hpp"
#include "det_post.hpp"
#include "det_post_tiled.hpp"
#include "det_post_mask.hpp"
#include "det_post_labels.hpp"

namespace {

thread_local std::string g_last_error;

template <class F>
int guard(F&& f) {
    try {
        f();
        g_last_error.clear();
        return 1;
    } catch (const std::exception& e) {
        g_last_error = e.what();
    } catch (...) {
        g_last_error = "unknown failure in boxmot_hip";
    }
    return 0;
}

// Handle <-> device affinity (include/boxmot_hip.h, "Devices"): a handle lives on the HIP device that was current on the thread
// that created it (its tables, streams, events and engines are that device's); every entry point that takes a handle makes that
// device current for the duration of the call and restores the caller's device on exit, so one process can drive handles of
// several GPUs from any thread (SURVEY.md section 8(e)'s "one process, G HIP devices" layout) without a handle silently following
// the caller's current device.  The reference's threading contract (reid_capi.h:61-70): distinct handles on distinct threads.
struct DeviceBound {
    int device = -1;
    DeviceBound() { if (hipGetDevice(&device) != hipSuccess) device = -1; }
};

class DeviceScope {
    int prev_ = -1;
    bool switched_ = false;
public:
    explicit DeviceScope(int device) {
        if (device < 0) return;
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        if (prev_ != device) {
            if (hipSetDevice(device) != hipSuccess) throw std::runtime_error("boxmot_hip: cannot make the handle's device current (hipSetDevice failed)");
            switched_ = true;
        }
    }
    ~DeviceScope() { if (switched_ && prev_ >= 0) (void)hipSetDevice(prev_); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

template <class H, class F>
int guard_on(H* h, F&& f) {
    return guard([&]() {
        DeviceScope scope(h ? h->device : -1);
        f();
    });
}

// destroy on the handle's own device (streams / events / allocations are released where they were made)
template <class H>
void destroy_on(H* h) {
    if (!h) return;
    try {
        DeviceScope scope(h->device);
        delete h;
    } catch (...) {
        delete h;
    }
}

constexpr int STEP_THREADS = 512;
constexpr int SS_STEP_THREADS_BIG = 1024;     // StrongSORT frame step with max_tracks >= 1024

template <int NTHR, bool DBG = false>
__global__ void __launch_bounds__(NTHR) botsort_step_kernel(bm::BotSortStepArgs args) {
    __shared__ int s_int[bm::MAX_WAVES + 1];
    __shared__ double s_dbl[bm::MAX_WAVES];
    __shared__ float sA[bm::COST_TILE][bm::COST_KC + 1];
    __shared__ float sB[bm::COST_TILE][bm::COST_KC + 1];
    BM_DYNAMIC_LDS_T(unsigned char, dyn_lds);       // assignment-solver state, sized by lap_lds_bytes(cap, max_dets)
    bm::botsort_step_stream<NTHR, DBG>(args, args.stream_base + blockIdx.x, s_int, s_dbl, sA, sB, dyn_lds);
}

// the same frame step for oriented detections (botsort_step.hpp: namespace bm::obb)
template <int NTHR>
__global__ void __launch_bounds__(NTHR) botsort_obb_step_kernel(bm::BotSortStepArgs args) {
    __shared__ int s_int[bm::MAX_WAVES + 1];
    __shared__ double s_dbl[bm::MAX_WAVES];
    __shared__ float sA[bm::COST_TILE][bm::COST_KC + 1];
    __shared__ float sB[bm::COST_TILE][bm::COST_KC + 1];
    BM_DYNAMIC_LDS_T(unsigned char, dyn_lds);
    bm::obb::botsort_step_stream<NTHR>(args, args.stream_base + blockIdx.x, s_int, s_dbl, sA, sB, dyn_lds);
}

// BotSort._obb_detections_to_cmc_boxes (botsort.py:126-132 over STrack.obb_to_xyxy, botsort_track.py:159-174): the enclosing axis-aligned
// box of every oriented detection of stream blockIdx.x + s0 -- what the reference hands its camera-motion estimator as the mask boxes --
// from the four corners as cv2.boxPoints lays them out (fp32; w, h floored at 1e-4; the angle in degrees as the fp32 product np.degrees is)
__global__ void obb_enclosing_boxes_kernel(const float* dets, const int* n_dets, int max_dets, float* boxes, int s0) {
    const int s = s0 + blockIdx.x;
    const int n = n_dets[s] > 0 ? n_dets[s] : 0;
    const float* d = dets + (long)s * max_dets * bm::obb::DET_COLS;
    float* o = boxes + (long)s * max_dets * 4;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const float* r = d + j * bm::obb::DET_COLS;
        const double rect[5] = {(double)r[0], (double)r[1], (double)r[2] > 1e-4 ? (double)r[2] : 1e-4, (double)r[3] > 1e-4 ? (double)r[3] : 1e-4, (double)r[4]};
        double p[4][2];
        bm::obb::obb_corners_deg(rect, (double)(r[4] * (180.0f / 3.14159274f)), p);
        float x0 = (float)p[0][0], x1 = x0, y0 = (float)p[0][1], y1 = y0;
        for (int k = 1; k < 4; ++k) {
            const float x = (float)p[k][0], y = (float)p[k][1];
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        }
        o[j * 4 + 0] = x0; o[j * 4 + 1] = y0; o[j * 4 + 2] = x1; o[j * 4 + 3] = y1;
    }
}

template <int NTHR>
__global__ void __launch_bounds__(NTHR) deepocsort_step_kernel(bm::DocsStepArgs args) {
    __shared__ int s_int[bm::MAX_WAVES + 1];
    __shared__ double s_dbl[bm::MAX_WAVES];
    BM_DYNAMIC_LDS_T(unsigned char, dyn_lds);       // assignment-solver state, docs_lap_lds_bytes(cap, max_dets)
    bm::docs_step_stream<NTHR>(args, args.stream_base + blockIdx.x, s_int, s_dbl, dyn_lds);
}

// the same frame step for oriented detections: OC-SORT with is_obb (deepocsort_step.hpp: namespace bm::obb)
template <int NTHR>
__global__ void __launch_bounds__(NTHR) deepocsort_obb_step_kernel(bm::DocsStepArgs args) {
    __shared__ int s_int[bm::MAX_WAVES + 1];
    __shared__ double s_dbl[bm::MAX_WAVES];
    BM_DYNAMIC_LDS_T(unsigned char, dyn_lds);
    bm::obb::docs_step_stream<NTHR>(args, args.stream_base + blockIdx.x, s_int, s_dbl, dyn_lds);
}

template <int NTHR>
__global__ void __launch_bounds__(NTHR) strongsort_detnorm_kernel(bm::SsStepArgs args) {
    bm::ss_det_norm_block<NTHR>(args, args.stream_base + blockIdx.x, blockIdx.y, gridDim.y);
}

template <int NTHR>
__global__ void __launch_bounds__(NTHR) strongsort_bank_kernel(bm::SsStepArgs args) {
    __shared__ float sA[bm::SS_KC][bm::SS_TILE + 1];
    __shared__ float sB[bm::SS_KC][bm::SS_TILE + 1];
    __shared__ float sMin[16][bm::SS_TILE];
    bm::ss_bank_distance_block<NTHR>(args, args.stream_base + blockIdx.y, blockIdx.x, sA, sB, sMin);
}

template <int NTHR>
__global__ void __launch_bounds__(NTHR) strongsort_bank_mfma_kernel(bm::SsStepArgs args) {
    __shared__ __attribute__((aligned(16))) float lds[bm::SS_MFMA_LDS_FLOATS(NTHR)];
    bm::ss_bank_distance_block_mfma<NTHR>(args, args.stream_base + blockIdx.y, blockIdx.x, lds);
}

template <int NTHR>
__global__ void __launch_bounds__(NTHR) strongsort_step_kernel(bm::SsStepArgs args) {
    __shared__ int s_int[bm::MAX_WAVES + 1];
    __shared__ double s_dbl[bm::MAX_WAVES];
    BM_DYNAMIC_LDS_T(unsigned char, dyn_lds);       // assignment-solver state, ss_lsa_lds_bytes(max(cap, max_dets))
    bm::ss_step_stream<NTHR>(args, args.stream_base + blockIdx.x, s_int, s_dbl, dyn_lds);
}

// A backbone family that sizes its launches on the host (the wide OSNets, CLIP-ReID) and a caller that declared an upper bound on the
// step's crops (set_crop_bound): the list is filled up to the bound with copies of its first entry -- the same crop computes the same
// embedding and writes it to the same row -- so the launches are sized by the bound and the count never travels to the host.  A
// count above the bound raises `flag` (reported by the next synchronize) and switches the frame off for the step.
// `ndets_out` (the detection counts the frame step of this call reads) = the caller's counts, or -1 for EVERY stream when the count
// exceeds the bound: the step kernels treat a negative count as "stream not stepped in this call", so a frame whose crops did not all
// get an embedding changes no tracker state and returns no rows (round-4 advisor finding: it used to step with stale embeddings).
// `crop_geo` (oriented handles, else null): the geometry rows [..][8] are padded the same way.
__global__ void pad_crop_list_kernel(const int* crop_count, int bound, int* crop_stream, float* crop_boxes, int* crop_row, int* flag,
                                     const int* ndets_in, int* ndets_out, int n_streams, double* crop_geo = nullptr) {
    const int n = *crop_count;
    if (blockIdx.x == 0)
        for (int s = threadIdx.x; s < n_streams; s += blockDim.x) ndets_out[s] = n > bound ? -1 : ndets_in[s];
    if (n > bound) { if (threadIdx.x == 0 && blockIdx.x == 0) *flag = 1; return; }
    const int s0 = n > 0 ? crop_stream[0] : 0, r0 = n > 0 ? crop_row[0] : 0;
    float b0[4];
    for (int q = 0; q < 4; ++q) b0[q] = n > 0 ? crop_boxes[q] : 0.0f;
    double g0[8];
    if (crop_geo) {
        if (n > 0) for (int q = 0; q < 8; ++q) g0[q] = crop_geo[q];
        else { const float nan_box[5] = {NAN, 0.f, 0.f, 0.f, 0.f}; bm::obb_crop_geometry(nan_box, g0); }      // no crops at all: blank ones
    }
    for (int i = n + blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += gridDim.x * blockDim.x) {
        crop_stream[i] = s0; crop_row[i] = r0;
        for (int q = 0; q < 4; ++q) crop_boxes[i * 4 + q] = b0[q];
        if (crop_geo) for (int q = 0; q < 8; ++q) crop_geo[(long)i * 8 + q] = g0[q];
    }
}

}  // namespace

struct BoxMOTHipReID : DeviceBound {
    std::unique_ptr<bm::ReidEngine> engine;
    std::vector<void*> owned;
    hipStream_t stream = nullptr;
    uint8_t* d_frame = nullptr;
    size_t frame_bytes = 0;
    const uint8_t** d_frames = nullptr;
    int* d_crop_stream = nullptr;
    float* d_boxes = nullptr;
    float* d_feat = nullptr;
    double* d_obb = nullptr;                     // [max_crops][8]: out_w, out_h, inverse 2x3 map of oriented boxes (base_backend.py:91-117)
    bool obb = false;                            // the boxes of the last reid_stage were oriented (5 / 7 / 9 columns)
    int staged_n = -1, staged_rows = 0, staged_cols = 0;      // boxmot_reid_capi_preprocess -> process -> postprocess
    bool staged_done = false;
    // boxmot_hip_reid_*_batch: one device buffer per image of the call, the table of their pointers, the {W, H} table the `_sized`
    // kernels read (uploaded when a size differs from the one the table holds), and the crop -> image table of the pass.
    // A buffer grows to the largest image seen at its index and is never shrunk: a caller that varies the order of its frames
    // ends up with a buffer of its largest frame at every index (freed with the handle).
    std::vector<uint8_t*> batch_bufs;
    std::vector<size_t> batch_bytes;
    std::vector<int> batch_dims;                 // host copy of d_batch_dims
    const uint8_t** d_batch_frames = nullptr;
    int* d_batch_dims = nullptr;
    int* d_batch_crop_stream = nullptr;          // [max_crops]
    ~BoxMOTHipReID() {
        engine.reset();
        for (void* p : owned) (void)hipFree(p);
        for (uint8_t* p : batch_bufs) if (p) (void)hipFree(p);
        if (d_batch_frames) (void)hipFree(d_batch_frames);
        if (d_batch_dims) (void)hipFree(d_batch_dims);
        if (d_frame) (void)hipFree(d_frame);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// ECC camera-motion estimator (csrc/cmc_ecc.hpp): per stream two small grayscale images (previous / current), gradients, scratch
struct BoxMOTHipEcc : DeviceBound {
    int S = 0, rows = 0, cols = 0, h = 0, w = 0, max_iter = 100;
    double scale = 0.15, eps = 1e-5;
    hipStream_t stream = nullptr;
    std::vector<void*> owned;
    float *img = nullptr, *gx = nullptr, *gy = nullptr, *scratch = nullptr;      // img: [S][2][h * w]
    double* d_warp = nullptr; int* d_info = nullptr;
    const uint8_t** d_frames = nullptr;          // host-API staging: one device frame per stream
    std::vector<uint8_t*> frame_bufs;
    std::vector<int> cur;                        // per stream: which of its two image buffers holds the newest frame
    std::vector<char> has_prev;
    bool owns_stream = true;                     // false: launches on a tracker handle's stream (estimation inside update)
    ~BoxMOTHipEcc() {
        for (void* p : owned) (void)hipFree(p);
        for (auto p : frame_bufs) if (p) (void)hipFree(p);
        if (stream && owns_stream) (void)hipStreamDestroy(stream);
    }
};

// Sparse-optical-flow camera-motion estimator (csrc/cmc_sof.hpp): per stream the previous and the current frame's 8-bit pyramid and
// Scharr derivatives, the keypoints the next frame tracks, scratch of the corner detector
struct BoxMOTHipSof : DeviceBound {
    int S = 0, rows = 0, cols = 0, max_dets = 0;
    bm::SofLevels lv{};
    bm::SofParams prm{};
    bm::SofBuffers buf{};
    hipStream_t stream = nullptr;
    std::vector<void*> owned;
    float* d_dets = nullptr; int* d_ndets = nullptr;        // host-API staging: [S][max_dets][4], [S]
    const uint8_t** d_frames = nullptr;
    std::vector<uint8_t*> frame_bufs;
    bool owns_stream = true;
    ~BoxMOTHipSof() {
        for (void* p : owned) (void)hipFree(p);
        for (auto p : frame_bufs) if (p) (void)hipFree(p);
        if (stream && owns_stream) (void)hipStreamDestroy(stream);
    }
};

// Frame ingest ring: n_slots x n_streams page-locked host frames, their device twins, a copy stream and
// one "uploaded" + one "consumed" event per slot.  The caller decodes frame t + 1 straight into slot (t + 1) % n_slots while the
// kernels of frame t run; submit() queues the slot's H2D DMA on the copy stream, wait() makes the consuming stream wait for it,
// release() lets the next upload into the slot wait for the consumer -- no host synchronisation anywhere.
// An NV12 ring (format 1) keeps the host slots and a device staging twin in NV12 (1.5 bytes per pixel over PCIe) and converts into the
// same BGR device frames with one k_nv12_to_bgr launch behind the DMA on the copy stream (csrc/ingest_nv12.hpp).
struct BoxMOTHipIngest : DeviceBound {
    int n_slots = 0, n_streams = 0, rows = 0, cols = 0;
    int format = 0;                                 // 0: the host slots hold BGR frames, 1: NV12 frames
    size_t frame_bytes = 0;
    std::vector<int> srows, scols;                  // [n_streams]: image size of each stream
    std::vector<size_t> offs;                       // [n_streams + 1]: byte offset of each stream's frame inside a slot (one allocation, one DMA)
    std::vector<size_t> nv_offs;                    // NV12 rings: the same for the NV12 frames of the host slot and its staging twin
    hipStream_t copy_stream = nullptr;
    std::vector<uint8_t*> h_slot, d_slot;           // [n_slots]: n_streams contiguous frames each (h_slot: in the ring's format; d_slot: BGR)
    std::vector<uint8_t*> d_nv;                     // [n_slots] NV12 rings: device twin of h_slot
    std::vector<const uint8_t**> d_ptrs;            // [n_slots]: device table of n_streams frame pointers
    std::vector<std::vector<bm::Nv12Desc>> nv_desc; // [n_slots] NV12 rings: staging twin -> BGR frames, and that table on the device
    std::vector<bm::Nv12Desc*> d_desc;
    std::vector<bm::Nv12Desc*> h_ext, d_ext;        // [n_slots] submit_device_nv12: pinned staging of the caller's surfaces and its device twin
    std::vector<char> ext_used;
    std::vector<hipEvent_t> uploaded, consumed;
    std::vector<char> has_consumer;
    // letterbox (csrc/ingest_letterbox.hpp); all of it is made by the first boxmot_hip_ingest_letterbox call, none by a ring that never calls it
    struct LetterboxTable { int H, W, mode; std::vector<bm::LetterboxGeom> geom; std::vector<char> ok; bm::LetterboxGeom* d_geom; };
    std::vector<LetterboxTable> lb_tables;          // per (H, W, mode): the streams' geometry, on the host and on the device
    uint32_t* d_lb_lut[4] = {nullptr, nullptr, nullptr, nullptr};      // [2 * unit + dtype]: the 256 table entries
    std::vector<hipEvent_t> lb_done;                // [n_slots]: the slot's last letterbox launch
    std::vector<char> has_lb;
    // letterbox of rectangles (csrc/ingest_letterbox_tiles.hpp): per (H, W, mode, rectangles) the [n_streams][n_tiles] geometry
    struct TileTable { int H, W, mode, n_streams, n_tiles; std::vector<int> rects; bm::LetterboxTileGeom* d_geom; };
    std::vector<TileTable> lb_tile_tables;
    ~BoxMOTHipIngest() {
        if (copy_stream) (void)hipStreamSynchronize(copy_stream);
        for (auto e : lb_done) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
        for (auto& t : lb_tables) if (t.d_geom) (void)hipFree(t.d_geom);
        for (auto& t : lb_tile_tables) if (t.d_geom) (void)hipFree(t.d_geom);
        for (auto p : d_lb_lut) if (p) (void)hipFree(p);
        for (auto p : h_slot) if (p) (void)hipHostFree(p);
        for (auto p : d_slot) if (p) (void)hipFree(p);
        for (auto p : d_nv) if (p) (void)hipFree(p);
        for (auto p : d_ptrs) if (p) (void)hipFree(p);
        for (auto p : d_desc) if (p) (void)hipFree(p);
        for (auto p : h_ext) if (p) (void)hipHostFree(p);
        for (auto p : d_ext) if (p) (void)hipFree(p);
        for (auto e : uploaded) (void)hipEventDestroy(e);
        for (auto e : consumed) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

// The geometry table of a detection post-processing handle, G per entry: the device array, what it holds, and the pinned staging
// of its uploads -- two buffers used in turn, an event each.  A steady-state run finds the table unchanged and copies nothing.
template <class G>
struct DetPostGeomTable {
    G* d = nullptr;                                 // [n of create()]: every stream of the handle
    G* h[2] = {nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr};
    int uploads = 0, valid = 0;                     // uploads so far; the streams whose device entries equal `held`
    std::vector<G> held;
    DetPostGeomTable() = default;
    DetPostGeomTable(const DetPostGeomTable&) = delete;
    DetPostGeomTable& operator=(const DetPostGeomTable&) = delete;
    void create(size_t n) {
        void* p = nullptr;
        BM_HIP(hipMalloc(&p, n * sizeof(G))); d = static_cast<G*>(p);
        for (int k = 0; k < 2; ++k) {
            BM_HIP(hipHostMalloc(&p, n * sizeof(G), hipHostMallocDefault)); h[k] = static_cast<G*>(p);
            BM_HIP(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
        }
        held.resize(n);
    }
    // the entries of the first n_streams streams become g, by a copy on `st` unless the device holds them already
    void set(const std::vector<G>& g, int n_streams, hipStream_t st) {
        if (n_streams <= valid && std::memcmp(g.data(), held.data(), g.size() * sizeof(G)) == 0) return;
        const int k = uploads & 1;
        if (uploads >= 2) BM_HIP(hipEventSynchronize(copied[k]));      // (two uploads ago: long done)
        std::memcpy(h[k], g.data(), g.size() * sizeof(G));
        BM_HIP(hipMemcpyAsync(d, h[k], g.size() * sizeof(G), hipMemcpyHostToDevice, st));
        BM_HIP(hipEventRecord(copied[k], st));
        uploads += 1;
        std::copy(g.begin(), g.end(), held.begin());
        if (valid < n_streams) valid = n_streams;
    }
    ~DetPostGeomTable() {                           // (the handle has waited for its last run)
        for (auto e : copied) if (e) (void)hipEventDestroy(e);
        for (auto p : h) if (p) (void)hipHostFree(p);
        if (d) (void)hipFree(d);
    }
};

// Detection post-processing (csrc/det_post.hpp): the handle owns the per-anchor scratch, the geometry table and the counters
struct BoxMOTHipDetPost : DeviceBound {
    BoxMOTHipDetPostConfig cfg{};
    int obb = 0, nms_mode = 0, regularize = 0;      // an oriented handle (boxmot_hip_detpost_create_obb): 7-column rows
    uint32_t* d_keys = nullptr;                     // [n_streams][n_anchors]
    int* d_cls = nullptr;                           // [n_streams][n_anchors]
    int* d_counters = nullptr;                      // [n_streams][3]
    uint8_t* d_allow = nullptr;                     // [n_classes] or null
    hipEvent_t done = nullptr;                      // the last run: the next one (on any stream) and counters() wait for it
    bool ran = false;
    // a tiled handle (boxmot_hip_detpost_create_tiled, csrc/det_post_tiled.hpp): the scratch is [n_streams * n_tiles][n_anchors] and the
    // geometry is per (stream, tile).  Of the two tables only the one of the handle's kind is created.
    int n_tiles = 0, merge = 0;
    DetPostGeomTable<bm::DetPostGeom> geom;         // [n_streams]
    DetPostGeomTable<bm::DetPostTileGeom> tgeom;    // [n_streams][n_tiles]
    // a handle with per-anchor extras (boxmot_hip_detpost_create_extra, csrc/det_post_extra.hpp), tiled or not
    int n_extra = 0, extra_kind = 0;
    int* d_src = nullptr;                           // [n_streams][max_det]: where the source anchors go when the caller gives no d_src
    // a mask handle (boxmot_hip_detpost_create_mask, csrc/det_post_mask.hpp): an extras handle of kind "raw" with these; mask_h 0: none
    int mask_h = 0, mask_w = 0;
    float mask_wr = 0.0f, mask_hr = 0.0f;           // (float)mask_w / (float)in_w, (float)mask_h / (float)in_h
    ~BoxMOTHipDetPost() {
        if (done) { if (ran) (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
        if (d_src) (void)hipFree(d_src);
        if (d_keys) (void)hipFree(d_keys);
        if (d_cls) (void)hipFree(d_cls);
        if (d_counters) (void)hipFree(d_counters);
        if (d_allow) (void)hipFree(d_allow);
    }
};

namespace {
struct DetPostLaunch {          // detpost_launch's launcher: the kernel sequence of det_post.hpp on the caller's stream
    hipStream_t stream;
    template <class K, class... A>
    void operator()(K kernel, int gx, int gy, int threads, size_t lds_bytes, A... args) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3((unsigned)threads), lds_bytes, stream, args...);
    }
};

// the workgroup's LDS grows with max_candidates and passes the 64 KB a kernel may take without saying so
template <class K>
void detpost_allow_lds(K select_f32, K select_f16, size_t lds) {
    BM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(select_f32), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    BM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(select_f16), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
}

// what the run entry points check before they read their geometry rows; tiled, extra: which of them was called
void detpost_check_run(const BoxMOTHipDetPost* handle, bool tiled, int n_streams, const void* d_pred, int dtype, const double* geom, const float* d_dets,
                       int out_stride_rows, const int* d_det_rows, bool extra = false) {
    if (!handle) throw std::runtime_error("boxmot_hip: null detpost handle");
    const BoxMOTHipDetPostConfig& c = handle->cfg;
    if (!extra && handle->n_extra) throw std::runtime_error("boxmot_hip: a detpost handle with extras is run with boxmot_hip_detpost_run_extra");
    if (extra && !handle->n_extra) throw std::runtime_error("boxmot_hip: boxmot_hip_detpost_run_extra needs a handle of boxmot_hip_detpost_create_extra");
    if (!tiled && handle->n_tiles) throw std::runtime_error("boxmot_hip: a tiled detpost handle is run with boxmot_hip_detpost_run_tiled");
    if (tiled && !handle->n_tiles) throw std::runtime_error("boxmot_hip: boxmot_hip_detpost_run_tiled needs a handle of boxmot_hip_detpost_create_tiled");
    if (n_streams < 1 || n_streams > c.n_streams)
        throw std::runtime_error("boxmot_hip: detpost stream count " + std::to_string(n_streams) + " out of range for a handle of " + std::to_string(c.n_streams));
    if (!d_pred || !geom || !d_dets || !d_det_rows) throw std::runtime_error("boxmot_hip: null detpost argument");
    if (dtype != 0 && dtype != 1) throw std::runtime_error("boxmot_hip: unknown detpost dtype " + std::to_string(dtype) + " (0 fp32, 1 fp16)");
    if ((uintptr_t)d_pred % (dtype ? 2 : 4) || (uintptr_t)d_dets % 4 || (uintptr_t)d_det_rows % 4)
        throw std::runtime_error("boxmot_hip: detpost device addresses must be aligned to their element size");
    if (out_stride_rows < c.max_det)
        throw std::runtime_error("boxmot_hip: detpost out_stride_rows " + std::to_string(out_stride_rows) + " is below max_det " + std::to_string(c.max_det));
}

// what both do with their checked geometry rows g: wait for the handle's last run (the scratch and the table are the handle's), bring
// the table up to date, launch(launcher) -- their own kernel sequence -- and record the run
template <class G, class Launch>
void detpost_run(BoxMOTHipDetPost* handle, DetPostGeomTable<G>& table, const std::vector<G>& g, int n_streams, void* hip_stream, const Launch& launch) {
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (handle->ran) BM_HIP(hipStreamWaitEvent(st, handle->done, 0));
    table.set(g, n_streams, st);
    DetPostLaunch on{st};
    launch(on);
    BM_HIP(hipGetLastError());
    BM_HIP(hipEventRecord(handle->done, st));
    handle->ran = true;
}
}  // namespace

// What the three tracker handles share on the host: the weight blob and ReID engine, the staging tables of the per-stream inputs and
// results, the frames a host update uploads, the crop list, pending camera-motion warps, the record of the tracker's tables
// (growth), the two-stage ReID pipeline and the per-stream frame sizes.
namespace {
struct HandleCore : DeviceBound {
    std::string reid_path;
    std::vector<float> reid_blob;            // host copy of the weight blob the engine was built from (path or set_reid_blob): growth rebuilds from it
    std::vector<void*> owned;
    hipStream_t stream = nullptr;
    int S = 1, cap = 0, nd = 0, dim = 0;
    int det_cols = bm::DET_COLS, out_cols = bm::OUT_COLS;      // 7 / 9 on an oriented handle; set at build
    // io staging
    float* d_dets = nullptr; int* d_ndets = nullptr; float* d_embs = nullptr; float* d_out = nullptr; int* d_out_n = nullptr;
    double* d_warp = nullptr;      // [S][6] camera-motion warps for the next update of each stream
    int* d_warp_flag = nullptr;
    std::vector<float> h_dets, h_out;
    std::vector<int> h_ndets, h_out_n, h_warp_flag;
    std::vector<double> h_warp;
    // frames owned by the handle (host API)
    std::vector<uint8_t*> frame_bufs;
    size_t frame_bytes = 0;
    int frame_rows = 0, frame_cols = 0;
    const uint8_t** d_frames = nullptr;
    std::unique_ptr<bm::ReidEngine> reid;
    int* d_crop_count = nullptr; int* d_crop_stream = nullptr; float* d_crop_boxes = nullptr; int* d_crop_row = nullptr;
    // [S * max_dets][8] crop geometry (obb_crop_geometry.hpp) of an oriented handle with in-handle ReID, made by the oriented
    // crop-list kernel; null on every other handle -- its presence is what makes a ReID pass an oriented one
    double* d_crop_geo = nullptr;
    // growth of the tables: what the tracker's allocate function handed out, in order; slots in use per stream after the last
    // host update (-1 = unknown: a device-resident step ran since)
    std::vector<std::pair<void*, size_t>> table_rec;
    std::vector<int> h_used;
    int n_grows = 0;
    // The device-resident step with in-handle ReID as a two-stage pipeline over consecutive (asynchronous) calls: the ReID pass of
    // frame t + 1 is enqueued on `reid_stream` and runs while the frame step of frame t -- a handful of workgroups, one per stream,
    // for milliseconds -- is still on `stream`.  A frame's embeddings do not depend on the previous frame's step (the crops come from
    // the detections), so only the embedding table is double-buffered: ReID(t) writes table t & 1 after step(t - 2) has read it
    // (ev_embs_free), step(t) starts after ReID(t) (ev_reid_done).  Every ReID pass is followed by its step on `stream`, so waiting
    // for `stream` waits for both.  BOXMOT_HIP_PIPELINE=0 keeps everything on `stream` (A/B switch, profiles/r5_pipeline_ab.txt).
    hipStream_t reid_stream = nullptr;
    float* d_embs_alt = nullptr;
    hipEvent_t ev_reid_done[2] = {}, ev_embs_free[2] = {}, ev_main = nullptr;
    int pipe_slot = 0;
    bool pipe = true;
    bool engine_on_main = false;        // the engine / crop list were last used on `stream` (host-update paths)
    bool stream_exposed = false;        // *_stream() was handed out: the caller may order its inputs on `stream` -- every ReID pass waits for it
    // per-stream frame sizes (*_set_frame_sizes): empty = one size per handle, taken from the calls' scalar arguments.  d_fs_dims is
    // the [S][2] {W, H} table the `_sized` crop kernels read (written when the sizes are set, not per frame); it is handed to the
    // engine only when the sizes differ.
    std::vector<int> fs_rows, fs_cols;
    int* d_fs_dims = nullptr;
    bool fs_mixed = false;

    void sync_streams() {
        if (reid_stream) (void)hipStreamSynchronize(reid_stream);
        if (stream) (void)hipStreamSynchronize(stream);
    }
    ~HandleCore() {
        sync_streams();
        for (hipEvent_t e : ev_reid_done) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_embs_free) if (e) (void)hipEventDestroy(e);
        if (ev_main) (void)hipEventDestroy(ev_main);
        if (reid_stream) (void)hipStreamDestroy(reid_stream);
        reid.reset();
        for (void* p : owned) (void)hipFree(p);
        for (auto* p : frame_bufs) if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
}  // namespace

struct BoxMOTHipBotSort : HandleCore {
    BoxMOTHipBotSortConfig cfg{};
    bm::BotSortStepArgs args{};
    hipEvent_t ev[2]{};
    hipEvent_t timer_ev[2]{};
    int n_lists = 1;
    int* d_list_sel = nullptr;
    int* d_fc_set = nullptr;
    std::vector<int> h_list_sel, h_fc_set;
    int reid_mode = 0, reid_pad = 0;
    bool is_obb = false;                         // oriented detections (7 columns in, 9 out, 10-state filter): config.is_obb
    float* d_cmc_boxes = nullptr;                // [S][nd][4] enclosing boxes of the oriented detections: the SOF estimator's mask boxes
    bool use_ecc = false;                        // cmc_method = "ecc": the estimator runs inside update on the uploaded frame
    std::unique_ptr<BoxMOTHipEcc> ecc;
    bool use_sof = false;                        // cmc_method = "sof" (configs/trackers/botsort.yaml): likewise, masked by the frame's detections
    bool cmc_with_fc_set = false;                // one update with a frame-counter preset that is NOT a per-class fan-out call (compat adapter's first
                                                 // real frame after empty ones): the estimator sees the frame as it does in the reference
    std::unique_ptr<BoxMOTHipSof> sof;
    // with per-stream frame sizes, handle-owned camera-motion estimation keeps one estimator per DISTINCT size; each is made for all
    // S streams and serves the streams of its size under their own indices
    std::map<std::pair<int, int>, std::unique_ptr<BoxMOTHipSof>> sof_by_size;
    std::map<std::pair<int, int>, std::unique_ptr<BoxMOTHipEcc>> ecc_by_size;
    long long* d_phase_clock = nullptr;
    // parity debugging (boxmot_hip_botsort_debug_costs_enable): copies of the association cost matrices of the last step
    bool dbg_costs = false;
    double* d_dbg_cost = nullptr;
    int* d_dbg_shape = nullptr;
    int dbg_cap = 0, dbg_nd = 0;
    double last_track_ms = 0, last_reid_pre_ms = 0, last_reid_proc_ms = 0;
    std::vector<int> h_count_buf;

    ~BoxMOTHipBotSort() {
        sync_streams();
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        for (auto& e : timer_ev) if (e) (void)hipEventDestroy(e);
    }
};

// The DeepOCSORT and StrongSORT handles: host updates stage through io_stage / io_read_back, device-resident steps upload pending
// warps from a ring and may size their ReID launches by a declared crop bound.
struct StreamIo : HandleCore {
    int reid_mode = -1;             // set_reid_mode's last value (-1: the engine's default), re-applied when the engine is re-made
    // set_crop_bound: host-declared upper bound on the ReID crops of a device-resident step (-1: none, the count is read back);
    // d_crop_count[1] = "the count exceeded the bound"
    int crop_bound = -1;
    bool bounded_step_pending = false;      // a step sized by crop_bound was queued since the overflow flag was last read (io_check_crop_bound)
    // device-resident steps upload pending warps from a small ring of staging slots (an event per slot): the host does not wait for
    // the stream -- i.e. for the previous step's ReID pass -- every time a warp is set
    static constexpr int WARP_SLOTS = 8;
    std::vector<double> warp_stage[WARP_SLOTS];
    std::vector<int> warp_flag_stage[WARP_SLOTS];
    hipEvent_t warp_ev[WARP_SLOTS] = {};
    unsigned warp_slot = 0;
    int* d_ndets_step[2] = {};          // [S] each: the detection counts a bounded step reads (-1 everywhere after a bound overflow)
    const int* step_ndets = nullptr;    // what the frame step of the current step_device_frames call takes as n_dets
    ~StreamIo() {
        sync_streams();
        for (hipEvent_t e : warp_ev) if (e) (void)hipEventDestroy(e);
    }
};

struct BoxMOTHipDeepOcSort : StreamIo {
    BoxMOTHipDeepOcSortConfig cfg{};
    bm::DocsStepArgs args{};
    int dbg_cap = 0, dbg_nd = 0;    // sizes the debug cost planes (args.dbg_cost) were made at
    bool is_obb = false;            // oriented detections: config.is_obb (7 columns in, 9 out, 9-state filter)
};

struct BoxMOTHipStrongSort : StreamIo {
    BoxMOTHipStrongSortConfig cfg{};
    bm::SsStepArgs args{};
    int dbg_big = 0;                // leading dimension the debug cost planes (args.dbg_cost) were made at
    bool bank_valu = false;         // BOXMOT_HIP_SS_BANK=valu: the scalar-FMA bank-distance kernel (A/B timing, cross-check)
};

namespace {

using bm::dev_alloc;

void require_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        throw std::runtime_error("boxmot_hip: no HIP device available (this library has no CPU fallback)");
}

template <typename T>
T* zalloc(size_t n, std::vector<void*>& owned) {
    T* p = dev_alloc<T>(n, owned);
    BM_HIP(hipMemset(p, 0, (n ? n : 1) * sizeof(T)));
    return p;
}

struct DevAlloc {
    std::vector<void*>* owned;
    template <typename T> T* get(size_t n) { return zalloc<T>(n, *owned); }
};

struct RecAlloc {         // DevAlloc that also notes every table (pointer, bytes) in allocation order
    std::vector<void*>* owned;
    std::vector<std::pair<void*, size_t>>* rec;
    template <typename T> T* get(size_t n) { T* p = zalloc<T>(n, *owned); rec->push_back({p, n * sizeof(T)}); return p; }
};

void release(std::vector<void*>& owned, void* p) {
    if (!p) return;
    for (size_t i = 0; i < owned.size(); ++i)
        if (owned[i] == p) { owned.erase(owned.begin() + (long)i); (void)hipFree(p); return; }
}

int grown(int have, int need) {           // at least double, in steps of 64
    int v = have * 2 > need ? have * 2 : need;
    return (v + 63) / 64 * 64;
}
// Growth targets (cap, nd) for a frame that needs (need_cap, need_nd): doubled as above, but when the doubled pair exceeds what
// `fits(cap, nd)` accepts (the assignment solver's LDS state) the sizes fall back towards the need itself in steps of 64 -- a frame
// that fits is never refused because its DOUBLE would not.
template <class Fits>
void grown_pair(int have_cap, int need_cap, int have_nd, int need_nd, Fits fits, int& cap, int& nd) {
    cap = need_cap > have_cap ? grown(have_cap, need_cap) : have_cap;
    nd = need_nd > have_nd ? grown(have_nd, need_nd) : have_nd;
    const int min_cap = need_cap > have_cap ? (need_cap + 63) / 64 * 64 : have_cap, min_nd = need_nd > have_nd ? (need_nd + 63) / 64 * 64 : have_nd;
    while (!fits(cap, nd) && (cap > min_cap || nd > min_nd)) {
        if (cap > min_cap) cap -= 64;
        else nd -= 64;
    }
}

struct StreamIn {
    const float* dets; int det_rows;
    const float* embs;
    const uint8_t* image;
};

// ---------------------------------------------------------------------------
// HandleCore: host plumbing shared by the BoT-SORT, DeepOCSORT and StrongSORT handles
// ---------------------------------------------------------------------------
// Per-frame buffers whose size follows max_dets / max_tracks (contents do not outlive an update).  The result rows are the one
// difference between the handles: `out_rows` per stream on the device, `h_out_rows` in the host staging vector.
void core_alloc_sized(HandleCore* h, size_t out_rows, size_t h_out_rows) {
    auto& o = h->owned;
    const size_t s = h->S, n = h->nd, d = h->dim;
    if (h->reid_stream) BM_HIP(hipStreamSynchronize(h->reid_stream));       // nothing in flight reads the tables being replaced
    release(o, h->d_dets); release(o, h->d_embs); release(o, h->d_embs_alt); release(o, h->d_out);
    release(o, h->d_crop_stream); release(o, h->d_crop_boxes); release(o, h->d_crop_row);
    h->d_dets = zalloc<float>(s * n * h->det_cols, o);
    h->d_embs = zalloc<float>(s * n * d, o);
    h->d_embs_alt = zalloc<float>(s * n * d, o);          // pipeline: frames alternate between the two tables
    h->d_out = zalloc<float>(s * out_rows * h->out_cols, o);
    h->d_crop_stream = zalloc<int>(s * n, o);
    h->d_crop_boxes = zalloc<float>(s * n * 4, o);
    h->d_crop_row = zalloc<int>(s * n, o);
    h->h_dets.assign(s * n * h->det_cols, 0.f);
    h->h_out.assign(h_out_rows * h->out_cols, 0.f);
}

// A ReID engine for S x nd crops from the handle's blob copy (read from reid_path the first time), as the weights configure it: the
// caller applies its handle's preprocess / mode.  Returned, not installed: the caller commits it together with whatever else
// changes size, so that a failure leaves the handle as it was.
std::unique_ptr<bm::ReidEngine> core_new_reid(HandleCore* h, int nd) {
    if (h->reid_blob.empty()) h->reid_blob = bm::read_blob_file(h->reid_path.c_str());
    const long crops = (long)h->S * nd;
    std::unique_ptr<bm::ReidEngine> e(new bm::ReidEngine(h->reid_blob.data(), (long)h->reid_blob.size(), bm::reid_chunk_for(crops), (int)crops));
    if (e->feature_dim() != h->dim) throw std::runtime_error("boxmot_hip: ReID feature dim != emb_dim");
    return e;
}

// State tables of a tracker carried over into a larger set (growth): `rec` = the new tables in allocation order, the state tables
// first, up to `first_scratch`; every state table is [stream][slot][...], so a stream's slab only gets longer (slot ids stay
// valid).  `tall` is the one table that holds `tall_rows` slabs per stream (BoT-SORT's per-class active lists).
void core_migrate(HandleCore* h, const std::vector<std::pair<void*, size_t>>& rec, const void* first_scratch,
                  const void* tall = nullptr, int tall_rows = 1) {
    if (rec.size() != h->table_rec.size()) throw std::runtime_error("boxmot_hip: table layout changed between allocations");
    for (size_t i = 0; i < rec.size() && rec[i].first != first_scratch; ++i) {
        const auto& od = h->table_rec[i];
        const size_t rows = (size_t)h->S * (tall && rec[i].first == tall ? tall_rows : 1);
        if (od.second == rec[i].second) BM_HIP(hipMemcpy(rec[i].first, od.first, od.second, hipMemcpyDeviceToDevice));
        else BM_HIP(hipMemcpy2D(rec[i].first, rec[i].second / rows, od.first, od.second / rows, od.second / rows, rows, hipMemcpyDeviceToDevice));
    }
    for (const auto& od : h->table_rec) release(h->owned, od.first);
    h->table_rec = rec;
}

// Room for the frames of streams [s0, s0 + n) before they are staged: more detections than max_dets, or slots in use + this
// frame's detections > max_tracks, re-makes the tables through `grow(new_cap, new_nd)` (the reference's lists have no limit; every
// detection of a frame can become a track).  `used_on_device(s)` reads stream s's slots in use back where the host no longer
// knows them (a device-resident step ran since the last count).
template <class Used, class Grow, class Fits>
void core_make_room(HandleCore* h, int s0, int n, const StreamIn* in, Used used_on_device, Grow grow, Fits fits) {
    if (s0 < 0 || n < 1 || s0 + n > h->S) throw std::runtime_error("boxmot_hip: stream index out of range");
    int need_nd = h->nd, need_cap = h->cap;
    for (int k = 0; k < n; ++k) {
        const int rows = in[k].det_rows > 0 ? in[k].det_rows : 0;
        need_nd = rows > need_nd ? rows : need_nd;
        if (h->h_used[s0 + k] < 0) {
            BM_HIP(hipStreamSynchronize(h->stream));
            h->h_used[s0 + k] = used_on_device(s0 + k);
        }
        need_cap = h->h_used[s0 + k] + rows > need_cap ? h->h_used[s0 + k] + rows : need_cap;
    }
    if (need_nd > h->nd || need_cap > h->cap) {
        int to_cap, to_nd;
        grown_pair(h->cap, need_cap, h->nd, need_nd, fits, to_cap, to_nd);
        grow(to_cap, to_nd);
    }
}

void core_set_warp(HandleCore* h, int stream, const double* warp_2x3) {
    if (stream < 0 || stream >= h->S) throw std::runtime_error("boxmot_hip: stream index out of range");
    if (warp_2x3 == nullptr) { h->h_warp_flag[stream] = 0; return; }
    for (int k = 0; k < 6; ++k) {
        if (!std::isfinite(warp_2x3[k])) throw std::runtime_error("boxmot_hip: camera-motion warp has non-finite entries");
        h->h_warp[(size_t)stream * 6 + k] = warp_2x3[k];
    }
    h->h_warp_flag[stream] = 1;
}

// *_set_frame_sizes, step 1: one (rows, cols) per stream; a stream's size is fixed by its first frame or an earlier declaration, so
// a stream that already has frames of another size is an error naming the stream.  Changes nothing.
void core_check_frame_sizes(const HandleCore* h, const int* image_rows, const int* image_cols, int n_streams) {
    if (!image_rows || !image_cols) throw std::runtime_error("boxmot_hip: null argument");
    if (n_streams != h->S) throw std::runtime_error("boxmot_hip: set_frame_sizes needs one (rows, cols) per stream of the handle (" + std::to_string(h->S) + ")");
    for (int s = 0; s < h->S; ++s) {
        if (image_rows[s] < 1 || image_cols[s] < 1) throw std::runtime_error("boxmot_hip: stream " + std::to_string(s) + ": frame dimensions must be positive");
        const bool seen = h->frame_bufs[s] != nullptr || !h->fs_rows.empty();
        const int r0 = h->fs_rows.empty() ? h->frame_rows : h->fs_rows[s], c0 = h->fs_cols.empty() ? h->frame_cols : h->fs_cols[s];
        if (seen && (r0 != image_rows[s] || c0 != image_cols[s]))
            throw std::runtime_error("boxmot_hip: stream " + std::to_string(s) + ": frame size changed (" + std::to_string(r0) + " x " + std::to_string(c0) +
                                     " -> " + std::to_string(image_rows[s]) + " x " + std::to_string(image_cols[s]) + ")");
    }
}
// step 2: the checked sizes become the handle's, and the {W, H} table of the `_sized` crop kernels is written
void core_commit_frame_sizes(HandleCore* h, const int* image_rows, const int* image_cols) {
    BM_HIP(hipStreamSynchronize(h->stream));
    if (h->reid_stream) BM_HIP(hipStreamSynchronize(h->reid_stream));
    h->fs_rows.assign(image_rows, image_rows + h->S);
    h->fs_cols.assign(image_cols, image_cols + h->S);
    h->fs_mixed = false;
    std::vector<int> dims((size_t)h->S * 2);
    for (int s = 0; s < h->S; ++s) {
        dims[2 * s] = image_cols[s]; dims[2 * s + 1] = image_rows[s];
        if (image_rows[s] != image_rows[0] || image_cols[s] != image_cols[0]) h->fs_mixed = true;
    }
    if (!h->d_fs_dims) h->d_fs_dims = dev_alloc<int>((size_t)h->S * 2, h->owned);
    BM_HIP(hipMemcpy(h->d_fs_dims, dims.data(), dims.size() * sizeof(int), hipMemcpyHostToDevice));
}

// The host frame of stream s into the handle's buffer of that stream (made on first use; the pointer table is re-uploaded then).
// With per-stream sizes the buffer has that stream's declared size and the scalar arguments are not used; without, the first
// frame fixes the one size of the handle.
void core_upload_frame(HandleCore* h, int s, const uint8_t* image, int rows, int cols) {
    const bool sized = !h->fs_rows.empty();
    const size_t bytes = sized ? (size_t)h->fs_rows[s] * h->fs_cols[s] * 3 : (size_t)rows * cols * 3;
    if (h->frame_bufs[s] == nullptr || (!sized && bytes != h->frame_bytes)) {
        if (!sized && h->frame_bytes != 0 && bytes != h->frame_bytes) throw std::runtime_error("boxmot_hip: frame size changed between updates");
        void* p = nullptr;
        BM_HIP(hipMalloc(&p, bytes));
        h->frame_bufs[s] = static_cast<uint8_t*>(p);
        if (!sized) { h->frame_bytes = bytes; h->frame_rows = rows; h->frame_cols = cols; }
        BM_HIP(hipMemcpy(h->d_frames, h->frame_bufs.data(), h->S * sizeof(uint8_t*), hipMemcpyHostToDevice));
    }
    BM_HIP(hipMemcpyAsync(h->frame_bufs[s], image, bytes, hipMemcpyHostToDevice, h->stream));
}

// the per-stream (or per-image) size table is handed to a ReID engine for one pass only
struct FrameDimsScope { bm::ReidEngine* e; ~FrameDimsScope() { if (e) e->set_frame_dims(nullptr); } };
// ... and so is the crop geometry of an oriented handle: a later axis-aligned user of the engine never sees it
struct CropGeoScope { bm::ReidEngine* e; ~CropGeoScope() { if (e) e->set_obb_geometry(nullptr); } };
static_assert(bm::OBB_CROP_DET_COLS == bm::obb::DET_COLS && bm::OBB_CROP_CONF_COL == bm::obb::CONF_COL,
              "the oriented crop-list kernel reads the oriented handle's detection rows");

// The crop list of streams [s0, s0 + n) -- every detection passing the confidence test (`conf > thresh`, or `>=` when inclusive)
// -- and the ReID pass over it on stream `st`, embeddings into the rows of `d_embs` (rows of skipped detections keep stale values;
// the step kernels never read them).  rows / cols: the one frame size (replaced by the declared sizes where there are any).
// On an oriented handle (d_crop_geo) the list carries the crops' geometry instead of boxes and the engine samples through it.
// Where the backbone sizes its launches on the host: by `bound` when the caller declared one (>= 0; `nd_step` then receives the
// detection counts the frame step is to read, see pad_crop_list_kernel, and `*bounded` is raised as soon as that kernel is
// queued; returns true), else by the count read back.
bool core_reid_pass(HandleCore* h, hipStream_t st, int s0, int n, const float* d_dets, const int* d_ndets, const uint8_t* const* d_frames,
                    int rows, int cols, double thresh, int inclusive, float* d_embs, int bound = -1, int* nd_step = nullptr,
                    bool* bounded = nullptr) {
    FrameDimsScope dims_scope{h->reid.get()};
    if (!h->fs_rows.empty()) {      // per-stream sizes: the table when they differ, else the one size as the scalars
        rows = h->fs_rows[0]; cols = h->fs_cols[0];
        h->reid->set_frame_dims(h->fs_mixed ? h->d_fs_dims : nullptr);
    }
    BM_HIP(hipMemsetAsync(h->d_crop_count, 0, 4, st));
    CropGeoScope geo_scope{h->d_crop_geo ? h->reid.get() : nullptr};
    if (h->d_crop_geo) {
        hipLaunchKernelGGL(bm::build_crop_list_obb_kernel, dim3(n), dim3(256), 0, st, d_dets, d_ndets, h->nd, thresh,
                           h->d_crop_count, h->d_crop_stream, h->d_crop_row, h->d_crop_geo, s0, inclusive);
        h->reid->set_obb_geometry(h->d_crop_geo);
    } else
    hipLaunchKernelGGL(bm::build_crop_list_kernel, dim3(n), dim3(256), 0, st, d_dets, d_ndets, h->nd, thresh,
                       h->d_crop_count, h->d_crop_stream, h->d_crop_boxes, h->d_crop_row, s0, inclusive);
    if (h->reid->counted_ok()) {
        // crop count stays on the device: launches cover the capacity, surplus workgroups exit at once
        h->reid->run_counted(d_frames, h->d_crop_stream, h->d_crop_boxes, 4, h->d_crop_count, n * h->nd, cols, rows, d_embs, h->d_crop_row, st);
        return false;
    }
    if (bound >= 0) {
        // launches sized by the caller's bound: no read-back, no stream synchronisation inside the step (the host keeps queueing)
        const int m = bound < n * h->nd ? bound : n * h->nd;
        // (a bound of 0 -- "no crops in this step" -- is checked like any other: one workgroup compares the count with it)
        hipLaunchKernelGGL(pad_crop_list_kernel, dim3(m > 0 ? (m + 255) / 256 : 1), dim3(256), 0, st, (const int*)h->d_crop_count, m,
                           h->d_crop_stream, h->d_crop_boxes, h->d_crop_row, h->d_crop_count + 1, d_ndets, nd_step, n, h->d_crop_geo);
        if (bounded) *bounded = true;
        if (m > 0) h->reid->run(d_frames, h->d_crop_stream, h->d_crop_boxes, 4, m, cols, rows, d_embs, h->d_crop_row, st);
        return true;
    }
    int n_crops = 0;
    BM_HIP(hipMemcpyAsync(&n_crops, h->d_crop_count, 4, hipMemcpyDeviceToHost, st));
    BM_HIP(hipStreamSynchronize(st));
    h->reid->run(d_frames, h->d_crop_stream, h->d_crop_boxes, 4, n_crops, cols, rows, d_embs, h->d_crop_row, st);
    return false;
}

// ---- the two-stage ReID pipeline of the device-resident steps (see HandleCore) ----
void core_pipe_create(HandleCore* h) {
    BM_HIP(hipStreamCreate(&h->reid_stream));
    for (int k = 0; k < 2; ++k) {
        BM_HIP(hipEventCreateWithFlags(&h->ev_reid_done[k], hipEventDisableTiming));
        BM_HIP(hipEventCreateWithFlags(&h->ev_embs_free[k], hipEventDisableTiming));
    }
    BM_HIP(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
}
bool core_pipe_on(const HandleCore* h) { return h->pipe && h->reid_stream; }
// the embedding table this call's ReID pass writes and its frame step reads
float* core_pipe_table(HandleCore* h) { return (core_pipe_on(h) && h->pipe_slot) ? h->d_embs_alt : h->d_embs; }
// stage 1: this frame's ReID goes on the returned stream -- `reid_stream`, once the step before last has finished reading the table
// (`stream` itself without the pipeline)
hipStream_t core_pipe_begin_reid(HandleCore* h) {
    if (!core_pipe_on(h)) return h->stream;
    hipStream_t rs = h->reid_stream;
    // a host-update path used the engine / the crop list on `stream` since, or the caller holds `stream` (it may have queued the
    // producers of this step's detections / frames there, e.g. boxmot_hip_ingest_wait): the ReID pass is ordered after `stream` --
    // correct always; such a caller gives up the overlap, its own stream order already serialises the frames
    if (h->engine_on_main || h->stream_exposed) {
        BM_HIP(hipEventRecord(h->ev_main, h->stream));
        BM_HIP(hipStreamWaitEvent(rs, h->ev_main, 0));
        h->engine_on_main = false;
    }
    BM_HIP(hipStreamWaitEvent(rs, h->ev_embs_free[h->pipe_slot], 0));
    return rs;
}
// the ReID pass is enqueued: the frame step on `stream` starts after it
void core_pipe_reid_done(HandleCore* h) {
    if (!core_pipe_on(h)) return;
    BM_HIP(hipEventRecord(h->ev_reid_done[h->pipe_slot], h->reid_stream));
    BM_HIP(hipStreamWaitEvent(h->stream, h->ev_reid_done[h->pipe_slot], 0));
}
// stage 2 enqueued (the frame step that reads this frame's embedding table is on `stream`): the table is free for the ReID pass
// after next once that step has run
void core_pipe_step_enqueued(HandleCore* h) {
    if (!core_pipe_on(h)) return;
    BM_HIP(hipEventRecord(h->ev_embs_free[h->pipe_slot], h->stream));
    h->pipe_slot ^= 1;
}

// `rows` result rows of `oc` columns into the caller's 9-column rows (an axis-aligned row has 8: the ninth is zeroed)
void copy_rows9(const float* src, int rows, int oc, float* dst) {
    for (int r = 0; r < rows; ++r, dst += 9) {
        for (int q = 0; q < oc; ++q) dst[q] = src[(size_t)r * oc + q];
        if (oc < 9) dst[8] = 0.0f;
    }
}

// ---------------------------------------------------------------------------
// BoT-SORT / ByteTrack host path
// ---------------------------------------------------------------------------
void alloc_det_io(BoxMOTHipBotSort* h) {
    core_alloc_sized(h, h->nd, (size_t)h->S * h->nd);
    release(h->owned, h->d_cmc_boxes);
    h->d_cmc_boxes = h->is_obb ? zalloc<float>((size_t)h->S * h->nd * 4, h->owned) : nullptr;
    release(h->owned, h->d_crop_geo);
    h->d_crop_geo = (h->is_obb && h->cfg.with_reid) ? zalloc<double>((size_t)h->S * h->nd * 8, h->owned) : nullptr;
}

std::unique_ptr<bm::ReidEngine> new_reid_engine(BoxMOTHipBotSort* h, int nd) {
    std::unique_ptr<bm::ReidEngine> e = core_new_reid(h, nd);
    e->set_preprocess(h->reid_pad);
    if (h->reid_mode) e->set_mode(h->reid_mode);
    return e;
}

void set_step_lds(BoxMOTHipBotSort* h) {
    const long lds = bm::lap_lds_bytes(h->cap, h->nd);
    BM_HIP(hipFuncSetAttribute(h->is_obb ? reinterpret_cast<const void*>(botsort_obb_step_kernel<STEP_THREADS>)
                                         : reinterpret_cast<const void*>(botsort_step_kernel<STEP_THREADS>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
}

// The reference's lists have no capacity (botsort.py:177-250); the device tables do.  They are created at max_tracks / max_dets and
// GROW when a host update would not fit: a new set of tables at the larger sizes, every state table copied stream by stream
// (slot ids stay valid: a stream's slab only gets longer), scratch and per-frame buffers simply re-made, the ReID engine re-created
// for the larger crop count.  The limit is the LDS state of the assignment solver (lap_lds_bytes <= 120 KB), reported loudly.
void grow_tables(BoxMOTHipBotSort* h, int new_cap, int new_nd) {
    if (bm::lap_lds_bytes(new_cap, new_nd) > 120 * 1024)
        throw std::runtime_error("boxmot_hip: " + std::to_string(new_cap) + " tracks x " + std::to_string(new_nd) +
                                 " detections per stream is beyond what the assignment solver's LDS state can hold");
    BM_HIP(hipStreamSynchronize(h->stream));
    // the larger ReID engine first: if it cannot be built (weights, memory) the handle keeps its tables, engine and LDS attribute
    std::unique_ptr<bm::ReidEngine> new_reid;
    if (h->reid && new_nd != h->nd) new_reid = new_reid_engine(h, new_nd);
    bm::BotSortStepArgs na = h->args;
    std::vector<std::pair<void*, size_t>> rec;
    RecAlloc ra{&h->owned, &rec};
    bm::BotSortSizes z{h->S, new_cap, new_nd, h->dim, h->n_lists, h->args.st.removed_alloc, h->is_obb ? 1 : 0};
    bm::botsort_allocate(na, z, ra);
    core_migrate(h, rec, na.sc.det_xywh, na.st.active_list, h->n_lists);          // the state tables come first
    h->args = na;
    const bool more_dets = new_nd != h->nd;
    h->cap = new_cap; h->nd = new_nd;
    if (more_dets) {
        alloc_det_io(h);
        if (new_reid) h->reid = std::move(new_reid);
    }
    set_step_lds(h);
    ++h->n_grows;
}

void zero_state(BoxMOTHipBotSort* h) {
    bm::BotSortState& st = h->args.st;
    const size_t S = h->S, cap = h->cap;
    BM_HIP(hipMemsetAsync(st.frame_count, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.id_count, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.n_active, 0, S * h->n_lists * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.n_lost, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.rm_head, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.rm_size, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.stamp, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.status, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.slot_used, 0, S * cap * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.mark, 0, S * cap * 4, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
}

void build(BoxMOTHipBotSort* h) {
    const BoxMOTHipBotSortConfig& c = h->cfg;
    h->use_ecc = c.cmc_method && std::strcmp(c.cmc_method, "ecc") == 0;
    h->use_sof = c.cmc_method && std::strcmp(c.cmc_method, "sof") == 0;
    if (c.cmc_method && c.cmc_method[0] && std::strcmp(c.cmc_method, "none") != 0 && !h->use_ecc && !h->use_sof)
        throw std::runtime_error(std::string("boxmot_hip: camera-motion estimator '") + c.cmc_method + "' is not implemented (have: sof, ecc, none); "
                                 "supply the warp per frame with boxmot_hip_botsort_set_warp");
    h->reid_pad = 0;
    if (c.reid_preprocess && c.reid_preprocess[0]) {
        if (std::strcmp(c.reid_preprocess, "resize_pad") == 0) h->reid_pad = 1;
        else if (std::strcmp(c.reid_preprocess, "resize") != 0)
            throw std::runtime_error("boxmot_hip: unknown ReID preprocess (have: resize, resize_pad)");
    }
    h->cfg.reid_preprocess = nullptr;
    if (c.n_streams < 1 || c.max_tracks < 8 || c.max_dets < 4 || c.emb_dim < 1 || c.n_class_lists < 1)
        throw std::runtime_error("boxmot_hip: invalid capacity configuration");
    if (c.removed_stracks_buffer < 0) throw std::runtime_error("boxmot_hip: removed_stracks_buffer must be >= 0");
    if (c.tracker_kind != 0 && c.tracker_kind != 1) throw std::runtime_error("boxmot_hip: tracker_kind must be 0 (BoT-SORT) or 1 (ByteTrack)");
    if (c.tracker_kind == 1) {
        h->cfg.with_reid = 0; h->cfg.fuse_first_associate = 1;
    }
    h->is_obb = c.is_obb != 0;
    if (h->is_obb) { h->det_cols = bm::obb::DET_COLS; h->out_cols = bm::obb::OUT_COLS; }
    if (h->is_obb) {
        // oriented detections (botsort.py:120-131, bytetrack.py:266-303).  Camera motion: a warp supplied with set_warp is applied to
        // the oriented tracks (STrack.multi_gmc_obb, botsort_track.py:197-230: kf_warp_wave of the oriented layout); the in-handle
        // estimators mask by axis-aligned detection boxes and are not wired to oriented tables (the reference estimates on the
        // enclosing boxes, botsort.py:147-158: the caller does that and supplies the warp).  Embeddings of oriented detections come
        // from the caller or from the handle's own ReID pass over the rotated rectangles (the reference's cv2.warpAffine crops,
        // reid/backends/base_backend.py:92-118: build_crop_list_obb_kernel + the k_crop_resize_obb* kernels); its weights arrive through
        // boxmot_hip_botsort_set_reid_blob -- a reid_model_path at creation is still refused, below.
        // (cmc_method ecc / sof run on an oriented handle too: SOF is masked by the enclosing boxes, obb_enclosing_boxes_kernel)
        if ((c.reid_model_path && c.reid_model_path[0]) || !h->reid_path.empty())      // (create() moves the path into the handle)
            throw std::runtime_error("boxmot_hip: an oriented-box handle takes embeddings from the caller (embs), not from in-handle ReID weights");
    }
    h->S = c.n_streams; h->cap = c.max_tracks; h->nd = c.max_dets; h->dim = c.emb_dim; h->n_lists = c.n_class_lists;
    BM_HIP(hipStreamCreate(&h->stream));
    {
        // The frame step of this tracker is one 512-thread workgroup per stream at 256 registers: it owns a whole CU.  With fewer
        // streams than CUs the rest of the device is free for the next frame's ReID pass (the pipeline pays, as in configurations 3 / 5);
        // with a stream per CU (the headline's 256) nothing can run beside it -- measured flat, 12.04 vs 12.11 k frames/s,
        // profiles/r5_pipeline_ab.txt -- so the pipeline is on by default only below half the device (BOXMOT_HIP_PIPELINE=1 / 0 forces it).
        const char* v = std::getenv("BOXMOT_HIP_PIPELINE");
        int cus = 0, dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
        h->pipe = (v && v[0]) ? v[0] != '0' : 2 * c.n_streams <= cus;
        if (h->pipe && !h->reid_stream) core_pipe_create(h);
    }
    BM_HIP(hipEventCreate(&h->ev[0]));
    BM_HIP(hipEventCreate(&h->ev[1]));
    BM_HIP(hipEventCreate(&h->timer_ev[0]));
    BM_HIP(hipEventCreate(&h->timer_ev[1]));
    const size_t S = h->S, cap = h->cap, nd = h->nd, dim = h->dim, nl = h->n_lists;
    auto& o = h->owned;
    h->args.cfg = bm::make_config_dev(c.track_high_thresh, c.track_low_thresh, c.new_track_thresh, c.match_thresh,
                                      c.proximity_thresh, c.appearance_thresh, c.second_match_thresh,
                                      c.unconfirmed_match_thresh, c.unconfirmed_emb_scale, c.fuse_first_associate,
                                      c.tracker_kind == 1 ? 0 : c.with_reid, c.frame_rate, c.track_buffer, c.removed_stracks_buffer,
                                      c.tracker_kind);
    bm::BotSortSizes z{h->S, h->cap, h->nd, h->dim, h->n_lists, c.removed_stracks_buffer > 0 ? c.removed_stracks_buffer : 1, h->is_obb ? 1 : 0};
    RecAlloc table_allocator{&o, &h->table_rec};
    bm::botsort_allocate(h->args, z, table_allocator);
    // io
    alloc_det_io(h);
    h->d_ndets = zalloc<int>(S, o);
    h->d_out_n = zalloc<int>(S, o);
    h->d_list_sel = zalloc<int>(S, o);
    h->d_fc_set = zalloc<int>(S, o);
    h->d_warp = zalloc<double>(S * 6, o);
    h->d_warp_flag = zalloc<int>(S, o);
    h->h_warp.assign(S * 6, 0.0); h->h_warp_flag.assign(S, 0);
    h->h_ndets.assign(S, 0); h->h_out_n.assign(S, 0); h->h_list_sel.assign(S, 0); h->h_fc_set.assign(S, 0);
    h->h_used.assign(S, 0); h->h_count_buf.assign(S * (nl + 1), 0);
    h->frame_bufs.assign(S, nullptr);
    h->d_frames = zalloc<const uint8_t*>(S, o);
    h->d_crop_count = zalloc<int>(1, o);
    h->d_phase_clock = zalloc<long long>(16, o);
    if (bm::lap_lds_bytes(h->cap, h->nd) > 120 * 1024)
        throw std::runtime_error("boxmot_hip: max_tracks/max_dets too large for the assignment solver's LDS state");
    set_step_lds(h);
    (void)cap; (void)nd; (void)dim;
    if (c.with_reid && !h->reid_path.empty()) h->reid = new_reid_engine(h, h->nd);
}

void launch_step(BoxMOTHipBotSort* h, int s0, int n_streams, const float* d_dets, const int* d_ndets, const float* d_embs,
                 const int* d_list_sel, const int* d_fc_set, float* d_out, int* d_out_n, bool with_warp = false) {
    bm::BotSortStepArgs a = h->args;
    a.dets = d_dets; a.n_dets = d_ndets; a.embs = d_embs; a.list_sel = d_list_sel; a.frame_count_set = d_fc_set;
    a.warp = with_warp ? h->d_warp : nullptr; a.warp_flag = with_warp ? h->d_warp_flag : nullptr;
    a.out = d_out; a.out_n = d_out_n; a.stream_base = s0; a.phase_clock = h->d_phase_clock;
    a.dbg_cost = nullptr; a.dbg_shape = nullptr;
    if (h->dbg_costs) {
        if (h->dbg_cap != h->cap || h->dbg_nd != h->nd) {           // (re-)made at the tables' current sizes (they may have grown)
            BM_HIP(hipStreamSynchronize(h->stream));
            if (h->d_dbg_cost) { release(h->owned, h->d_dbg_cost); release(h->owned, h->d_dbg_shape); }
            h->d_dbg_cost = zalloc<double>((size_t)h->S * bm::DBG_STAGES * bm::DBG_PLANES * h->nd * h->cap, h->owned);
            h->d_dbg_shape = zalloc<int>((size_t)h->S * bm::DBG_STAGES * 2, h->owned);
            h->dbg_cap = h->cap; h->dbg_nd = h->nd;
        }
        a.dbg_cost = h->d_dbg_cost; a.dbg_shape = h->d_dbg_shape;
    }
    if (h->is_obb)
        hipLaunchKernelGGL((botsort_obb_step_kernel<STEP_THREADS>), dim3(n_streams), dim3(STEP_THREADS),
                           (size_t)bm::lap_lds_bytes(h->cap, h->nd), h->stream, a);
    else if (a.dbg_cost) {          // the parity-debugging instantiation (same source, debug writes compiled in)
        BM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(botsort_step_kernel<STEP_THREADS, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)bm::lap_lds_bytes(h->cap, h->nd)));
        hipLaunchKernelGGL((botsort_step_kernel<STEP_THREADS, true>), dim3(n_streams), dim3(STEP_THREADS),
                           (size_t)bm::lap_lds_bytes(h->cap, h->nd), h->stream, a);
    } else
        hipLaunchKernelGGL((botsort_step_kernel<STEP_THREADS>), dim3(n_streams), dim3(STEP_THREADS),
                           (size_t)bm::lap_lds_bytes(h->cap, h->nd), h->stream, a);
    BM_HIP(hipGetLastError());
}

// ReID on stream `st` for every detection above track_high_thresh (botsort.py:191-192, :260) of streams [s0, s0 + n_streams);
// writes d_embs rows
void run_reid(BoxMOTHipBotSort* h, hipStream_t st, int s0, int n_streams, const float* d_dets, const int* d_ndets,
              const uint8_t* const* d_frames, int rows, int cols, float* d_embs) {
    if (!h->reid) throw std::runtime_error("boxmot_hip: with_reid=1 and no embeddings supplied, but no ReID weights are loaded");
    if (st == h->stream) h->engine_on_main = true;
    core_reid_pass(h, st, s0, n_streams, d_dets, d_ndets, d_frames, rows, cols, h->cfg.track_high_thresh, 0, d_embs);
}

// Status words of streams [s0, s0 + n): a non-zero word is reported once and cleared, so that one overflow neither poisons the
// later updates of this stream nor the updates of the handle's other streams (the step has already run: the caller still
// receives the rows of this frame, see host_update).  Returns the message of the first failing stream ("" when all are ok).
std::string take_status(hipStream_t stream, int* d_status, int s0, int n, const char* tracker) {
    std::vector<int> st(n);
    BM_HIP(hipMemcpy(st.data(), d_status + s0, n * 4, hipMemcpyDeviceToHost));
    std::string msg;
    bool any = false;
    for (int k = 0; k < n; ++k) {
        if (st[k] == bm::STATUS_OK) continue;
        any = true;
        if (!msg.empty()) continue;
        const char* what = st[k] == bm::STATUS_TRACK_CAPACITY ? "track capacity (max_tracks) exceeded: the births of this frame were clamped"
                         : st[k] == bm::STATUS_CLASS_CAPACITY ? "more than 8 classes voted on one track"
                         : st[k] == bm::STATUS_LAP_STALL ? "assignment solver did not converge (non-finite costs?)"
                                                         : "innovation covariance is not positive definite";
        msg = std::string("boxmot_hip: ") + tracker + " stream " + std::to_string(s0 + k) + ": " + what;
    }
    if (any) {
        BM_HIP(hipMemsetAsync(d_status + s0, 0, n * 4, stream));
        BM_HIP(hipStreamSynchronize(stream));
    }
    return msg;
}

// ---- ECC estimator plumbing (C ABI boxmot_hip_ecc_*; also owned by a BoT-SORT handle created with cmc_method = "ecc") ----
void ecc_init(BoxMOTHipEcc* h, int n_streams, int image_rows, int image_cols, double scale, double eps, int max_iter, hipStream_t external) {
    if (n_streams < 1 || image_rows < 8 || image_cols < 8) throw std::runtime_error("boxmot_hip: ECC needs >= 1 stream and a frame of at least 8 x 8");
    if (!(scale > 0.0) || scale > 1.0 || !(eps > 0.0) || max_iter < 1) throw std::runtime_error("boxmot_hip: ECC scale must be in (0, 1], eps > 0, max_iter >= 1");
    h->S = n_streams; h->rows = image_rows; h->cols = image_cols; h->scale = scale; h->eps = eps; h->max_iter = max_iter;
    h->w = (int)std::nearbyint(image_cols * scale); h->h = (int)std::nearbyint(image_rows * scale);     // saturate_cast<int>(ssize * fx)
    if (h->w < 4 || h->h < 4) throw std::runtime_error("boxmot_hip: ECC image too small after scaling");
    if (external) { h->stream = external; h->owns_stream = false; }
    else BM_HIP(hipStreamCreate(&h->stream));
    const size_t P = (size_t)h->h * h->w, S = n_streams;
    h->img = zalloc<float>(S * 2 * P, h->owned);
    h->gx = zalloc<float>(S * P, h->owned); h->gy = zalloc<float>(S * P, h->owned);
    h->scratch = zalloc<float>(S * 3 * P, h->owned);
    h->d_warp = zalloc<double>(S * 6, h->owned); h->d_info = zalloc<int>(S * 2, h->owned);
    h->d_frames = zalloc<const uint8_t*>(S, h->owned);
    h->frame_bufs.assign(S, nullptr); h->cur.assign(S, 0); h->has_prev.assign(S, 0);
}

// one stream, frames d_frames[0]: preprocess into the stream's other buffer; estimate against the previous one when there is one
void ecc_run_one(BoxMOTHipEcc* h, int s, const uint8_t* const* d_frame_ptr, double* out_warp6, int* out_iterations) {
    const long P = (long)h->h * h->w;
    const int nxt = 1 - h->cur[s];
    float* imgs = h->img + (size_t)s * 2 * P;
    const unsigned blocks = (unsigned)((P + 255) / 256);
    hipLaunchKernelGGL(bm::k_ecc_preprocess, dim3(blocks, 1), dim3(256), 0, h->stream, d_frame_ptr, imgs + nxt * P, P, h->rows, h->cols, h->h,
                       h->w, 1.0 / h->scale);
    double warp[6] = {1, 0, 0, 0, 1, 0};
    int info[2] = {0, 0};
    if (h->has_prev[s]) {
        hipLaunchKernelGGL(bm::k_ecc_gradients, dim3(blocks, 1), dim3(256), 0, h->stream, imgs + nxt * P, P, h->gx + s * P, h->gy + s * P, h->h, h->w);
        hipLaunchKernelGGL(bm::k_ecc_solve, dim3(1), dim3(bm::ECC_THREADS), 0, h->stream, imgs + h->cur[s] * P, imgs + nxt * P, P, h->gx + s * P,
                           h->gy + s * P, h->scratch + (size_t)s * 3 * P, h->d_warp + s * 6, h->d_info + s * 2, h->h, h->w, h->eps, h->max_iter,
                           (float)h->scale);
        BM_HIP(hipMemcpyAsync(warp, h->d_warp + s * 6, sizeof(warp), hipMemcpyDeviceToHost, h->stream));
        BM_HIP(hipMemcpyAsync(info, h->d_info + s * 2, sizeof(info), hipMemcpyDeviceToHost, h->stream));
    }
    BM_HIP(hipStreamSynchronize(h->stream));
    BM_HIP(hipGetLastError());
    h->cur[s] = nxt; h->has_prev[s] = 1;
    for (int k = 0; k < 6; ++k) out_warp6[k] = warp[k];
    if (out_iterations) *out_iterations = info[1];
}

// ---- SOF estimator plumbing (C ABI boxmot_hip_sof_*; also owned by a BoT-SORT handle created with cmc_method = "sof") ----
struct HipLaunch {            // sof_frame's launcher: the kernel sequence of cmc_sof.hpp on the handle's stream
    hipStream_t stream;
    template <class K, class... A>
    void operator()(K kernel, int gx, int gy, int threads, A... args) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy), dim3((unsigned)threads), 0, stream, args...);
    }
};

void sof_alloc_dets(BoxMOTHipSof* h, int max_dets) {
    release(h->owned, h->d_dets);
    h->max_dets = max_dets;
    h->d_dets = zalloc<float>((size_t)h->S * max_dets * 4, h->owned);
}

void sof_init(BoxMOTHipSof* h, int n_streams, int image_rows, int image_cols, double scale, int min_inliers, double min_inlier_ratio,
              double thresh, hipStream_t external) {
    if (n_streams < 1) throw std::runtime_error("boxmot_hip: SOF needs >= 1 stream");
    if (!(scale > 0.0) || scale > 1.0 || min_inliers < 0 || !(thresh > 0.0)) throw std::runtime_error("boxmot_hip: SOF scale must be in (0, 1], ransac threshold > 0");
    h->S = n_streams; h->rows = image_rows; h->cols = image_cols;
    const int w = (int)std::nearbyint(image_cols * scale), hh = (int)std::nearbyint(image_rows * scale);     // saturate_cast<int>(ssize * fx)
    // the 21-pixel window borders are reflected: every pyramid level (level 0 included) must be larger than the window
    if (w <= bm::SOF_WIN + 1 || hh <= bm::SOF_WIN + 1) throw std::runtime_error("boxmot_hip: SOF image too small after scaling (needs > 22 x 22)");
    h->lv = bm::sof_levels(hh, w);
    h->prm = bm::SofParams{scale, min_inliers, min_inlier_ratio, thresh};
    if (external) { h->stream = external; h->owns_stream = false; }
    else BM_HIP(hipStreamCreate(&h->stream));
    const size_t T = (size_t)h->lv.total, P = (size_t)hh * w, S = n_streams, K = bm::SOF_MAX_CORNERS;
    auto& o = h->owned;
    bm::SofBuffers& b = h->buf;
    b.pyr_prev = zalloc<uint8_t>(S * T, o); b.pyr_cur = zalloc<uint8_t>(S * T, o);
    b.der_prev = zalloc<short>(S * T * 2, o); b.der_cur = zalloc<short>(S * T * 2, o);
    b.eig = zalloc<float>(S * P, o); b.mask = zalloc<uint8_t>(S * P, o); b.cand = zalloc<int>(S * P, o);
    b.prev_kps = zalloc<float>(S * K * 2, o); b.new_kps = zalloc<float>(S * K * 2, o);
    b.next_pts = zalloc<float>(S * K * 2, o); b.valid_to = zalloc<float>(S * K * 2, o);
    b.status = zalloc<uint8_t>(S * K, o);
    b.st = zalloc<bm::SofState>(S, o);
    b.warp = zalloc<double>(S * 6, o);
    h->d_ndets = zalloc<int>(S, o);
    h->d_frames = zalloc<const uint8_t*>(S, o);
    h->frame_bufs.assign(S, nullptr);
    sof_alloc_dets(h, 64);
}

// streams [s0, s0 + n): d_frame_ptrs = device table of n frame pointers; dets already on the device (d_dets [n][max_dets][stride],
// d_ndets [n], may be null); waits, copies the n warps (and the n state words, 8 ints each) out
void sof_run(BoxMOTHipSof* h, int s0, int n, const uint8_t* const* d_frame_ptrs, const float* d_dets, const int* d_ndets, int max_dets,
             int det_stride, double* out_warps, int* out_info8) {
    HipLaunch launch{h->stream};
    bm::sof_frame(launch, h->buf, h->lv, s0, n, d_frame_ptrs, h->rows, h->cols, d_dets, d_ndets, max_dets, det_stride, h->prm);
    BM_HIP(hipGetLastError());
    std::vector<bm::SofState> st((size_t)n);
    BM_HIP(hipMemcpyAsync(out_warps, h->buf.warp + (size_t)s0 * 6, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (out_info8) BM_HIP(hipMemcpyAsync(st.data(), h->buf.st + s0, (size_t)n * sizeof(bm::SofState), hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    if (out_info8)
        for (int k = 0; k < n; ++k) {
            const bm::SofState& t = st[(size_t)k];
            const int v[8] = {t.mode, t.n_prev, t.n_valid, t.n_inliers, t.ransac_iters, t.estimated, t.n_kps, t.initialized};
            for (int i = 0; i < 8; ++i) out_info8[k * 8 + i] = v[i];
        }
}

// host detections of one stream -> the handle's staging rows (first four columns: tlbr in frame pixels)
void sof_stage_dets(BoxMOTHipSof* h, int stream, const float* dets, int n_dets, int det_stride) {
    if (n_dets < 0 || (n_dets > 0 && (!dets || det_stride < 4))) throw std::runtime_error("boxmot_hip: SOF detections need >= 4 columns (tlbr)");
    if (n_dets > h->max_dets) {
        BM_HIP(hipStreamSynchronize(h->stream));
        sof_alloc_dets(h, grown(h->max_dets, n_dets));
    }
    std::vector<float> rows((size_t)(n_dets > 0 ? n_dets : 1) * 4, 0.f);
    for (int k = 0; k < n_dets; ++k) for (int c = 0; c < 4; ++c) rows[(size_t)k * 4 + c] = dets[(size_t)k * det_stride + c];
    if (n_dets > 0) BM_HIP(hipMemcpyAsync(h->d_dets + (size_t)stream * h->max_dets * 4, rows.data(), (size_t)n_dets * 16, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_ndets + stream, &n_dets, 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));            // rows / n_dets are stack and local storage
}

// The estimator that owns stream s: the handle's one estimator (one frame size per handle, from the call's arguments), or -- with
// per-stream sizes -- the estimator of that stream's size, made when a stream of the size is first estimated.
BoxMOTHipSof* sof_of(BoxMOTHipBotSort* h, int s, int image_rows, int image_cols) {
    if (h->fs_rows.empty()) {
        if (!h->sof) {
            h->sof.reset(new BoxMOTHipSof());
            sof_init(h->sof.get(), h->S, image_rows, image_cols, 0.15, 8, 0.2, 3.0, h->stream);
        }
        if (h->sof->rows != image_rows || h->sof->cols != image_cols) throw std::runtime_error("boxmot_hip: frame size changed between updates");
        return h->sof.get();
    }
    auto& e = h->sof_by_size[{h->fs_rows[s], h->fs_cols[s]}];
    if (!e) { e.reset(new BoxMOTHipSof()); sof_init(e.get(), h->S, h->fs_rows[s], h->fs_cols[s], 0.15, 8, 0.2, 3.0, h->stream); }
    return e.get();
}
BoxMOTHipEcc* ecc_of(BoxMOTHipBotSort* h, int s, int image_rows, int image_cols) {
    if (h->fs_rows.empty()) {
        if (!h->ecc) {
            h->ecc.reset(new BoxMOTHipEcc());
            ecc_init(h->ecc.get(), h->S, image_rows, image_cols, 0.15, 1e-5, 100, h->stream);
        }
        if (h->ecc->rows != image_rows || h->ecc->cols != image_cols) throw std::runtime_error("boxmot_hip: frame size changed between updates");
        return h->ecc.get();
    }
    auto& e = h->ecc_by_size[{h->fs_rows[s], h->fs_cols[s]}];
    if (!e) { e.reset(new BoxMOTHipEcc()); ecc_init(e.get(), h->S, h->fs_rows[s], h->fs_cols[s], 0.15, 1e-5, 100, h->stream); }
    return e.get();
}

// Shared host path: stage inputs of streams [s0, s0+n), run ReID if needed, step, read back.
void host_update(BoxMOTHipBotSort* h, int s0, int n, const StreamIn* in, int det_cols, int emb_cols,
                 int image_rows, int image_cols, int image_channels, const int* list_sel, const int* fc_set,
                 float* const* out, int out_capacity_rows, int* out_rows, const uint8_t* const* d_frames_ext = nullptr) {
    core_make_room(h, s0, n, in, [&](int s) {       // slots in use = tracked + lost tracks (removed ones give their slot back)
        std::vector<int> cnt(h->n_lists + 1);
        BM_HIP(hipMemcpy(cnt.data(), h->args.st.n_active + (size_t)s * h->n_lists, h->n_lists * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(cnt.data() + h->n_lists, h->args.st.n_lost + s, 4, hipMemcpyDeviceToHost));
        int used = 0;
        for (int v : cnt) used += v;
        return used;
    }, [&](int cap, int nd) { grow_tables(h, cap, nd); }, [](int c, int d) { return bm::lap_lds_bytes(c, d) <= 120 * 1024; });
    const int nd = h->nd, dim = h->dim;
    const int DC = h->det_cols, OC = h->out_cols;
    bool need_reid = false;
    for (int k = 0; k < n; ++k) {
        const int rows = in[k].det_rows;
        if (rows < -1) throw std::runtime_error("Negative matrix dimensions are not allowed.");
        if (rows > 0 && det_cols == 7 && !h->is_obb)
            throw std::runtime_error("boxmot_hip: oriented detections (7 columns) need a handle created with is_obb = 1");
        if (rows > 0 && det_cols == 6 && h->is_obb)
            throw std::runtime_error("boxmot_hip: this handle was created for oriented detections (7 columns)");
        if (rows > 0 && det_cols != DC) throw std::runtime_error("boxmot_hip live tracking supports AABB detections with 6 columns (7 with is_obb).");
        if (rows > 0 && in[k].dets == nullptr) throw std::runtime_error("Detection data pointer is null.");
        if (out_capacity_rows < rows) throw std::runtime_error("boxmot_hip: output buffer is too small for the current frame.");
        if (in[k].embs != nullptr && emb_cols != dim && rows > 0)
            throw std::runtime_error("boxmot_hip: embedding width does not match emb_dim");
        if (h->cfg.with_reid && in[k].embs == nullptr && rows > 0) need_reid = true;
    }
    if (need_reid)
        for (int k = 0; k < n; ++k)
            if (in[k].embs != nullptr && in[k].det_rows > 0)
                throw std::runtime_error("boxmot_hip: either every stream of a batch supplies embeddings or none does");
    // one staging buffer for the whole group
    float* hd = h->h_dets.data() + (size_t)s0 * nd * DC;
    for (int k = 0; k < n; ++k) {
        h->h_ndets[s0 + k] = in[k].det_rows;
        if (in[k].det_rows > 0)
            std::memcpy(hd + (size_t)k * nd * DC, in[k].dets, (size_t)in[k].det_rows * DC * 4);
        h->h_list_sel[s0 + k] = list_sel ? list_sel[k] : 0;
        h->h_fc_set[s0 + k] = fc_set ? fc_set[k] : 0;
    }
    float* d_dets = h->d_dets + (size_t)s0 * nd * DC;
    BM_HIP(hipMemcpyAsync(d_dets, hd, (size_t)n * nd * DC * 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_ndets + s0, h->h_ndets.data() + s0, n * 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_list_sel + s0, h->h_list_sel.data() + s0, n * 4, hipMemcpyHostToDevice, h->stream));
    if (fc_set) BM_HIP(hipMemcpyAsync(h->d_fc_set + s0, h->h_fc_set.data() + s0, n * 4, hipMemcpyHostToDevice, h->stream));
    const bool fanout = fc_set && !h->cmc_with_fc_set;          // per-class fan-out: the caller estimated once and supplied the warp
    const bool sof_here = h->use_sof && !fanout;
    if (sof_here) {
        // cmc_method = "sof" (botsort.py:116-117, :141-145): SOF.apply(img, dets) with the frame's whole detection table as the mask
        for (int k = 0; k < n; ++k) {
            if (in[k].det_rows < 0) continue;
            if (!in[k].image && !d_frames_ext) throw std::runtime_error("boxmot_hip: cmc_method=sof needs the frame (image pointer is null)");
            if (image_channels != 3) throw std::runtime_error("boxmot_hip: cmc_method=sof needs a 3-channel uint8 BGR image");
            if (!d_frames_ext) core_upload_frame(h, s0 + k, in[k].image, image_rows, image_cols);
        }
        for (int k = 0; k < n; ++k) {
            if (in[k].det_rows < 0) continue;
            const uint8_t* const* fp = (d_frames_ext ? d_frames_ext : h->d_frames) + (s0 + k);
            BoxMOTHipSof* sof = sof_of(h, s0 + k, image_rows, image_cols);
            if (h->is_obb) {        // botsort.py:147-158: the estimator sees the enclosing boxes of the oriented detections
                hipLaunchKernelGGL(obb_enclosing_boxes_kernel, dim3(1), dim3(256), 0, h->stream, h->d_dets, h->d_ndets, nd, h->d_cmc_boxes, s0 + k);
                sof_run(sof, s0 + k, 1, fp, h->d_cmc_boxes + (size_t)(s0 + k) * nd * 4, h->d_ndets + s0 + k, nd, 4,
                        h->h_warp.data() + (size_t)(s0 + k) * 6, nullptr);
            } else
            sof_run(sof, s0 + k, 1, fp, d_dets + (size_t)k * nd * DC, h->d_ndets + s0 + k, nd, DC,
                    h->h_warp.data() + (size_t)(s0 + k) * 6, nullptr);
            h->h_warp_flag[s0 + k] = 1;
        }
    }
    const bool ecc_here = (h->use_ecc && !fanout) || sof_here;       // below: "the frame is already uploaded"
    if (h->use_ecc && !fanout) {
        // cmc_method = "ecc" (botsort.py:116-117, :141-145): the estimator sees every frame of the stream; its warp is applied to
        // the predicted pool by this update.  (Per-class fan-out calls rewind the frame counter, fc_set: the same frame is updated
        // once per class there -- the estimate is made once by the caller and supplied with set_warp.)
        for (int k = 0; k < n; ++k) {
            if (in[k].det_rows < 0) continue;
            if (!in[k].image) throw std::runtime_error("boxmot_hip: cmc_method=ecc needs the frame (image pointer is null)");
            if (image_channels != 3) throw std::runtime_error("boxmot_hip: cmc_method=ecc needs a 3-channel uint8 BGR image");
            if (!d_frames_ext) core_upload_frame(h, s0 + k, in[k].image, image_rows, image_cols);
        }
        for (int k = 0; k < n; ++k) {
            if (in[k].det_rows < 0) continue;
            const uint8_t* const* fp = (d_frames_ext ? d_frames_ext : h->d_frames) + (s0 + k);
            ecc_run_one(ecc_of(h, s0 + k, image_rows, image_cols), s0 + k, fp, h->h_warp.data() + (size_t)(s0 + k) * 6, nullptr);
            h->h_warp_flag[s0 + k] = 1;
        }
    }
    bool any_warp = false;
    for (int k = 0; k < n; ++k) any_warp = any_warp || h->h_warp_flag[s0 + k] != 0;
    if (any_warp) {     // warps set with boxmot_hip_botsort_set_warp are consumed by this update
        BM_HIP(hipMemcpyAsync(h->d_warp + (size_t)s0 * 6, h->h_warp.data() + (size_t)s0 * 6, (size_t)n * 6 * 8, hipMemcpyHostToDevice, h->stream));
        BM_HIP(hipMemcpyAsync(h->d_warp_flag + s0, h->h_warp_flag.data() + s0, n * 4, hipMemcpyHostToDevice, h->stream));
    }
    float* d_embs = h->d_embs + (size_t)s0 * nd * dim;
    for (int k = 0; k < n; ++k)
        if (in[k].embs && in[k].det_rows > 0)
            BM_HIP(hipMemcpyAsync(d_embs + (size_t)k * nd * dim, in[k].embs, (size_t)in[k].det_rows * dim * 4,
                                  hipMemcpyHostToDevice, h->stream));
    h->last_reid_pre_ms = h->last_reid_proc_ms = 0;
    if (need_reid && d_frames_ext) {       // frames already on the device (ingest ring slot): no upload
        if (s0 != 0) throw std::runtime_error("boxmot_hip: device frames are addressed from stream 0");
        run_reid(h, h->stream, s0, n, h->d_dets, h->d_ndets, d_frames_ext, image_rows, image_cols, h->d_embs);
    } else if (need_reid) {
        for (int k = 0; k < n; ++k) {
            if (in[k].image && !ecc_here) {
                if (image_channels != 3) throw std::runtime_error("boxmot_hip: ReID needs a 3-channel uint8 BGR image");
                core_upload_frame(h, s0 + k, in[k].image, image_rows, image_cols);
            } else if (!in[k].image && h->frame_bufs[s0 + k] == nullptr) throw std::runtime_error("Image data pointer is null.");
        }
        run_reid(h, h->stream, s0, n, h->d_dets, h->d_ndets, h->d_frames, h->frame_rows, h->frame_cols, h->d_embs);
    }
    BM_HIP(hipEventRecord(h->ev[0], h->stream));
    launch_step(h, s0, n, h->d_dets, h->d_ndets, h->cfg.with_reid ? h->d_embs : nullptr, h->d_list_sel,
                fc_set ? h->d_fc_set : nullptr, h->d_out, h->d_out_n, any_warp);
    BM_HIP(hipEventRecord(h->ev[1], h->stream));
    BM_HIP(hipMemcpyAsync(h->h_out_n.data(), h->d_out_n + s0, n * 4, hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipMemcpyAsync(h->h_out.data(), h->d_out + (size_t)s0 * nd * OC, (size_t)n * nd * OC * 4,
                          hipMemcpyDeviceToHost, h->stream));
    const int nl = h->n_lists;
    BM_HIP(hipMemcpyAsync(h->h_count_buf.data(), h->args.st.n_active + (size_t)s0 * nl, (size_t)n * nl * 4, hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipMemcpyAsync(h->h_count_buf.data() + (size_t)n * nl, h->args.st.n_lost + s0, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < n; ++k) {           // slots in use = tracked + lost tracks (removed ones give their slot back)
        int used = h->h_count_buf[(size_t)n * nl + k];
        for (int l = 0; l < nl; ++l) used += h->h_count_buf[(size_t)k * nl + l];
        h->h_used[s0 + k] = used;
    }
    for (int k = 0; k < n; ++k) h->h_warp_flag[s0 + k] = 0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess) h->last_track_ms = ms;
    if (need_reid) h->reid->last_times(h->last_reid_pre_ms, h->last_reid_proc_ms);
    const std::string status_msg = take_status(h->stream, h->args.st.status, s0, n, h->cfg.tracker_kind == 1 ? "ByteTrack" : "BoT-SORT");
    for (int k = 0; k < n; ++k) {
        const int rows = h->h_out_n[k];
        if (rows > out_capacity_rows) throw std::runtime_error("boxmot_hip: output buffer is too small for the current frame.");
        copy_rows9(h->h_out.data() + (size_t)k * nd * OC, rows, OC, out[k]);
        out_rows[k] = rows;
    }
    if (!status_msg.empty()) throw std::runtime_error(status_msg);      // rows of this frame are in `out` all the same
}

// single stream at an arbitrary index: run it as a one-stream group by offsetting the args
void host_update_one(BoxMOTHipBotSort* h, int stream, int class_list, int frame_count, const StreamIn& in,
                     int det_cols, int emb_cols, int rows, int cols, int channels, float* out, int out_cap,
                     int* out_rows) {
    if (stream < 0 || stream >= h->S) throw std::runtime_error("boxmot_hip: stream index out of range");
    if (class_list < 0 || class_list >= h->n_lists) throw std::runtime_error("boxmot_hip: class list out of range");
    float* outs[1] = {out};
    const int sel[1] = {class_list};
    const int fc[1] = {frame_count};
    host_update(h, stream, 1, &in, det_cols, emb_cols, rows, cols, channels, sel, frame_count >= 0 ? fc : nullptr, outs,
                out_cap, out_rows);
}


// ---------------------------------------------------------------------------
// StreamIo: shared host plumbing of the DeepOCSORT / StrongSORT handles
// ---------------------------------------------------------------------------
std::unique_ptr<bm::ReidEngine> io_new_reid(StreamIo* h, int nd) {
    std::unique_ptr<bm::ReidEngine> e = core_new_reid(h, nd);
    if (h->reid_mode >= 0) e->set_mode(h->reid_mode);
    return e;
}

void io_allocate(StreamIo* h, int S, int cap, int nd, int dim, bool with_reid) {
    h->S = S; h->cap = cap; h->nd = nd; h->dim = dim;
    BM_HIP(hipStreamCreate(&h->stream));
    {
        const char* v = std::getenv("BOXMOT_HIP_PIPELINE");
        h->pipe = !(v && v[0] == '0');
        if (h->pipe) core_pipe_create(h);
    }
    auto& o = h->owned;
    const size_t s = S;
    core_alloc_sized(h, h->cap, h->cap);        // result rows: [S][cap] on the device, one stream's at a time on the host
    h->d_ndets = zalloc<int>(s, o);
    h->d_out_n = zalloc<int>(s, o);
    h->d_warp = zalloc<double>(s * 6, o);
    h->d_warp_flag = zalloc<int>(s, o);
    h->h_ndets.assign(s, 0); h->h_out_n.assign(s, 0); h->h_used.assign(s, 0);
    h->h_warp.assign(s * 6, 0.0); h->h_warp_flag.assign(s, 0);
    h->frame_bufs.assign(s, nullptr);
    h->d_frames = zalloc<const uint8_t*>(s, o);
    h->d_crop_count = zalloc<int>(2, o);        // [0] the count, [1] the bound-overflow flag
    h->d_ndets_step[0] = zalloc<int>(s, o); h->d_ndets_step[1] = zalloc<int>(s, o);
    if (with_reid && !h->reid_path.empty()) h->reid = io_new_reid(h, h->nd);
}

// core_make_room for these handles: the slots in use are the tracker's n_tracks word, and the stream is drained before the tables
// are re-made
template <class Grow, class Fits>
void io_make_room(StreamIo* h, int s0, int n, const StreamIn* in, const int* d_n_tracks, Grow grow, Fits fits) {
    core_make_room(h, s0, n, in,
                   [&](int s) { int used = 0; BM_HIP(hipMemcpy(&used, d_n_tracks + s, 4, hipMemcpyDeviceToHost)); return used; },
                   [&](int cap, int nd) { BM_HIP(hipStreamSynchronize(h->stream)); grow(cap, nd); }, fits);
}

// Device-resident steps: the warps set with *_set_warp since the last step are consumed by this one (identity for the streams
// without a pending warp).  Returns whether any stream had one; the caller clears the flags after launching.
bool io_consume_warps(StreamIo* h) {
    bool any_warp = false;
    for (int s = 0; s < h->S; ++s) any_warp = any_warp || h->h_warp_flag[s] != 0;
    if (!any_warp) return false;
    for (int s = 0; s < h->S; ++s)
        if (!h->h_warp_flag[s]) { double* w = h->h_warp.data() + (size_t)s * 6; w[0] = 1; w[1] = 0; w[2] = 0; w[3] = 0; w[4] = 1; w[5] = 0; }
    // h_warp / h_warp_flag are rewritten by the next set_warp: the copies read a staging slot of their own, reused (after its event)
    // eight steps later -- no wait for the stream here
    const int k = (int)(h->warp_slot++ % StreamIo::WARP_SLOTS);
    if (h->warp_ev[k]) BM_HIP(hipEventSynchronize(h->warp_ev[k]));
    else BM_HIP(hipEventCreateWithFlags(&h->warp_ev[k], hipEventDisableTiming));
    h->warp_stage[k].assign(h->h_warp.begin(), h->h_warp.begin() + (size_t)h->S * 6);
    h->warp_flag_stage[k].assign(h->h_warp_flag.begin(), h->h_warp_flag.begin() + h->S);
    BM_HIP(hipMemcpyAsync(h->d_warp, h->warp_stage[k].data(), (size_t)h->S * 6 * 8, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_warp_flag, h->warp_flag_stage[k].data(), h->S * 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipEventRecord(h->warp_ev[k], h->stream));
    return true;
}
// after a device-resident step: pending warps are consumed, and the host no longer knows the track counts (io_make_room asks)
void io_clear_warps(StreamIo* h) { for (int s = 0; s < h->S; ++s) { h->h_warp_flag[s] = 0; h->h_used[s] = -1; } }

// Validate and upload the inputs of the first n streams; run the ReID engine on every detection passing the confidence
// test (`conf > thresh`, or `>=` when inclusive) when embeddings are wanted and not supplied.  Streams without a pending
// warp get the identity.  Returns whether any stream has a pending warp.
bool io_stage(StreamIo* h, int n, const StreamIn* in, int det_cols, int emb_cols, bool want_emb, int image_rows, int image_cols,
              int image_channels, int out_capacity_rows, double reid_thresh, int inclusive, int s0 = 0) {
    const int nd = h->nd, dim = h->dim;
    const size_t DC = h->det_cols;
    if (s0 < 0 || n < 1 || s0 + n > h->S) throw std::runtime_error("boxmot_hip: stream index out of range");
    bool need_reid = false;
    for (int k = 0; k < n; ++k) {
        const int rows = in[k].det_rows;
        if (rows < -1) throw std::runtime_error("Negative matrix dimensions are not allowed.");
        if (rows > 0 && det_cols != h->det_cols)
            throw std::runtime_error(h->det_cols == 7 ? "boxmot_hip: this handle was created for oriented detections (7 columns)"
                                     : det_cols == 7 ? "boxmot_hip: oriented detections (7 columns) need a handle created with is_obb = 1 (BoT-SORT, ByteTrack, OC-SORT)"
                                                     : "boxmot_hip live tracking supports AABB detections with 6 columns.");
        if (rows > nd) throw std::runtime_error("boxmot_hip: internal: detection tables were not grown before staging");
        if (rows > 0 && in[k].dets == nullptr) throw std::runtime_error("Detection data pointer is null.");
        if (out_capacity_rows < rows) throw std::runtime_error("boxmot_hip: output buffer is too small for the current frame.");
        if (want_emb && in[k].embs != nullptr && emb_cols != dim && rows > 0)
            throw std::runtime_error("boxmot_hip: embedding width does not match emb_dim");
        if (want_emb && in[k].embs == nullptr && rows > 0) need_reid = true;
    }
    if (need_reid)
        for (int k = 0; k < n; ++k)
            if (in[k].embs != nullptr && in[k].det_rows > 0)
                throw std::runtime_error("boxmot_hip: either every stream of a batch supplies embeddings or none does");
    bool any_warp = false;
    for (int k = 0; k < n; ++k) {
        const size_t sk = (size_t)(s0 + k);
        h->h_ndets[sk] = in[k].det_rows;
        if (in[k].det_rows > 0)
            std::memcpy(h->h_dets.data() + sk * nd * DC, in[k].dets, (size_t)in[k].det_rows * DC * 4);
        if (h->h_warp_flag[sk]) any_warp = true;
        else { double* w = h->h_warp.data() + sk * 6; w[0] = 1; w[1] = 0; w[2] = 0; w[3] = 0; w[4] = 1; w[5] = 0; }
    }
    const size_t o = (size_t)s0;
    BM_HIP(hipMemcpyAsync(h->d_dets + o * nd * DC, h->h_dets.data() + o * nd * DC, (size_t)n * nd * DC * 4,
                          hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_ndets + o, h->h_ndets.data() + o, n * 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_warp + o * 6, h->h_warp.data() + o * 6, (size_t)n * 6 * 8, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_warp_flag + o, h->h_warp_flag.data() + o, n * 4, hipMemcpyHostToDevice, h->stream));
    if (want_emb)
        for (int k = 0; k < n; ++k)
            if (in[k].embs && in[k].det_rows > 0)
                BM_HIP(hipMemcpyAsync(h->d_embs + (size_t)(s0 + k) * nd * dim, in[k].embs, (size_t)in[k].det_rows * dim * 4,
                                      hipMemcpyHostToDevice, h->stream));
    if (!need_reid) return any_warp;
    if (!h->reid) throw std::runtime_error("boxmot_hip: embeddings are needed and none were supplied, but no ReID weights are loaded");
    if (image_channels != 3) throw std::runtime_error("boxmot_hip: ReID needs a 3-channel uint8 BGR image");
    for (int k = 0; k < n; ++k) {
        if (in[k].image) core_upload_frame(h, s0 + k, in[k].image, image_rows, image_cols);
        else if (!h->frame_bufs[s0 + k]) throw std::runtime_error("Image data pointer is null.");
    }
    h->engine_on_main = true;           // (a later pipelined step_device_frames orders its ReID pass after this use)
    core_reid_pass(h, h->stream, s0, n, h->d_dets, h->d_ndets, h->d_frames, h->frame_rows, h->frame_cols, reid_thresh, inclusive, h->d_embs);
    return any_warp;
}

// Device-resident ReID for the DeepOCSORT / StrongSORT step_device_frames entry points: crop list from the caller's device
// detections, backbone over the caller's device frames, embeddings into h->d_embs (rows of skipped detections keep stale
// values; the step kernels never read them).
float* io_device_reid(StreamIo* h, const float* d_dets, const int* d_ndets, const uint8_t* const* d_frames, int image_rows,
                      int image_cols, double reid_thresh, int inclusive) {
    if (!h->reid) throw std::runtime_error("boxmot_hip: embeddings are needed and none were supplied, but no ReID weights are loaded");
    if (!d_frames || (h->fs_rows.empty() && (image_rows <= 0 || image_cols <= 0))) throw std::runtime_error("boxmot_hip: step_device_frames needs device frames");
    // pipeline stage 1: this frame's ReID on `reid_stream`, into the table the step before last has finished reading
    hipStream_t rs = core_pipe_begin_reid(h);
    float* embs = core_pipe_table(h);
    int* nd_step = h->d_ndets_step[core_pipe_on(h) ? h->pipe_slot : 0];        // (alternates with the embedding table: read by this call's step)
    h->step_ndets = d_ndets;
    if (core_reid_pass(h, rs, 0, h->S, d_dets, d_ndets, d_frames, image_rows, image_cols, reid_thresh, inclusive, embs, h->crop_bound, nd_step,
                       &h->bounded_step_pending))
        h->step_ndets = nd_step;
    core_pipe_reid_done(h);
    return embs;
}

void io_set_crop_bound(StreamIo* h, int max_total_crops) {
    if (max_total_crops < -1) throw std::runtime_error("boxmot_hip: crop bound must be >= 0, or -1 to read the count back");
    h->crop_bound = max_total_crops;
}
// after a stream synchronisation: a step whose crops exceeded the declared bound left detections without an embedding
// (latched on the host when a bounded step is queued, not read off the CURRENT bound: a caller that runs bounded steps and then
// sets the bound back to -1 before synchronising still sees the overflow of the earlier steps)
void io_check_crop_bound(StreamIo* h) {
    if (!h->bounded_step_pending || !h->d_crop_count) return;
    h->bounded_step_pending = false;
    int flag = 0;
    BM_HIP(hipMemcpy(&flag, h->d_crop_count + 1, 4, hipMemcpyDeviceToHost));
    if (flag) {
        BM_HIP(hipMemset(h->d_crop_count + 1, 0, 4));
        throw std::runtime_error("boxmot_hip: a device-resident step had more ReID crops than the bound declared with set_crop_bound");
    }
}

// After the step kernel: wait, clear the consumed warps, turn a non-zero status word into an exception, copy the rows out.
void io_read_back(StreamIo* h, int n, const int* d_status, const char* tracker, float* const* out, int out_capacity_rows, int* out_rows,
                  int s0 = 0, const int* d_n_tracks = nullptr) {
    BM_HIP(hipGetLastError());
    BM_HIP(hipMemcpyAsync(h->h_out_n.data(), h->d_out_n + s0, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (d_n_tracks) BM_HIP(hipMemcpyAsync(h->h_used.data() + s0, d_n_tracks + s0, n * 4, hipMemcpyDeviceToHost, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    // an earlier device-resident step whose crops exceeded the declared bound (that frame was not stepped): reported AFTER this
    // update's read-back is complete -- its step has run on the device, so its rows are returned and its warps are cleared first
    std::string bound_msg;
    try { io_check_crop_bound(h); } catch (const std::exception& e) { bound_msg = e.what(); }
    for (int k = 0; k < n; ++k) h->h_warp_flag[s0 + k] = 0;
    const std::string status_msg = take_status(h->stream, const_cast<int*>(d_status), s0, n, tracker);
    for (int k = 0; k < n; ++k) {
        const int rows = h->h_out_n[k];
        if (rows > out_capacity_rows) throw std::runtime_error("boxmot_hip: output buffer is too small for the current frame.");
        const size_t OC = h->out_cols;
        if (rows) BM_HIP(hipMemcpy(h->h_out.data(), h->d_out + (size_t)(s0 + k) * h->cap * OC, (size_t)rows * OC * 4, hipMemcpyDeviceToHost));
        copy_rows9(h->h_out.data(), rows, (int)OC, out[k]);
        out_rows[k] = rows;
    }
    if (!status_msg.empty()) throw std::runtime_error(status_msg);      // rows of this frame are in `out` all the same
    if (!bound_msg.empty())         // (the "<tracker> stream <n>: " shape tells the host classes that this update's step ran: _lib.step_ran)
        throw std::runtime_error(std::string("boxmot_hip: ") + tracker + " stream " + std::to_string(s0) + ": an EARLIER step reported: " + bound_msg);
}

// ---------------------------------------------------------------------------
// DeepOCSORT host path
// ---------------------------------------------------------------------------
const void* docs_kernel(const BoxMOTHipDeepOcSort* h) {
    return h->is_obb ? reinterpret_cast<const void*>(deepocsort_obb_step_kernel<STEP_THREADS>)
                     : reinterpret_cast<const void*>(deepocsort_step_kernel<STEP_THREADS>);
}
void docs_set_lds(BoxMOTHipDeepOcSort* h, long lds) {
    BM_HIP(hipFuncSetAttribute(docs_kernel(h), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
}
void docs_launch(BoxMOTHipDeepOcSort* h, int n_streams, const bm::DocsStepArgs& a) {
    const size_t lds = (size_t)bm::docs_lap_lds_bytes(h->cap, h->nd);
    if (h->is_obb) hipLaunchKernelGGL((deepocsort_obb_step_kernel<STEP_THREADS>), dim3(n_streams), dim3(STEP_THREADS), lds, h->stream, a);
    else hipLaunchKernelGGL((deepocsort_step_kernel<STEP_THREADS>), dim3(n_streams), dim3(STEP_THREADS), lds, h->stream, a);
}

void docs_zero_state(BoxMOTHipDeepOcSort* h) {
    bm::DocsState& st = h->args.st;
    const size_t S = h->S, cap = h->cap;
    BM_HIP(hipMemsetAsync(st.frame_count, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.id_count, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.n_tracks, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.status, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.slot_used, 0, S * cap * 4, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
}

// centroid's norm_factor = np.sqrt(self.w**2 + self.h**2) (iou.py:266) of the frame size the tracker read off its first image
// (basetracker.py:175-180); 0 x 0 = not known yet
void docs_set_frame_size(BoxMOTHipDeepOcSort* h, int w, int hgt) {
    if (w < 0 || hgt < 0) throw std::runtime_error("boxmot_hip: frame size must not be negative");
    h->args.cfg.asso_diag = (w > 0 && hgt > 0) ? std::sqrt((double)((long)w * w + (long)hgt * hgt)) : 0.0;
}
// a step is about to run: `centroid` needs the frame size (host updates carry it with the image; device-resident steps do not)
void docs_need_frame_size(BoxMOTHipDeepOcSort* h, int image_rows, int image_cols) {
    if (h->args.cfg.asso_mode != BOXMOT_HIP_ASSO_CENTROID || h->args.cfg.asso_diag > 0.0) return;
    if (image_rows > 0 && image_cols > 0) { docs_set_frame_size(h, image_cols, image_rows); return; }
    throw std::runtime_error("boxmot_hip: asso_func centroid needs the frame size (config frame_w / frame_h, or a host update with an image first)");
}

void docs_build(BoxMOTHipDeepOcSort* h) {
    const BoxMOTHipDeepOcSortConfig& c = h->cfg;
    if (c.n_streams < 1 || c.max_tracks < 8 || c.max_dets < 4 || c.emb_dim < 1)
        throw std::runtime_error("boxmot_hip: invalid capacity configuration");
    if (c.max_age < 0 || c.max_age > 45)
        throw std::runtime_error("boxmot_hip: DeepOCSORT max_age must be in [0, 45] (the reference's 50-entry observation history, xysr.py:18)");
    if (c.delta_t < 1 || c.delta_t > 3) throw std::runtime_error("boxmot_hip: DeepOCSORT delta_t must be 1..3");
    if (!(c.aw_param < 1.0)) throw std::runtime_error("boxmot_hip: aw_param must be < 1");
    h->is_obb = c.is_obb != 0;
    if (h->is_obb) {
        // oriented detections: OC-SORT (ocsort.py:332 supports_obb; DeepOcSort does not): no appearance, no camera motion, and the
        // association function is the rotated IoU (detection_layout.py:25-26 turns "iou" into "iou_obb")
        if (!c.embedding_off) throw std::runtime_error("boxmot_hip: oriented detections run on OC-SORT (embedding_off = 1); DeepOCSORT takes axis-aligned boxes only");
        if (c.asso_func != BOXMOT_HIP_ASSO_IOU && c.asso_func != BOXMOT_HIP_ASSO_CENTROID)
            throw std::runtime_error("boxmot_hip: the oriented step has the rotated IoU and the centroid distance (asso_func must be BOXMOT_HIP_ASSO_IOU or _CENTROID)");
        h->det_cols = bm::obb::DOCS_DET_COLS; h->out_cols = bm::obb::DOCS_OUT_COLS;
    }
    io_allocate(h, c.n_streams, c.max_tracks, c.max_dets, c.embedding_off ? 1 : c.emb_dim, !c.embedding_off);
    bm::DocsConfigDev& d = h->args.cfg;
    d.det_thresh = c.det_thresh; d.det_thresh_f32 = (float)c.det_thresh; d.max_age = c.max_age; d.min_hits = c.min_hits;
    d.delta_t = c.delta_t; d.iou_threshold = c.iou_threshold; d.inertia = c.inertia; d.w_emb = c.w_association_emb;
    d.alpha_fixed = c.alpha_fixed_emb; d.aw_param = c.aw_param; d.q_xy = c.Q_xy_scaling; d.q_s = c.Q_s_scaling;
    d.embedding_off = c.embedding_off; d.aw_off = c.aw_off;
    if (c.use_byte && !c.embedding_off) throw std::runtime_error("boxmot_hip: use_byte is OC-SORT's option and needs embedding_off = 1");
    d.use_byte = c.use_byte ? 1 : 0; d.min_conf_f32 = (float)c.min_conf;
    if (c.asso_func < BOXMOT_HIP_ASSO_IOU || c.asso_func > BOXMOT_HIP_ASSO_CENTROID)
        throw std::runtime_error("boxmot_hip: asso_func must be one of BOXMOT_HIP_ASSO_* (iou, giou, diou, ciou, hmiou, centroid)");
    d.asso_mode = c.asso_func;
    docs_set_frame_size(h, c.frame_w, c.frame_h);
    RecAlloc table_allocator{&h->owned, &h->table_rec};
    bm::DocsSizes z{h->S, h->cap, h->nd, h->dim, h->is_obb ? 1 : 0};
    bm::docs_allocate(h->args, z, table_allocator);
    const long lds = bm::docs_lap_lds_bytes(h->cap, h->nd);
    if (lds > 120 * 1024) throw std::runtime_error("boxmot_hip: max_tracks/max_dets too large for the assignment solver's LDS state");
    docs_set_lds(h, lds);
}

// debug cost planes of the DeepOCSORT step (boxmot_hip_deepocsort_debug_costs_enable): made at the tables' current sizes
void docs_make_dbg(BoxMOTHipDeepOcSort* h) {
    if (h->args.dbg_cost) { release(h->owned, h->args.dbg_cost); release(h->owned, h->args.dbg_shape); }
    h->args.dbg_cost = zalloc<double>((size_t)h->S * bm::DOCS_DBG_PLANES * h->nd * h->cap, h->owned);
    h->args.dbg_shape = zalloc<int>((size_t)h->S * 4, h->owned);
    h->dbg_cap = h->cap; h->dbg_nd = h->nd;
}

void docs_grow(BoxMOTHipDeepOcSort* h, int new_cap, int new_nd) {
    const long lds = bm::docs_lap_lds_bytes(new_cap, new_nd);
    if (lds > 120 * 1024)
        throw std::runtime_error("boxmot_hip: " + std::to_string(new_cap) + " tracks x " + std::to_string(new_nd) +
                                 " detections per stream is beyond what the assignment solver's LDS state can hold");
    BM_HIP(hipStreamSynchronize(h->stream));
    std::unique_ptr<bm::ReidEngine> new_reid;           // first: a failure leaves the handle as it was
    if (h->reid && new_nd != h->nd) new_reid = io_new_reid(h, new_nd);
    bm::DocsStepArgs na = h->args;
    std::vector<std::pair<void*, size_t>> rec;
    RecAlloc ra{&h->owned, &rec};
    bm::docs_allocate(na, bm::DocsSizes{h->S, new_cap, new_nd, h->dim, h->is_obb ? 1 : 0}, ra);
    core_migrate(h, rec, na.sc.keep);
    h->args = na;
    const bool more_dets = new_nd != h->nd;
    h->cap = new_cap; h->nd = new_nd;
    core_alloc_sized(h, h->cap, h->cap);        // result rows: [S][cap] on the device, one stream's at a time on the host
    if (new_reid) h->reid = std::move(new_reid);
    docs_set_lds(h, lds);
    if (h->args.dbg_cost) docs_make_dbg(h);
    ++h->n_grows;
}

// Stage the inputs of the first n streams (ReID on every detection above det_thresh when embeddings are not supplied,
// deepocsort.py:337-345), step, read back.
void docs_host_update(BoxMOTHipDeepOcSort* h, int n, const StreamIn* in, int det_cols, int emb_cols, int image_rows,
                      int image_cols, int image_channels, float* const* out, int out_capacity_rows, int* out_rows, int s0 = 0,
                      int frame_count = -1, int* id_count_inout = nullptr) {
    const bool want_emb = !h->cfg.embedding_off;
    io_make_room(h, s0, n, in, h->args.st.n_tracks, [&](int cap, int nd) { docs_grow(h, cap, nd); },
                 [](int cap, int nd) { return bm::docs_lap_lds_bytes(cap, nd) <= 120 * 1024; });
    const bool any_warp = io_stage(h, n, in, det_cols, emb_cols, want_emb, image_rows, image_cols, image_channels, out_capacity_rows,
                                   (double)(float)h->cfg.det_thresh, 0, s0);
    // per-class fan-out (basetracker.py:223-263): the frame counter is rewound for every class and the id counter
    // (KalmanBoxTracker.count, deepocsort.py:57,117-118) is shared by all of them
    if (frame_count >= 0) BM_HIP(hipMemcpyAsync(h->args.st.frame_count + s0, &frame_count, 4, hipMemcpyHostToDevice, h->stream));
    if (id_count_inout) BM_HIP(hipMemcpyAsync(h->args.st.id_count + s0, id_count_inout, 4, hipMemcpyHostToDevice, h->stream));
    bm::DocsStepArgs a = h->args;
    a.dets = h->d_dets; a.n_dets = h->d_ndets; a.embs = want_emb ? h->d_embs : nullptr;
    a.warp = any_warp ? h->d_warp : nullptr; a.warp_flag = any_warp ? h->d_warp_flag : nullptr;
    a.out = h->d_out; a.out_n = h->d_out_n; a.stream_base = s0;
    docs_launch(h, n, a);
    io_read_back(h, n, h->args.st.status, "DeepOCSORT", out, out_capacity_rows, out_rows, s0, h->args.st.n_tracks);
    if (id_count_inout) BM_HIP(hipMemcpy(id_count_inout, h->args.st.id_count + s0, 4, hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------------------
// StrongSORT host path
// ---------------------------------------------------------------------------
constexpr int SS_BANK_THREADS = 256;

void ss_zero_state(BoxMOTHipStrongSort* h) {
    bm::SsState& st = h->args.st;
    const size_t S = h->S, cap = h->cap;
    std::vector<int> ones(S, 1);
    BM_HIP(hipMemsetAsync(st.frame_count, 0, S * 4, h->stream));
    BM_HIP(hipMemcpyAsync(st.next_id, ones.data(), S * 4, hipMemcpyHostToDevice, h->stream));     // Tracker._next_id = 1, tracker.py:59
    BM_HIP(hipMemsetAsync(st.n_tracks, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.status, 0, S * 4, h->stream));
    BM_HIP(hipMemsetAsync(st.slot_used, 0, S * cap * 4, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
}

void ss_build(BoxMOTHipStrongSort* h) {
    const BoxMOTHipStrongSortConfig& c = h->cfg;
    if (c.n_streams < 1 || c.max_tracks < 8 || c.max_dets < 4 || c.emb_dim < 1)
        throw std::runtime_error("boxmot_hip: invalid capacity configuration");
    if (c.nn_budget < 1 || c.nn_budget > 1024) throw std::runtime_error("boxmot_hip: StrongSORT nn_budget must be in [1, 1024] (None is not supported)");
    if (c.n_init < 1 || c.max_age < 0) throw std::runtime_error("boxmot_hip: invalid n_init / max_age");
    { const char* v = std::getenv("BOXMOT_HIP_SS_BANK"); h->bank_valu = v && std::strcmp(v, "valu") == 0; }
    io_allocate(h, c.n_streams, c.max_tracks, c.max_dets, c.emb_dim, true);
    bm::SsConfigDev& d = h->args.cfg;
    d.min_conf = c.min_conf; d.max_cos_dist = c.max_cos_dist; d.max_iou_dist = c.max_iou_dist; d.mc_lambda = c.mc_lambda;
    d.ema_alpha_f32 = (float)c.ema_alpha; d.one_minus_alpha_f32 = (float)(1 - c.ema_alpha);
    d.max_age = c.max_age; d.n_init = c.n_init; d.budget = c.nn_budget;
    RecAlloc table_allocator{&h->owned, &h->table_rec};
    bm::SsSizes z{h->S, h->cap, h->nd, h->dim, c.nn_budget};
    bm::ss_allocate(h->args, z, table_allocator);
    const long lds = bm::ss_lsa_lds_bytes(h->cap > h->nd ? h->cap : h->nd);
    if (lds > 120 * 1024) throw std::runtime_error("boxmot_hip: max_tracks/max_dets too large for the assignment solver's LDS state");
    BM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(strongsort_step_kernel<STEP_THREADS>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    BM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(strongsort_step_kernel<SS_STEP_THREADS_BIG>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ss_zero_state(h);
}

// debug cost planes of the StrongSORT step (boxmot_hip_strongsort_debug_costs_enable)
void ss_make_dbg(BoxMOTHipStrongSort* h) {
    if (h->args.dbg_cost) { release(h->owned, h->args.dbg_cost); release(h->owned, h->args.dbg_shape); }
    const size_t big = h->cap > h->nd ? h->cap : h->nd;
    h->args.dbg_cost = zalloc<double>((size_t)h->S * 4 * big * big, h->owned);
    h->args.dbg_shape = zalloc<int>((size_t)h->S * 4, h->owned);
    h->dbg_big = (int)big;
}

void ss_grow(BoxMOTHipStrongSort* h, int new_cap, int new_nd) {
    const long lds = bm::ss_lsa_lds_bytes(new_cap > new_nd ? new_cap : new_nd);
    if (lds > 120 * 1024)
        throw std::runtime_error("boxmot_hip: " + std::to_string(new_cap) + " tracks x " + std::to_string(new_nd) +
                                 " detections per stream is beyond what the assignment solver's LDS state can hold");
    BM_HIP(hipStreamSynchronize(h->stream));
    bm::SsStepArgs na = h->args;
    std::vector<std::pair<void*, size_t>> rec;
    RecAlloc ra{&h->owned, &rec};
    bm::ss_allocate(na, bm::SsSizes{h->S, new_cap, new_nd, h->dim, h->cfg.nn_budget}, ra);
    core_migrate(h, rec, na.sc.app);
    h->args = na;
    const bool more_dets = new_nd != h->nd;
    h->cap = new_cap; h->nd = new_nd;
    core_alloc_sized(h, h->cap, h->cap);        // result rows: [S][cap] on the device, one stream's at a time on the host
    if (more_dets && h->reid) h->reid = io_new_reid(h, h->nd);
    BM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(strongsort_step_kernel<STEP_THREADS>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    BM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(strongsort_step_kernel<SS_STEP_THREADS_BIG>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (h->args.dbg_cost) ss_make_dbg(h);
    ++h->n_grows;
}

#ifdef BM_SS_PROF
// tools only: phase clocks of strongsort_step_kernel (workgroup 0), cleared on read
extern "C" int boxmot_hip_debug_ss_prof(unsigned long long* out16) {
    unsigned long long zero[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(bm::g_ss_prof), sizeof(zero)) != hipSuccess) return 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(bm::g_ss_prof), zero, sizeof(zero)) == hipSuccess;
}
#endif

// detection norms -> sample-bank distances of every confirmed track (state BEFORE this frame's step) -> frame step
void ss_launch(BoxMOTHipStrongSort* h, const bm::SsStepArgs& a, int n) {
    hipLaunchKernelGGL((strongsort_detnorm_kernel<SS_BANK_THREADS>), dim3(n, h->nd >= 128 ? 16 : 1), dim3(SS_BANK_THREADS), 0, h->stream, a);
    // sample-bank distances: fp32 matrix pipe (budgets up to 112 samples; bit-identical sums), else / on request the scalar-FMA kernel
    if (h->cfg.nn_budget <= bm::SS_MT * 16 && !h->bank_valu)
        hipLaunchKernelGGL((strongsort_bank_mfma_kernel<SS_BANK_THREADS>), dim3(h->cap, n), dim3(SS_BANK_THREADS), 0, h->stream, a);
    else
        hipLaunchKernelGGL((strongsort_bank_kernel<SS_BANK_THREADS>), dim3(h->cap, n), dim3(SS_BANK_THREADS), 0, h->stream, a);
    // one workgroup per stream: 16 waves when the track table is large (the per-match / per-track phases run a wave per item)
    if (h->cap >= 1024)
        hipLaunchKernelGGL((strongsort_step_kernel<SS_STEP_THREADS_BIG>), dim3(n), dim3(SS_STEP_THREADS_BIG),
                           (size_t)bm::ss_lsa_lds_bytes(h->cap > h->nd ? h->cap : h->nd), h->stream, a);
    else
        hipLaunchKernelGGL((strongsort_step_kernel<STEP_THREADS>), dim3(n), dim3(STEP_THREADS),
                           (size_t)bm::ss_lsa_lds_bytes(h->cap > h->nd ? h->cap : h->nd), h->stream, a);
}

// Stage the inputs of the first n streams (ReID on every detection with conf >= min_conf when embeddings are not supplied,
// strongsort.py:74-91), step, read back.
void ss_host_update(BoxMOTHipStrongSort* h, int n, const StreamIn* in, int det_cols, int emb_cols, int image_rows,
                    int image_cols, int image_channels, float* const* out, int out_capacity_rows, int* out_rows) {
    io_make_room(h, 0, n, in, h->args.st.n_tracks, [&](int cap, int nd) { ss_grow(h, cap, nd); },
                 [](int cap, int nd) { return bm::ss_lsa_lds_bytes(cap > nd ? cap : nd) <= 120 * 1024; });
    io_stage(h, n, in, det_cols, emb_cols, true, image_rows, image_cols, image_channels, out_capacity_rows, h->cfg.min_conf, 1);
    bm::SsStepArgs a = h->args;
    a.dets = h->d_dets; a.n_dets = h->d_ndets; a.embs = h->d_embs; a.warp = h->d_warp;     // identity where no warp is pending
    a.out = h->d_out; a.out_n = h->d_out_n; a.stream_base = 0;
    ss_launch(h, a, n);
    io_read_back(h, n, h->args.st.status, "StrongSORT", out, out_capacity_rows, out_rows, 0, h->args.st.n_tracks);
}

// ---------------------------------------------------------------------------
// Entry points that are the same for every tracker handle: `name` is the tracker as the messages spell it
// ---------------------------------------------------------------------------
void need_handle(const void* h, const char* name, const char* what) {
    if (!h) throw std::runtime_error(std::string("boxmot_hip ") + name + " handle is " + what);
}

template <class H, class Zero>
int ep_reset(H* h, const char* name, Zero zero_state) {
    return guard_on(h, [&]() {
        need_handle(h, name, "null.");
        zero_state(h);
        h->h_used.assign(h->S, 0);
    });
}

template <class H, class Grow>
int ep_reserve(H* h, const char* name, int max_tracks, int max_dets, Grow grow) {
    return guard_on(h, [&]() {
        need_handle(h, name, "null.");
        const int cap = max_tracks > h->cap ? (max_tracks + 63) / 64 * 64 : h->cap;
        const int nd = max_dets > h->nd ? (max_dets + 63) / 64 * 64 : h->nd;
        if (cap != h->cap || nd != h->nd) grow(h, cap, nd);
    });
}

template <class H>
int ep_capacity(H* h, const char* name, int* max_tracks, int* max_dets, int* n_grows) {
    return guard_on(h, [&]() {
        need_handle(h, name, "null.");
        if (max_tracks) *max_tracks = h->cap;
        if (max_dets) *max_dets = h->nd;
        if (n_grows) *n_grows = h->n_grows;
    });
}

template <class H>
int ep_set_warp(H* h, const char* name, int stream, const double* warp_2x3) {
    return guard_on(h, [&]() {
        need_handle(h, name, "null.");
        core_set_warp(h, stream, warp_2x3);
    });
}

template <class H>
int ep_reid_kernel_ms(H* h, double* out_ms, int* out_launches) {
    return guard_on(h, [&]() {
        if (!h || !out_ms || !out_launches) throw std::runtime_error("boxmot_hip: null argument");
        *out_ms = 0; *out_launches = 0;
        if (h->reid) h->reid->drain_kernel_timing(*out_ms, *out_launches);
    });
}

void* ep_stream(HandleCore* h) {
    if (!h) return nullptr;
    h->stream_exposed = true;
    return (void*)h->stream;
}

// ---- DeepOCSORT / StrongSORT ----
template <class H>
int io_ep_set_reid_mode(H* h, int mode) {
    return guard_on(h, [&]() {
        if (!h || !h->reid) throw std::runtime_error("boxmot_hip: no ReID weights are loaded in this handle");
        h->reid->set_mode(mode);
        h->reid_mode = mode;
    });
}

template <class H>
int io_ep_synchronize(H* h, const char* name) {
    return guard_on(h, [&]() {
        need_handle(h, name, "not initialized.");
        BM_HIP(hipStreamSynchronize(h->stream));
        io_check_crop_bound(h);
    });
}

template <class H>
int io_ep_set_crop_bound(H* h, const char* name, int max_total_crops) {
    return guard_on(h, [&]() {
        need_handle(h, name, "not initialized.");
        io_set_crop_bound(h, max_total_crops);
    });
}

template <class H, class MakeDbg>
int io_ep_debug_costs_enable(H* h, int on, MakeDbg make_dbg) {
    return guard_on(h, [&]() {
        if (!h) throw std::runtime_error("boxmot_hip: null argument");
        BM_HIP(hipStreamSynchronize(h->stream));
        if (on) make_dbg(h);
        else if (h->args.dbg_cost) {
            release(h->owned, h->args.dbg_cost); release(h->owned, h->args.dbg_shape);
            h->args.dbg_cost = nullptr; h->args.dbg_shape = nullptr;
        }
    });
}

}  // namespace

extern "C" {

const char* boxmot_hip_last_error(void) { return g_last_error.c_str(); }

int boxmot_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int boxmot_hip_botsort_device(BoxMOTHipBotSort* handle) { return handle ? handle->device : -1; }

void boxmot_hip_botsort_default_config(BoxMOTHipBotSortConfig* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->track_high_thresh = 0.5; c->track_low_thresh = 0.1; c->new_track_thresh = 0.6; c->track_buffer = 30;
    c->match_thresh = 0.8; c->proximity_thresh = 0.5; c->appearance_thresh = 0.25; c->cmc_method = nullptr;
    c->frame_rate = 30; c->fuse_first_associate = 0; c->with_reid = 1; c->max_obs = 50;
    c->reid_model_path = nullptr; c->reid_preprocess = nullptr;
    c->second_match_thresh = 0.5; c->unconfirmed_match_thresh = 0.7; c->unconfirmed_emb_scale = 2.0;
    c->removed_stracks_buffer = 100;
    c->n_streams = 1; c->max_tracks = 1024; c->max_dets = 256; c->emb_dim = 512; c->n_class_lists = 1;
}

void boxmot_hip_bytetrack_default_config(BoxMOTHipBotSortConfig* c) {
    if (!c) return;
    boxmot_hip_botsort_default_config(c);
    c->tracker_kind = 1;
    c->track_low_thresh = 0.1; c->track_high_thresh = 0.45; c->new_track_thresh = 0.45;     // min_conf, track_thresh, det_thresh
    c->match_thresh = 0.8; c->track_buffer = 25; c->frame_rate = 30;
    c->second_match_thresh = 0.5; c->unconfirmed_match_thresh = 0.7;                          // bytetrack.py:338, 358
    c->with_reid = 0; c->fuse_first_associate = 1; c->emb_dim = 1;
}

BoxMOTHipBotSort* boxmot_hip_botsort_create(const BoxMOTHipBotSortConfig* config) {
    BoxMOTHipBotSort* h = nullptr;
    const int ok = guard([&]() {
        if (config == nullptr) throw std::runtime_error("boxmot_hip BoT-SORT config is required.");
        require_device();
        h = new BoxMOTHipBotSort();
        h->cfg = *config;
        if (config->reid_model_path) h->reid_path = config->reid_model_path;
        h->cfg.reid_model_path = nullptr;
        build(h);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

void boxmot_hip_botsort_destroy(BoxMOTHipBotSort* handle) { destroy_on(handle); }

int boxmot_hip_botsort_reset(BoxMOTHipBotSort* handle) { return ep_reset(handle, "BoT-SORT", zero_state); }

int boxmot_hip_botsort_reserve(BoxMOTHipBotSort* handle, int max_tracks, int max_dets) {
    return ep_reserve(handle, "BoT-SORT", max_tracks, max_dets, grow_tables);
}

int boxmot_hip_botsort_capacity(BoxMOTHipBotSort* handle, int* max_tracks, int* max_dets, int* n_grows) {
    return ep_capacity(handle, "BoT-SORT", max_tracks, max_dets, n_grows);
}

int boxmot_hip_botsort_update(BoxMOTHipBotSort* handle, const float* dets, int det_rows, int det_cols,
                              const float* embs, int emb_rows, int emb_cols, const uint8_t* image, int image_rows,
                              int image_cols, int image_channels, float* out_tracks, int out_capacity_rows,
                              int out_cols, int* out_rows, int* out_is_obb) {
    return boxmot_hip_botsort_update_stream(handle, 0, 0, -1, dets, det_rows, det_cols, embs, emb_rows, emb_cols, image,
                                            image_rows, image_cols, image_channels, out_tracks, out_capacity_rows,
                                            out_cols, out_rows, out_is_obb);
}

int boxmot_hip_botsort_update_stream(BoxMOTHipBotSort* handle, int stream, int class_list, int frame_count,
                                     const float* dets, int det_rows, int det_cols, const float* embs, int emb_rows,
                                     int emb_cols, const uint8_t* image, int image_rows, int image_cols,
                                     int image_channels, float* out_tracks, int out_capacity_rows, int out_cols,
                                     int* out_rows, int* out_is_obb) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        if (!out_rows || !out_is_obb) throw std::runtime_error("Output pointers are null.");
        if (out_cols != 9) throw std::runtime_error("boxmot_hip live tracking expects an output buffer with 9 columns.");
        if (embs != nullptr && emb_rows != det_rows) throw std::runtime_error("Detection and embedding row counts must match.");
        if (image_rows <= 0 || image_cols <= 0) throw std::runtime_error("Image dimensions must be positive.");
        StreamIn in{dets, det_rows, (embs && emb_cols > 0) ? embs : nullptr, image};
        host_update_one(handle, stream, class_list, frame_count, in, det_cols, emb_cols, image_rows, image_cols,
                        image_channels, out_tracks, out_capacity_rows, out_rows);
        *out_is_obb = handle->is_obb ? 1 : 0;
    });
}

int boxmot_hip_botsort_update_batch(BoxMOTHipBotSort* handle, int n_streams, const float* const* dets,
                                    const int* det_rows, const float* const* embs, int emb_cols,
                                    const uint8_t* const* images, int image_rows, int image_cols, int image_channels,
                                    float* const* out_tracks, int out_capacity_rows, int* out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        if (n_streams < 1 || n_streams > handle->S) throw std::runtime_error("boxmot_hip: n_streams out of range");
        if (!dets || !det_rows || !out_tracks || !out_rows) throw std::runtime_error("boxmot_hip: null batch pointers");
        std::vector<StreamIn> in(n_streams);
        for (int s = 0; s < n_streams; ++s)
            in[s] = StreamIn{dets[s], det_rows[s], (embs && emb_cols > 0) ? embs[s] : nullptr, images ? images[s] : nullptr};
        host_update(handle, 0, n_streams, in.data(), handle->det_cols, emb_cols, image_rows, image_cols, image_channels, nullptr, nullptr,
                    out_tracks, out_capacity_rows, out_rows);
    });
}

int boxmot_hip_botsort_update_batch_frames(BoxMOTHipBotSort* handle, int n_streams, const float* const* dets,
                                           const int* det_rows, const float* const* embs, int emb_cols,
                                           const uint8_t* const* d_frames, int image_rows, int image_cols,
                                           float* const* out_tracks, int out_capacity_rows, int* out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        if (n_streams < 1 || n_streams > handle->S) throw std::runtime_error("boxmot_hip: n_streams out of range");
        if (!dets || !det_rows || !out_tracks || !out_rows) throw std::runtime_error("boxmot_hip: null batch pointers");
        if (!d_frames || (handle->fs_rows.empty() && (image_rows < 1 || image_cols < 1))) throw std::runtime_error("boxmot_hip: update_batch_frames needs device frames");
        std::vector<StreamIn> in(n_streams);
        for (int s = 0; s < n_streams; ++s) in[s] = StreamIn{dets[s], det_rows[s], (embs && emb_cols > 0) ? embs[s] : nullptr, nullptr};
        host_update(handle, 0, n_streams, in.data(), handle->det_cols, emb_cols, image_rows, image_cols, 3, nullptr, nullptr, out_tracks,
                    out_capacity_rows, out_rows, d_frames);
    });
}

int boxmot_hip_botsort_set_frame_sizes(BoxMOTHipBotSort* handle, const int* image_rows, const int* image_cols, int n_streams) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null argument");
        core_check_frame_sizes(handle, image_rows, image_cols, n_streams);
        if ((handle->sof || handle->ecc) && handle->fs_rows.empty())
            throw std::runtime_error("boxmot_hip: set_frame_sizes comes before the first update of a handle that estimates camera motion itself");
        core_commit_frame_sizes(handle, image_rows, image_cols);
    });
}

int boxmot_hip_botsort_step_device(BoxMOTHipBotSort* handle, const float* d_dets, const int* d_det_rows,
                                   const float* d_embs, const uint8_t* const* d_frames, int image_rows, int image_cols,
                                   float* d_out, int* d_out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        if (!d_dets || !d_det_rows || !d_out || !d_out_rows) throw std::runtime_error("boxmot_hip: null device pointers");
        const float* embs = d_embs;
        bool reid_here = false;
        if (handle->cfg.with_reid && d_embs == nullptr) {
            if (!d_frames) throw std::runtime_error("boxmot_hip: with_reid needs d_embs or d_frames");
            // pipeline stage 1: this frame's ReID on `reid_stream`, into the table the step before last has finished reading
            hipStream_t rs = core_pipe_begin_reid(handle);
            float* tab = core_pipe_table(handle);
            run_reid(handle, rs, 0, handle->S, d_dets, d_det_rows, d_frames, image_rows, image_cols, tab);
            core_pipe_reid_done(handle);
            embs = tab; reid_here = true;
        }
        // cmc_method = "sof" / "ecc": the estimator runs inside the step here too, on the device-resident frames, for every stream
        // that was not given a warp with set_warp (the estimate comes back to the host: one synchronisation per step; callers that
        // want none estimate ahead with boxmot_hip_sof_* / boxmot_hip_ecc_* and set_warp, or create the handle with cmc_method "none")
        if (handle->use_sof || handle->use_ecc) {
            BoxMOTHipBotSort* h = handle;
            bool missing = false;
            for (int s = 0; s < h->S; ++s) missing = missing || h->h_warp_flag[s] == 0;
            if (missing) {
                if (!d_frames || (h->fs_rows.empty() && (image_rows < 1 || image_cols < 1)))
                    throw std::runtime_error("boxmot_hip: cmc_method=sof/ecc in a device-resident step needs d_frames (or a warp per stream from set_warp)");
                std::vector<double> w(6);
                for (int s = 0; s < h->S; ++s) {
                    if (h->h_warp_flag[s]) continue;
                    if (h->use_sof && h->is_obb) {
                        hipLaunchKernelGGL(obb_enclosing_boxes_kernel, dim3(1), dim3(256), 0, h->stream, d_dets, d_det_rows, h->nd, h->d_cmc_boxes, s);
                        sof_run(sof_of(h, s, image_rows, image_cols), s, 1, d_frames + s, h->d_cmc_boxes + (size_t)s * h->nd * 4, d_det_rows + s, h->nd, 4, w.data(), nullptr);
                    } else if (h->use_sof) sof_run(sof_of(h, s, image_rows, image_cols), s, 1, d_frames + s, d_dets + (size_t)s * h->nd * bm::DET_COLS, d_det_rows + s, h->nd, bm::DET_COLS, w.data(), nullptr);
                    else ecc_run_one(ecc_of(h, s, image_rows, image_cols), s, d_frames + s, w.data(), nullptr);
                    for (int k = 0; k < 6; ++k) h->h_warp[(size_t)s * 6 + k] = w[k];
                    h->h_warp_flag[s] = 1;
                }
            }
        }
        // warps set with boxmot_hip_botsort_set_warp since the last step are consumed by this one
        bool any_warp = false;
        for (int s = 0; s < handle->S; ++s) any_warp = any_warp || handle->h_warp_flag[s] != 0;
        if (any_warp) {
            BM_HIP(hipMemcpyAsync(handle->d_warp, handle->h_warp.data(), (size_t)handle->S * 6 * 8, hipMemcpyHostToDevice, handle->stream));
            BM_HIP(hipMemcpyAsync(handle->d_warp_flag, handle->h_warp_flag.data(), handle->S * 4, hipMemcpyHostToDevice, handle->stream));
            // the staging vectors are reused by the next set_warp: the copies must have left the host before returning
            BM_HIP(hipStreamSynchronize(handle->stream));
        }
        launch_step(handle, 0, handle->S, d_dets, d_det_rows, handle->cfg.with_reid ? embs : nullptr, nullptr, nullptr,
                    d_out, d_out_rows, any_warp);
        if (reid_here) core_pipe_step_enqueued(handle);
        for (int s = 0; s < handle->S; ++s) { handle->h_warp_flag[s] = 0; handle->h_used[s] = -1; }      // slot counts: unknown to the host now
    });
}

int boxmot_hip_botsort_set_warp(BoxMOTHipBotSort* handle, int stream, const double* warp_2x3) {
    return ep_set_warp(handle, "BoT-SORT", stream, warp_2x3);
}

int boxmot_hip_botsort_synchronize(BoxMOTHipBotSort* handle) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        BM_HIP(hipStreamSynchronize(handle->stream));
    });
}

int boxmot_hip_botsort_timer_start(BoxMOTHipBotSort* handle) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        BM_HIP(hipEventRecord(handle->timer_ev[0], handle->stream));
    });
}

int boxmot_hip_botsort_timer_stop_ms(BoxMOTHipBotSort* handle, double* out_ms) {
    return guard_on(handle, [&]() {
        if (!handle || !out_ms) throw std::runtime_error("boxmot_hip: null argument");
        BM_HIP(hipEventRecord(handle->timer_ev[1], handle->stream));
        BM_HIP(hipEventSynchronize(handle->timer_ev[1]));
        float ms = 0;
        BM_HIP(hipEventElapsedTime(&ms, handle->timer_ev[0], handle->timer_ev[1]));
        *out_ms = ms;
    });
}

int boxmot_hip_botsort_reid_kernel_ms(BoxMOTHipBotSort* handle, double* out_ms, int* out_launches) { return ep_reid_kernel_ms(handle, out_ms, out_launches); }

int boxmot_hip_botsort_phase_clocks(BoxMOTHipBotSort* handle, long long* out16) {
    return guard_on(handle, [&]() {
        if (!handle || !out16) throw std::runtime_error("boxmot_hip: null argument");
        BM_HIP(hipStreamSynchronize(handle->stream));
        BM_HIP(hipMemcpy(out16, handle->d_phase_clock, 16 * sizeof(long long), hipMemcpyDeviceToHost));
    });
}

void* boxmot_hip_botsort_stream(BoxMOTHipBotSort* handle) { return ep_stream(handle); }

int boxmot_hip_botsort_status(BoxMOTHipBotSort* handle, int* out_status, int capacity) {
    return guard_on(handle, [&]() {
        if (!handle || !out_status) throw std::runtime_error("boxmot_hip: null argument");
        const int n = capacity < handle->S ? capacity : handle->S;
        BM_HIP(hipStreamSynchronize(handle->stream));
        BM_HIP(hipMemcpy(out_status, handle->args.st.status, n * 4, hipMemcpyDeviceToHost));
    });
}

int boxmot_hip_botsort_set_reid_blob(BoxMOTHipBotSort* handle, const float* blob, long n_floats) {
    return guard_on(handle, [&]() {
        if (!handle || !blob || n_floats <= 0) throw std::runtime_error("boxmot_hip: null argument");
        // the handle keeps a host copy: growing max_dets (reserve, or an update with more detections) rebuilds the engine from it
        std::vector<float> keep(blob, blob + n_floats), old;
        old.swap(handle->reid_blob);
        handle->reid_blob.swap(keep);
        try {
            handle->reid = new_reid_engine(handle, handle->nd);
        } catch (...) {
            handle->reid_blob.swap(old);
            throw;
        }
    });
}

int boxmot_hip_botsort_set_reid_mode(BoxMOTHipBotSort* handle, int mode) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null argument");
        if (handle->reid) handle->reid->set_mode(mode);
        handle->reid_mode = mode;
    });
}

static int get_ms(BoxMOTHipBotSort* h, double* out, double BoxMOTHipBotSort::*field, bool sum_reid) {
    return guard_on(h, [&]() {
        if (!h) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        if (!out) throw std::runtime_error("Output timing pointer is null.");
        *out = sum_reid ? h->last_reid_pre_ms + h->last_reid_proc_ms : h->*field;
    });
}
int boxmot_hip_botsort_last_reid_time_ms(BoxMOTHipBotSort* h, double* o) { return get_ms(h, o, &BoxMOTHipBotSort::last_reid_pre_ms, true); }
int boxmot_hip_botsort_last_reid_preprocess_time_ms(BoxMOTHipBotSort* h, double* o) { return get_ms(h, o, &BoxMOTHipBotSort::last_reid_pre_ms, false); }
int boxmot_hip_botsort_last_reid_process_time_ms(BoxMOTHipBotSort* h, double* o) { return get_ms(h, o, &BoxMOTHipBotSort::last_reid_proc_ms, false); }
int boxmot_hip_botsort_last_reid_postprocess_time_ms(BoxMOTHipBotSort* h, double* o) {
    return guard_on(h, [&]() {
        if (!h) throw std::runtime_error("boxmot_hip BoT-SORT handle is not initialized.");
        if (!o) throw std::runtime_error("Output timing pointer is null.");
        *o = 0.0;   // L2 normalisation is fused into the head kernel
    });
}
int boxmot_hip_botsort_last_track_time_ms(BoxMOTHipBotSort* h, double* o) { return get_ms(h, o, &BoxMOTHipBotSort::last_track_ms, false); }

int boxmot_hip_botsort_state_dump(BoxMOTHipBotSort* handle, int stream, int which, int class_list, int* ints,
                                  double* kf, float* smooth, float* misc, int* out_rows, int* out_frame_count,
                                  int* out_id_count) {
    return guard_on(handle, [&]() {
        if (!handle || !out_rows) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        BM_HIP(hipStreamSynchronize(handle->stream));
        const bm::BotSortState& st = handle->args.st;
        const size_t cap = handle->cap, dim = handle->dim, s = stream;
        int n = 0;
        std::vector<int> list(cap);
        if (which == 0) {
            BM_HIP(hipMemcpy(&n, st.n_active + s * handle->n_lists + class_list, 4, hipMemcpyDeviceToHost));
            BM_HIP(hipMemcpy(list.data(), st.active_list + (s * handle->n_lists + class_list) * cap, cap * 4, hipMemcpyDeviceToHost));
        } else {
            BM_HIP(hipMemcpy(&n, st.n_lost + s, 4, hipMemcpyDeviceToHost));
            BM_HIP(hipMemcpy(list.data(), st.lost_list + s * cap, cap * 4, hipMemcpyDeviceToHost));
        }
        auto pull_i = [&](const int* src) { std::vector<int> v(cap); BM_HIP(hipMemcpy(v.data(), src + s * cap, cap * 4, hipMemcpyDeviceToHost)); return v; };
        auto pull_f = [&](const float* src) { std::vector<float> v(cap); BM_HIP(hipMemcpy(v.data(), src + s * cap, cap * 4, hipMemcpyDeviceToHost)); return v; };
        const auto id = pull_i(st.id), state = pull_i(st.state), act = pull_i(st.is_activated), fid = pull_i(st.frame_id),
                   sf = pull_i(st.start_frame), tl = pull_i(st.tracklet_len);
        const auto conf = pull_f(st.conf), cls = pull_f(st.cls), di = pull_f(st.det_ind);
        const size_t KS = handle->is_obb ? bm::obb::KF_STRIDE : bm::KF_STRIDE;        // 72 doubles per track (mean 8 + cov 64), 110 for oriented boxes (10 + 100)
        std::vector<double> kfall(cap * KS);
        BM_HIP(hipMemcpy(kfall.data(), st.kf + s * cap * KS, kfall.size() * 8, hipMemcpyDeviceToHost));
        std::vector<float> sm;
        if (smooth) { sm.resize(cap * dim); BM_HIP(hipMemcpy(sm.data(), st.smooth + s * cap * dim, sm.size() * 4, hipMemcpyDeviceToHost)); }
        for (int r = 0; r < n; ++r) {
            const int sl = list[r];
            if (ints) { int* o = ints + r * 6; o[0] = id[sl]; o[1] = state[sl]; o[2] = act[sl]; o[3] = fid[sl]; o[4] = sf[sl]; o[5] = tl[sl]; }
            if (kf) std::memcpy(kf + (size_t)r * KS, kfall.data() + (size_t)sl * KS, KS * 8);
            if (smooth) std::memcpy(smooth + (size_t)r * dim, sm.data() + (size_t)sl * dim, dim * 4);
            if (misc) { misc[r * 3] = conf[sl]; misc[r * 3 + 1] = cls[sl]; misc[r * 3 + 2] = di[sl]; }
        }
        *out_rows = n;
        if (out_frame_count) BM_HIP(hipMemcpy(out_frame_count, st.frame_count + s, 4, hipMemcpyDeviceToHost));
        if (out_id_count) BM_HIP(hipMemcpy(out_id_count, st.id_count + s, 4, hipMemcpyDeviceToHost));
    });
}

int boxmot_hip_botsort_debug_costs_enable(BoxMOTHipBotSort* handle, int on) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null argument");
        if (on && handle->is_obb) throw std::runtime_error("boxmot_hip: debug_costs is built for the axis-aligned frame step only");
        BM_HIP(hipStreamSynchronize(handle->stream));
        handle->dbg_costs = on != 0;
    });
}

int boxmot_hip_botsort_debug_costs(BoxMOTHipBotSort* handle, int stream, int stage, int plane, double* out, long out_capacity,
                                   int* out_rows, int* out_cols) {
    return guard_on(handle, [&]() {
        if (!handle || !out_rows || !out_cols) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        if (stage < 0 || stage >= bm::DBG_STAGES || plane < 0 || plane >= bm::DBG_PLANES)
            throw std::runtime_error("boxmot_hip: debug_costs stage must be 0..2 and plane 0..2");
        if (!handle->dbg_costs || !handle->d_dbg_cost)
            throw std::runtime_error("boxmot_hip: debug_costs needs boxmot_hip_botsort_debug_costs_enable(handle, 1) before the update");
        BM_HIP(hipStreamSynchronize(handle->stream));
        int shape[2] = {0, 0};
        BM_HIP(hipMemcpy(shape, handle->d_dbg_shape + ((size_t)stream * bm::DBG_STAGES + stage) * 2, 8, hipMemcpyDeviceToHost));
        const int R = shape[0], C = shape[1];
        *out_rows = R; *out_cols = C;
        if (R == 0 || C == 0) return;
        if (!out || out_capacity < (long)R * C) throw std::runtime_error("boxmot_hip: debug_costs output capacity is smaller than rows x cols");
        const size_t cap = handle->dbg_cap, nd = handle->dbg_nd;
        std::vector<double> m(nd * cap);
        BM_HIP(hipMemcpy(m.data(), handle->d_dbg_cost + (((size_t)stream * bm::DBG_STAGES + stage) * bm::DBG_PLANES + plane) * nd * cap,
                         m.size() * 8, hipMemcpyDeviceToHost));
        for (int r = 0; r < R; ++r)                       // the device stores detection-major; the caller gets the reference's (tracks, dets)
            for (int c = 0; c < C; ++c) out[(size_t)r * C + c] = m[(size_t)c * cap + r];
    });
}

// ---- ReID C ABI ----
BoxMOTHipReID* boxmot_hip_reid_create(const char* model_path, const float* blob, long n_floats, int max_crops) {
    BoxMOTHipReID* h = nullptr;
    const int ok = guard([&]() {
        require_device();
        if (max_crops < 1) throw std::runtime_error("boxmot_hip: max_crops must be >= 1");
        h = new BoxMOTHipReID();
        BM_HIP(hipStreamCreate(&h->stream));
        if (blob) h->engine.reset(new bm::ReidEngine(blob, n_floats, max_crops));
        else if (model_path) {
            const std::vector<float> v = bm::read_blob_file(model_path);
            h->engine.reset(new bm::ReidEngine(v.data(), (long)v.size(), max_crops));
        } else throw std::runtime_error("boxmot_hip: ReID needs a weight blob or a model path");
        h->d_frames = dev_alloc<const uint8_t*>(1, h->owned);
        h->d_crop_stream = zalloc<int>(max_crops, h->owned);
        h->d_boxes = dev_alloc<float>((size_t)max_crops * 4, h->owned);
        h->d_feat = dev_alloc<float>((size_t)max_crops * h->engine->feature_dim(), h->owned);
        h->d_obb = dev_alloc<double>((size_t)max_crops * 8, h->owned);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

void boxmot_hip_reid_destroy(BoxMOTHipReID* handle) { destroy_on(handle); }

int boxmot_hip_reid_feature_dim(BoxMOTHipReID* handle) { return handle && handle->engine ? handle->engine->feature_dim() : 0; }

int boxmot_hip_reid_set_preprocess(BoxMOTHipReID* handle, const char* name) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null ReID handle");
        if (name == nullptr || std::strcmp(name, "resize") == 0) handle->engine->set_preprocess(0);
        else if (std::strcmp(name, "resize_pad") == 0) handle->engine->set_preprocess(1);
        else throw std::runtime_error("boxmot_hip: unknown ReID preprocess (have: resize, resize_pad)");
    });
}

int boxmot_hip_reid_set_mode(BoxMOTHipReID* handle, int mode) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null ReID handle");
        handle->engine->set_mode(mode);
    });
}

// Host side of the box table: xyxy rows copied to 4 columns, or -- rows of 5 / 7 / 9 values (base_backend.py:119-122, 157) -- the
// geometry of oriented boxes [cx, cy, w, h, angle, ...] (8 doubles per box: out_w, out_h, inverse 2x3 map).  Returns whether the
// boxes are oriented.
static bool reid_host_boxes(const float* boxes, int n, int box_cols, std::vector<float>& b, std::vector<double>& geo) {
    const bool obb = n > 0 && (box_cols == 5 || box_cols == 7 || box_cols == 9);
    b.assign((size_t)n * 4, 0.f);
    geo.clear();
    if (obb) {
        // _crop_obb (base_backend.py:91-117): getRotationMatrix2D about the box centre, shifted so that the centre lands on the middle
        // of the (round(w), round(h)) output; cv2.warpAffine inverts the matrix in double precision before it samples
        // (obb_crop_geometry.hpp: the one function the device's crop-list kernel uses too; a non-finite box is a blank crop)
        geo.resize((size_t)n * 8);
        for (int i = 0; i < n; ++i) bm::obb_crop_geometry(boxes + (size_t)i * box_cols, geo.data() + (size_t)i * 8);
    } else {
        for (int i = 0; i < n; ++i)
            for (int q = 0; q < 4; ++q) b[i * 4 + q] = boxes[(size_t)i * box_cols + q];
    }
    return obb;
}

static void reid_stage(BoxMOTHipReID* h, const uint8_t* image, int rows, int cols, int channels, const float* boxes,
                       int n, int box_cols) {
    if (!h) throw std::runtime_error("boxmot_hip: null ReID handle");
    if (!image) throw std::runtime_error("Image data pointer is null.");
    if (channels != 3) throw std::runtime_error("boxmot_hip: ReID needs a 3-channel uint8 BGR image");
    if (rows <= 0 || cols <= 0) throw std::runtime_error("Image dimensions must be positive.");
    if (n < 0 || box_cols < 4) throw std::runtime_error("boxmot_hip: boxes must have at least 4 columns");
    if (n > h->engine->max_crops()) throw std::runtime_error("boxmot_hip: more boxes than max_crops");
    const size_t bytes = (size_t)rows * cols * 3;
    if (bytes > h->frame_bytes) {
        if (h->d_frame) BM_HIP(hipFree(h->d_frame));
        void* p = nullptr;
        BM_HIP(hipMalloc(&p, bytes));
        h->d_frame = static_cast<uint8_t*>(p);
        h->frame_bytes = bytes;
        BM_HIP(hipMemcpy(h->d_frames, &h->d_frame, sizeof(uint8_t*), hipMemcpyHostToDevice));
    }
    BM_HIP(hipMemcpyAsync(h->d_frame, image, bytes, hipMemcpyHostToDevice, h->stream));
    std::vector<float> b;
    std::vector<double> geo;
    h->obb = reid_host_boxes(boxes, n, box_cols, b, geo);
    if (h->obb) BM_HIP(hipMemcpyAsync(h->d_obb, geo.data(), geo.size() * 8, hipMemcpyHostToDevice, h->stream));
    if (n) BM_HIP(hipMemcpyAsync(h->d_boxes, b.data(), b.size() * 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    h->engine->set_obb_geometry(h->obb ? h->d_obb : nullptr);
}

// oriented-box geometry is valid for one staged batch only
struct ObbScope {
    BoxMOTHipReID* h;
    ~ObbScope() { if (h && h->engine) h->engine->set_obb_geometry(nullptr); }
};

int boxmot_hip_reid_compute_features(BoxMOTHipReID* handle, const uint8_t* image, int image_rows, int image_cols,
                                     int image_channels, const float* boxes, int n_boxes, int box_cols,
                                     float* out_features, int out_capacity_rows) {
    return guard_on(handle, [&]() {
        ObbScope scope{handle};
        reid_stage(handle, image, image_rows, image_cols, image_channels, boxes, n_boxes, box_cols);
        if (out_capacity_rows < n_boxes) throw std::runtime_error("boxmot_hip: feature buffer too small");
        if (n_boxes == 0) return;
        handle->engine->run(handle->d_frames, handle->d_crop_stream, handle->d_boxes, 4, n_boxes, image_cols, image_rows,
                            handle->d_feat, nullptr, handle->stream);
        BM_HIP(hipMemcpyAsync(out_features, handle->d_feat, (size_t)n_boxes * handle->engine->feature_dim() * 4,
                              hipMemcpyDeviceToHost, handle->stream));
        BM_HIP(hipStreamSynchronize(handle->stream));
    });
}

// ---- boxes of many images, of any sizes, in one device pass ----
// (the per-image frame sizes, like the oriented-box geometry, are valid for one batch call only: FrameDimsScope, ObbScope)

// Validate, upload the images, bring the pointer and {W, H} tables up to date.  Returns whether the images differ in size (the
// engine then reads the table; with one size the scalar-form kernels run, as for a single image).
static bool reid_stage_images(BoxMOTHipReID* h, const uint8_t* const* images, const int* rows, const int* cols, int n_images,
                              const int* box_image, int n_boxes, int box_cols) {
    if (!h) throw std::runtime_error("boxmot_hip: null ReID handle");
    if (!images || !rows || !cols || n_images < 1) throw std::runtime_error("boxmot_hip: ReID batch needs at least one image and its size");
    if (n_boxes < 0 || box_cols < 4) throw std::runtime_error("boxmot_hip: boxes must have at least 4 columns");
    if (n_boxes > 0 && !box_image) throw std::runtime_error("boxmot_hip: ReID batch needs the image index of every box");
    for (int k = 0; k < n_images; ++k) {
        if (!images[k]) throw std::runtime_error("boxmot_hip: ReID batch image " + std::to_string(k) + ": data pointer is null");
        if (rows[k] <= 0 || cols[k] <= 0) throw std::runtime_error("boxmot_hip: ReID batch image " + std::to_string(k) + ": dimensions must be positive");
    }
    for (int i = 0; i < n_boxes; ++i)
        if (box_image[i] < 0 || box_image[i] >= n_images)
            throw std::runtime_error("boxmot_hip: ReID batch box " + std::to_string(i) + ": image index out of range");
    bool tables_stale = false;
    if ((int)h->batch_bufs.size() < n_images) {
        BM_HIP(hipStreamSynchronize(h->stream));
        if (h->d_batch_frames) BM_HIP(hipFree(h->d_batch_frames));
        if (h->d_batch_dims) BM_HIP(hipFree(h->d_batch_dims));
        h->d_batch_frames = nullptr; h->d_batch_dims = nullptr;
        void* p = nullptr;
        BM_HIP(hipMalloc(&p, (size_t)n_images * sizeof(uint8_t*)));
        h->d_batch_frames = static_cast<const uint8_t**>(p);
        BM_HIP(hipMalloc(&p, (size_t)n_images * 2 * sizeof(int)));
        h->d_batch_dims = static_cast<int*>(p);
        h->batch_bufs.resize(n_images, nullptr);
        h->batch_bytes.resize(n_images, 0);
        h->batch_dims.resize((size_t)n_images * 2, 0);
        tables_stale = true;
    }
    bool mixed = false;
    for (int k = 0; k < n_images; ++k) {
        const size_t bytes = (size_t)rows[k] * cols[k] * 3;
        if (bytes > h->batch_bytes[k]) {
            if (h->batch_bufs[k]) { BM_HIP(hipFree(h->batch_bufs[k])); h->batch_bufs[k] = nullptr; h->batch_bytes[k] = 0; }
            void* p = nullptr;
            BM_HIP(hipMalloc(&p, bytes));
            h->batch_bufs[k] = static_cast<uint8_t*>(p);
            h->batch_bytes[k] = bytes;
            tables_stale = true;
        }
        if (h->batch_dims[2 * k] != cols[k] || h->batch_dims[2 * k + 1] != rows[k]) {
            h->batch_dims[2 * k] = cols[k]; h->batch_dims[2 * k + 1] = rows[k];
            tables_stale = true;
        }
        if (rows[k] != rows[0] || cols[k] != cols[0]) mixed = true;
        BM_HIP(hipMemcpyAsync(h->batch_bufs[k], images[k], bytes, hipMemcpyHostToDevice, h->stream));
    }
    if (tables_stale) {     // sizes are a property of the caller's streams: the tables change when one of them does, not per call
        BM_HIP(hipMemcpyAsync(h->d_batch_frames, h->batch_bufs.data(), h->batch_bufs.size() * sizeof(uint8_t*), hipMemcpyHostToDevice, h->stream));
        BM_HIP(hipMemcpyAsync(h->d_batch_dims, h->batch_dims.data(), h->batch_dims.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        BM_HIP(hipStreamSynchronize(h->stream));       // (the copies read pageable vectors of the handle)
    }
    if (!h->d_batch_crop_stream) h->d_batch_crop_stream = zalloc<int>(h->engine->max_crops(), h->owned);
    return mixed;
}

// boxes [i0, i0 + m) of the batch -> the handle's device tables (boxes, oriented geometry, crop -> image)
static void reid_stage_box_chunk(BoxMOTHipReID* h, const float* boxes, const int* box_image, int i0, int m, int box_cols) {
    std::vector<float> b;
    std::vector<double> geo;
    h->obb = reid_host_boxes(boxes + (size_t)i0 * box_cols, m, box_cols, b, geo);
    if (h->obb) BM_HIP(hipMemcpyAsync(h->d_obb, geo.data(), geo.size() * 8, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_boxes, b.data(), b.size() * 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipMemcpyAsync(h->d_batch_crop_stream, box_image + i0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
    BM_HIP(hipStreamSynchronize(h->stream));
    h->engine->set_obb_geometry(h->obb ? h->d_obb : nullptr);
}

int boxmot_hip_reid_compute_features_batch(BoxMOTHipReID* handle, const uint8_t* const* images, const int* image_rows,
                                           const int* image_cols, int n_images, const float* boxes, const int* box_image, int n_boxes,
                                           int box_cols, float* out_features, int out_capacity_rows) {
    return guard_on(handle, [&]() {
        ObbScope obb_scope{handle};
        FrameDimsScope dims_scope{handle ? handle->engine.get() : nullptr};
        const bool mixed = reid_stage_images(handle, images, image_rows, image_cols, n_images, box_image, n_boxes, box_cols);
        if (out_capacity_rows < n_boxes) throw std::runtime_error("boxmot_hip: feature buffer too small");
        if (n_boxes > 0 && !out_features) throw std::runtime_error("boxmot_hip: null argument");
        if (n_boxes == 0) { BM_HIP(hipStreamSynchronize(handle->stream)); return; }     // (the uploads read the caller's memory: done before returning)
        handle->engine->set_frame_dims(mixed ? handle->d_batch_dims : nullptr);
        const int step = handle->engine->max_crops(), dim = handle->engine->feature_dim();
        for (int i0 = 0; i0 < n_boxes; i0 += step) {         // the handle's box / feature tables hold max_crops rows
            const int m = n_boxes - i0 < step ? n_boxes - i0 : step;
            reid_stage_box_chunk(handle, boxes, box_image, i0, m, box_cols);
            handle->engine->run(handle->d_batch_frames, handle->d_batch_crop_stream, handle->d_boxes, 4, m, image_cols[0], image_rows[0],
                                handle->d_feat, nullptr, handle->stream);
            BM_HIP(hipMemcpyAsync(out_features + (size_t)i0 * dim, handle->d_feat, (size_t)m * dim * 4, hipMemcpyDeviceToHost, handle->stream));
            BM_HIP(hipStreamSynchronize(handle->stream));
        }
    });
}

int boxmot_hip_reid_preprocess_batch(BoxMOTHipReID* handle, const uint8_t* const* images, const int* image_rows, const int* image_cols,
                                     int n_images, const float* boxes, const int* box_image, int n_boxes, int box_cols, float* out_crops) {
    return guard_on(handle, [&]() {
        ObbScope obb_scope{handle};
        FrameDimsScope dims_scope{handle ? handle->engine.get() : nullptr};
        const bool mixed = reid_stage_images(handle, images, image_rows, image_cols, n_images, box_image, n_boxes, box_cols);
        if (n_boxes > handle->engine->max_crops()) throw std::runtime_error("boxmot_hip: more boxes than max_crops");
        if (n_boxes == 0) { BM_HIP(hipStreamSynchronize(handle->stream)); return; }
        if (!out_crops) throw std::runtime_error("boxmot_hip: null argument");
        handle->engine->set_frame_dims(mixed ? handle->d_batch_dims : nullptr);
        reid_stage_box_chunk(handle, boxes, box_image, 0, n_boxes, box_cols);
        handle->engine->preprocess_fp32(handle->d_batch_frames, handle->d_batch_crop_stream, handle->d_boxes, 4, n_boxes, image_cols[0],
                                        image_rows[0], handle->stream);
        BM_HIP(hipMemcpyAsync(out_crops, handle->engine->crops_buffer(),
                              (size_t)n_boxes * bm::REID_IN_H * bm::REID_IN_W * 3 * 4, hipMemcpyDeviceToHost, handle->stream));
        BM_HIP(hipStreamSynchronize(handle->stream));
    });
}

int boxmot_hip_reid_last_time_ms(BoxMOTHipReID* handle, double* out_preprocess_ms, double* out_process_ms) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null ReID handle");
        double pre = 0, proc = 0;
        handle->engine->last_times(pre, proc);
        if (out_preprocess_ms) *out_preprocess_ms = pre;
        if (out_process_ms) *out_process_ms = proc;
    });
}

int boxmot_hip_reid_preprocess(BoxMOTHipReID* handle, const uint8_t* image, int image_rows, int image_cols,
                               int image_channels, const float* boxes, int n_boxes, int box_cols, float* out_crops) {
    return guard_on(handle, [&]() {
        ObbScope scope{handle};
        reid_stage(handle, image, image_rows, image_cols, image_channels, boxes, n_boxes, box_cols);
        if (n_boxes == 0) return;
        handle->engine->preprocess_fp32(handle->d_frames, handle->d_crop_stream, handle->d_boxes, 4, n_boxes, image_cols,
                                        image_rows, handle->stream);
        BM_HIP(hipMemcpyAsync(out_crops, handle->engine->crops_buffer(),
                              (size_t)n_boxes * bm::REID_IN_H * bm::REID_IN_W * 3 * 4, hipMemcpyDeviceToHost, handle->stream));
        BM_HIP(hipStreamSynchronize(handle->stream));
    });
}

// Debug read-back of what the fp32-grade family (mode 2) takes as its input: the (hi, lo) fp16 RGBX planes [n][262][136][4] of the
// boxes' crops, border included, as raw halves.
int boxmot_hip_reid_debug_crop_planes(BoxMOTHipReID* handle, const uint8_t* image, int image_rows, int image_cols, int image_channels,
                                      const float* boxes, int n_boxes, int box_cols, uint16_t* out_hi, uint16_t* out_lo) {
    return guard_on(handle, [&]() {
        ObbScope scope{handle};
        reid_stage(handle, image, image_rows, image_cols, image_channels, boxes, n_boxes, box_cols);
        const _Float16 *hi = nullptr, *lo = nullptr;
        if (!handle->engine->hp_crop_planes(hi, lo)) throw std::runtime_error("boxmot_hip: the (hi, lo) crop planes exist in ReID mode 2 only");
        if (n_boxes == 0) return;
        if (!out_hi || !out_lo) throw std::runtime_error("boxmot_hip: null argument");
        handle->engine->preprocess(handle->d_frames, handle->d_crop_stream, handle->d_boxes, 4, n_boxes, image_cols, image_rows, handle->stream);
        const size_t bytes = (size_t)n_boxes * bm::STEM_ROWS * bm::STEM_COLS * 4 * 2;
        BM_HIP(hipMemcpyAsync(out_hi, hi, bytes, hipMemcpyDeviceToHost, handle->stream));
        BM_HIP(hipMemcpyAsync(out_lo, lo, bytes, hipMemcpyDeviceToHost, handle->stream));
        BM_HIP(hipStreamSynchronize(handle->stream));
    });
}

// Debug: the crop geometry of n oriented boxes [cx, cy, w, h, angle, ...] as the DEVICE computes it (obb_geometry_kernel; the
// crop-list kernel of an oriented tracker handle calls the same function) -> out_geo [n][8] doubles.
int boxmot_hip_reid_debug_obb_geometry(BoxMOTHipReID* handle, const float* boxes, int n_boxes, int box_cols, double* out_geo) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null ReID handle");
        if (n_boxes < 0 || box_cols < 5) throw std::runtime_error("boxmot_hip: oriented boxes have at least 5 columns");
        if (n_boxes == 0) return;
        if (!boxes || !out_geo) throw std::runtime_error("boxmot_hip: null argument");
        std::vector<void*> tmp;
        struct Free { std::vector<void*>& v; ~Free() { for (void* p : v) (void)hipFree(p); } } free_tmp{tmp};
        float* d_b = dev_alloc<float>((size_t)n_boxes * box_cols, tmp);
        double* d_g = dev_alloc<double>((size_t)n_boxes * 8, tmp);
        BM_HIP(hipMemcpyAsync(d_b, boxes, (size_t)n_boxes * box_cols * 4, hipMemcpyHostToDevice, handle->stream));
        hipLaunchKernelGGL(bm::obb_geometry_kernel, dim3((n_boxes + 63) / 64), dim3(64), 0, handle->stream, (const float*)d_b, box_cols, n_boxes, d_g);
        BM_HIP(hipGetLastError());
        BM_HIP(hipMemcpyAsync(out_geo, d_g, (size_t)n_boxes * 64, hipMemcpyDeviceToHost, handle->stream));
        BM_HIP(hipStreamSynchronize(handle->stream));
    });
}

// ---- ECC camera-motion estimation ----
BoxMOTHipEcc* boxmot_hip_ecc_create(int n_streams, int image_rows, int image_cols, double scale, double eps, int max_iter) {
    BoxMOTHipEcc* h = nullptr;
    const int ok = guard([&]() {
        require_device();
        h = new BoxMOTHipEcc();
        ecc_init(h, n_streams, image_rows, image_cols, scale, eps, max_iter, nullptr);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

void boxmot_hip_ecc_destroy(BoxMOTHipEcc* handle) { destroy_on(handle); }

int boxmot_hip_ecc_reset(BoxMOTHipEcc* handle, int stream) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null ECC handle");
        if (stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        for (int s = 0; s < handle->S; ++s) if (stream < 0 || s == stream) handle->has_prev[s] = 0;
    });
}

int boxmot_hip_ecc_apply(BoxMOTHipEcc* handle, int stream, const uint8_t* image, int image_rows, int image_cols, int image_channels,
                         double* out_warp_2x3, int* out_iterations) {
    return guard_on(handle, [&]() {
        if (!handle || !out_warp_2x3) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        if (!image) throw std::runtime_error("Image data pointer is null.");
        if (image_channels != 3 || image_rows != handle->rows || image_cols != handle->cols)
            throw std::runtime_error("boxmot_hip: ECC was created for a different frame size (3-channel BGR uint8)");
        const size_t bytes = (size_t)image_rows * image_cols * 3;
        if (!handle->frame_bufs[stream]) {
            void* p = nullptr;
            BM_HIP(hipMalloc(&p, bytes));
            handle->frame_bufs[stream] = static_cast<uint8_t*>(p);
            BM_HIP(hipMemcpy(handle->d_frames, handle->frame_bufs.data(), handle->S * sizeof(uint8_t*), hipMemcpyHostToDevice));
        }
        BM_HIP(hipMemcpyAsync(handle->frame_bufs[stream], image, bytes, hipMemcpyHostToDevice, handle->stream));
        ecc_run_one(handle, stream, handle->d_frames + stream, out_warp_2x3, out_iterations);
    });
}

int boxmot_hip_ecc_apply_device(BoxMOTHipEcc* handle, int stream, const uint8_t* d_frame, double* out_warp_2x3, int* out_iterations) {
    return guard_on(handle, [&]() {
        if (!handle || !out_warp_2x3 || !d_frame) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        // the pointer table lives on the device: one slot per stream, written on the handle's stream before the kernels read it
        BM_HIP(hipMemcpyAsync(handle->d_frames + stream, &d_frame, sizeof(uint8_t*), hipMemcpyHostToDevice, handle->stream));
        BM_HIP(hipStreamSynchronize(handle->stream));       // &d_frame is a stack address
        ecc_run_one(handle, stream, handle->d_frames + stream, out_warp_2x3, out_iterations);
    });
}

// ---- SOF camera-motion estimation ----
BoxMOTHipSof* boxmot_hip_sof_create(int n_streams, int image_rows, int image_cols, double scale, int min_inliers, double min_inlier_ratio,
                                    double ransac_reproj_threshold) {
    BoxMOTHipSof* h = nullptr;
    const int ok = guard([&]() {
        require_device();
        h = new BoxMOTHipSof();
        sof_init(h, n_streams, image_rows, image_cols, scale, min_inliers, min_inlier_ratio, ransac_reproj_threshold, nullptr);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

void boxmot_hip_sof_destroy(BoxMOTHipSof* handle) { destroy_on(handle); }

int boxmot_hip_sof_reset(BoxMOTHipSof* handle, int stream) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null SOF handle");
        if (stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        BM_HIP(hipStreamSynchronize(handle->stream));
        if (stream < 0) BM_HIP(hipMemset(handle->buf.st, 0, (size_t)handle->S * sizeof(bm::SofState)));
        else BM_HIP(hipMemset(handle->buf.st + stream, 0, sizeof(bm::SofState)));
    });
}

int boxmot_hip_sof_apply(BoxMOTHipSof* handle, int stream, const uint8_t* image, int image_rows, int image_cols, int image_channels,
                         const float* dets, int n_dets, int det_stride, double* out_warp_2x3, int* out_info8) {
    return guard_on(handle, [&]() {
        if (!handle || !out_warp_2x3) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        if (!image) throw std::runtime_error("Image data pointer is null.");
        if (image_channels != 3 || image_rows != handle->rows || image_cols != handle->cols)
            throw std::runtime_error("boxmot_hip: SOF was created for a different frame size (3-channel BGR uint8)");
        const size_t bytes = (size_t)image_rows * image_cols * 3;
        if (!handle->frame_bufs[stream]) {
            void* p = nullptr;
            BM_HIP(hipMalloc(&p, bytes));
            handle->frame_bufs[stream] = static_cast<uint8_t*>(p);
            BM_HIP(hipMemcpy(handle->d_frames, handle->frame_bufs.data(), handle->S * sizeof(uint8_t*), hipMemcpyHostToDevice));
        }
        BM_HIP(hipMemcpyAsync(handle->frame_bufs[stream], image, bytes, hipMemcpyHostToDevice, handle->stream));
        sof_stage_dets(handle, stream, dets, n_dets, det_stride);
        sof_run(handle, stream, 1, handle->d_frames + stream, handle->d_dets + (size_t)stream * handle->max_dets * 4, handle->d_ndets + stream,
                handle->max_dets, 4, out_warp_2x3, out_info8);
    });
}

int boxmot_hip_sof_apply_device(BoxMOTHipSof* handle, const uint8_t* const* d_frames, const float* d_dets, const int* d_ndets, int max_dets,
                                int det_stride, double* out_warps, int* out_info8) {
    return guard_on(handle, [&]() {
        if (!handle || !out_warps || !d_frames) throw std::runtime_error("boxmot_hip: null argument");
        if (d_dets && (!d_ndets || max_dets < 1 || det_stride < 4)) throw std::runtime_error("boxmot_hip: SOF device detections need d_ndets, max_dets >= 1 and >= 4 columns");
        sof_run(handle, 0, handle->S, d_frames, d_dets, d_dets ? d_ndets : nullptr, max_dets, det_stride, out_warps, out_info8);
    });
}

int boxmot_hip_sof_keypoints(BoxMOTHipSof* handle, int stream, float* out_xy, int capacity, int* out_n) {
    return guard_on(handle, [&]() {
        if (!handle || !out_n) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        bm::SofState st{};
        BM_HIP(hipStreamSynchronize(handle->stream));
        BM_HIP(hipMemcpy(&st, handle->buf.st + stream, sizeof(st), hipMemcpyDeviceToHost));
        *out_n = st.n_prev;
        const int n = st.n_prev < capacity ? st.n_prev : capacity;
        if (n > 0 && out_xy) BM_HIP(hipMemcpy(out_xy, handle->buf.prev_kps + (size_t)stream * bm::SOF_MAX_CORNERS * 2, (size_t)n * 8, hipMemcpyDeviceToHost));
    });
}

// test access to the detector's intermediate images of the last frame: which = 0 minimum-eigenvalue map (fp32 [h][w]), 1 detection mask
// (uint8 [h][w]), 2 the scaled grayscale frame (uint8 [h][w])
int boxmot_hip_sof_debug_map(BoxMOTHipSof* handle, int stream, int which, void* out, int capacity_bytes, int* out_h, int* out_w) {
    return guard_on(handle, [&]() {
        if (!handle || !out) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        const size_t P = (size_t)handle->lv.h[0] * handle->lv.w[0];
        const size_t bytes = which == 0 ? P * 4 : P;
        if ((size_t)capacity_bytes < bytes) throw std::runtime_error("boxmot_hip: output buffer is too small");
        BM_HIP(hipStreamSynchronize(handle->stream));
        const void* src = which == 0 ? (const void*)(handle->buf.eig + stream * P)
                        : which == 1 ? (const void*)(handle->buf.mask + stream * P)
                                     : (const void*)(handle->buf.pyr_prev + (size_t)stream * handle->lv.total);
        BM_HIP(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
        if (out_h) *out_h = handle->lv.h[0];
        if (out_w) *out_w = handle->lv.w[0];
    });
}

// ---- frame ingest ring ----
// slots of a ring whose per-stream offsets (h->offs) are set: pinned host frames, device twins, pointer tables, events
static void ingest_build(BoxMOTHipIngest* h) {
    const int n_slots = h->n_slots, n_streams = h->n_streams;
    BM_HIP(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    const size_t slot_bytes = h->offs[n_streams], host_bytes = h->format ? h->nv_offs[n_streams] : slot_bytes;
    for (int k = 0; k < n_slots; ++k) {
        void *hp = nullptr, *dp = nullptr, *tp = nullptr;
        BM_HIP(hipHostMalloc(&hp, host_bytes, hipHostMallocDefault));
        h->h_slot.push_back(static_cast<uint8_t*>(hp));
        BM_HIP(hipMalloc(&dp, slot_bytes));
        h->d_slot.push_back(static_cast<uint8_t*>(dp));
        BM_HIP(hipMalloc(&tp, n_streams * sizeof(uint8_t*)));
        h->d_ptrs.push_back(static_cast<const uint8_t**>(tp));
        std::vector<const uint8_t*> table(n_streams);
        for (int s = 0; s < n_streams; ++s) table[s] = h->d_slot[k] + h->offs[s];
        BM_HIP(hipMemcpy(tp, table.data(), n_streams * sizeof(uint8_t*), hipMemcpyHostToDevice));
        if (h->format) {                // NV12 staging twin (pitch = cols, UV directly after Y) and its conversion descriptors
            void *np = nullptr, *qp = nullptr;
            BM_HIP(hipMalloc(&np, host_bytes));
            h->d_nv.push_back(static_cast<uint8_t*>(np));
            std::vector<bm::Nv12Desc> desc(n_streams);
            for (int s = 0; s < n_streams; ++s) {
                const uint8_t* y = h->d_nv[k] + h->nv_offs[s];
                desc[s] = bm::Nv12Desc{y, y + (size_t)h->srows[s] * h->scols[s], h->scols[s], h->scols[s], h->srows[s], h->scols[s],
                                       h->d_slot[k] + h->offs[s]};
            }
            BM_HIP(hipMalloc(&qp, n_streams * sizeof(bm::Nv12Desc)));
            h->d_desc.push_back(static_cast<bm::Nv12Desc*>(qp));
            BM_HIP(hipMemcpy(qp, desc.data(), n_streams * sizeof(bm::Nv12Desc), hipMemcpyHostToDevice));
            h->nv_desc.push_back(std::move(desc));
        }
        hipEvent_t a, b;
        BM_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        BM_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        h->uploaded.push_back(a); h->consumed.push_back(b);
    }
    h->has_consumer.assign(n_slots, 0);
}

BoxMOTHipIngest* boxmot_hip_ingest_create(int n_slots, int n_streams, int image_rows, int image_cols) {
    BoxMOTHipIngest* h = nullptr;
    const int ok = guard([&]() {
        require_device();
        if (n_slots < 2 || n_streams < 1 || image_rows < 1 || image_cols < 1)
            throw std::runtime_error("boxmot_hip: ingest ring needs >= 2 slots, >= 1 stream and positive frame dimensions");
        h = new BoxMOTHipIngest();
        h->n_slots = n_slots; h->n_streams = n_streams; h->rows = image_rows; h->cols = image_cols;
        h->frame_bytes = (size_t)image_rows * image_cols * 3;
        h->srows.assign(n_streams, image_rows); h->scols.assign(n_streams, image_cols);
        h->offs.resize((size_t)n_streams + 1);
        for (int s = 0; s <= n_streams; ++s) h->offs[s] = (size_t)s * h->frame_bytes;
        ingest_build(h);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

// a ring whose streams have frames of different sizes: stream s is (image_rows[s], image_cols[s], 3); the frames of a slot lie in one
// allocation at 256-byte aligned offsets, so submit stays one DMA per slot
BoxMOTHipIngest* boxmot_hip_ingest_create_sized(int n_slots, int n_streams, const int* image_rows, const int* image_cols) {
    BoxMOTHipIngest* h = nullptr;
    const int ok = guard([&]() {
        require_device();
        if (n_slots < 2 || n_streams < 1 || !image_rows || !image_cols)
            throw std::runtime_error("boxmot_hip: ingest ring needs >= 2 slots, >= 1 stream and a (rows, cols) per stream");
        for (int s = 0; s < n_streams; ++s)
            if (image_rows[s] < 1 || image_cols[s] < 1)
                throw std::runtime_error("boxmot_hip: ingest ring stream " + std::to_string(s) + ": frame dimensions must be positive");
        h = new BoxMOTHipIngest();
        h->n_slots = n_slots; h->n_streams = n_streams; h->rows = image_rows[0]; h->cols = image_cols[0];
        h->frame_bytes = 0;             // (no single frame size)
        h->srows.assign(image_rows, image_rows + n_streams); h->scols.assign(image_cols, image_cols + n_streams);
        h->offs.assign((size_t)n_streams + 1, 0);
        for (int s = 0; s < n_streams; ++s)
            h->offs[s + 1] = (h->offs[s] + (size_t)image_rows[s] * image_cols[s] * 3 + 255) / 256 * 256;
        ingest_build(h);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

// a ring whose host slots hold NV12 frames (tightly packed: pitch = cols, the UV plane directly after the Y plane; frames at 256-byte
// aligned offsets): submit moves the NV12 bytes and converts them into the BGR device frames -- laid out as create_sized lays them
// out -- on the copy stream.  Sizes are per stream (a uniform ring passes equal entries) and even.
BoxMOTHipIngest* boxmot_hip_ingest_create_nv12(int n_slots, int n_streams, const int* image_rows, const int* image_cols) {
    BoxMOTHipIngest* h = nullptr;
    const int ok = guard([&]() {
        require_device();
        if (n_slots < 2 || n_streams < 1 || !image_rows || !image_cols)
            throw std::runtime_error("boxmot_hip: ingest ring needs >= 2 slots, >= 1 stream and a (rows, cols) per stream");
        for (int s = 0; s < n_streams; ++s) {
            if (image_rows[s] < 1 || image_cols[s] < 1)
                throw std::runtime_error("boxmot_hip: ingest ring stream " + std::to_string(s) + ": frame dimensions must be positive");
            if (image_rows[s] % 2 || image_cols[s] % 2)
                throw std::runtime_error("boxmot_hip: ingest ring stream " + std::to_string(s) + ": NV12 frames have even rows and cols, got " +
                                         std::to_string(image_rows[s]) + " x " + std::to_string(image_cols[s]));
        }
        h = new BoxMOTHipIngest();
        h->n_slots = n_slots; h->n_streams = n_streams; h->rows = image_rows[0]; h->cols = image_cols[0];
        h->format = 1;
        h->srows.assign(image_rows, image_rows + n_streams); h->scols.assign(image_cols, image_cols + n_streams);
        h->offs.assign((size_t)n_streams + 1, 0);
        h->nv_offs.assign((size_t)n_streams + 1, 0);
        for (int s = 0; s < n_streams; ++s) {
            const size_t px = (size_t)image_rows[s] * image_cols[s];
            h->offs[s + 1] = (h->offs[s] + px * 3 + 255) / 256 * 256;
            h->nv_offs[s + 1] = (h->nv_offs[s] + px * 3 / 2 + 255) / 256 * 256;
        }
        ingest_build(h);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

int boxmot_hip_ingest_format(BoxMOTHipIngest* handle) { return handle ? handle->format : -1; }

void boxmot_hip_ingest_destroy(BoxMOTHipIngest* handle) { destroy_on(handle); }

static void ingest_slot(BoxMOTHipIngest* h, int slot) {
    if (!h) throw std::runtime_error("boxmot_hip: null ingest handle");
    if (slot < 0 || slot >= h->n_slots) throw std::runtime_error("boxmot_hip: ingest slot out of range");
}

// a letterbox launch that reads the slot's frames (boxmot_hip_ingest_letterbox) must be done before they are overwritten; a ring
// that never letterboxes has no such event and makes no call here
static void ingest_wait_letterbox(BoxMOTHipIngest* h, int slot) {
    if (!h->has_lb.empty() && h->has_lb[slot]) BM_HIP(hipStreamWaitEvent(h->copy_stream, h->lb_done[slot], 0));
}

uint8_t* boxmot_hip_ingest_host_ptr(BoxMOTHipIngest* handle, int slot, int stream) {
    uint8_t* p = nullptr;
    guard_on(handle, [&]() {
        ingest_slot(handle, slot);
        if (stream < 0 || stream >= handle->n_streams) throw std::runtime_error("boxmot_hip: stream index out of range");
        p = handle->h_slot[slot] + (handle->format ? handle->nv_offs : handle->offs)[stream];
    });
    return p;
}

const uint8_t* const* boxmot_hip_ingest_device_frames(BoxMOTHipIngest* handle, int slot) {
    const uint8_t* const* p = nullptr;
    guard_on(handle, [&]() { ingest_slot(handle, slot); p = handle->d_ptrs[slot]; });
    return p;
}

int boxmot_hip_ingest_submit(BoxMOTHipIngest* handle, int slot, int n_streams) {
    return guard_on(handle, [&]() {
        ingest_slot(handle, slot);
        if (n_streams < 1 || n_streams > handle->n_streams) throw std::runtime_error("boxmot_hip: stream count out of range");
        // the previous consumer of this slot must be done with the device frames before they are overwritten
        if (handle->has_consumer[slot]) BM_HIP(hipStreamWaitEvent(handle->copy_stream, handle->consumed[slot], 0));
        ingest_wait_letterbox(handle, slot);
        if (handle->format) {           // the NV12 bytes, then their conversion into the slot's BGR frames
            BM_HIP(hipMemcpyAsync(handle->d_nv[slot], handle->h_slot[slot], handle->nv_offs[n_streams], hipMemcpyHostToDevice,
                                  handle->copy_stream));
            hipLaunchKernelGGL(bm::k_nv12_to_bgr, dim3((unsigned)bm::nv12_grid_x(handle->nv_desc[slot].data(), n_streams), (unsigned)n_streams),
                               dim3(bm::NV12_THREADS), 0, handle->copy_stream, (const bm::Nv12Desc*)handle->d_desc[slot]);
            BM_HIP(hipGetLastError());
        } else {
            BM_HIP(hipMemcpyAsync(handle->d_slot[slot], handle->h_slot[slot], handle->offs[n_streams], hipMemcpyHostToDevice,
                                  handle->copy_stream));
        }
        BM_HIP(hipEventRecord(handle->uploaded[slot], handle->copy_stream));
    });
}

// NV12 surfaces that already are in device memory (a hardware decoder's output): no DMA, the conversion reads them and writes the
// slot's BGR frames under the same consumer wait / uploaded event.  Any ring: only the device side is used.
int boxmot_hip_ingest_submit_device_nv12(BoxMOTHipIngest* handle, int slot, int n_streams, const uint8_t* const* d_y, const uint8_t* const* d_uv,
                                         const int* pitch_y, const int* pitch_uv) {
    return guard_on(handle, [&]() {
        ingest_slot(handle, slot);
        if (n_streams < 1 || n_streams > handle->n_streams) throw std::runtime_error("boxmot_hip: stream count out of range");
        if (!d_y || !d_uv || !pitch_y || !pitch_uv) throw std::runtime_error("boxmot_hip: null argument");
        for (int s = 0; s < n_streams; ++s) {
            const std::string who = "boxmot_hip: ingest ring stream " + std::to_string(s);
            if (handle->srows[s] % 2 || handle->scols[s] % 2)
                throw std::runtime_error(who + ": NV12 frames have even rows and cols, this stream is " + std::to_string(handle->srows[s]) + " x " +
                                         std::to_string(handle->scols[s]));
            if (!d_y[s] || !d_uv[s]) throw std::runtime_error(who + ": null NV12 plane");
            if (pitch_y[s] < handle->scols[s] || pitch_uv[s] < handle->scols[s])
                throw std::runtime_error(who + ": pitch below the " + std::to_string(handle->scols[s]) + " columns of the frame");
        }
        if (handle->h_ext.empty()) {
            handle->ext_used.assign(handle->n_slots, 0);
            for (int k = 0; k < handle->n_slots; ++k) {
                void *hp = nullptr, *dp = nullptr;
                BM_HIP(hipHostMalloc(&hp, handle->n_streams * sizeof(bm::Nv12Desc), hipHostMallocDefault));
                handle->h_ext.push_back(static_cast<bm::Nv12Desc*>(hp));
                BM_HIP(hipMalloc(&dp, handle->n_streams * sizeof(bm::Nv12Desc)));
                handle->d_ext.push_back(static_cast<bm::Nv12Desc*>(dp));
            }
        }
        // the slot's pinned descriptor staging is rewritten: its previous copy must have left it (long done in a ring that is cycled)
        if (handle->ext_used[slot]) BM_HIP(hipEventSynchronize(handle->uploaded[slot]));
        bm::Nv12Desc* desc = handle->h_ext[slot];
        for (int s = 0; s < n_streams; ++s)
            desc[s] = bm::Nv12Desc{d_y[s], d_uv[s], pitch_y[s], pitch_uv[s], handle->srows[s], handle->scols[s], handle->d_slot[slot] + handle->offs[s]};
        const int gx = bm::nv12_grid_x(desc, n_streams);
        if (handle->has_consumer[slot]) BM_HIP(hipStreamWaitEvent(handle->copy_stream, handle->consumed[slot], 0));
        ingest_wait_letterbox(handle, slot);
        BM_HIP(hipMemcpyAsync(handle->d_ext[slot], desc, n_streams * sizeof(bm::Nv12Desc), hipMemcpyHostToDevice, handle->copy_stream));
        handle->ext_used[slot] = 1;
        hipLaunchKernelGGL(bm::k_nv12_to_bgr, dim3((unsigned)gx, (unsigned)n_streams), dim3(bm::NV12_THREADS), 0, handle->copy_stream,
                           (const bm::Nv12Desc*)handle->d_ext[slot]);
        BM_HIP(hipGetLastError());
        BM_HIP(hipEventRecord(handle->uploaded[slot], handle->copy_stream));
    });
}

// test / utility access: the slot's BGR device frame of `stream` (rows x cols x 3 bytes) once its upload is done
int boxmot_hip_ingest_download(BoxMOTHipIngest* handle, int slot, int stream, uint8_t* out) {
    return guard_on(handle, [&]() {
        ingest_slot(handle, slot);
        if (stream < 0 || stream >= handle->n_streams) throw std::runtime_error("boxmot_hip: stream index out of range");
        if (!out) throw std::runtime_error("boxmot_hip: null argument");
        BM_HIP(hipEventSynchronize(handle->uploaded[slot]));
        BM_HIP(hipMemcpy(out, handle->d_slot[slot] + handle->offs[stream], (size_t)handle->srows[stream] * handle->scols[stream] * 3,
                         hipMemcpyDeviceToHost));
    });
}

int boxmot_hip_ingest_wait(BoxMOTHipIngest* handle, int slot, void* consumer_stream) {
    return guard_on(handle, [&]() {
        ingest_slot(handle, slot);
        BM_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), handle->uploaded[slot], 0));
    });
}

int boxmot_hip_ingest_release(BoxMOTHipIngest* handle, int slot, void* consumer_stream) {
    return guard_on(handle, [&]() {
        ingest_slot(handle, slot);
        BM_HIP(hipEventRecord(handle->consumed[slot], static_cast<hipStream_t>(consumer_stream)));
        handle->has_consumer[slot] = 1;
    });
}

int boxmot_hip_ingest_host_done(BoxMOTHipIngest* handle, int slot) {
    return guard_on(handle, [&]() {
        ingest_slot(handle, slot);
        BM_HIP(hipEventSynchronize(handle->uploaded[slot]));       // the host buffer of the slot may be refilled
    });
}

// ---- letterboxed detector input from a slot (csrc/ingest_letterbox.hpp has the definition) ----
static void letterbox_check_config(const BoxMOTHipLetterbox* cfg) {
    if (!cfg) throw std::runtime_error("boxmot_hip: null letterbox config");
    if (cfg->out_rows < 1 || cfg->out_cols < 1) throw std::runtime_error("boxmot_hip: letterbox output size must be positive");
    if (cfg->mode != 0 && cfg->mode != 1) throw std::runtime_error("boxmot_hip: unknown letterbox mode " + std::to_string(cfg->mode) + " (0 center, 1 topleft)");
}

int boxmot_hip_letterbox_geometry(int image_rows, int image_cols, const BoxMOTHipLetterbox* cfg, double* out) {
    return guard([&]() {
        letterbox_check_config(cfg);
        if (!out) throw std::runtime_error("boxmot_hip: null argument");
        if (image_rows < 1 || image_cols < 1) throw std::runtime_error("boxmot_hip: frame dimensions must be positive");
        bm::LetterboxGeom g;
        const bool ok = bm::letterbox_geometry(image_rows, image_cols, cfg->out_rows, cfg->out_cols, cfg->mode, &out[0], &g);
        out[1] = g.new_w; out[2] = g.new_h; out[3] = g.top; out[4] = g.left;
        if (!ok)
            throw std::runtime_error("boxmot_hip: letterbox of a " + std::to_string(image_rows) + " x " + std::to_string(image_cols) + " frame into " +
                                     std::to_string(cfg->out_rows) + " x " + std::to_string(cfg->out_cols) + " leaves no picture (" +
                                     std::to_string(g.new_h) + " x " + std::to_string(g.new_w) + ")");
    });
}

// fp32 -> fp16 bits, round to nearest even, for the table's values (0 or a normal fp16: 1 / 255 .. 255)
static uint32_t letterbox_half_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    if (x == 0) return 0;
    uint32_t h = ((((x >> 23) & 255u) - 127u + 15u) << 10) | ((x & 0x7fffffu) >> 13);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h += 1;             // (a carry out of the mantissa raises the exponent)
    return h;
}

// what every letterbox launch checks of its arguments before it touches the handle's tables
static void letterbox_check_call(BoxMOTHipIngest* handle, int slot, int n_streams, const BoxMOTHipLetterbox* cfg, const void* d_out) {
    ingest_slot(handle, slot);
    if (n_streams < 1 || n_streams > handle->n_streams) throw std::runtime_error("boxmot_hip: stream count out of range");
    letterbox_check_config(cfg);
    if (cfg->dtype != 0 && cfg->dtype != 1) throw std::runtime_error("boxmot_hip: unknown letterbox dtype " + std::to_string(cfg->dtype) + " (0 fp32, 1 fp16)");
    if (cfg->out_cols % bm::LB_PX) throw std::runtime_error("boxmot_hip: letterbox out_cols must be a multiple of 8, got " + std::to_string(cfg->out_cols));
    if (cfg->pad_value < 0 || cfg->pad_value > 255) throw std::runtime_error("boxmot_hip: letterbox pad_value must be within 0..255, got " + std::to_string(cfg->pad_value));
    if (!d_out) throw std::runtime_error("boxmot_hip: null letterbox output");
    if ((uintptr_t)d_out & 15) throw std::runtime_error("boxmot_hip: the letterbox output must be 16-byte aligned");
}

// the 256-entry table of (unit, dtype) and the slots' letterbox events, made on first use; returns the table's index in d_lb_lut
static int letterbox_table_and_events(BoxMOTHipIngest* handle, const BoxMOTHipLetterbox* cfg) {
    const int which = 2 * (cfg->unit ? 1 : 0) + cfg->dtype;
    if (!handle->d_lb_lut[which]) {
        uint32_t lut[256];
        for (int v = 0; v < 256; ++v) {
            const float f = cfg->unit ? (float)v / 255.0f : (float)v;
            if (cfg->dtype) lut[v] = letterbox_half_bits(f);
            else std::memcpy(&lut[v], &f, 4);
        }
        void* lp = nullptr;
        BM_HIP(hipMalloc(&lp, sizeof(lut)));
        handle->d_lb_lut[which] = static_cast<uint32_t*>(lp);
        BM_HIP(hipMemcpy(lp, lut, sizeof(lut), hipMemcpyHostToDevice));
    }
    if (handle->lb_done.empty()) {
        for (int k = 0; k < handle->n_slots; ++k) {
            hipEvent_t e;
            BM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            handle->lb_done.push_back(e);
        }
        handle->has_lb.assign(handle->n_slots, 0);
    }
    return which;
}

// What the two letterbox entry points do around their own launch, once they have their geometry table.  Before it: the 256-entry
// table and the events on first use, and the wait for the slot's upload; returns the table.  After it: the slot's letterbox event.
static const uint32_t* letterbox_before_launch(BoxMOTHipIngest* handle, int slot, const BoxMOTHipLetterbox* cfg, hipStream_t st) {
    const int which = letterbox_table_and_events(handle, cfg);
    BM_HIP(hipStreamWaitEvent(st, handle->uploaded[slot], 0));
    return handle->d_lb_lut[which];
}
static void letterbox_after_launch(BoxMOTHipIngest* handle, int slot, hipStream_t st) {
    BM_HIP(hipGetLastError());
    BM_HIP(hipEventRecord(handle->lb_done[slot], st));
    handle->has_lb[slot] = 1;
}

int boxmot_hip_ingest_letterbox(BoxMOTHipIngest* handle, int slot, int n_streams, const BoxMOTHipLetterbox* cfg, void* d_out,
                                void* consumer_hip_stream) {
    return guard_on(handle, [&]() {
        letterbox_check_call(handle, slot, n_streams, cfg, d_out);
        const int H = cfg->out_rows, W = cfg->out_cols;
        // the streams' geometry for this (H, W, mode): computed and copied to the device once, so a steady-state call copies nothing
        BoxMOTHipIngest::LetterboxTable* tab = nullptr;
        for (auto& t : handle->lb_tables) if (t.H == H && t.W == W && t.mode == cfg->mode) tab = &t;
        if (!tab) {
            if (handle->lb_tables.size() >= 16) {           // a caller that keeps changing the size: drop the oldest (hipFree waits for the device)
                BM_HIP(hipFree(handle->lb_tables.front().d_geom));
                handle->lb_tables.erase(handle->lb_tables.begin());
            }
            BoxMOTHipIngest::LetterboxTable t{H, W, cfg->mode, {}, {}, nullptr};
            t.geom.resize(handle->n_streams); t.ok.resize(handle->n_streams);
            for (int s = 0; s < handle->n_streams; ++s)
                t.ok[s] = bm::letterbox_geometry(handle->srows[s], handle->scols[s], H, W, cfg->mode, nullptr, &t.geom[s]) ? 1 : 0;
            void* dp = nullptr;
            BM_HIP(hipMalloc(&dp, handle->n_streams * sizeof(bm::LetterboxGeom)));
            t.d_geom = static_cast<bm::LetterboxGeom*>(dp);
            handle->lb_tables.push_back(std::move(t));
            tab = &handle->lb_tables.back();
            BM_HIP(hipMemcpy(dp, tab->geom.data(), handle->n_streams * sizeof(bm::LetterboxGeom), hipMemcpyHostToDevice));
        }
        for (int s = 0; s < n_streams; ++s)
            if (!tab->ok[s])
                throw std::runtime_error("boxmot_hip: ingest ring stream " + std::to_string(s) + ": letterbox of a " + std::to_string(handle->srows[s]) +
                                         " x " + std::to_string(handle->scols[s]) + " frame into " + std::to_string(H) + " x " + std::to_string(W) +
                                         " leaves no picture (" + std::to_string(tab->geom[s].new_h) + " x " + std::to_string(tab->geom[s].new_w) + ")");
        hipStream_t st = static_cast<hipStream_t>(consumer_hip_stream);
        const uint32_t* lut = letterbox_before_launch(handle, slot, cfg, st);
        hipLaunchKernelGGL(bm::k_letterbox, dim3((unsigned)bm::letterbox_grid_x(H, W), (unsigned)n_streams), dim3(bm::LB_THREADS), 0, st,
                           (const uint8_t* const*)handle->d_ptrs[slot], (const bm::LetterboxGeom*)tab->d_geom, lut, d_out, H, W, cfg->dtype,
                           cfg->rgb ? 1 : 0, cfg->pad_value);
        letterbox_after_launch(handle, slot, st);
    });
}

// ---- letterboxed rectangles of the frames: sliced inference (csrc/ingest_letterbox_tiles.hpp has the definition) ----
static std::string letterbox_tile_name(int s, int t, const int* r) {
    return "stream " + std::to_string(s) + " tile " + std::to_string(t) + " (x0 " + std::to_string(r[0]) + ", y0 " + std::to_string(r[1]) + ", w " +
           std::to_string(r[2]) + ", h " + std::to_string(r[3]) + ")";
}

int boxmot_hip_letterbox_tile_geometry(int image_rows, int image_cols, const int* rect, const BoxMOTHipLetterbox* cfg, double* out) {
    return guard([&]() {
        letterbox_check_config(cfg);
        if (!out || !rect) throw std::runtime_error("boxmot_hip: null argument");
        if (image_rows < 1 || image_cols < 1) throw std::runtime_error("boxmot_hip: frame dimensions must be positive");
        for (int k = 0; k < 9; ++k) out[k] = 0.0;
        out[5] = rect[3]; out[6] = rect[2]; out[7] = rect[0]; out[8] = rect[1];
        if (!bm::letterbox_tile_inside(image_rows, image_cols, rect[0], rect[1], rect[2], rect[3]))
            throw std::runtime_error("boxmot_hip: letterbox rectangle (x0 " + std::to_string(rect[0]) + ", y0 " + std::to_string(rect[1]) + ", w " +
                                     std::to_string(rect[2]) + ", h " + std::to_string(rect[3]) + ") is not inside the " + std::to_string(image_rows) +
                                     " x " + std::to_string(image_cols) + " frame");
        bm::LetterboxTileGeom g;
        const bool ok = bm::letterbox_tile_geometry(image_cols, rect[0], rect[1], rect[2], rect[3], cfg->out_rows, cfg->out_cols, cfg->mode, &out[0], &g);
        out[1] = g.g.new_w; out[2] = g.g.new_h; out[3] = g.g.top; out[4] = g.g.left;
        if (!ok)
            throw std::runtime_error("boxmot_hip: letterbox of a " + std::to_string(rect[3]) + " x " + std::to_string(rect[2]) + " rectangle into " +
                                     std::to_string(cfg->out_rows) + " x " + std::to_string(cfg->out_cols) + " leaves no picture (" +
                                     std::to_string(g.g.new_h) + " x " + std::to_string(g.g.new_w) + ")");
    });
}

int boxmot_hip_ingest_letterbox_tiles(BoxMOTHipIngest* handle, int slot, int n_streams, int n_tiles, const int* rects, const BoxMOTHipLetterbox* cfg,
                                      void* d_out, void* consumer_hip_stream) {
    return guard_on(handle, [&]() {
        letterbox_check_call(handle, slot, n_streams, cfg, d_out);
        if (n_tiles < 1 || n_tiles > bm::LB_TILES_MAX)
            throw std::runtime_error("boxmot_hip: letterbox n_tiles must be within 1.." + std::to_string(bm::LB_TILES_MAX) + ", got " + std::to_string(n_tiles));
        if (!rects) throw std::runtime_error("boxmot_hip: null letterbox rectangles");
        const int H = cfg->out_rows, W = cfg->out_cols;
        const size_t n = (size_t)n_streams * n_tiles;
        if (n > 65535) throw std::runtime_error("boxmot_hip: letterbox n_streams * n_tiles must not exceed 65535 (grid.y), got " + std::to_string(n));
        // every rectangle is checked on every call, before anything is launched: the kernel reads what the table says
        for (int s = 0; s < n_streams; ++s)
            for (int t = 0; t < n_tiles; ++t) {
                const int* r = rects + ((size_t)s * n_tiles + t) * 4;
                if (!bm::letterbox_tile_inside(handle->srows[s], handle->scols[s], r[0], r[1], r[2], r[3]))
                    throw std::runtime_error("boxmot_hip: ingest ring " + letterbox_tile_name(s, t, r) + " is not inside the " +
                                             std::to_string(handle->srows[s]) + " x " + std::to_string(handle->scols[s]) + " frame");
            }
        // the geometry of these rectangles for this (H, W, mode): computed and copied to the device once
        BoxMOTHipIngest::TileTable* tab = nullptr;
        for (auto& t : handle->lb_tile_tables)
            if (t.H == H && t.W == W && t.mode == cfg->mode && t.n_streams == n_streams && t.n_tiles == n_tiles &&
                std::memcmp(t.rects.data(), rects, n * 4 * sizeof(int)) == 0)
                tab = &t;
        if (!tab) {
            std::vector<bm::LetterboxTileGeom> geom(n);
            for (int s = 0; s < n_streams; ++s)
                for (int t = 0; t < n_tiles; ++t) {
                    const int* r = rects + ((size_t)s * n_tiles + t) * 4;
                    bm::LetterboxTileGeom& g = geom[(size_t)s * n_tiles + t];
                    if (!bm::letterbox_tile_geometry(handle->scols[s], r[0], r[1], r[2], r[3], H, W, cfg->mode, nullptr, &g))
                        throw std::runtime_error("boxmot_hip: ingest ring " + letterbox_tile_name(s, t, r) + ": letterbox into " + std::to_string(H) + " x " +
                                                 std::to_string(W) + " leaves no picture (" + std::to_string(g.g.new_h) + " x " + std::to_string(g.g.new_w) + ")");
                }
            if (handle->lb_tile_tables.size() >= 16) {      // a caller that keeps changing the rectangles: drop the oldest (hipFree waits for the device)
                BM_HIP(hipFree(handle->lb_tile_tables.front().d_geom));
                handle->lb_tile_tables.erase(handle->lb_tile_tables.begin());
            }
            void* dp = nullptr;
            BM_HIP(hipMalloc(&dp, n * sizeof(bm::LetterboxTileGeom)));
            const hipError_t copied = hipMemcpy(dp, geom.data(), n * sizeof(bm::LetterboxTileGeom), hipMemcpyHostToDevice);
            if (copied != hipSuccess) { (void)hipFree(dp); BM_HIP(copied); }
            handle->lb_tile_tables.push_back(BoxMOTHipIngest::TileTable{H, W, cfg->mode, n_streams, n_tiles, std::vector<int>(rects, rects + n * 4),
                                                                         static_cast<bm::LetterboxTileGeom*>(dp)});
            tab = &handle->lb_tile_tables.back();
        }
        hipStream_t st = static_cast<hipStream_t>(consumer_hip_stream);
        const uint32_t* lut = letterbox_before_launch(handle, slot, cfg, st);
        hipLaunchKernelGGL(bm::k_letterbox_tiles, dim3((unsigned)bm::letterbox_grid_x(H, W), (unsigned)n), dim3(bm::LB_THREADS), 0, st,
                           (const uint8_t* const*)handle->d_ptrs[slot], (const bm::LetterboxTileGeom*)tab->d_geom, lut, d_out, n_tiles, H, W,
                           cfg->dtype, cfg->rgb ? 1 : 0, cfg->pad_value);
        letterbox_after_launch(handle, slot, st);
    });
}

// ---- detection post-processing (csrc/det_post.hpp has the definition) ----
namespace {
// the create entry points; oc: the oriented options, or null for an axis-aligned handle; tc: the tiled options, or null; ec: the
// per-anchor extras (with tc made of its n_tiles and merge when tiled), or null; mc: the mask options (with ec its extras), or null
BoxMOTHipDetPost* detpost_create(const BoxMOTHipDetPostConfig* c, const BoxMOTHipDetPostObbConfig* oc, const BoxMOTHipDetPostTiledConfig* tc = nullptr,
                                 const BoxMOTHipDetPostExtraConfig* ec = nullptr, const BoxMOTHipDetPostMaskConfig* mc = nullptr) {
    BoxMOTHipDetPost* h = nullptr;
    const int ok = guard([&]() {
        if (!c) throw std::runtime_error("boxmot_hip: null detpost config");
        if (ec && (ec->n_extra < 1 || ec->n_extra > bm::DP_EXTRA_MAX))
            throw std::runtime_error("boxmot_hip: detpost n_extra must be within 1.." + std::to_string(bm::DP_EXTRA_MAX) + ", got " + std::to_string(ec->n_extra));
        if (ec && (ec->extra_kind < 0 || ec->extra_kind >= bm::DP_EXTRA_KINDS))
            throw std::runtime_error("boxmot_hip: unknown detpost extra_kind " + std::to_string(ec->extra_kind) + " (0 raw, 1 kpt2, 2 kpt3)");
        if (ec && ec->n_extra % bm::detpost_extra_group(ec->extra_kind))
            throw std::runtime_error("boxmot_hip: detpost n_extra " + std::to_string(ec->n_extra) + " is no multiple of the " +
                                     std::to_string(bm::detpost_extra_group(ec->extra_kind)) + " values per keypoint of extra_kind " + std::to_string(ec->extra_kind));
        if (mc && ec->extra_kind != 0)
            throw std::runtime_error("boxmot_hip: a detpost mask handle needs extra_kind 0 (raw), got " + std::to_string(ec->extra_kind));
        if (mc && ec->n_extra > bm::DP_MASK_E_MAX)
            throw std::runtime_error("boxmot_hip: a detpost mask handle needs n_extra within 1.." + std::to_string(bm::DP_MASK_E_MAX) + ", got " + std::to_string(ec->n_extra));
        if (mc && (mc->mask_h < 1 || mc->mask_h > bm::DP_MASK_DIM_MAX || mc->mask_w < 1 || mc->mask_w > bm::DP_MASK_DIM_MAX))
            throw std::runtime_error("boxmot_hip: detpost mask_h and mask_w must be within 1.." + std::to_string(bm::DP_MASK_DIM_MAX) + ", got " +
                                     std::to_string(mc->mask_h) + " x " + std::to_string(mc->mask_w));
        if (mc && (mc->in_h < 1 || mc->in_w < 1))
            throw std::runtime_error("boxmot_hip: detpost in_h and in_w must be >= 1, got " + std::to_string(mc->in_h) + " x " + std::to_string(mc->in_w));
        if (oc && c->layout != 0)
            throw std::runtime_error("boxmot_hip: an oriented detpost handle needs base.layout 0 (cn), got " + std::to_string(c->layout));
        if (oc && oc->nms_mode != 0 && oc->nms_mode != 1)
            throw std::runtime_error("boxmot_hip: unknown detpost nms_mode " + std::to_string(oc->nms_mode) + " (0 greedy, 1 fast)");
        if (c->n_streams < 1 || c->n_anchors < 1 || c->n_classes < 1)
            throw std::runtime_error("boxmot_hip: detpost needs n_streams, n_anchors and n_classes >= 1");
        if (c->layout != 0 && c->layout != 1) throw std::runtime_error("boxmot_hip: unknown detpost layout " + std::to_string(c->layout) + " (0 cn, 1 nc_obj)");
        if (!(c->conf_thres >= 0.0f) || !(c->conf_thres < 1.0f)) throw std::runtime_error("boxmot_hip: detpost conf_thres must be within [0, 1)");
        if (!(c->iou_thres >= 0.0f) || !(c->iou_thres <= 1.0f)) throw std::runtime_error("boxmot_hip: detpost iou_thres must be within [0, 1]");
        if (c->max_candidates < bm::DP_K_MIN || c->max_candidates > bm::DP_K_MAX)
            throw std::runtime_error("boxmot_hip: detpost max_candidates must be within 64..4096, got " + std::to_string(c->max_candidates));
        if (c->max_det < 1) throw std::runtime_error("boxmot_hip: detpost max_det must be >= 1");
        if (ec && (long)c->max_det * ec->n_extra > (1L << 30)) throw std::runtime_error("boxmot_hip: detpost max_det * n_extra is too large");
        if ((long)c->n_streams * c->n_anchors > (1L << 30)) throw std::runtime_error("boxmot_hip: detpost n_streams * n_anchors is too large");
        if (tc && (tc->n_tiles < 1 || tc->n_tiles > bm::DP_TILES_MAX))
            throw std::runtime_error("boxmot_hip: detpost n_tiles must be within 1.." + std::to_string(bm::DP_TILES_MAX) + ", got " + std::to_string(tc->n_tiles));
        if (tc && tc->merge != 0 && tc->merge != 1) throw std::runtime_error("boxmot_hip: unknown detpost merge " + std::to_string(tc->merge) + " (0 iou, 1 ios)");
        const int n_tensors = tc ? tc->n_tiles : 1;         // per stream
        if ((long)c->n_streams * n_tensors * c->n_anchors > (1L << 30))
            throw std::runtime_error("boxmot_hip: detpost n_streams * n_tiles * n_anchors is too large");
        if ((long)c->n_streams * n_tensors > 65535) throw std::runtime_error("boxmot_hip: detpost n_streams * n_tiles must not exceed 65535 (grid.y)");
        require_device();
        h = new BoxMOTHipDetPost();
        h->cfg = *c;
        h->cfg.class_allow = nullptr;
        if (oc) { h->obb = 1; h->nms_mode = oc->nms_mode; h->regularize = oc->regularize ? 1 : 0; }
        if (tc) { h->n_tiles = tc->n_tiles; h->merge = tc->merge; }
        if (ec) { h->n_extra = ec->n_extra; h->extra_kind = ec->extra_kind; }
        if (mc) {
            h->mask_h = mc->mask_h; h->mask_w = mc->mask_w;
            h->mask_wr = (float)mc->mask_w / (float)mc->in_w; h->mask_hr = (float)mc->mask_h / (float)mc->in_h;
        }
        const size_t SA = (size_t)c->n_streams * n_tensors * c->n_anchors;
        void* p = nullptr;
        BM_HIP(hipMalloc(&p, SA * sizeof(uint32_t))); h->d_keys = static_cast<uint32_t*>(p);
        BM_HIP(hipMalloc(&p, SA * sizeof(int))); h->d_cls = static_cast<int*>(p);
        BM_HIP(hipMalloc(&p, (size_t)c->n_streams * bm::DP_COUNTERS * sizeof(int))); h->d_counters = static_cast<int*>(p);
        BM_HIP(hipMemset(h->d_counters, 0, (size_t)c->n_streams * bm::DP_COUNTERS * sizeof(int)));
        if (c->class_allow) {
            std::vector<uint8_t> allow(c->n_classes);
            for (int k = 0; k < c->n_classes; ++k) allow[k] = c->class_allow[k] ? 1 : 0;
            BM_HIP(hipMalloc(&p, allow.size())); h->d_allow = static_cast<uint8_t*>(p);
            BM_HIP(hipMemcpy(h->d_allow, allow.data(), allow.size(), hipMemcpyHostToDevice));
        }
        BM_HIP(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
        if (ec) { BM_HIP(hipMalloc(&p, (size_t)c->n_streams * c->max_det * sizeof(int))); h->d_src = static_cast<int*>(p); }
        if (tc) {
            h->tgeom.create((size_t)c->n_streams * tc->n_tiles);
            if (ec) detpost_allow_lds(bm::k_detpost_select_tiled_src<float>, bm::k_detpost_select_tiled_src<_Float16>, bm::detpost_lds_bytes(c->max_candidates));
            else detpost_allow_lds(bm::k_detpost_select_tiled<float>, bm::k_detpost_select_tiled<_Float16>, bm::detpost_lds_bytes(c->max_candidates));
        } else {
            h->geom.create((size_t)c->n_streams);
            if (oc) detpost_allow_lds(bm::k_detpost_select_obb<float>, bm::k_detpost_select_obb<_Float16>, bm::detpost_obb_lds_bytes(c->max_candidates));
            else if (ec) detpost_allow_lds(bm::k_detpost_select_src<float>, bm::k_detpost_select_src<_Float16>, bm::detpost_lds_bytes(c->max_candidates));
            else detpost_allow_lds(bm::k_detpost_select<float>, bm::k_detpost_select<_Float16>, bm::detpost_lds_bytes(c->max_candidates));
        }
    });
    if (!ok) { const std::string e = g_last_error; destroy_on(h); g_last_error = e; return nullptr; }
    return h;
}

// the checked geometry rows of an untiled / a tiled call, and the kernels' arguments (d_extra / d_src: a handle with extras)
void detpost_geom_rows(const double* geom, int n_streams, std::vector<bm::DetPostGeom>& g) {
    g.resize(n_streams);
    for (int s = 0; s < n_streams; ++s) {
        const double* v = geom + 5 * s;
        if (!(v[0] > 0.0) || !std::isfinite(v[0]) || !(v[3] >= 1.0) || !(v[4] >= 1.0) || !std::isfinite(v[1]) || !std::isfinite(v[2]) ||
            !std::isfinite(v[3]) || !std::isfinite(v[4]))
            throw std::runtime_error("boxmot_hip: detpost stream " + std::to_string(s) + ": geometry needs gain > 0 and a frame of >= 1 x 1 (gain " +
                                     std::to_string(v[0]) + ", rows " + std::to_string(v[3]) + ", cols " + std::to_string(v[4]) + ")");
        g[s] = bm::DetPostGeom{(float)v[0], (float)v[1], (float)v[2], (float)v[3], (float)v[4]};
    }
}
void detpost_tile_geom_rows(const double* geom, int n_streams, int T, std::vector<bm::DetPostTileGeom>& g) {
    g.resize((size_t)n_streams * T);
    for (size_t k = 0; k < g.size(); ++k) {
        const double* v = geom + 7 * k;
        bool finite = true;
        for (int q = 0; q < 7; ++q) finite = finite && std::isfinite(v[q]);
        if (!finite || !(v[0] > 0.0) || !(v[5] >= 1.0) || !(v[6] >= 1.0))
            throw std::runtime_error("boxmot_hip: detpost stream " + std::to_string(k / T) + " tile " + std::to_string(k % T) +
                                     ": geometry needs finite values, gain > 0 and a tile of >= 1 x 1 (gain " + std::to_string(v[0]) + ", w " +
                                     std::to_string(v[5]) + ", h " + std::to_string(v[6]) + ")");
        g[k] = bm::DetPostTileGeom{(float)v[0], (float)v[1], (float)v[2], (float)v[3], (float)v[4], (float)v[5], (float)v[6]};
    }
}
bm::DetPostArgs detpost_args(const BoxMOTHipDetPost* handle, const void* d_pred, float* d_dets, int out_stride_rows, int* d_det_rows,
                             float* d_extra = nullptr, int* d_src = nullptr) {
    const BoxMOTHipDetPostConfig& c = handle->cfg;
    bm::DetPostArgs a{d_pred, handle->n_tiles ? nullptr : handle->geom.d, handle->d_allow, handle->d_keys, handle->d_cls, d_dets, d_det_rows, handle->d_counters,
                      c.n_anchors, c.n_classes, c.layout, c.max_candidates, c.max_det, c.agnostic ? 1 : 0, out_stride_rows, c.conf_thres,
                      c.iou_thres, handle->obb, handle->nms_mode, handle->regularize};
    if (handle->n_extra) {
        a.src = d_src ? d_src : handle->d_src;
        a.src_stride = d_src ? out_stride_rows : c.max_det;
        a.extra = d_extra; a.n_extra = handle->n_extra; a.extra_kind = handle->extra_kind;
    }
    return a;
}
// a mask handle is run with boxmot_hip_detpost_run_mask alone
void detpost_refuse_mask(const BoxMOTHipDetPost* handle) {
    if (handle && handle->mask_h) throw std::runtime_error("boxmot_hip: a detpost mask handle is run with boxmot_hip_detpost_run_mask");
}
// an untiled or a tiled run, by the handle's kind
void detpost_run_checked(BoxMOTHipDetPost* handle, int n_streams, int dtype, const double* geom, const bm::DetPostArgs& a, void* hip_stream) {
    if (handle->n_tiles) {
        const bm::DetPostTiledArgs ta{a, handle->tgeom.d, handle->n_tiles, handle->merge};
        std::vector<bm::DetPostTileGeom> g;
        detpost_tile_geom_rows(geom, n_streams, handle->n_tiles, g);
        detpost_run(handle, handle->tgeom, g, n_streams, hip_stream, [&](DetPostLaunch& on) { bm::detpost_launch_tiled(on, ta, n_streams, dtype); });
    } else {
        std::vector<bm::DetPostGeom> g;
        detpost_geom_rows(geom, n_streams, g);
        detpost_run(handle, handle->geom, g, n_streams, hip_stream, [&](DetPostLaunch& on) { bm::detpost_launch(on, a, n_streams, dtype); });
    }
}
// ... and of a mask handle: the same sequences with k_detpost_mask fourth (csrc/det_post_mask.hpp)
void detpost_run_checked_mask(BoxMOTHipDetPost* handle, int n_streams, int dtype, const double* geom, const bm::DetPostArgs& a, const bm::DetPostMaskArgs& m,
                              int proto_dtype, void* hip_stream) {
    if (handle->n_tiles) {
        const bm::DetPostTiledArgs ta{a, handle->tgeom.d, handle->n_tiles, handle->merge};
        std::vector<bm::DetPostTileGeom> g;
        detpost_tile_geom_rows(geom, n_streams, handle->n_tiles, g);
        detpost_run(handle, handle->tgeom, g, n_streams, hip_stream,
                    [&](DetPostLaunch& on) { bm::detpost_launch_tiled_with_mask(on, ta, m, n_streams, dtype, proto_dtype); });
    } else {
        std::vector<bm::DetPostGeom> g;
        detpost_geom_rows(geom, n_streams, g);
        detpost_run(handle, handle->geom, g, n_streams, hip_stream, [&](DetPostLaunch& on) { bm::detpost_launch_with_mask(on, a, m, n_streams, dtype, proto_dtype); });
    }
}
}  // namespace

BoxMOTHipDetPost* boxmot_hip_detpost_create(const BoxMOTHipDetPostConfig* c) { return detpost_create(c, nullptr); }

BoxMOTHipDetPost* boxmot_hip_detpost_create_obb(const BoxMOTHipDetPostObbConfig* c) {
    if (!c) { g_last_error = "boxmot_hip: null detpost config"; return nullptr; }
    return detpost_create(&c->base, c);
}

void boxmot_hip_detpost_destroy(BoxMOTHipDetPost* handle) { destroy_on(handle); }

int boxmot_hip_detpost_run(BoxMOTHipDetPost* handle, int n_streams, const void* d_pred, int dtype, const double* geom, float* d_dets,
                           int out_stride_rows, int* d_det_rows, void* hip_stream) {
    return guard_on(handle, [&]() {
        detpost_refuse_mask(handle);
        detpost_check_run(handle, false, n_streams, d_pred, dtype, geom, d_dets, out_stride_rows, d_det_rows);
        detpost_run_checked(handle, n_streams, dtype, geom, detpost_args(handle, d_pred, d_dets, out_stride_rows, d_det_rows), hip_stream);
    });
}

BoxMOTHipDetPost* boxmot_hip_detpost_create_tiled(const BoxMOTHipDetPostTiledConfig* c) {
    if (!c) { g_last_error = "boxmot_hip: null detpost config"; return nullptr; }
    return detpost_create(&c->base, nullptr, c);
}

int boxmot_hip_detpost_run_tiled(BoxMOTHipDetPost* handle, int n_streams, const void* d_pred, int dtype, const double* geom, float* d_dets,
                                 int out_stride_rows, int* d_det_rows, void* hip_stream) {
    return guard_on(handle, [&]() {
        detpost_refuse_mask(handle);
        detpost_check_run(handle, true, n_streams, d_pred, dtype, geom, d_dets, out_stride_rows, d_det_rows);
        detpost_run_checked(handle, n_streams, dtype, geom, detpost_args(handle, d_pred, d_dets, out_stride_rows, d_det_rows), hip_stream);
    });
}

BoxMOTHipDetPost* boxmot_hip_detpost_create_extra(const BoxMOTHipDetPostExtraConfig* c) {
    if (!c) { g_last_error = "boxmot_hip: null detpost config"; return nullptr; }
    const BoxMOTHipDetPostTiledConfig tc{c->base, c->n_tiles, c->merge};
    return detpost_create(&c->base, nullptr, c->n_tiles ? &tc : nullptr, c);        // n_tiles 0: untiled
}

int boxmot_hip_detpost_run_extra(BoxMOTHipDetPost* handle, int n_streams, const void* d_pred, int dtype, const double* geom, float* d_dets,
                                 int out_stride_rows, int* d_det_rows, float* d_extra, int* d_src, void* hip_stream) {
    return guard_on(handle, [&]() {
        detpost_refuse_mask(handle);
        detpost_check_run(handle, handle && handle->n_tiles, n_streams, d_pred, dtype, geom, d_dets, out_stride_rows, d_det_rows, true);
        if (!d_extra) throw std::runtime_error("boxmot_hip: null detpost d_extra");
        if ((uintptr_t)d_extra % 4 || (uintptr_t)d_src % 4) throw std::runtime_error("boxmot_hip: detpost d_extra and d_src must be aligned to their element size");
        detpost_run_checked(handle, n_streams, dtype, geom, detpost_args(handle, d_pred, d_dets, out_stride_rows, d_det_rows, d_extra, d_src), hip_stream);
    });
}

BoxMOTHipDetPost* boxmot_hip_detpost_create_mask(const BoxMOTHipDetPostMaskConfig* c) {
    if (!c) { g_last_error = "boxmot_hip: null detpost config"; return nullptr; }
    const BoxMOTHipDetPostTiledConfig tc{c->extra.base, c->extra.n_tiles, c->extra.merge};
    return detpost_create(&c->extra.base, nullptr, c->extra.n_tiles ? &tc : nullptr, &c->extra, c);
}

int boxmot_hip_detpost_run_mask(BoxMOTHipDetPost* handle, int n_streams, const void* d_pred, int dtype, const double* geom, float* d_dets,
                                int out_stride_rows, int* d_det_rows, float* d_extra, int* d_src, const void* d_proto, int proto_dtype,
                                unsigned char* d_masks, void* hip_stream) {
    return guard_on(handle, [&]() {
        if (handle && !handle->mask_h) throw std::runtime_error("boxmot_hip: boxmot_hip_detpost_run_mask needs a handle of boxmot_hip_detpost_create_mask");
        detpost_check_run(handle, handle && handle->n_tiles, n_streams, d_pred, dtype, geom, d_dets, out_stride_rows, d_det_rows, true);
        if (!d_extra) throw std::runtime_error("boxmot_hip: null detpost d_extra");
        if ((uintptr_t)d_extra % 4 || (uintptr_t)d_src % 4) throw std::runtime_error("boxmot_hip: detpost d_extra and d_src must be aligned to their element size");
        if (!d_proto) throw std::runtime_error("boxmot_hip: null detpost d_proto");
        if (!d_masks) throw std::runtime_error("boxmot_hip: null detpost d_masks");
        if (proto_dtype != 0 && proto_dtype != 1)
            throw std::runtime_error("boxmot_hip: unknown detpost proto_dtype " + std::to_string(proto_dtype) + " (0 fp32, 1 fp16)");
        if ((uintptr_t)d_proto % (proto_dtype ? 2 : 4)) throw std::runtime_error("boxmot_hip: detpost d_proto must be aligned to its element size");
        const int plane = handle->mask_h * handle->mask_w;
        const bm::DetPostMaskArgs m{d_proto, d_masks, (long)handle->n_extra * plane, plane, handle->mask_h, handle->mask_w, handle->mask_wr, handle->mask_hr, 0};
        detpost_run_checked_mask(handle, n_streams, dtype, geom, detpost_args(handle, d_pred, d_dets, out_stride_rows, d_det_rows, d_extra, d_src), m,
                                 proto_dtype, hip_stream);
    });
}

int boxmot_hip_detpost_labels(BoxMOTHipDetPost* handle, int n_streams, const double* geom, const void* d_proto, int proto_dtype, const float* d_dets,
                              int det_stride, const int* d_det_rows, const float* d_extra, short* d_labels, int label_rows, int label_cols,
                              void* hip_stream) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip: null detpost handle");
        const BoxMOTHipDetPostConfig& c = handle->cfg;
        if (!handle->mask_h) throw std::runtime_error("boxmot_hip: boxmot_hip_detpost_labels needs a handle of boxmot_hip_detpost_create_mask");
        if (handle->n_tiles)
            throw std::runtime_error("boxmot_hip: boxmot_hip_detpost_labels takes an untiled mask handle: label maps of tiled handles are out of scope");
        if (c.max_det > bm::DP_LABEL_MAX_DET)
            throw std::runtime_error("boxmot_hip: boxmot_hip_detpost_labels writes int16 labels: max_det " + std::to_string(c.max_det) + " exceeds " +
                                     std::to_string(bm::DP_LABEL_MAX_DET));
        if (n_streams < 1 || n_streams > c.n_streams)
            throw std::runtime_error("boxmot_hip: detpost stream count " + std::to_string(n_streams) + " out of range for a handle of " + std::to_string(c.n_streams));
        if (!geom) throw std::runtime_error("boxmot_hip: null detpost geom");
        if (!d_proto) throw std::runtime_error("boxmot_hip: null detpost d_proto");
        if (!d_dets) throw std::runtime_error("boxmot_hip: null detpost d_dets");
        if (!d_det_rows) throw std::runtime_error("boxmot_hip: null detpost d_det_rows");
        if (!d_extra) throw std::runtime_error("boxmot_hip: null detpost d_extra");
        if (!d_labels) throw std::runtime_error("boxmot_hip: null detpost d_labels");
        if (proto_dtype != 0 && proto_dtype != 1)
            throw std::runtime_error("boxmot_hip: unknown detpost proto_dtype " + std::to_string(proto_dtype) + " (0 fp32, 1 fp16)");
        if ((uintptr_t)d_proto % (proto_dtype ? 2 : 4) || (uintptr_t)d_dets % 4 || (uintptr_t)d_det_rows % 4 || (uintptr_t)d_extra % 4 || (uintptr_t)d_labels % 2)
            throw std::runtime_error("boxmot_hip: detpost device addresses must be aligned to their element size");
        if (det_stride < c.max_det)
            throw std::runtime_error("boxmot_hip: detpost det_stride " + std::to_string(det_stride) + " is below max_det " + std::to_string(c.max_det));
        if (label_rows < 1 || label_cols < 1 || (long)label_rows * label_cols > (1L << 30))
            throw std::runtime_error("boxmot_hip: detpost label_rows x label_cols must be at least 1 x 1 and at most 2^30 pixels, got " +
                                     std::to_string(label_rows) + " x " + std::to_string(label_cols));
        std::vector<bm::DetPostGeom> g;
        detpost_geom_rows(geom, n_streams, g);
        int frame_rows = 1, frame_cols = 1;
        for (int s = 0; s < n_streams; ++s) {
            if (g[s].rows > (float)label_rows || g[s].cols > (float)label_cols)
                throw std::runtime_error("boxmot_hip: detpost stream " + std::to_string(s) + ": the frame of " + std::to_string((long)g[s].rows) + " x " +
                                         std::to_string((long)g[s].cols) + " does not fit label planes of " + std::to_string(label_rows) + " x " +
                                         std::to_string(label_cols));
            if ((int)g[s].rows > frame_rows) frame_rows = (int)g[s].rows;
            if ((int)g[s].cols > frame_cols) frame_cols = (int)g[s].cols;
        }
        const int plane = handle->mask_h * handle->mask_w;
        const bm::DetPostLabelArgs a{handle->geom.d, d_proto, d_dets, d_det_rows, d_extra, reinterpret_cast<int16_t*>(d_labels), (long)handle->n_extra * plane, (long)label_rows * label_cols,
                                     label_cols, det_stride, c.max_det, handle->n_extra, handle->mask_h, handle->mask_w, plane, handle->mask_wr, handle->mask_hr,
                                     0, 0};
        detpost_run(handle, handle->geom, g, n_streams, hip_stream, [&](DetPostLaunch& on) { bm::detpost_launch_labels(on, a, n_streams, frame_rows, frame_cols, proto_dtype); });
    });
}

int boxmot_hip_detpost_counters(BoxMOTHipDetPost* handle, int* out, int n_streams) {
    return guard_on(handle, [&]() {
        if (!handle || !out) throw std::runtime_error("boxmot_hip: null detpost argument");
        if (n_streams < 1 || n_streams > handle->cfg.n_streams) throw std::runtime_error("boxmot_hip: detpost stream count out of range");
        if (handle->ran) BM_HIP(hipEventSynchronize(handle->done));
        BM_HIP(hipMemcpy(out, handle->d_counters, (size_t)n_streams * bm::DP_COUNTERS * sizeof(int), hipMemcpyDeviceToHost));
    });
}

// ---- DeepOCSORT ----
void boxmot_hip_deepocsort_default_config(BoxMOTHipDeepOcSortConfig* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->det_thresh = 0.3; c->max_age = 30; c->max_obs = 50; c->min_hits = 3; c->iou_threshold = 0.3;
    c->delta_t = 3; c->inertia = 0.2; c->w_association_emb = 0.5; c->alpha_fixed_emb = 0.95; c->aw_param = 0.5;
    c->embedding_off = 0; c->cmc_off = 0; c->aw_off = 0; c->Q_xy_scaling = 0.01; c->Q_s_scaling = 0.0001;
    c->reid_model_path = nullptr;
    c->n_streams = 1; c->max_tracks = 1024; c->max_dets = 256; c->emb_dim = 512;
    c->use_byte = 0; c->min_conf = 0.1;
    c->asso_func = BOXMOT_HIP_ASSO_IOU; c->frame_w = 0; c->frame_h = 0;
}

BoxMOTHipDeepOcSort* boxmot_hip_deepocsort_create(const BoxMOTHipDeepOcSortConfig* config) {
    BoxMOTHipDeepOcSort* h = nullptr;
    const int ok = guard([&]() {
        if (config == nullptr) throw std::runtime_error("boxmot_hip DeepOCSORT config is required.");
        require_device();
        h = new BoxMOTHipDeepOcSort();
        h->cfg = *config;
        if (config->reid_model_path) h->reid_path = config->reid_model_path;
        h->cfg.reid_model_path = nullptr;
        docs_build(h);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

void boxmot_hip_deepocsort_destroy(BoxMOTHipDeepOcSort* handle) { destroy_on(handle); }

int boxmot_hip_deepocsort_reset(BoxMOTHipDeepOcSort* handle) { return ep_reset(handle, "DeepOCSORT", docs_zero_state); }

int boxmot_hip_deepocsort_reserve(BoxMOTHipDeepOcSort* handle, int max_tracks, int max_dets) {
    return ep_reserve(handle, "DeepOCSORT", max_tracks, max_dets, docs_grow);
}

int boxmot_hip_deepocsort_capacity(BoxMOTHipDeepOcSort* handle, int* max_tracks, int* max_dets, int* n_grows) {
    return ep_capacity(handle, "DeepOCSORT", max_tracks, max_dets, n_grows);
}

int boxmot_hip_deepocsort_set_warp(BoxMOTHipDeepOcSort* handle, int stream, const double* warp_2x3) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip DeepOCSORT handle is null.");
        if (handle->is_obb && warp_2x3) throw std::runtime_error("boxmot_hip: camera-motion warps are not applied to oriented detections");
        core_set_warp(handle, stream, warp_2x3);
    });
}

int boxmot_hip_deepocsort_update_batch(BoxMOTHipDeepOcSort* handle, int n_streams, const float* const* dets,
                                       const int* det_rows, const float* const* embs, int emb_cols,
                                       const uint8_t* const* images, int image_rows, int image_cols, int image_channels,
                                       float* const* out_tracks, int out_capacity_rows, int* out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip DeepOCSORT handle is not initialized.");
        if (n_streams < 1 || n_streams > handle->S) throw std::runtime_error("boxmot_hip: n_streams out of range");
        if (!dets || !det_rows || !out_tracks || !out_rows) throw std::runtime_error("boxmot_hip: null batch pointers");
        std::vector<StreamIn> in(n_streams);
        for (int s = 0; s < n_streams; ++s)
            in[s] = StreamIn{dets[s], det_rows[s], (embs && emb_cols > 0) ? embs[s] : nullptr, images ? images[s] : nullptr};
        docs_need_frame_size(handle, image_rows, image_cols);
        docs_host_update(handle, n_streams, in.data(), handle->det_cols, emb_cols, image_rows, image_cols, image_channels, out_tracks,
                         out_capacity_rows, out_rows);
    });
}

int boxmot_hip_deepocsort_update(BoxMOTHipDeepOcSort* handle, const float* dets, int det_rows, int det_cols,
                                 const float* embs, int emb_rows, int emb_cols, const uint8_t* image, int image_rows,
                                 int image_cols, int image_channels, float* out_tracks, int out_capacity_rows,
                                 int out_cols, int* out_rows, int* out_is_obb) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip DeepOCSORT handle is not initialized.");
        if (!out_rows || !out_is_obb) throw std::runtime_error("Output pointers are null.");
        if (out_cols != 9) throw std::runtime_error("boxmot_hip live tracking expects an output buffer with 9 columns.");
        if (embs != nullptr && emb_rows != det_rows) throw std::runtime_error("Detection and embedding row counts must match.");
        if (image_rows <= 0 || image_cols <= 0) throw std::runtime_error("Image dimensions must be positive.");
        StreamIn in{dets, det_rows, (embs && emb_cols > 0) ? embs : nullptr, image};
        float* outs[1] = {out_tracks};
        docs_need_frame_size(handle, image_rows, image_cols);
        docs_host_update(handle, 1, &in, det_cols, emb_cols, image_rows, image_cols, image_channels, outs, out_capacity_rows, out_rows);
        *out_is_obb = handle->is_obb ? 1 : 0;
    });
}

int boxmot_hip_deepocsort_update_stream(BoxMOTHipDeepOcSort* handle, int stream, int frame_count, int* id_count_inout,
                                        const float* dets, int det_rows, int det_cols, const float* embs, int emb_rows,
                                        int emb_cols, const uint8_t* image, int image_rows, int image_cols, int image_channels,
                                        float* out_tracks, int out_capacity_rows, int out_cols, int* out_rows, int* out_is_obb) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip DeepOCSORT handle is not initialized.");
        if (!out_rows || !out_is_obb) throw std::runtime_error("Output pointers are null.");
        if (out_cols != 9) throw std::runtime_error("boxmot_hip live tracking expects an output buffer with 9 columns.");
        if (embs != nullptr && emb_rows != det_rows) throw std::runtime_error("Detection and embedding row counts must match.");
        if (image_rows <= 0 || image_cols <= 0) throw std::runtime_error("Image dimensions must be positive.");
        StreamIn in{dets, det_rows, (embs && emb_cols > 0) ? embs : nullptr, image};
        float* outs[1] = {out_tracks};
        docs_need_frame_size(handle, image_rows, image_cols);
        docs_host_update(handle, 1, &in, det_cols, emb_cols, image_rows, image_cols, image_channels, outs, out_capacity_rows, out_rows,
                         stream, frame_count, id_count_inout);
        *out_is_obb = handle->is_obb ? 1 : 0;
    });
}

int boxmot_hip_deepocsort_step_device(BoxMOTHipDeepOcSort* handle, const float* d_dets, const int* d_det_rows,
                                       const float* d_embs, float* d_out, int* d_out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip DeepOCSORT handle is not initialized.");
        if (!d_dets || !d_det_rows || !d_out || !d_out_rows) throw std::runtime_error("boxmot_hip: null device pointers");
        if (!handle->cfg.embedding_off && !d_embs) throw std::runtime_error("boxmot_hip: step_device needs d_embs unless embedding_off");
        docs_need_frame_size(handle, 0, 0);
        bm::DocsStepArgs a = handle->args;
        a.dets = d_dets; a.n_dets = d_det_rows; a.embs = handle->cfg.embedding_off ? nullptr : d_embs;
        const bool any_warp = io_consume_warps(handle);         // boxmot_hip_deepocsort_set_warp since the last step
        a.warp = any_warp ? handle->d_warp : nullptr; a.warp_flag = any_warp ? handle->d_warp_flag : nullptr;
        a.out = d_out; a.out_n = d_out_rows; a.stream_base = 0;
        docs_launch(handle, handle->S, a);
        BM_HIP(hipGetLastError());
        io_clear_warps(handle);
    });
}

int boxmot_hip_deepocsort_step_device_frames(BoxMOTHipDeepOcSort* handle, const float* d_dets, const int* d_det_rows,
                                              const uint8_t* const* d_frames, int image_rows, int image_cols, float* d_out,
                                              int* d_out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip DeepOCSORT handle is not initialized.");
        if (!d_dets || !d_det_rows || !d_out || !d_out_rows) throw std::runtime_error("boxmot_hip: null device pointers");
        const float* embs = nullptr;
        if (!handle->cfg.embedding_off)      // deepocsort.py:337-345: every detection above det_thresh is embedded
            embs = io_device_reid(handle, d_dets, d_det_rows, d_frames, image_rows, image_cols, (double)(float)handle->cfg.det_thresh, 0);
        docs_need_frame_size(handle, image_rows, image_cols);
        bm::DocsStepArgs a = handle->args;
        a.dets = d_dets; a.n_dets = embs ? handle->step_ndets : d_det_rows; a.embs = embs;
        const bool any_warp = io_consume_warps(handle);
        a.warp = any_warp ? handle->d_warp : nullptr; a.warp_flag = any_warp ? handle->d_warp_flag : nullptr;
        a.out = d_out; a.out_n = d_out_rows; a.stream_base = 0;
        docs_launch(handle, handle->S, a);
        BM_HIP(hipGetLastError());
        if (embs) core_pipe_step_enqueued(handle);
        io_clear_warps(handle);
    });
}

int boxmot_hip_deepocsort_set_frame_sizes(BoxMOTHipDeepOcSort* handle, const int* image_rows, const int* image_cols, int n_streams) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip DeepOCSORT handle is not initialized.");
        // asso_func centroid normalises by the frame diagonal, ONE number per handle inside the step (docs_set_frame_size): it is
        // refused on a handle whose streams differ in size, not approximated
        if (handle->args.cfg.asso_mode == BOXMOT_HIP_ASSO_CENTROID && image_rows && image_cols && n_streams == handle->S)
            for (int s = 1; s < n_streams; ++s)
                if (image_rows[s] != image_rows[0] || image_cols[s] != image_cols[0])
                    throw std::runtime_error("boxmot_hip: asso_func centroid normalises by one frame diagonal per handle: streams of different "
                                             "frame sizes (stream " + std::to_string(s) + " differs from stream 0) need another asso_func or one handle per size");
        core_check_frame_sizes(handle, image_rows, image_cols, n_streams);
        core_commit_frame_sizes(handle, image_rows, image_cols);
        docs_need_frame_size(handle, image_rows[0], image_cols[0]);       // (one size: centroid takes it, if the config gave none)
    });
}

int boxmot_hip_deepocsort_set_reid_mode(BoxMOTHipDeepOcSort* handle, int mode) { return io_ep_set_reid_mode(handle, mode); }

int boxmot_hip_deepocsort_reid_kernel_ms(BoxMOTHipDeepOcSort* handle, double* out_ms, int* out_launches) { return ep_reid_kernel_ms(handle, out_ms, out_launches); }

void* boxmot_hip_deepocsort_stream(BoxMOTHipDeepOcSort* handle) { return ep_stream(handle); }

int boxmot_hip_deepocsort_synchronize(BoxMOTHipDeepOcSort* handle) { return io_ep_synchronize(handle, "DeepOCSORT"); }

int boxmot_hip_deepocsort_set_crop_bound(BoxMOTHipDeepOcSort* handle, int max_total_crops) {
    return io_ep_set_crop_bound(handle, "DeepOCSORT", max_total_crops);
}

int boxmot_hip_deepocsort_state_dump(BoxMOTHipDeepOcSort* handle, int stream, int* ints5, double* kf72, double* emb,
                                     int* out_rows, int* out_frame_count, int* out_id_count) {
    return guard_on(handle, [&]() {
        if (!handle || !out_rows) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        BM_HIP(hipStreamSynchronize(handle->stream));
        const bm::DocsState& st = handle->args.st;
        const size_t cap = handle->cap, dim = handle->dim, off = (size_t)stream * cap;
        int n = 0, fc = 0, ic = 0;
        BM_HIP(hipMemcpy(&n, st.n_tracks + stream, 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(&fc, st.frame_count + stream, 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(&ic, st.id_count + stream, 4, hipMemcpyDeviceToHost));
        std::vector<int> list(cap), id(cap), age(cap), tsu(cap), hs(cap), obs(cap);
        BM_HIP(hipMemcpy(list.data(), st.list + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(id.data(), st.id + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(age.data(), st.age + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(tsu.data(), st.tsu + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(hs.data(), st.hit_streak + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(obs.data(), st.observed + off, cap * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < n; ++r) {
            const int sl = list[r];
            if (ints5) { int* o = ints5 + r * 5; o[0] = id[sl]; o[1] = age[sl]; o[2] = tsu[sl]; o[3] = hs[sl]; o[4] = obs[sl]; }
            const size_t KS = bm::docs_kf_stride(handle->is_obb);      // 72 doubles per track, 90 (x[9] ++ P[9][9]) on an oriented handle
            if (kf72) BM_HIP(hipMemcpy(kf72 + (size_t)r * KS, st.kf + (off + sl) * KS, KS * 8, hipMemcpyDeviceToHost));
            if (emb) BM_HIP(hipMemcpy(emb + (size_t)r * dim, st.emb + (off + sl) * dim, dim * 8, hipMemcpyDeviceToHost));
        }
        *out_rows = n;
        if (out_frame_count) *out_frame_count = fc;
        if (out_id_count) *out_id_count = ic;
    });
}

// ---- StrongSORT ----
void boxmot_hip_strongsort_default_config(BoxMOTHipStrongSortConfig* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->max_age = 30; c->min_conf = 0.1; c->max_cos_dist = 0.2; c->max_iou_dist = 0.7; c->n_init = 3; c->nn_budget = 100;
    c->mc_lambda = 0.98; c->ema_alpha = 0.9; c->reid_model_path = nullptr;
    c->n_streams = 1; c->max_tracks = 1024; c->max_dets = 256; c->emb_dim = 512;
}

BoxMOTHipStrongSort* boxmot_hip_strongsort_create(const BoxMOTHipStrongSortConfig* config) {
    BoxMOTHipStrongSort* h = nullptr;
    const int ok = guard([&]() {
        if (config == nullptr) throw std::runtime_error("boxmot_hip StrongSORT config is required.");
        require_device();
        h = new BoxMOTHipStrongSort();
        h->cfg = *config;
        if (config->reid_model_path) h->reid_path = config->reid_model_path;
        h->cfg.reid_model_path = nullptr;
        ss_build(h);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}

void boxmot_hip_strongsort_destroy(BoxMOTHipStrongSort* handle) { destroy_on(handle); }

int boxmot_hip_strongsort_reset(BoxMOTHipStrongSort* handle) { return ep_reset(handle, "StrongSORT", ss_zero_state); }

int boxmot_hip_strongsort_reserve(BoxMOTHipStrongSort* handle, int max_tracks, int max_dets) {
    return ep_reserve(handle, "StrongSORT", max_tracks, max_dets, ss_grow);
}

int boxmot_hip_strongsort_capacity(BoxMOTHipStrongSort* handle, int* max_tracks, int* max_dets, int* n_grows) {
    return ep_capacity(handle, "StrongSORT", max_tracks, max_dets, n_grows);
}

int boxmot_hip_strongsort_set_warp(BoxMOTHipStrongSort* handle, int stream, const double* warp_2x3) {
    return ep_set_warp(handle, "StrongSORT", stream, warp_2x3);
}

int boxmot_hip_strongsort_update_batch(BoxMOTHipStrongSort* handle, int n_streams, const float* const* dets,
                                       const int* det_rows, const float* const* embs, int emb_cols,
                                       const uint8_t* const* images, int image_rows, int image_cols, int image_channels,
                                       float* const* out_tracks, int out_capacity_rows, int* out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip StrongSORT handle is not initialized.");
        if (n_streams < 1 || n_streams > handle->S) throw std::runtime_error("boxmot_hip: n_streams out of range");
        if (!dets || !det_rows || !out_tracks || !out_rows) throw std::runtime_error("boxmot_hip: null batch pointers");
        std::vector<StreamIn> in(n_streams);
        for (int s = 0; s < n_streams; ++s)
            in[s] = StreamIn{dets[s], det_rows[s], (embs && emb_cols > 0) ? embs[s] : nullptr, images ? images[s] : nullptr};
        ss_host_update(handle, n_streams, in.data(), 6, emb_cols, image_rows, image_cols, image_channels, out_tracks,
                       out_capacity_rows, out_rows);
    });
}

int boxmot_hip_strongsort_update(BoxMOTHipStrongSort* handle, const float* dets, int det_rows, int det_cols,
                                 const float* embs, int emb_rows, int emb_cols, const uint8_t* image, int image_rows,
                                 int image_cols, int image_channels, float* out_tracks, int out_capacity_rows,
                                 int out_cols, int* out_rows, int* out_is_obb) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip StrongSORT handle is not initialized.");
        if (!out_rows || !out_is_obb) throw std::runtime_error("Output pointers are null.");
        if (out_cols != 9) throw std::runtime_error("boxmot_hip live tracking expects an output buffer with 9 columns.");
        if (embs != nullptr && emb_rows != det_rows) throw std::runtime_error("Detection and embedding row counts must match.");
        if (image_rows <= 0 || image_cols <= 0) throw std::runtime_error("Image dimensions must be positive.");
        StreamIn in{dets, det_rows, (embs && emb_cols > 0) ? embs : nullptr, image};
        float* outs[1] = {out_tracks};
        ss_host_update(handle, 1, &in, det_cols, emb_cols, image_rows, image_cols, image_channels, outs, out_capacity_rows, out_rows);
        *out_is_obb = 0;
    });
}

int boxmot_hip_strongsort_step_device(BoxMOTHipStrongSort* handle, const float* d_dets, const int* d_det_rows,
                                       const float* d_embs, float* d_out, int* d_out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip StrongSORT handle is not initialized.");
        if (!d_dets || !d_det_rows || !d_embs || !d_out || !d_out_rows) throw std::runtime_error("boxmot_hip: null device pointers");
        bm::SsStepArgs a = handle->args;
        a.dets = d_dets; a.n_dets = d_det_rows; a.embs = d_embs;
        a.warp = io_consume_warps(handle) ? handle->d_warp : nullptr;       // boxmot_hip_strongsort_set_warp since the last step
        a.out = d_out; a.out_n = d_out_rows; a.stream_base = 0;
        ss_launch(handle, a, handle->S);
        BM_HIP(hipGetLastError());
        io_clear_warps(handle);
    });
}

int boxmot_hip_strongsort_step_device_frames(BoxMOTHipStrongSort* handle, const float* d_dets, const int* d_det_rows,
                                              const uint8_t* const* d_frames, int image_rows, int image_cols, float* d_out,
                                              int* d_out_rows) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip StrongSORT handle is not initialized.");
        if (!d_dets || !d_det_rows || !d_out || !d_out_rows) throw std::runtime_error("boxmot_hip: null device pointers");
        const float* embs = io_device_reid(handle, d_dets, d_det_rows, d_frames, image_rows, image_cols, handle->cfg.min_conf, 1);    // strongsort.py:74-91
        bm::SsStepArgs a = handle->args;
        a.dets = d_dets; a.n_dets = handle->step_ndets; a.embs = embs;
        a.warp = io_consume_warps(handle) ? handle->d_warp : nullptr;
        a.out = d_out; a.out_n = d_out_rows; a.stream_base = 0;
        ss_launch(handle, a, handle->S);
        BM_HIP(hipGetLastError());
        core_pipe_step_enqueued(handle);
        io_clear_warps(handle);
    });
}

int boxmot_hip_strongsort_set_frame_sizes(BoxMOTHipStrongSort* handle, const int* image_rows, const int* image_cols, int n_streams) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip StrongSORT handle is not initialized.");
        core_check_frame_sizes(handle, image_rows, image_cols, n_streams);
        core_commit_frame_sizes(handle, image_rows, image_cols);
    });
}

int boxmot_hip_strongsort_set_reid_mode(BoxMOTHipStrongSort* handle, int mode) { return io_ep_set_reid_mode(handle, mode); }

int boxmot_hip_strongsort_reid_kernel_ms(BoxMOTHipStrongSort* handle, double* out_ms, int* out_launches) { return ep_reid_kernel_ms(handle, out_ms, out_launches); }

int boxmot_hip_strongsort_track_count(BoxMOTHipStrongSort* handle, int stream, int* out_tracks) {
    return guard_on(handle, [&]() {
        if (!handle) throw std::runtime_error("boxmot_hip StrongSORT handle is null.");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        if (!out_tracks) throw std::runtime_error("Output pointers are null.");
        BM_HIP(hipStreamSynchronize(handle->stream));
        BM_HIP(hipMemcpy(out_tracks, handle->args.st.n_tracks + stream, 4, hipMemcpyDeviceToHost));
    });
}

void* boxmot_hip_strongsort_stream(BoxMOTHipStrongSort* handle) { return ep_stream(handle); }

int boxmot_hip_strongsort_synchronize(BoxMOTHipStrongSort* handle) { return io_ep_synchronize(handle, "StrongSORT"); }

int boxmot_hip_strongsort_set_crop_bound(BoxMOTHipStrongSort* handle, int max_total_crops) {
    return io_ep_set_crop_bound(handle, "StrongSORT", max_total_crops);
}

int boxmot_hip_deepocsort_debug_costs_enable(BoxMOTHipDeepOcSort* handle, int on) { return io_ep_debug_costs_enable(handle, on, docs_make_dbg); }

int boxmot_hip_deepocsort_debug_costs(BoxMOTHipDeepOcSort* handle, int stream, int plane, double* out, long out_capacity,
                                      int* out_rows, int* out_cols, int* out_branch) {
    return guard_on(handle, [&]() {
        if (!handle || !out_rows || !out_cols) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        if (plane < 0 || plane >= bm::DOCS_DBG_PLANES) throw std::runtime_error("boxmot_hip: debug_costs plane must be 0..2");
        if (!handle->args.dbg_cost)
            throw std::runtime_error("boxmot_hip: debug_costs needs boxmot_hip_deepocsort_debug_costs_enable(handle, 1) before the update");
        BM_HIP(hipStreamSynchronize(handle->stream));
        int shape[4] = {0, 0, 0, 0};
        BM_HIP(hipMemcpy(shape, handle->args.dbg_shape + (size_t)stream * 4, 16, hipMemcpyDeviceToHost));
        const int R = shape[0], C = shape[1];             // (detections, tracks): association.py's iou_matrix / final_cost orientation
        *out_rows = R; *out_cols = C;
        if (out_branch) *out_branch = shape[2];
        if (R == 0 || C == 0) return;
        if (!out || out_capacity < (long)R * C) throw std::runtime_error("boxmot_hip: debug_costs output capacity is smaller than rows x cols");
        const size_t cap = handle->dbg_cap, nd = handle->dbg_nd;
        std::vector<double> m(nd * cap);
        BM_HIP(hipMemcpy(m.data(), handle->args.dbg_cost + ((size_t)stream * bm::DOCS_DBG_PLANES + plane) * nd * cap, m.size() * 8, hipMemcpyDeviceToHost));
        for (int r = 0; r < R; ++r) std::memcpy(out + (size_t)r * C, m.data() + (size_t)r * cap, (size_t)C * 8);
    });
}

int boxmot_hip_strongsort_debug_costs_enable(BoxMOTHipStrongSort* handle, int on) { return io_ep_debug_costs_enable(handle, on, ss_make_dbg); }

int boxmot_hip_strongsort_debug_costs(BoxMOTHipStrongSort* handle, int stream, int stage, int plane, double* out, long out_capacity,
                                      int* out_rows, int* out_cols) {
    return guard_on(handle, [&]() {
        if (!handle || !out_rows || !out_cols) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        if (stage < 0 || stage > 1 || plane < 0 || plane > 1) throw std::runtime_error("boxmot_hip: debug_costs stage and plane must be 0 or 1");
        if (!handle->args.dbg_cost)
            throw std::runtime_error("boxmot_hip: debug_costs needs boxmot_hip_strongsort_debug_costs_enable(handle, 1) before the update");
        BM_HIP(hipStreamSynchronize(handle->stream));
        int shape[4] = {0, 0, 0, 0};
        BM_HIP(hipMemcpy(shape, handle->args.dbg_shape + (size_t)stream * 4, 16, hipMemcpyDeviceToHost));
        const int R = shape[stage * 2], C = shape[stage * 2 + 1];        // (tracks, detections)
        *out_rows = R; *out_cols = C;
        if (R == 0 || C == 0) return;
        if (!out || out_capacity < (long)R * C) throw std::runtime_error("boxmot_hip: debug_costs output capacity is smaller than rows x cols");
        const size_t big = handle->dbg_big;
        std::vector<double> m(big * big);
        BM_HIP(hipMemcpy(m.data(), handle->args.dbg_cost + ((size_t)stream * 4 + stage * 2 + plane) * big * big, m.size() * 8, hipMemcpyDeviceToHost));
        for (int r = 0; r < R; ++r) std::memcpy(out + (size_t)r * C, m.data() + (size_t)r * big, (size_t)C * 8);
    });
}

int boxmot_hip_strongsort_state_dump(BoxMOTHipStrongSort* handle, int stream, int* ints6, double* kf72, float* feat,
                                     int* out_rows, int* out_frame_count, int* out_next_id) {
    return guard_on(handle, [&]() {
        if (!handle || !out_rows) throw std::runtime_error("boxmot_hip: null argument");
        if (stream < 0 || stream >= handle->S) throw std::runtime_error("boxmot_hip: stream index out of range");
        BM_HIP(hipStreamSynchronize(handle->stream));
        const bm::SsState& st = handle->args.st;
        const size_t cap = handle->cap, dim = handle->dim, off = (size_t)stream * cap;
        int n = 0, fc = 0, ni = 0;
        BM_HIP(hipMemcpy(&n, st.n_tracks + stream, 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(&fc, st.frame_count + stream, 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(&ni, st.next_id + stream, 4, hipMemcpyDeviceToHost));
        std::vector<int> list(cap), id(cap), state(cap), hits(cap), age(cap), tsu(cap), bank(cap);
        BM_HIP(hipMemcpy(list.data(), st.list + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(id.data(), st.id + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(state.data(), st.state + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(hits.data(), st.hits + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(age.data(), st.age + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(tsu.data(), st.tsu + off, cap * 4, hipMemcpyDeviceToHost));
        BM_HIP(hipMemcpy(bank.data(), st.bank_n + off, cap * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < n; ++r) {
            const int sl = list[r];
            if (ints6) {
                int* o = ints6 + r * 6;
                o[0] = id[sl]; o[1] = state[sl]; o[2] = hits[sl]; o[3] = age[sl]; o[4] = tsu[sl];
                o[5] = bank[sl] < st.budget ? bank[sl] : st.budget;
            }
            if (kf72) BM_HIP(hipMemcpy(kf72 + (size_t)r * bm::KF_STRIDE, st.kf + (off + sl) * bm::KF_STRIDE, bm::KF_STRIDE * 8, hipMemcpyDeviceToHost));
            if (feat) BM_HIP(hipMemcpy(feat + (size_t)r * dim, st.feat + (off + sl) * dim, dim * 4, hipMemcpyDeviceToHost));
        }
        *out_rows = n;
        if (out_frame_count) *out_frame_count = fc;
        if (out_next_id) *out_next_id = ni;
    });
}


// ---------------------------------------------------------------------------------------------------------------------
// Reference-named exports (include/boxmot_compat.h): the exact symbol names, struct layouts and signatures of the
// reference's native FFI, so that its own ctypes bindings load this library unchanged:
//   boxmot_botsort_*    boxmot/native/cpp/trackers/botsort/include/botsort/c_api.hpp:17-61   (native/trackers/botsort.py:94-146)
//   boxmot_bytetrack_*  boxmot/native/cpp/trackers/bytetrack/include/bytetrack/c_api.hpp:16-46
//   boxmot_ocsort_*     boxmot/native/cpp/trackers/ocsort/include/ocsort/c_api.hpp:16-52
//   boxmot_reid_capi_*  boxmot/native/cpp/trackers/base/include/boxmot/trackers/base/reid_capi.h:36-94
// They are thin adapters over the boxmot_hip_* entry points above (float thresholds widened to double; the knobs the C++
// reference hard-codes -- second/unconfirmed thresholds 0.5 / 0.7, embedding scale 2.0, tracker.cpp:435,465,476 -- at
// those values; capacities from BOXMOT_HIP_MAX_TRACKS / BOXMOT_HIP_MAX_DETS, default 1024 / 512).
// ---------------------------------------------------------------------------------------------------------------------
// The embedding width is a create-time capacity of the device state; the reference learns it from the first embeddings it
// sees.  The adapter therefore builds the inner handle at create when the width is known (ReID weights given: their feature
// width; with_reid = 0: none needed) and otherwise at the first update that brings embeddings.
// The reference's native trackers take a table of 6 (AABB) or 7 (OBB) columns per call (live_c_api.hpp:22-60: `detection.is_obb =
// det_cols == 7`, out_is_obb = det_cols == 7, :147-149) and its Python wrappers fix the layout with the first table ("cannot switch
// between AABB and OBB inputs", native/trackers/botsort.py).  A device handle is sized for one layout, so the adapters keep the
// configuration, decide the layout with the first non-empty table and re-make the (still unused) inner handle when it is oriented.
struct CompatLayout : DeviceBound {          // the device current at create: a lazily built inner handle lands there too
    int layout = -1;                // -1 undecided, 0 axis-aligned, 1 oriented
    bool stepped = false;           // an update has run on the inner handle: its layout is final
    int empty_frames = 0;           // updates that only counted: before the inner handle exists (BoT-SORT without an embedding width yet,
                                    // botsort.py:183) or 0 x 0 tables before the layout is known; replayed into the frame counter
};
struct BoxMOTBotSortHandle : CompatLayout {
    BoxMOTHipBotSortConfig cfg{};
    std::string reid_path, reid_pre, cmc;
    BoxMOTHipBotSort* inner = nullptr;
    ~BoxMOTBotSortHandle() { delete inner; }
};
struct BoxMOTByteTrackHandle : CompatLayout { BoxMOTHipBotSortConfig cfg{}; BoxMOTHipBotSort* inner = nullptr; ~BoxMOTByteTrackHandle() { delete inner; } };
struct BoxMOTOCSORTHandle : CompatLayout { BoxMOTHipDeepOcSortConfig cfg{}; BoxMOTHipDeepOcSort* inner = nullptr; ~BoxMOTOCSORTHandle() { delete inner; } };

namespace {
int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    const int x = std::atoi(v);
    return x > 0 ? x : dflt;
}
// Layout of this call's table against the handle's: returns true when the inner handle has to be (re-)made with `is_obb`.
// ValidateLiveDetectionShape (live_c_api.hpp:22-33): an empty 0 x 0 table is accepted and keeps the layout.
bool compat_layout(CompatLayout* h, int det_rows, int det_cols, int& is_obb, const char* tracker) {
    is_obb = h->layout == 1 ? 1 : 0;
    if (det_rows < 0 || det_cols < 0) throw std::runtime_error("Negative matrix dimensions are not allowed.");
    if (det_cols == 0 && det_rows == 0) return false;
    if (det_cols != 6 && det_cols != 7)
        throw std::runtime_error(std::string(tracker) + " live tracking expects detections with 6 (AABB) or 7 (OBB) columns.");
    const int want = det_cols == 7 ? 1 : 0;
    if (h->layout == want) return false;
    if (h->layout >= 0 && h->stepped)
        throw std::runtime_error(std::string(tracker) + ": cannot switch between AABB and OBB inputs");
    h->layout = want;
    is_obb = want;
    return true;
}

void compat_build_inner(BoxMOTBotSortHandle* h, int emb_dim) {
    h->cfg.emb_dim = emb_dim;
    h->cfg.reid_model_path = h->reid_path.empty() ? nullptr : h->reid_path.c_str();
    h->cfg.reid_preprocess = h->reid_pre.empty() ? nullptr : h->reid_pre.c_str();
    h->cfg.cmc_method = h->cmc.empty() ? nullptr : h->cmc.c_str();
    BoxMOTHipBotSort* inner = boxmot_hip_botsort_create(&h->cfg);
    if (!inner) throw std::runtime_error(g_last_error);
    delete h->inner;
    h->inner = inner;
}
// feature width declared in the header of an OSN1 weight blob (reid_layout.hpp)
int blob_feature_dim(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open ReID weight blob: " + path);
    int32_t hdr[bm::REID_HEADER_INTS] = {0};
    const size_t got = std::fread(hdr, 4, bm::REID_HEADER_INTS, f);
    std::fclose(f);
    if (got == (size_t)bm::REID_HEADER_INTS && hdr[0] == bm::CLIP_MAGIC) return hdr[1] + hdr[7];       // CLIP-ReID: width + projection
    if (got != (size_t)bm::REID_HEADER_INTS || hdr[0] != bm::REID_MAGIC)
        throw std::runtime_error("ReID weights must be an OSN1 (OSNet) or CLP1 (CLIP-ReID) blob (boxmot_amd.reid_weights / clip_weights): " + path);
    return hdr[5];
}
}  // namespace

BoxMOTBotSortHandle* boxmot_botsort_create(const BoxMOTBotSortConfig* c) {
    BoxMOTBotSortHandle* h = nullptr;
    const int ok = guard([&]() {
        if (c == nullptr) throw std::runtime_error("BoTSORT config is required.");
        require_device();
        h = new BoxMOTBotSortHandle();
        BoxMOTHipBotSortConfig& k = h->cfg;
        boxmot_hip_botsort_default_config(&k);          // second 0.5, unconfirmed 0.7, scale 2.0, removed buffer 100
        k.track_high_thresh = (double)c->track_high_thresh; k.track_low_thresh = (double)c->track_low_thresh;
        k.new_track_thresh = (double)c->new_track_thresh; k.track_buffer = c->track_buffer;
        k.match_thresh = (double)c->match_thresh; k.proximity_thresh = (double)c->proximity_thresh;
        k.appearance_thresh = (double)c->appearance_thresh;
        k.frame_rate = c->frame_rate; k.fuse_first_associate = c->fuse_first_associate; k.with_reid = c->with_reid ? 1 : 0;
        k.max_obs = c->max_obs;
        if (c->cmc_method) h->cmc = c->cmc_method;
        if (!h->cmc.empty() && h->cmc != "none" && h->cmc != "ecc" && h->cmc != "sof")     // checked here: the inner handle may only be built at the first update
            throw std::runtime_error("boxmot_hip: camera-motion estimator '" + h->cmc + "' is not implemented (have: sof, ecc, none); "
                                     "supply the warp per frame with boxmot_hip_botsort_set_warp");
        if (c->reid_model_path) h->reid_path = c->reid_model_path;
        if (c->reid_preprocess) h->reid_pre = c->reid_preprocess;
        k.n_streams = 1; k.n_class_lists = 1; k.tracker_kind = 0;
        k.max_tracks = env_int("BOXMOT_HIP_MAX_TRACKS", 1024);
        k.max_dets = env_int("BOXMOT_HIP_MAX_DETS", 512);
        if (!k.with_reid) compat_build_inner(h, 1);
        else if (!h->reid_path.empty()) compat_build_inner(h, blob_feature_dim(h->reid_path));
        // else: embeddings will be supplied by the caller; their width is known at the first update
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}
void boxmot_botsort_destroy(BoxMOTBotSortHandle* h) { destroy_on(h); }
int boxmot_botsort_reset(BoxMOTBotSortHandle* h) {
    if (h) { h->empty_frames = 0; h->stepped = false; h->layout = -1; }          // the next table decides the layout again
    if (h && !h->inner) return guard([]() {});
    return boxmot_hip_botsort_reset(h ? h->inner : nullptr);
}
int boxmot_botsort_update(BoxMOTBotSortHandle* h, const float* dets, int det_rows, int det_cols, const float* embs,
                          int emb_rows, int emb_cols, const uint8_t* image, int image_rows, int image_cols,
                          int image_channels, float* out_tracks, int out_capacity_rows, int out_cols, int* out_rows,
                          int* out_is_obb) {
    if (!h) return boxmot_hip_botsort_update(nullptr, dets, det_rows, det_cols, embs, emb_rows, emb_cols, image, image_rows, image_cols,
                                             image_channels, out_tracks, out_capacity_rows, out_cols, out_rows, out_is_obb);
    const int ok = guard_on(h, [&]() {
        int is_obb = 0;
        if (compat_layout(h, det_rows, det_cols, is_obb, "BoTSORT") && is_obb != h->cfg.is_obb) {
            h->cfg.is_obb = is_obb;
            if (h->inner) compat_build_inner(h, h->cfg.emb_dim);           // not stepped yet: the tables of the other layout
        }
        if (!h->inner && embs != nullptr && emb_cols > 0) compat_build_inner(h, emb_cols);
        if (!h->inner && det_rows > 0)
            throw std::runtime_error("BoTSORT: with_reid is set, no ReID weights were given and no embeddings were supplied.");
    });
    if (!ok) return 0;
    if (det_rows == 0 && det_cols == 0) det_cols = h->layout == 1 ? 7 : 6;
    if (!h->inner || (h->layout < 0 && det_rows == 0)) {        // nothing to track yet (no width / no layout known): the frame only counts
        h->empty_frames += 1;
        if (out_rows) *out_rows = 0;
        if (out_is_obb) *out_is_obb = h->layout == 1 ? 1 : 0;
        return 1;
    }
    int rc;
    if (h->empty_frames > 0) {      // the frames that went by count (a first detection on frame > 1 is not activated at once)
        const int fc = h->empty_frames;
        h->empty_frames = 0;
        // the reference's estimator saw the empty frames (botsort.py:141-145 runs cmc.apply on every frame); there were no tracks to
        // warp, so all that matters is that it sees THIS frame as its newest: run it although the frame counter is preset
        h->inner->cmc_with_fc_set = true;
        rc = boxmot_hip_botsort_update_stream(h->inner, 0, 0, fc, dets, det_rows, det_cols, embs, emb_rows, emb_cols, image,
                                              image_rows, image_cols, image_channels, out_tracks, out_capacity_rows, out_cols,
                                              out_rows, out_is_obb);
        h->inner->cmc_with_fc_set = false;
    } else {
        rc = boxmot_hip_botsort_update(h->inner, dets, det_rows, det_cols, embs, emb_rows, emb_cols, image, image_rows, image_cols,
                                       image_channels, out_tracks, out_capacity_rows, out_cols, out_rows, out_is_obb);
    }
    if (rc) h->stepped = true;
    return rc;
}
#define BM_COMPAT_TIME(name, fn)                                                         \
    int name(BoxMOTBotSortHandle* h, double* out) {                                      \
        if (h && !h->inner) { if (out) *out = 0.0; return 1; }                           \
        return fn(h ? h->inner : nullptr, out);                                          \
    }
BM_COMPAT_TIME(boxmot_botsort_last_reid_time_ms, boxmot_hip_botsort_last_reid_time_ms)
BM_COMPAT_TIME(boxmot_botsort_last_reid_preprocess_time_ms, boxmot_hip_botsort_last_reid_preprocess_time_ms)
BM_COMPAT_TIME(boxmot_botsort_last_reid_process_time_ms, boxmot_hip_botsort_last_reid_process_time_ms)
BM_COMPAT_TIME(boxmot_botsort_last_reid_postprocess_time_ms, boxmot_hip_botsort_last_reid_postprocess_time_ms)
#undef BM_COMPAT_TIME
const char* boxmot_botsort_last_error() { return g_last_error.c_str(); }

BoxMOTByteTrackHandle* boxmot_bytetrack_create(const BoxMOTByteTrackConfig* c) {
    BoxMOTByteTrackHandle* h = nullptr;
    const int ok = guard([&]() {
        if (c == nullptr) throw std::runtime_error("ByteTrack config is required.");
        BoxMOTHipBotSortConfig k;
        boxmot_hip_bytetrack_default_config(&k);
        k.track_low_thresh = (double)c->min_conf; k.track_high_thresh = (double)c->track_thresh;
        k.new_track_thresh = (double)c->track_thresh;       // det_thresh = track_thresh, bytetrack.py:250
        k.match_thresh = (double)c->match_thresh; k.track_buffer = c->track_buffer; k.frame_rate = c->frame_rate;
        k.max_obs = c->max_obs;
        k.max_tracks = env_int("BOXMOT_HIP_MAX_TRACKS", 1024);
        k.max_dets = env_int("BOXMOT_HIP_MAX_DETS", 512);
        h = new BoxMOTByteTrackHandle();
        h->cfg = k;
        h->inner = boxmot_hip_botsort_create(&k);
        if (!h->inner) throw std::runtime_error(g_last_error);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}
void boxmot_bytetrack_destroy(BoxMOTByteTrackHandle* h) { destroy_on(h); }
int boxmot_bytetrack_reset(BoxMOTByteTrackHandle* h) {
    if (h) { h->empty_frames = 0; h->stepped = false; h->layout = -1; }
    return boxmot_hip_botsort_reset(h ? h->inner : nullptr);
}
int boxmot_bytetrack_update(BoxMOTByteTrackHandle* h, const float* dets, int det_rows, int det_cols, const uint8_t* image,
                            int image_rows, int image_cols, int image_channels, float* out_tracks, int out_capacity_rows,
                            int out_cols, int* out_rows, int* out_is_obb) {
    if (!h) return boxmot_hip_botsort_update(nullptr, dets, det_rows, det_cols, nullptr, 0, 0, image, image_rows, image_cols,
                                             image_channels, out_tracks, out_capacity_rows, out_cols, out_rows, out_is_obb);
    const int ok = guard_on(h, [&]() {
        int is_obb = 0;
        if (compat_layout(h, det_rows, det_cols, is_obb, "ByteTrack") && is_obb != h->cfg.is_obb) {
            h->cfg.is_obb = is_obb;
            BoxMOTHipBotSort* inner = boxmot_hip_botsort_create(&h->cfg);          // not stepped yet: the tables of the other layout
            if (!inner) throw std::runtime_error(g_last_error);
            delete h->inner;
            h->inner = inner;
        }
    });
    if (!ok) return 0;
    if (det_rows == 0 && det_cols == 0) det_cols = h->layout == 1 ? 7 : 6;
    if (h->layout < 0 && det_rows == 0) {          // a 0 x 0 table before the layout is known: the frame only counts
        h->empty_frames += 1;
        if (out_rows) *out_rows = 0;
        if (out_is_obb) *out_is_obb = 0;
        return 1;
    }
    const int fc = h->empty_frames > 0 ? h->empty_frames : -1;
    h->empty_frames = 0;
    const int rc = boxmot_hip_botsort_update_stream(h->inner, 0, 0, fc, dets, det_rows, det_cols, nullptr, 0, 0, image, image_rows,
                                                    image_cols, image_channels, out_tracks, out_capacity_rows, out_cols, out_rows, out_is_obb);
    if (rc) h->stepped = true;
    return rc;
}
const char* boxmot_bytetrack_last_error() { return g_last_error.c_str(); }

BoxMOTOCSORTHandle* boxmot_ocsort_create(const BoxMOTOCSORTConfig* c) {
    BoxMOTOCSORTHandle* h = nullptr;
    const int ok = guard([&]() {
        if (c == nullptr) throw std::runtime_error("OCSORT config is required.");
        BoxMOTHipDeepOcSortConfig k;
        boxmot_hip_deepocsort_default_config(&k);
        k.embedding_off = 1; k.cmc_off = 1; k.aw_off = 1;          // OC-SORT = this step without appearance / camera terms
        k.min_conf = (double)c->min_conf; k.det_thresh = (double)c->det_thresh; k.iou_threshold = (double)c->iou_threshold;
        k.max_age = c->max_age; k.min_hits = c->min_hits; k.delta_t = c->delta_t; k.use_byte = c->use_byte ? 1 : 0;
        k.inertia = (double)c->inertia; k.Q_xy_scaling = (double)c->q_xy_scaling; k.Q_s_scaling = (double)c->q_s_scaling;
        k.max_obs = c->max_obs;
        k.max_tracks = env_int("BOXMOT_HIP_MAX_TRACKS", 1024);
        k.max_dets = env_int("BOXMOT_HIP_MAX_DETS", 512);
        h = new BoxMOTOCSORTHandle();
        h->cfg = k;
        h->inner = boxmot_hip_deepocsort_create(&k);
        if (!h->inner) throw std::runtime_error(g_last_error);
    });
    if (!ok) { delete h; return nullptr; }
    return h;
}
void boxmot_ocsort_destroy(BoxMOTOCSORTHandle* h) { destroy_on(h); }
int boxmot_ocsort_reset(BoxMOTOCSORTHandle* h) {
    if (h) { h->empty_frames = 0; h->stepped = false; h->layout = -1; }
    return boxmot_hip_deepocsort_reset(h ? h->inner : nullptr);
}
int boxmot_ocsort_update(BoxMOTOCSORTHandle* h, const float* dets, int det_rows, int det_cols, const uint8_t* image,
                         int image_rows, int image_cols, int image_channels, float* out_tracks, int out_capacity_rows,
                         int out_cols, int* out_rows, int* out_is_obb) {
    if (!h) return boxmot_hip_deepocsort_update(nullptr, dets, det_rows, det_cols, nullptr, 0, 0, image, image_rows, image_cols,
                                                image_channels, out_tracks, out_capacity_rows, out_cols, out_rows, out_is_obb);
    const int ok = guard_on(h, [&]() {
        int is_obb = 0;
        if (compat_layout(h, det_rows, det_cols, is_obb, "OCSORT") && is_obb != h->cfg.is_obb) {
            h->cfg.is_obb = is_obb;
            BoxMOTHipDeepOcSort* inner = boxmot_hip_deepocsort_create(&h->cfg);    // not stepped yet: the tables of the other layout
            if (!inner) throw std::runtime_error(g_last_error);
            delete h->inner;
            h->inner = inner;
        }
    });
    if (!ok) return 0;
    if (det_rows == 0 && det_cols == 0) det_cols = h->layout == 1 ? 7 : 6;
    if (h->layout < 0 && det_rows == 0) {          // a 0 x 0 table before the layout is known: the frame only counts
        h->empty_frames += 1;
        if (out_rows) *out_rows = 0;
        if (out_is_obb) *out_is_obb = 0;
        return 1;
    }
    const int fc = h->empty_frames > 0 ? h->empty_frames : -1;
    h->empty_frames = 0;
    const int rc = boxmot_hip_deepocsort_update_stream(h->inner, 0, fc, nullptr, dets, det_rows, det_cols, nullptr, 0, 0, image, image_rows,
                                                       image_cols, image_channels, out_tracks, out_capacity_rows, out_cols, out_rows, out_is_obb);
    if (rc) h->stepped = true;
    return rc;
}
const char* boxmot_ocsort_last_error() { return g_last_error.c_str(); }

// ---- boxmot_reid_capi_* (reid_capi.h:36-94) ----
// model_path: an OSN1 weight blob (the reference takes an ONNX file; this library reads the folded OSNet weights written by
// boxmot_amd.reid_weights.save_blob).  preprocess NULL -> "resize_pad", the reference's default (reid_capi.h:33-34).
// BOXMOT_HIP_REID_MODE selects the kernel family (0 per-layer fp32 = default, 1 fused fp16 MFMA), BOXMOT_HIP_REID_MAX_CROPS
// the per-call capacity (default 1024).
int boxmot_reid_capi_create(const char* model_path, const char* preprocess, void** out_handle) {
    return guard([&]() {
        if (out_handle == nullptr) throw std::runtime_error("out_handle is null.");
        *out_handle = nullptr;
        if (model_path == nullptr || !*model_path) throw std::runtime_error("ReID model path is required.");
        BoxMOTHipReID* h = boxmot_hip_reid_create(model_path, nullptr, 0, env_int("BOXMOT_HIP_REID_MAX_CROPS", 1024));
        if (!h) throw std::runtime_error(g_last_error);
        const std::string err_keep;
        if (!boxmot_hip_reid_set_preprocess(h, preprocess ? preprocess : "resize_pad")) {
            const std::string e = g_last_error; delete h; throw std::runtime_error(e);
        }
        const char* m = std::getenv("BOXMOT_HIP_REID_MODE");
        if (m && *m && !boxmot_hip_reid_set_mode(h, std::atoi(m))) { const std::string e = g_last_error; delete h; throw std::runtime_error(e); }
        *out_handle = h;
    });
}
void boxmot_reid_capi_destroy(void* handle) { destroy_on(static_cast<BoxMOTHipReID*>(handle)); }
int boxmot_reid_capi_feature_dim(void* handle, int* out_feature_dim) {
    return guard([&]() {
        if (!handle) throw std::runtime_error("ReID handle is null.");
        if (!out_feature_dim) throw std::runtime_error("out_feature_dim is null.");
        *out_feature_dim = boxmot_hip_reid_feature_dim(static_cast<BoxMOTHipReID*>(handle));
    });
}
int boxmot_reid_capi_compute_features(void* handle, const float* boxes_xyxy, int n_boxes, const uint8_t* image_data,
                                      int image_rows, int image_cols, int image_channels, float* out_features,
                                      int out_capacity_floats) {
    BoxMOTHipReID* h = static_cast<BoxMOTHipReID*>(handle);
    const int ok = guard([&]() {
        if (!h) throw std::runtime_error("ReID handle is null.");
        if (n_boxes > 0 && (long)out_capacity_floats < (long)n_boxes * h->engine->feature_dim())
            throw std::runtime_error("Output feature buffer is too small.");
    });
    if (!ok) return 0;
    // the reference takes any number of boxes per call: walk them in chunks of the engine's capacity
    const int step = h->engine->max_crops(), dim = h->engine->feature_dim();
    int i0 = 0;
    do {
        const int m = n_boxes - i0 < step ? n_boxes - i0 : step;
        if (!boxmot_hip_reid_compute_features(h, image_data, image_rows, image_cols, image_channels, boxes_xyxy + (size_t)i0 * 4, m, 4,
                                              out_features + (size_t)i0 * dim, m)) return 0;
        i0 += m;
    } while (i0 < n_boxes);
    return 1;
}
// Staged calls: preprocess stages frame + boxes on the device and (per-layer path) writes the normalised crop blob into the
// engine; process runs the forward pass into the handle's feature buffer (the head kernel already L2-normalises -- the
// norm is idempotent); postprocess copies the rows out.  preprocess -> process -> postprocess == compute_features, bit for bit.
int boxmot_reid_capi_preprocess(void* handle, const float* boxes_xyxy, int n_boxes, const uint8_t* image_data, int image_rows,
                                int image_cols, int image_channels) {
    BoxMOTHipReID* h = static_cast<BoxMOTHipReID*>(handle);
    return guard_on(h, [&]() {
        if (!h) throw std::runtime_error("ReID handle is null.");
        h->staged_n = -1;
        reid_stage(h, image_data, image_rows, image_cols, image_channels, boxes_xyxy, n_boxes, 4);
        h->staged_n = n_boxes; h->staged_rows = image_rows; h->staged_cols = image_cols; h->staged_done = false;
    });
}
int boxmot_reid_capi_process(void* handle) {
    BoxMOTHipReID* h = static_cast<BoxMOTHipReID*>(handle);
    return guard_on(h, [&]() {
        if (!h) throw std::runtime_error("ReID handle is null.");
        if (h->staged_n < 0) throw std::runtime_error("boxmot_reid_capi_process called before boxmot_reid_capi_preprocess.");
        if (h->staged_n > 0) {
            h->engine->run(h->d_frames, h->d_crop_stream, h->d_boxes, 4, h->staged_n, h->staged_cols, h->staged_rows, h->d_feat,
                           nullptr, h->stream);
            BM_HIP(hipStreamSynchronize(h->stream));
        }
        h->staged_done = true;
    });
}
int boxmot_reid_capi_postprocess(void* handle, float* out_features, int out_capacity_floats) {
    BoxMOTHipReID* h = static_cast<BoxMOTHipReID*>(handle);
    return guard_on(h, [&]() {
        if (!h) throw std::runtime_error("ReID handle is null.");
        if (h->staged_n < 0 || !h->staged_done) throw std::runtime_error("boxmot_reid_capi_postprocess called before boxmot_reid_capi_process.");
        const long need = (long)h->staged_n * h->engine->feature_dim();
        if ((long)out_capacity_floats < need) throw std::runtime_error("Output feature buffer is too small.");
        if (need) BM_HIP(hipMemcpy(out_features, h->d_feat, (size_t)need * 4, hipMemcpyDeviceToHost));
        h->staged_n = -1; h->staged_done = false;
    });
}
const char* boxmot_reid_capi_last_error(void) { return g_last_error.c_str(); }

}  // extern "C"


