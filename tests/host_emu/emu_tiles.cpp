// TEST-ONLY harness: runs the two tiled-detection kernels on CPU threads, the device source unchanged --
//   k_letterbox_tiles (boxmot_amd/csrc/ingest_letterbox_tiles.hpp) with the grid the library launches (bm::letterbox_grid_x x
//   n_streams * n_tiles, LB_THREADS threads) and the geometry the library computes (bm::letterbox_tile_geometry).  It has no barrier
//   and no cross-lane operation: the emulated threads of a workgroup run one after the other, the workgroups on a few OS threads;
//   the tiled post-processing (boxmot_amd/csrc/det_post_tiled.hpp) through its kernel sequence detpost_launch_tiled.
//   k_detpost_select_tiled has workgroup barriers, ballots and LDS atomics, so its workgroups run on emu_detpost.cpp's launcher,
//   included as emu_detpost_obb.cpp includes it: the barrier-capable emulation of hip_shim.hpp (fibers; pthreads under the
//   sanitizers), the dynamic LDS poisoned before every workgroup.  The scratch is poisoned before every call.
#include "emu_detpost.cpp"

#define BM_GLOBAL
#include "../../boxmot_amd/csrc/ingest_letterbox_tiles.hpp"
#include "../../boxmot_amd/csrc/det_post_tiled.hpp"

namespace {
struct Job {
    const uint8_t* const* frames; const bm::LetterboxTileGeom* geom; const uint32_t* lut; void* out;
    int T, H, W, fp16, rgb, pad, gx, gy, first, step;
};
void* worker(void* p) {
    const Job* j = static_cast<const Job*>(p);
    for (int b = j->first; b < j->gx * j->gy; b += j->step) {
        blockIdx.x = b % j->gx; blockIdx.y = b / j->gx;
        for (int t = 0; t < bm::LB_THREADS; ++t) {
            threadIdx.x = t;
            bm::k_letterbox_tiles(j->frames, j->geom, j->lut, j->out, j->T, j->H, j->W, j->fp16, j->rgb, j->pad);
        }
    }
    return nullptr;
}
}  // namespace

// the library's geometry of one rectangle: out5 = gain, new_w, new_h, top, left; returns 1, 0 where the picture would vanish, -1
// where the rectangle is not inside the frame
extern "C" int emu_letterbox_tile_geometry(int rows, int cols, const int* rect, int H, int W, int mode, double* out5) {
    if (!bm::letterbox_tile_inside(rows, cols, rect[0], rect[1], rect[2], rect[3])) return -1;
    bm::LetterboxTileGeom g;
    const bool ok = bm::letterbox_tile_geometry(cols, rect[0], rect[1], rect[2], rect[3], H, W, mode, &out5[0], &g);
    out5[1] = g.g.new_w; out5[2] = g.g.new_h; out5[3] = g.g.top; out5[4] = g.g.left;
    return ok ? 1 : 0;
}

// n streams x T rectangles in one launch: per stream the (rows, cols, 3) BGR frame; rects: [n][T][4] x0 y0 w h; lut: the 256
// table entries as 32-bit words; out: (n * T, 3, H, W) elements of 2 (fp16) or 4 bytes.  Returns grid.x, or -1 - (s * T + t) where
// that rectangle is outside its frame or its picture would vanish (nothing is launched then).
extern "C" int emu_letterbox_tiles_run(int n, int T, const uint8_t* const* frames, const int* rows, const int* cols, const int* rects, int H, int W,
                                       int mode, int fp16, int rgb, int pad, const uint32_t* lut, void* out, int os_threads) {
    std::vector<bm::LetterboxTileGeom> g((size_t)n * T);
    for (int s = 0; s < n; ++s)
        for (int t = 0; t < T; ++t) {
            const int* r = rects + ((size_t)s * T + t) * 4;
            if (!bm::letterbox_tile_inside(rows[s], cols[s], r[0], r[1], r[2], r[3]) ||
                !bm::letterbox_tile_geometry(cols[s], r[0], r[1], r[2], r[3], H, W, mode, nullptr, &g[(size_t)s * T + t]))
                return -1 - (s * T + t);
        }
    const int gx = bm::letterbox_grid_x(H, W);
    blockDim.x = bm::LB_THREADS; gridDim.x = gx; gridDim.y = n * T;
    if (os_threads < 1) os_threads = 1;
    std::vector<Job> jobs(os_threads);
    std::vector<pthread_t> th(os_threads);
    for (int k = 0; k < os_threads; ++k) {
        jobs[k] = Job{frames, g.data(), lut, out, T, H, W, fp16, rgb, pad, gx, n * T, k, os_threads};
        pthread_create(&th[k], nullptr, worker, &jobs[k]);
    }
    for (int k = 0; k < os_threads; ++k) pthread_join(th[k], nullptr);
    return gx;
}

// pred: (S * T, 4 + nc, A) or (S * T, A, 5 + nc) of 2- (fp16) or 4-byte elements; geom: [S][T][7] float32 gain, top, left, x0, y0, w,
// h; allow: nc bytes or null; dets: [S][out_stride][6]; det_rows: [S]; counters: [S][3].  Returns the LDS bytes of the launch.
extern "C" long emu_detpost_tiled_run(int n_streams, int T, int A, int nc, int layout, int fp16, const void* pred, const float* geom, const uint8_t* allow,
                                      int K, int max_det, int agnostic, int merge, float conf_thres, float iou_thres, float* dets, int out_stride,
                                      int* det_rows, int* counters) {
    std::vector<uint32_t> keys((size_t)n_streams * T * A, 0xCDCDCDCDu);
    std::vector<int> cls((size_t)n_streams * T * A, (int)0xCDCDCDCD);
    bm::DetPostTiledArgs g{bm::DetPostArgs{pred, nullptr, allow, keys.data(), cls.data(), dets, det_rows, counters, A, nc, layout, K, max_det, agnostic,
                                           out_stride, conf_thres, iou_thres, 0, 0, 0},
                           reinterpret_cast<const bm::DetPostTileGeom*>(geom), T, merge};
    Launcher L;
    size_t lds = 0;
    bm::detpost_launch_tiled(L, g, n_streams, fp16, &lds);
    return (long)lds;
}
