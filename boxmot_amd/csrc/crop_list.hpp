// The ReID crop lists of the tracker handles, built on the device from the detection tables of a frame: which detections are
// embedded (conf > thresh, or >= with `inclusive`), in which stream and detection row they sit, and what the crop kernels need of
// them -- the xyxy box of an axis-aligned detection, the crop geometry (obb_crop_geometry.hpp) of an oriented one.
#pragma once

#include "botsort_types.hpp"
#include "obb_crop_geometry.hpp"

namespace bm {

constexpr int OBB_CROP_DET_COLS = 7;              // [cx, cy, w, h, angle, conf, cls] rows of an oriented handle (bm::obb::DET_COLS)
constexpr int OBB_CROP_CONF_COL = 5;

// Build the ReID crop list on the device: every detection with conf > track_high_thresh
// (botsort.py:191-192, :260).  One workgroup per stream; ranges reserved with one atomic.
__global__ void build_crop_list_kernel(const float* dets, const int* n_dets, int max_dets, double high,
                                       int* crop_count, int* crop_stream, float* crop_boxes, int* crop_row,
                                       int stream_base, int inclusive = 0) {
    __shared__ int s_base;
    __shared__ int s_cnt;
    const int s = stream_base + blockIdx.x;
    const int n = n_dets[s];
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const float* d = dets + (long)s * max_dets * DET_COLS;
    int mine = 0;
    auto pass = [&](int j) { const double cf = (double)d[j * DET_COLS + 4]; return inclusive ? cf >= high : cf > high; };
    for (int j = threadIdx.x; j < n; j += blockDim.x)
        if (pass(j)) ++mine;
    const int local = atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) s_base = atomicAdd(crop_count, s_cnt);
    __syncthreads();
    int k = s_base + local;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        if (pass(j)) {
            crop_stream[k] = s;
            crop_row[k] = s * max_dets + j;
            for (int q = 0; q < 4; ++q) crop_boxes[k * 4 + q] = d[j * DET_COLS + q];
            ++k;
        }
    }
}

// The ReID crop list of an oriented handle, built on the device: every detection with conf > high (>= when inclusive) of the
// 7-column rows, as build_crop_list_kernel above does for axis-aligned rows -- one workgroup per stream, ranges reserved
// with one atomic per stream, the same order of entries -- with the crop geometry [S * max_dets][8] in place of the boxes.
__global__ void build_crop_list_obb_kernel(const float* dets, const int* n_dets, int max_dets, double high, int* crop_count,
                                           int* crop_stream, int* crop_row, double* crop_geo, int stream_base, int inclusive) {
    __shared__ int s_base;
    __shared__ int s_cnt;
    const int s = stream_base + blockIdx.x;
    const int n = n_dets[s];
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const float* d = dets + (long)s * max_dets * OBB_CROP_DET_COLS;
    int mine = 0;
    auto pass = [&](int j) { const double cf = (double)d[j * OBB_CROP_DET_COLS + OBB_CROP_CONF_COL]; return inclusive ? cf >= high : cf > high; };
    for (int j = threadIdx.x; j < n; j += blockDim.x)
        if (pass(j)) ++mine;
    const int local = atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) s_base = atomicAdd(crop_count, s_cnt);
    __syncthreads();
    int k = s_base + local;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        if (pass(j)) {
            crop_stream[k] = s;
            crop_row[k] = s * max_dets + j;
            obb_crop_geometry(d + j * OBB_CROP_DET_COLS, crop_geo + (long)k * 8);
            ++k;
        }
    }
}

}  // namespace bm
