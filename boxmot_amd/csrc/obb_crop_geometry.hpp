// Crop geometry of oriented boxes -- BaseModelBackend._crop_obb (base_backend.py:91-117) -- as one function for the host and
// the device (the oriented crop-list kernel of crop_list.hpp makes the table of it that the crop kernels read).
//
// _crop_obb = cv2.getRotationMatrix2D about the box centre, shifted so that the centre lands on the middle of the
// (round(w), round(h)) output, then cv2.warpAffine, which inverts the 2x3 matrix in double precision before it samples.  The
// geometry of a box [cx, cy, w, h, angle] (float32 fields) is g[8] (double): out_w, out_h and the inverted map im0 .. im5 that
// obb_pixel (reid_kernels_v1.hpp) samples with.  The definition is the NumPy restatement the tests compare with (obb_crop_geometry in
// the test tree's crops module); the operation order and the float32 -> double conversions here are its own:
//   * angle * (180f / pi_f) in float32 (np.degrees on a float32 scalar), then * (pi / 180) in double;
//   * cos / sin in double (the host's libm on the host, the device's double-precision routines on the device: the two may differ
//     in the last place, everything else is the same sequence of IEEE operations);
//   * nearbyint rounds half to even; max(w, 1), max(h, 1) before rounding and max(.., 1) after;
//   * no fused multiply-add (the function switches contraction off itself).
//
// Non-finite boxes.  A box with a NaN or an infinity in cx, cy, w, h or angle has no geometry in the reference (the cast of a NaN to
// an integer size is undefined).  Here, host and device alike, it gets the geometry of a BLANK crop: out_w = out_h = 1 and the map
// [0, 0, OBB_BLANK_OFFSET, 0, 0, OBB_BLANK_OFFSET], which sends every crop pixel far outside any frame (warpAffine's border value 0).
// Under "resize" the crop tensor is that of an all-zero crop -- what the axis-aligned path makes of an empty box; under "resize_pad"
// the 1 x 1 zero crop is scaled to 128 x 128 and centred in the usual mean-colour border.  No non-finite value is ever cast to int.
#pragma once

#include <cmath>

namespace bm {

constexpr double OBB_BLANK_OFFSET = -1.0e6;       // pixels; saturates warpAffine's 16-bit source coordinates below zero

__host__ __device__ inline bool obb_field_finite(float v) { return v - v == 0.0f; }      // false for NaN and +-inf

__host__ __device__ inline void obb_crop_geometry(const float* bx, double* g) {
#pragma clang fp contract(off)
    if (!(obb_field_finite(bx[0]) && obb_field_finite(bx[1]) && obb_field_finite(bx[2]) && obb_field_finite(bx[3]) &&
          obb_field_finite(bx[4]))) {
        g[0] = 1.0; g[1] = 1.0;
        g[2] = 0.0; g[3] = 0.0; g[4] = OBB_BLANK_OFFSET;
        g[5] = 0.0; g[6] = 0.0; g[7] = OBB_BLANK_OFFSET;
        return;
    }
    const float rad2deg = 180.0f / 3.14159265358979323846f;         // np.degrees on a float32 scalar
    const double cx = bx[0], cy = bx[1];
    const double bw = bx[2] > 1.0f ? (double)bx[2] : 1.0, bh = bx[3] > 1.0f ? (double)bx[3] : 1.0;
    const int rw = (int)nearbyint(bw), rh = (int)nearbyint(bh);
    const int ow = rw > 1 ? rw : 1, oh = rh > 1 ? rh : 1;
    const double a = (double)(bx[4] * rad2deg) * (3.14159265358979323846 / 180.0);
    const double alpha = cos(a), beta = sin(a);
    double m00 = alpha, m01 = beta, m02 = (1 - alpha) * cx - beta * cy, m10 = -beta, m11 = alpha, m12 = beta * cx + (1 - alpha) * cy;
    m02 += ow / 2.0 - cx;
    m12 += oh / 2.0 - cy;
    double D = m00 * m11 - m01 * m10;
    D = D != 0 ? 1.0 / D : 0.0;
    const double A11 = m11 * D, A22 = m00 * D;
    g[0] = ow; g[1] = oh;
    g[2] = A11; g[3] = m01 * (-D); g[5] = m10 * (-D); g[6] = A22;
    g[4] = -g[2] * m02 - g[3] * m12;
    g[7] = -g[5] * m02 - g[6] * m12;
}

// geo[i] = obb_crop_geometry(boxes[i]) for n boxes of `box_stride` floats
__global__ void obb_geometry_kernel(const float* boxes, int box_stride, int n, double* geo) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) obb_crop_geometry(boxes + (long)i * box_stride, geo + (long)i * 8);
}

}  // namespace bm
