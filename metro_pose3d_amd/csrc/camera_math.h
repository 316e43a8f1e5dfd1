// The 3x3 and camera arithmetic of the geometry kernels (crops from frames, placement, views, device boxes, triangulation,
// matching, box prediction), each piece written once.  Every function restates a NumPy expression of the reference or of the
// host code operation by operation, so its rounding sequence is part of what it is: a site uses a function here only where its
// own expression is literally these operations in this order and these types; a site that differs (another summation order, an
// fma where the host has one) keeps its own form and says why.
// FP contraction: every function states `#pragma clang fp contract(off)` as the first thing in its body, and the header has
// none at file scope.  A file-scope pragma in a header stays in force for the rest of every file that includes it, and
// warp_crops.hip and the files it shares headers with are compiled with contraction on.
#pragma once

#include "metro_common.h"

namespace metro {

// ---- 3x3 matrices, row-major ----------------------------------------------------------------------------------------------

// (x0 y0 + x1 y1) + x2 y2, every product rounded: np.sum over three fp64 products
__host__ __device__ inline double dot3_rounded(const double* x, const double* y) {
#pragma clang fp contract(off)
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// o = a b, every product rounded, each entry ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j): the order where the host's LAPACK solve
// leaves no gemm order to follow
__host__ __device__ inline void mm3_rounded(const double* a, const double* b, double* o) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = (a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j]) + a[i * 3 + 2] * b[2 * 3 + j];
}

// a0 b0 + a1 b1 + a2 b2 as the gemm kernels of the host's BLAS add it: fma(a2, b2, fma(a1, b1, a0 b0))
__host__ __device__ inline float dot3_gemm(float a0, float a1, float a2, float b0, float b1, float b2) {
#pragma clang fp contract(off)
    return fmaf(a2, b2, fmaf(a1, b1, a0 * b0));
}
__host__ __device__ inline double dot3_gemm(double a0, double a1, double a2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
    return fma(a2, b2, fma(a1, b1, a0 * b0));
}

// o = a b in the element type T, each entry a dot3_gemm
template <typename T>
__host__ __device__ inline void mm3_gemm(const T* a, const T* b, T* o) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = dot3_gemm(a[i * 3 + 0], a[i * 3 + 1], a[i * 3 + 2], b[j], b[3 + j], b[6 + j]);
}

__host__ __device__ inline void transpose3(const double* a, double* o) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = a[j * 3 + i];
}

// inverse in closed form: the adjugate (cofactors transposed) divided by the determinant.  Not LAPACK's pivoted solve: a result
// agrees with the host's to a few ulp, not bit for bit.
__host__ __device__ inline void inv3(const double* a, double* o) {
#pragma clang fp contract(off)
    const double c00 = a[4] * a[8] - a[5] * a[7];
    const double c01 = a[5] * a[6] - a[3] * a[8];
    const double c02 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    o[0] = c00 / det;
    o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = c01 / det;
    o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = c02 / det;
    o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// det of an fp32 3x3 evaluated in fp64: tf.linalg.det's sign is what to_orig_cam tests (volumetric.py:279-281)
__host__ __device__ inline double det3_f64(const float* r) {
#pragma clang fp contract(off)
    return (double)r[0] * ((double)r[4] * r[8] - (double)r[5] * r[7]) -
           (double)r[1] * ((double)r[3] * r[8] - (double)r[5] * r[6]) +
           (double)r[2] * ((double)r[3] * r[7] - (double)r[4] * r[6]);
}

// whether to_orig_cam reads the mirror joint under rotation `rot`: det R <= 0, and a NaN determinant counts as mirrored
__host__ __device__ inline bool mirrored(const float* rot) { return !(det3_f64(rot) > 0.0); }

// ---- pixels, rays and rotations of the head's back-projection ---------------------------------------------------------------
// The fp32 forms mirror NumPy on the fp32 tensors TF hands to the py_func.

// heatmap_to_image (volumetric.py:288-295): coords * last_receptive_center (+ stride // 2)
__host__ __device__ inline void crop_pixel(const float* c01j, float lrc, float half_off, float& u, float& v) {
#pragma clang fp contract(off)
    u = c01j[0] * lrc; v = c01j[1] * lrc;
    u = u + half_off; v = v + half_off;
}

// inv_intrinsics . [u, v, 1] (volumetric.py:221-222), evaluated ((k0 u + k1 v) + k2 1)
__host__ __device__ inline void ray_through(const float* k, float u, float v, float* cam) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) cam[i] = (k[i * 3 + 0] * u + k[i * 3 + 1] * v) + k[i * 3 + 2] * 1.0f;
}

// R . p, evaluated ((r0 p0 + r1 p1) + r2 p2) per row (matmul_joint_coords in to_orig_cam, volumetric.py:277-278)
__host__ __device__ inline void rotate3(const float* r, const float* p, float* o) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) o[i] = (r[i * 3 + 0] * p[0] + r[i * 3 + 1] * p[1]) + r[i * 3 + 2] * p[2];
}

// crop_pixel, ray_through and rotate3 on the same fp32 inputs with every product and sum in fp64, in the same order
// (triangulate.hip, whose reference is an fp64 restatement of the fp32 records)
__host__ __device__ inline void crop_pixel_f64(const float* c01j, float lrc, float half_off, double& u, double& v) {
#pragma clang fp contract(off)
    u = (double)c01j[0] * (double)lrc; v = (double)c01j[1] * (double)lrc;
    u = u + (double)half_off; v = v + (double)half_off;
}

__host__ __device__ inline void ray_through_f64(const float* k, double u, double v, double* cam) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) cam[i] = ((double)k[i * 3 + 0] * u + (double)k[i * 3 + 1] * v) + (double)k[i * 3 + 2] * 1.0;
}

__host__ __device__ inline void rotate3_f64(const float* r, const double* p, double* o) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) o[i] = ((double)r[i * 3 + 0] * p[0] + (double)r[i * 3 + 1] * p[1]) + (double)r[i * 3 + 2] * p[2];
}

// ---- lens distortion ------------------------------------------------------------------------------------------------------

// project_points (cameralib.py:375-397) from the normalised point (x / z, y / z) to the distorted one, in its statement order,
// fp32; d = k1 k2 p1 p2 k3.  The division by z in front, the rule for a point behind the camera and the application of K
// behind differ between the callers and stay with them.
__host__ __device__ inline void distort_normalized(const float* d, float& px, float& py) {
#pragma clang fp contract(off)
    const float r2 = px * px + py * py;
    const float r4 = r2 * r2;
    float dist = d[0] * r2;
    dist += d[1] * r4;
    const float r6 = r4 * r2;
    dist += d[4] * r6;
    dist += 1.f;
    dist += px * (2.f * d[3]);
    dist += py * (2.f * d[2]);
    px = px * dist;
    px = px + r2 * d[3];
    py = py * dist;
    py = py + r2 * d[2];
}

}  // namespace metro
