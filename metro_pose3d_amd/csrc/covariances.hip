// Per-joint heat-map covariances of crops in millimetres and in the requested coordinates, in ONE launch
// (metro_place_covariances, include/metro_hip.h).  The input is what the MOMENTS forward writes: cov01 [rows][J_head][6]
// (xx, yy, zz, xy, xz, yz of the joint's softmax distribution over its S x S x D volume, in linspace(0,1,.) units) and
// peak [rows][J_head] (its largest probability).  Per (box, output joint):
//   * gather head order -> output order through spec.permutation (main.py:119-127);
//   * scale with the linear part of heatmap_to_metric (volumetric.py:288-306): Cov_mm = diag(s) Cov01 diag(s),
//     s = (lrc box / proc_side, lrc box / proc_side, box); the additive half stride does not enter a covariance;
//   * `camera` / `world`: R Cov R^T with the crop record's rot_to_orig_cam / rot_to_world, and, as metro_to_orig_cam does for
//     the poses (volumetric.py:277-281), the MIRROR joint's covariance when det R <= 0;
//   * n_views rows per box (box-major, row i * n_views + v): the mean of the views' rotated covariances and of their peaks.
// This is the covariance of the joint's own heat-map in the crop's virtual-camera axes (then rotated): not the covariance of
// the root-relative difference the poses are, and it stays in MeTRo's metric scale whatever scale recovery placed the poses.
// One thread per (box, output joint); fp64 products of the fp32 inputs, one rounding to fp32 per output.
#include "metro_common.h"
#include "camera_math.h"

#pragma clang fp contract(off)

namespace metro {

struct CovArgs {
    const float* cov01;
    const float* peak;
    const MetroPlacement* rec;        // [n * n_views]; not read in METRO_COORDS_CROP
    const int* mirror;                // [n_out] output-order mirror joints; not read in METRO_COORDS_CROP
    float* cov_out;                   // [n][n_out][9] row-major symmetric 3x3, mm^2
    float* peak_out;                  // [n][n_out]
    int n, n_views, nj, n_out, coords;
    double sxy, sz;
    int perm[METRO_MAX_JOINTS];
};

__global__ __launch_bounds__(64) void place_covariances_kernel(CovArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n * a.n_out) return;
    const int box = idx / a.n_out, r = idx - box * a.n_out;
    const double s[3] = {a.sxy, a.sxy, a.sz};
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pk = 0.0;
    for (int v = 0; v < a.n_views; ++v) {
        const size_t row = (size_t)box * a.n_views + v;
        const float* rot = nullptr;
        bool flipped = false;
        if (a.coords != METRO_COORDS_CROP) {
            rot = a.coords == METRO_COORDS_CAMERA ? a.rec[row].rot_to_orig_cam : a.rec[row].rot_to_world;
            flipped = mirrored(rot);
        }
        const int j = a.perm[flipped ? a.mirror[r] : r];
        const float* c6 = a.cov01 + (row * a.nj + j) * 6;
        double c[3][3];
        c[0][0] = c6[0]; c[1][1] = c6[1]; c[2][2] = c6[2];
        c[0][1] = c[1][0] = c6[3]; c[0][2] = c[2][0] = c6[4]; c[1][2] = c[2][1] = c6[5];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) c[i][k] *= s[i] * s[k];
        if (rot != nullptr) {
            double t[3][3];            // R C, then (R C) R^T; written out: column by column through rotate3_f64 hipcc emits another kernel
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k)
                    t[i][k] = ((double)rot[i * 3 + 0] * c[0][k] + (double)rot[i * 3 + 1] * c[1][k]) + (double)rot[i * 3 + 2] * c[2][k];
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k)
                    c[i][k] = (t[i][0] * (double)rot[k * 3 + 0] + t[i][1] * (double)rot[k * 3 + 1]) + t[i][2] * (double)rot[k * 3 + 2];
        }
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) acc[i * 3 + k] += c[i][k];
        pk += (double)a.peak[row * a.nj + j];
    }
    float* o = a.cov_out + (size_t)idx * 9;
    for (int k = 0; k < 9; ++k) o[k] = (float)(acc[k] / a.n_views);
    a.peak_out[idx] = (float)(pk / a.n_views);
}

int launch_place_covariances(const float* cov01, const float* peak, const MetroPlacement* rec, int n, int n_views,
                             const MetroSpec& spec, const int* mirror, int coords, float* cov_out, float* peak_out,
                             hipStream_t stream) {
    if (note_kernel("place_covariances")) return METRO_OK;
    CovArgs a;
    a.cov01 = cov01; a.peak = peak; a.rec = rec; a.mirror = mirror; a.cov_out = cov_out; a.peak_out = peak_out;
    a.n = n; a.n_views = n_views; a.nj = spec.n_joints_head; a.n_out = spec.n_joints_out; a.coords = coords;
    a.sxy = (double)head_pixel_scale(spec).lrc * (double)spec.box_size_mm / (double)spec.proc_side;
    a.sz = (double)spec.box_size_mm;
    head_permutation(spec, a.perm);
    const int total = n * spec.n_joints_out;
    hipLaunchKernelGGL(place_covariances_kernel, dim3((total + 63) / 64), dim3(64), 0, stream, a);
    return launch_status("place_covariances");
}

}  // namespace metro
