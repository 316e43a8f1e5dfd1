// Test-time augmentation of frame crops (metro_expand_views, metro_merge_views, include/metro_hip.h): several views per person
// box, as the reference's loader cuts them under --test-aug (src/data/data_loading.py:60-68, 77-79) and its head undoes them
// (to_orig_cam, src/model/volumetric.py:277-281, with rot_to_orig_cam = orig.R virt.R^T, data_loading.py:110).
//   expand  n per-box records -> n * V MetroCropWarp + MetroPlacement records on the device, one thread per (box, view), in
//           fp64: the view camera (zoom, roll, flip applied to the look_at_box camera) and frames._frame_params' formulas with
//           it, 3x3 inverses in closed form (inv3, camera_math.h).  The identity view copies the box's own records.
//   merge   the V placed views of each box -> one pose, keypoints, z offset and a per-joint spread, one thread per
//           (box, joint), fp64 sums in view order.
// Both are tiny next to the forward (a few hundred threads of scalar fp64); they exist so that the host packs one record per
// box, not one per view, and never waits on the device between the warp and the merge.
// No FMA contraction in this file: the expansion is compared with its host restatement (frames.view_params) to the ulp, and
// n copies of one view must merge to that view's bits.
#include "metro_common.h"
#include "camera_math.h"

#pragma clang fp contract(off)

namespace metro {

struct ViewTable { MetroView v[METRO_MAX_VIEWS]; };

__global__ __launch_bounds__(64) void expand_views_kernel(const MetroViewBase* __restrict__ bases, int n, ViewTable views,
                                                          int n_views, double half_side, MetroCropWarp* __restrict__ crops,
                                                          MetroPlacement* __restrict__ places) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_views) return;
    const int box = t / n_views;
    const MetroView& v = views.v[t - box * n_views];
    const MetroViewBase& b = bases[box];
    MetroCropWarp& c = crops[t];
    MetroPlacement& p = places[t];
    c.frame = b.frame;
    c.mode = b.mode;
    p.keypoint_mode = b.mode;
    p.reserved = 0;
    for (int k = 0; k < 6; ++k) c.intrinsics[k] = p.intrinsics[k] = b.intrinsics[k];
    for (int k = 0; k < 5; ++k) c.distortion[k] = p.distortion[k] = b.distortion[k];
    for (int k = 0; k < 3; ++k) p.cam_loc[k] = b.cam_loc[k];
    if (v.cos_roll == 1.0 && v.sin_roll == 0.0 && v.zoom == 1.0 && !v.flip) {      // the identity view: the box's own records
        for (int k = 0; k < 9; ++k) {
            c.partial[k] = b.partial[k];
            c.homography[k] = p.homography[k] = b.homography[k];
            p.inv_intrinsics[k] = b.inv_intrinsics[k];
            p.rot_to_orig_cam[k] = b.rot_to_orig_cam[k];
            p.rot_to_world[k] = b.rot_to_world[k];
        }
        return;
    }
    // the view camera: cam.zoom(zoom) (cameralib.py:167-170), cam.rotate(roll=r) (R <- euler2mat(0, 0, r, 'ryxz')^T R,
    // cameralib.py:95-98), cam.horizontal_flip() (R[0] *= -1, :191-192); without a camera the look_at_box camera is the square
    // crop itself: K = [[1, 0, side/2], [0, 1, side/2], [0, 0, 1]], R = I (roll, zoom and flip do not depend on the focal length)
    double k[9], r0[9], m[9], r[9], rt[9];
    if (b.has_camera) {
        for (int e = 0; e < 9; ++e) { k[e] = b.virt_k[e]; r0[e] = b.virt_r[e]; }
    } else {
        for (int e = 0; e < 9; ++e) { k[e] = 0.0; r0[e] = (e % 4 == 0) ? 1.0 : 0.0; }
        k[0] = k[4] = k[8] = 1.0;
        k[2] = k[5] = half_side;
    }
    const double base_k[9] = {k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8]};
    k[0] *= v.zoom; k[1] *= v.zoom; k[3] *= v.zoom; k[4] *= v.zoom;
    const double cr = v.cos_roll, sr = v.sin_roll;
    const double rz_t[9] = {cr, sr, 0.0, -sr, cr, 0.0, 0.0, 0.0, 1.0};
    mm3_rounded(rz_t, r0, m);
    for (int e = 0; e < 9; ++e) r[e] = (v.flip && e < 3) ? -m[e] : m[e];
    transpose3(r, rt);
    double new_matrix[9], inv_new[9], h[9];
    mm3_rounded(k, r, new_matrix);
    if (!b.has_camera || b.mode == METRO_WARP_HOMOGRAPHY) {
        // homography = old_matrix inv(K R)  (frames._frame_params; cameras=None: the square crop's matrix times K_base inv(K R))
        inv3(new_matrix, inv_new);
        if (b.has_camera) {
            mm3_rounded(b.old_matrix, inv_new, h);
        } else {
            double g[9], h0[9];
            mm3_rounded(base_k, inv_new, g);
            for (int e = 0; e < 9; ++e) h0[e] = (double)b.homography[e];
            mm3_rounded(h0, g, h);
        }
        for (int e = 0; e < 9; ++e) { c.homography[e] = p.homography[e] = (float)h[e]; c.partial[e] = 0.0; }
    } else {
        // partial_homography = orig.R inv(R) inv(K)  (reproject_image case 2, cameralib.py:294-306)
        double inv_r[9], inv_k[9], q[9], pm[9];
        inv3(r, inv_r);
        inv3(k, inv_k);
        mm3_rounded(b.orig_r, inv_r, q);
        mm3_rounded(q, inv_k, pm);
        for (int e = 0; e < 9; ++e) { c.partial[e] = pm[e]; c.homography[e] = p.homography[e] = 0.f; }
    }
    // the rotations back (data_loading.py:110-112): orig.R R^T (orig.R = I without a camera), R^T, inv(K) (0 without a camera)
    double back[9], inv_k[9];
    if (b.has_camera) mm3_rounded(b.orig_r, rt, back);
    else for (int e = 0; e < 9; ++e) back[e] = rt[e];
    if (b.has_camera) inv3(k, inv_k);
    for (int e = 0; e < 9; ++e) {
        p.rot_to_orig_cam[e] = (float)back[e];
        p.rot_to_world[e] = (float)rt[e];
        p.inv_intrinsics[e] = b.has_camera ? (float)inv_k[e] : 0.f;
    }
}

int launch_expand_views(const MetroViewBase* bases, int n, const MetroView* views, int n_views, int side, MetroCropWarp* crops,
                        MetroPlacement* places, hipStream_t stream) {
    if (note_kernel("expand_views")) return METRO_OK;
    ViewTable table = {};
    for (int v = 0; v < n_views; ++v) table.v[v] = views[v];
    const int total = n * n_views;
    hipLaunchKernelGGL(expand_views_kernel, dim3((total + 63) / 64), dim3(64), 0, stream, bases, n, table, n_views,
                       0.5 * (double)side, crops, places);
    return launch_status("expand_views");
}

struct MergeArgs {
    const float* poses;               // [n * V][nj][3]
    const float* keypoints;           // [n * V][nj][2] or null
    const float* z;                   // [n * V] or null
    const MetroPlacement* rec;        // [n * V]
    const int* mirror;                // [nj]
    float* poses_out;                 // [n][nj][3]
    float* keypoints_out;             // [n][nj][2]
    float* z_out;                     // [n]
    float* spread_out;                // [n][nj]
    int n, n_views, nj;
};

__global__ __launch_bounds__(256) void merge_views_kernel(MergeArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n * a.nj) return;
    const int box = t / a.nj, j = t - box * a.nj;
    const int V = a.n_views;
    const size_t row0 = (size_t)box * V;
    double s[3] = {0.0, 0.0, 0.0};
    for (int v = 0; v < V; ++v) {
        const float* p = a.poses + ((row0 + v) * a.nj + j) * 3;
        for (int e = 0; e < 3; ++e) s[e] += (double)p[e];
    }
    double mean[3];
    for (int e = 0; e < 3; ++e) {
        mean[e] = s[e] / (double)V;
        a.poses_out[(size_t)t * 3 + e] = (float)mean[e];
    }
    if (a.spread_out) {
        double q = 0.0;
        for (int v = 0; v < V; ++v) {
            const float* p = a.poses + ((row0 + v) * a.nj + j) * 3;
            const double d0 = (double)p[0] - mean[0], d1 = (double)p[1] - mean[1], d2 = (double)p[2] - mean[2];
            q += (d0 * d0 + d1 * d1) + d2 * d2;
        }
        a.spread_out[t] = (float)sqrt(q / (double)V);
    }
    if (a.keypoints) {
        // a mirrored view (det <= 0, as metro_place_poses decides it) saw joint j where it labels mirror[j]
        double sx = 0.0, sy = 0.0;
        int cnt = 0;
        for (int v = 0; v < V; ++v) {
            const bool flipped = mirrored(a.rec[row0 + v].rot_to_orig_cam);
            const float* kp = a.keypoints + ((row0 + v) * a.nj + (flipped ? a.mirror[j] : j)) * 2;
            const float x = kp[0], y = kp[1];
            if (__builtin_isfinite(x) && __builtin_isfinite(y)) {
                sx += (double)x;
                sy += (double)y;
                ++cnt;
            }
        }
        const float nan = __builtin_nanf("");
        a.keypoints_out[(size_t)t * 2 + 0] = cnt ? (float)(sx / (double)cnt) : nan;
        a.keypoints_out[(size_t)t * 2 + 1] = cnt ? (float)(sy / (double)cnt) : nan;
    }
    if (a.z && j == 0) {
        double sz = 0.0;
        for (int v = 0; v < V; ++v) sz += (double)a.z[row0 + v];
        a.z_out[box] = (float)(sz / (double)V);
    }
}

int launch_merge_views(const float* poses, const float* keypoints, const float* z, const MetroPlacement* rec, const int* mirror,
                       int n, int n_views, int nj, float* poses_out, float* keypoints_out, float* z_out, float* spread_out,
                       hipStream_t stream) {
    if (note_kernel("merge_views")) return METRO_OK;
    MergeArgs a;
    a.poses = poses; a.keypoints = keypoints; a.z = z; a.rec = rec; a.mirror = mirror;
    a.poses_out = poses_out; a.keypoints_out = keypoints_out; a.z_out = z_out; a.spread_out = spread_out;
    a.n = n; a.n_views = n_views; a.nj = nj;
    const int total = n * nj;
    hipLaunchKernelGGL(merge_views_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, a);
    return launch_status("merge_views");
}

}  // namespace metro
