// Alternative decode heads of the reference: the step AFTER the soft-argmax.
//   * backproject_kernel: `bone-lengths` / `bone-lengths-true` / `true-root-depth` scale recovery
//     (reference src/model/volumetric.py:171-199): image coordinates (heatmap_to_image :288-295), camera rays
//     (matmul_joint_coords with inv_intrinsics :221-222), delta_z, the per-pose z-offset solve
//     (src/model/bone_length_based_backproj.py:38-62) and back_project (:284-285), optional root-relative
//     (tfu3d.py:23-25) and export permutation (main.py:119-127).
//   * to_orig_cam_kernel: rotation to the original camera with joints mirrored when det(R) <= 0
//     (volumetric.py:277-281).
// The ray, delta_z and z-offset pieces (MINPACK lmder restated for one unknown) come from backproject.h, the determinant and
// the rotation from camera_math.h.  No FMA contraction anywhere in this file.
// One thread per pose (E, J <= 64): the work is a few hundred flops per pose, the point is parity, not speed.
#include "metro_common.h"
#include "gfx950_prims.h"
#include "backproject.h"

#pragma clang fp contract(off)

namespace metro {

struct BackprojectArgs {
    const float* coords01;      // [n][nj][3]  soft-argmax output in [0,1], head order, (x,y,z)
    const float* inv_k;         // [n][9]
    const double* targets;      // [ne] or [n][ne]   (mode 0)
    const float* root_z;        // [n]               (mode 1: true-root-depth)
    const int* edges;           // [ne][2] head joint indices
    float* out;                 // [n][n_out][3]
    float* z_out;               // [n] or null
    int n, nj, ne, per_pose_targets, mode;
    float lrc, half_off, box;
    int root_relative, n_out;
    int perm[HEAD_MAX];
};

__global__ __launch_bounds__(64) void backproject_kernel(BackprojectArgs a) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= a.n) return;
    const float* c01 = a.coords01 + (size_t)img * a.nj * 3;
    const float* k = a.inv_k + (size_t)img * 9;
    float cam[HEAD_MAX][3], dz[HEAD_MAX];
    rays_and_delta_z(c01, k, a.nj, a.lrc, a.half_off, a.box, cam, dz);
    const float z_off = a.mode == 1 ? a.root_z[img]
                                    : z_offset_by_bones(cam, dz, a.edges, a.ne, a.targets + (a.per_pose_targets ? (size_t)img * a.ne : 0));
    if (a.z_out) a.z_out[img] = z_off;
    // back_project (volumetric.py:284-285), then optional root_relative + export gather
    float root[3];
    for (int t = 0; t < 3; ++t) root[t] = a.root_relative ? cam[a.nj - 1][t] * (dz[a.nj - 1] + z_off) : 0.0f;
    float* o = a.out + (size_t)img * a.n_out * 3;
    for (int r = 0; r < a.n_out; ++r) {
        const int j = a.perm[r];
        const float s = dz[j] + z_off;
        for (int t = 0; t < 3; ++t) o[r * 3 + t] = cam[j][t] * s - root[t];
    }
}

__global__ __launch_bounds__(64) void to_orig_cam_kernel(const float* __restrict__ x, const float* __restrict__ rot,
                                                         const int* __restrict__ mirror, float* __restrict__ out,
                                                         int n, int nj) {
    const int img = blockIdx.x;
    const int j = threadIdx.x;
    if (img >= n || j >= nj) return;
    const float* r = rot + (size_t)img * 9;
    const int src = mirrored(r) ? mirror[j] : j;
    rotate3(r, x + ((size_t)img * nj + src) * 3, out + ((size_t)img * nj + j) * 3);
}

int launch_backproject(const float* coords01, const float* inv_k, const double* targets, int per_pose_targets,
                       const float* root_z, const int* edges, int n, int nj, int ne, const MetroSpec& spec,
                       int root_relative, int permute, float* out, float* z_out, hipStream_t stream) {
    BackprojectArgs a;
    a.coords01 = coords01; a.inv_k = inv_k; a.targets = targets; a.root_z = root_z; a.edges = edges;
    a.out = out; a.z_out = z_out;
    a.n = n; a.nj = nj; a.ne = ne; a.per_pose_targets = per_pose_targets; a.mode = root_z != nullptr ? 1 : 0;
    const HeadPixelScale px = head_pixel_scale(spec);
    a.lrc = (float)px.lrc; a.half_off = (float)px.half_off;
    a.box = spec.box_size_mm;
    a.root_relative = root_relative;
    a.n_out = permute ? spec.n_joints_out : nj;
    if (permute) head_permutation(spec, a.perm);
    else for (int i = 0; i < HEAD_MAX; ++i) a.perm[i] = i;          // head order out
    hipLaunchKernelGGL(backproject_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, a);
    return launch_status("backproject");
}

// heatmap_to_25d (volumetric.py:298-300): image-pixel x, y and z * box_size per head joint
__global__ __launch_bounds__(256) void heatmap_to_25d_kernel(const float* __restrict__ c01, float* __restrict__ out, int total,
                                                             float lrc, float half_off, float box) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // one (pose, joint)
    if (i >= total) return;
    float u = c01[i * 3 + 0] * lrc, v = c01[i * 3 + 1] * lrc;
    out[i * 3 + 0] = u + half_off;
    out[i * 3 + 1] = v + half_off;
    out[i * 3 + 2] = c01[i * 3 + 2] * box;
}

int launch_heatmap_to_25d(const float* coords01, float* out, int n, const MetroSpec& spec, hipStream_t stream) {
    const HeadPixelScale px = head_pixel_scale(spec);
    const int total = n * spec.n_joints_head;
    hipLaunchKernelGGL(heatmap_to_25d_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, coords01, out, total,
                       (float)px.lrc, (float)px.half_off, spec.box_size_mm);
    return launch_status("heatmap_to_25d");
}

int launch_to_orig_cam(const float* x, const float* rot, const int* mirror, float* out, int n, int nj, hipStream_t stream) {
    hipLaunchKernelGGL(to_orig_cam_kernel, dim3(n), dim3(64), 0, stream, x, rot, mirror, out, n, nj);
    return launch_status("to_orig_cam");
}

}  // namespace metro
