// Absolute poses and frame keypoints of the crops of full frames, in ONE launch (metro_place_poses, include/metro_hip.h).
// What the reference's test path does after the soft-argmax when the loader hands it each crop's virtual camera
// (src/data/data_loading.py:110-112 -> src/model/volumetric.py:171-216):
//   * 3D, scale recovery `bone-lengths` / `true-root-depth`: heatmap_to_image (volumetric.py:288-295), rays through the
//     virtual K^-1 (:221-222), delta_z, the per-pose z offset (bone_length_based_backproj.py:38-62, or the given root depth,
//     :192-199) and back_project (:284-285) -- backproject_kernel's arithmetic (heads.hip), from the same backproject.h;
//     then the export permutation (main.py:119-127) and, for `camera` / `world`, to_orig_cam (:277-281: R x, joints mirrored
//     when det R <= 0) plus cam_loc for `world` (:206-208).
//   * 3D, `metro`: the engine's root-relative poses, rotated as metro_to_orig_cam does (no translation: they carry none).
//   * 2D: the crop pixel heatmap_to_image(coords01.xy) of every output joint mapped to the frame the crop was cut from --
//     reference cameralib.reproject_image_points (src/cameralib.py:241-262) from the virtual camera to the original one:
//       HOMOGRAPHY  the crop -> frame matrix the warp samples through (crop pixel (x, y, 1) -> frame pixel, divided by w);
//       DISTORTED   ray = rot_to_orig_cam . K^-1 . (u, v, 1), then project_points' fp32 chain (cameralib.py:375-397).
//     A ray with z <= 0 in the original camera (w <= 0 after the homography) gives NaN: the reference projects it through the
//     origin onto a mirrored image point.
// Thread layout: one thread per crop, like backproject_kernel, so that both kernels run lmder1 from backproject.h as the same
// sequential fp64 code and agree bit for bit (tests/test_gpu_placement.py).  The cost of that choice: the per-crop arrays (rays,
// delta_z, c / d / e and lmder1's four fp64 vectors at J, E <= 64) are indexed dynamically and live in scratch --
// hipcc -Rpass-analysis=kernel-resource-usage reports 4624 bytes of scratch per lane, 84 VGPRs, 70 SGPRs, no spills, no LDS,
// no dynamic stack (backproject_kernel: the same 4624 bytes, 72 VGPRs) -- and every step of the serial solve walks them
// through that scratch.  This latency chain sets the launch time (748 us at 64 crops, 814 us at 256,
// profiles/frames_place_probe.json), not the crop count.  The untried alternative is a wave per crop with lanes over edges
// (E <= 64): the LM vectors would sit one element per lane in VGPRs and the norms and dot products would become wave-wide
// operations, removing the scratch chain.  To keep the bits, those reductions would have to add in lmder1's sequential order
// (e.g. lane 0 summing an LDS copy), not as a shuffle tree; backproject_kernel would move to the same form.
// No FMA contraction anywhere in this file (backproject.h).
#include "metro_common.h"
#include "backproject.h"

#pragma clang fp contract(off)

namespace metro {

struct PlaceArgs {
    const float* coords01;            // [n][nj][3]  soft-argmax output in [0,1], head order
    const float* poses;               // [n][n_out][3] the engine's root-relative poses (mode METRO_SCALE_METRO)
    const MetroPlacement* rec;        // [n]
    const double* targets;            // [ne] or [n][ne]  (bone-lengths)
    const float* root_z;              // [n]              (true-root-depth)
    const int* edges;                 // [ne][2] head joint indices
    const int* mirror;                // [n_out] output-order mirror joints
    float* out;                       // [n][n_out][3]
    float* keypoints;                 // [n][n_out][2] or null
    float* z_out;                     // [n] or null
    int n, nj, ne, n_out, per_pose_targets, scale, coords;
    float lrc, half_off, box;
    int perm[HEAD_MAX];
};

// project_points (cameralib.py:375-397), fp32; K[:2,:2] . p + K[:2,2]
__device__ inline void project_distorted(const MetroPlacement& r, const float* ray, float& x, float& y) {
    float px = ray[0] / ray[2], py = ray[1] / ray[2];
    distort_normalized(r.distortion, px, py);
    const float* K = r.intrinsics;              // K00 K01 K02 K10 K11 K12
    x = (K[0] * px + K[1] * py) + K[2];
    y = (K[3] * px + K[4] * py) + K[5];
}

__global__ __launch_bounds__(64) void place_poses_kernel(PlaceArgs a) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= a.n) return;
    const MetroPlacement& rec = a.rec[img];
    const float* c01 = a.coords01 + (size_t)img * a.nj * 3;
    float* o = a.out + (size_t)img * a.n_out * 3;
    const float* rot = a.coords == METRO_COORDS_CAMERA ? rec.rot_to_orig_cam : rec.rot_to_world;
    const bool flipped = a.coords != METRO_COORDS_CROP && mirrored(rot);
    if (a.scale == METRO_SCALE_METRO) {
        const float* p = a.poses + (size_t)img * a.n_out * 3;
        for (int r = 0; r < a.n_out; ++r) {
            if (a.coords == METRO_COORDS_CROP) {
                for (int t = 0; t < 3; ++t) o[r * 3 + t] = p[r * 3 + t];
            } else {
                rotate3(rot, p + (flipped ? a.mirror[r] : r) * 3, o + r * 3);
            }
        }
    } else {
        float cam[HEAD_MAX][3], dz[HEAD_MAX];
        rays_and_delta_z(c01, rec.inv_intrinsics, a.nj, a.lrc, a.half_off, a.box, cam, dz);
        const float z_off = a.scale == METRO_SCALE_TRUE_ROOT_DEPTH
                                ? a.root_z[img]
                                : z_offset_by_bones(cam, dz, a.edges, a.ne, a.targets + (a.per_pose_targets ? (size_t)img * a.ne : 0));
        if (a.z_out) a.z_out[img] = z_off;
        // back_project (volumetric.py:284-285) in output order; to_orig_cam reads the mirror joint's crop-frame position
        for (int r = 0; r < a.n_out; ++r) {
            const int j = a.perm[flipped ? a.mirror[r] : r];
            const float s = dz[j] + z_off;
            float x[3];
            for (int t = 0; t < 3; ++t) x[t] = cam[j][t] * s;
            if (a.coords == METRO_COORDS_CROP) {
                for (int t = 0; t < 3; ++t) o[r * 3 + t] = x[t];
            } else {
                float y[3];
                rotate3(rot, x, y);
                if (a.coords == METRO_COORDS_WORLD)
                    for (int t = 0; t < 3; ++t) y[t] = y[t] + rec.cam_loc[t];
                for (int t = 0; t < 3; ++t) o[r * 3 + t] = y[t];
            }
        }
    }
    if (a.keypoints == nullptr) return;
    float* kp = a.keypoints + (size_t)img * a.n_out * 2;
    const float nan = __builtin_nanf("");
    for (int r = 0; r < a.n_out; ++r) {
        float u, v, x, y;
        crop_pixel(c01 + a.perm[r] * 3, a.lrc, a.half_off, u, v);
        if (rec.keypoint_mode == METRO_WARP_DISTORTED) {
            float c[3], ray[3];
            ray_through(rec.inv_intrinsics, u, v, c);
            rotate3(rec.rot_to_orig_cam, c, ray);
            if (ray[2] > 0.f) project_distorted(rec, ray, x, y);
            else x = y = nan;                                  // behind the original camera (or NaN)
        } else {
            const float* H = rec.homography;
            const float hx = (H[0] * u + H[1] * v) + H[2];
            const float hy = (H[3] * u + H[4] * v) + H[5];
            const float hw = (H[6] * u + H[7] * v) + H[8];
            if (hw > 0.f) { x = hx / hw; y = hy / hw; }
            else x = y = nan;
        }
        kp[r * 2 + 0] = x;
        kp[r * 2 + 1] = y;
    }
}

int launch_place_poses(const float* coords01, const float* poses, const MetroPlacement* rec, int n, const MetroSpec& spec,
                       int scale, const double* targets, int per_pose_targets, const float* root_z, const int* edges, int ne,
                       const int* mirror, int coords, float* out, float* keypoints, float* z_out, hipStream_t stream) {
    if (note_kernel("place_poses")) return METRO_OK;
    PlaceArgs a;
    a.coords01 = coords01; a.poses = poses; a.rec = rec; a.targets = targets; a.root_z = root_z; a.edges = edges;
    a.mirror = mirror; a.out = out; a.keypoints = keypoints; a.z_out = z_out;
    a.n = n; a.nj = spec.n_joints_head; a.ne = ne; a.n_out = spec.n_joints_out; a.per_pose_targets = per_pose_targets;
    a.scale = scale; a.coords = coords;
    const HeadPixelScale px = head_pixel_scale(spec);
    a.lrc = (float)px.lrc; a.half_off = (float)px.half_off;
    a.box = spec.box_size_mm;
    head_permutation(spec, a.perm);
    hipLaunchKernelGGL(place_poses_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, a);
    return launch_status("place_poses");
}

}  // namespace metro
