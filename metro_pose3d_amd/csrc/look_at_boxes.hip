// The per-box crop geometry of full frames on the device (metro_look_at_boxes, include/metro_hip.h): one MetroViewBase per
// person box, the record frames.pack_view_bases writes on the host, so that boxes from a detector on the GPU never go back to
// the host and the per-box NumPy geometry (look_at_box, ~0.2 ms a box) leaves the call.
//   with a camera  frames.look_at_box step by step (the reference's cameralib.look_at_box, src/cameralib.py:337-358: turn
//                  towards the box centre, undistort, square the pixels, zoom, centre the principal point), each step in the
//                  dtype NumPy gives it on the host (the comments name them), then frames._frame_params_and_cameras' records;
//   without        preprocess.box_homography's axis-aligned square crop (a few fp64 operations and a cast: the host's bits).
// One thread per box, every matrix in scalar registers: all array indices are compile-time constants after unrolling, so no
// private array goes to scratch (cdna_hip_programming.md item 20; the code object's .private_segment_fixed_size is 0).
// The 3x3 inverses are closed forms (inv3, camera_math.h), not LAPACK's pivoted solves: the records agree with the host's to a
// few fp32 ulp, not bit for bit (tests/test_gpu_device_geometry.py measures it).  The matrix products take the order NumPy's
// BLAS (OpenBLAS' gemm kernels) takes on the host, a fused multiply-add chain a0 b0 -> +a1 b1 -> +a2 b2 (dot3_gemm, mm3_gemm),
// except the homography behind the LAPACK solve, which has no gemm order to follow (mm3_rounded), and the one-row fp32 product
// of the box centre (a gemv: every product rounded): camera_to_world adds the camera centre t (mm) to a ray of depth 1 in fp32
// and world_to_camera takes it off again, so one ulp of a world point is a visible share of the ray, and the zoom inherits it.
// No FMA contraction in this file: every fused multiply-add is written out.
#include "metro_common.h"
#include "camera_math.h"

#pragma clang fp contract(off)

namespace metro {

namespace {

struct Vec3f { float x, y, z; };

// Camera.image_to_world of one pixel (frames.py): undistort_points (float32 input, fp64 iteration, float32 result), depth 1,
// then camera_to_world = p @ inv(R).T + t in fp32: gemm order for the two side points (gemm = true), every product rounded,
// ((p0 a0 + p1 a1) + p2 a2), for the lone centre (a gemv); then + t
__host__ __device__ inline Vec3f image_to_world(const MetroFrameCamera& c, double u, double v, bool gemm) {
    const double px = (double)(float)u, py = (double)(float)v;
    const double fx = c.intrinsics[0], fy = c.intrinsics[4], cx = c.intrinsics[2], cy = c.intrinsics[5];
    const double ifx = 1. / fx, ify = 1. / fy;
    double x = (px - cx) * ifx;
    double y = (py - cy) * ify;
    if (c.has_distortion) {
        // k = zeros(14); k[:5] = d: the terms of k[5..11] are kept, they are zero times r2 (NaN for an infinite r2, as there)
        const double k0 = c.distortion[0], k1 = c.distortion[1], k2 = c.distortion[2], k3 = c.distortion[3],
                     k4 = c.distortion[4], z = 0.0;
        const double x0 = x, y0 = y;
        for (int it = 0; it < 5; ++it) {                                    // frames.UNDISTORT_ITERATIONS
            const double r2 = x * x + y * y;
            const double icdist = (1. + ((z * r2 + z) * r2 + z) * r2) / (1. + ((k4 * r2 + k1) * r2 + k0) * r2);
            const double dx = (((2. * k2) * x) * y + k3 * (r2 + (2. * x) * x)) + z * r2 + (z * r2) * r2;
            const double dy = (k2 * (r2 + (2. * y) * y) + ((2. * k3) * x) * y) + z * r2 + (z * r2) * r2;
            x = (x0 - dx) * icdist;
            y = (y0 - dy) * icdist;
        }
    }
    const float p0 = (float)x, p1 = (float)y, p2 = 1.f;
    const float* a = c.r_inv;
    if (gemm)
        return {dot3_gemm(p0, p1, p2, a[0], a[1], a[2]) + c.t[0], dot3_gemm(p0, p1, p2, a[3], a[4], a[5]) + c.t[1],
                dot3_gemm(p0, p1, p2, a[6], a[7], a[8]) + c.t[2]};
    return {((p0 * a[0] + p1 * a[1]) + p2 * a[2]) + c.t[0],
            ((p0 * a[3] + p1 * a[4]) + p2 * a[5]) + c.t[1],
            ((p0 * a[6] + p1 * a[7]) + p2 * a[8]) + c.t[2]};
}

// preprocess.box_homography: the axis-aligned square of side max(w, h) (Python's max: w unless h > w) centred on the box
__host__ __device__ inline void square_crop_record(const double* box, int side, MetroViewBase& o) {
    const double x = box[0], y = box[1], w = box[2], h = box[3];
    const double crop = h > w ? h : w;
    const double cx = x + w / 2, cy = y + h / 2;
    const double s = crop / side;
    const float hom[9] = {(float)s, 0.f, (float)(((cx - crop / 2) + 0.5 * s) - 0.5),
                          0.f, (float)s, (float)(((cy - crop / 2) + 0.5 * s) - 0.5),
                          0.f, 0.f, 1.f};
    o.mode = METRO_WARP_HOMOGRAPHY;
    o.has_camera = 0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const float eye = (e % 4 == 0) ? 1.f : 0.f;
        o.old_matrix[e] = o.orig_r[e] = o.virt_k[e] = o.virt_r[e] = o.partial[e] = 0.0;
        o.homography[e] = hom[e];
        o.inv_intrinsics[e] = 0.f;
        o.rot_to_orig_cam[e] = o.rot_to_world[e] = eye;
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) o.cam_loc[e] = 0.f;
#pragma unroll
    for (int e = 0; e < 6; ++e) o.intrinsics[e] = 0.f;
#pragma unroll
    for (int e = 0; e < 5; ++e) o.distortion[e] = 0.f;
}

// frames.look_at_box + _frame_params_and_cameras + pack_view_bases for one box on camera c
__host__ __device__ inline void camera_record(const double* box, const MetroFrameCamera& c, int side, MetroViewBase& o) {
    const double bx = box[0], by = box[1], bw = box[2], bh = box[3];
    // look_at_box: the centre and the two midpoints of the box's longer side (fp64; undistort_points rounds them to fp32)
    const double cx = bx + bw / 2, cy = by + bh / 2;
    const bool tall = bw < bh;
    const double s0x = tall ? cx : cx - bw / 2, s0y = tall ? cy - bh / 2 : cy;
    const double s1x = tall ? cx : cx + bw / 2, s1y = tall ? cy + bh / 2 : cy;
    const Vec3f w0 = image_to_world(c, s0x, s0y, true), w1 = image_to_world(c, s1x, s1y, true);
    // turn_towards: new_z = (target - t) / |.| in fp32; new_x = cross(new_z, world_up) in fp64 (an integer or fp64 up vector
    // promotes the cross product), normalised; new_y = cross(new_z, new_x); R = rows (x, y, z) cast to fp32
    const Vec3f tw = image_to_world(c, cx, cy, false);
    float zf0 = tw.x - c.t[0], zf1 = tw.y - c.t[1], zf2 = tw.z - c.t[2];
    // np.linalg.norm of fp32: sdot (fp32 products added in fp64, the sum rounded to fp32), then an fp32 sqrt
    const float nzf = sqrtf((float)(((double)(zf0 * zf0) + (double)(zf1 * zf1)) + (double)(zf2 * zf2)));
    zf0 = zf0 / nzf; zf1 = zf1 / nzf; zf2 = zf2 / nzf;
    const double z0 = zf0, z1 = zf1, z2 = zf2;
    const double u0 = c.world_up[0], u1 = c.world_up[1], u2 = c.world_up[2];
    double x0 = z1 * u2 - z2 * u1, x1 = z2 * u0 - z0 * u2, x2 = z0 * u1 - z1 * u0;
    const double nx = sqrt(dot3_gemm(x0, x1, x2, x0, x1, x2));
    x0 = x0 / nx; x1 = x1 / nx; x2 = x2 / nx;
    const double y0 = z1 * x2 - z2 * x1, y1 = z2 * x0 - z0 * x2, y2 = z0 * x1 - z1 * x0;
    const float r[9] = {(float)x0, (float)x1, (float)x2, (float)y0, (float)y1, (float)y2, zf0, zf1, zf2};
    // square_pixels: fmean = 0.5 (fx + fy) and fmean / fx in fp32 (NumPy scalars), the multiplier fp64: K becomes fp64
    const float* K = c.intrinsics;
    const float fmean = 0.5f * (K[0] + K[4]);
    const double m0 = (double)(fmean / K[0]), m1 = (double)(fmean / K[4]);
    double k[9] = {m0 * K[0], m0 * K[1], m0 * K[2], m1 * K[3], m1 * K[4], m1 * K[5], K[6], K[7], K[8]};
    // the side points through the new camera: world_to_camera in fp32, then the undistorted projection against the fp64 K
    double img[2];
    const Vec3f ws[2] = {w0, w1};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float d0 = ws[s].x - c.t[0], d1 = ws[s].y - c.t[1], d2 = ws[s].z - c.t[2];
        const float q0 = dot3_gemm(d0, d1, d2, r[0], r[1], r[2]);
        const float q1 = dot3_gemm(d0, d1, d2, r[3], r[4], r[5]);
        const float q2 = dot3_gemm(d0, d1, d2, r[6], r[7], r[8]);
        const double p0 = q0 / q2, p1 = q1 / q2;
        img[s] = tall ? fma(p1, k[4], p0 * k[3]) + k[5] : fma(p1, k[1], p0 * k[0]) + k[2];
    }
    // zoom so the side spans `side` pixels, then center_principal_point((side, side))
    const double crop_side = fabs(img[0] - img[1]);
    const double zoom = side / crop_side;
    k[0] *= zoom; k[1] *= zoom; k[3] *= zoom; k[4] *= zoom;
    k[2] = k[5] = side / 2.;

    double rd[9], inv_k[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) rd[e] = r[e];
    inv3(k, inv_k);
    float back[9];                                                      // orig.R @ virt.R.T in fp32
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            back[i * 3 + j] = dot3_gemm(c.r[i * 3 + 0], c.r[i * 3 + 1], c.r[i * 3 + 2], r[j * 3 + 0], r[j * 3 + 1], r[j * 3 + 2]);
    o.has_camera = 1;
    if (!c.has_distortion) {
        // reproject_image_fast: solve(new.T, old.T).T = old_matrix inv(K R), K R in fp64, cast to fp32
        double nm[9], inv_nm[9], h[9];
        mm3_gemm(k, rd, nm);
        inv3(nm, inv_nm);
        mm3_rounded(c.old_matrix, inv_nm, h);
        o.mode = METRO_WARP_HOMOGRAPHY;
#pragma unroll
        for (int e = 0; e < 9; ++e) { o.homography[e] = (float)h[e]; o.partial[e] = 0.0; }
#pragma unroll
        for (int e = 0; e < 6; ++e) o.intrinsics[e] = 0.f;
#pragma unroll
        for (int e = 0; e < 5; ++e) o.distortion[e] = 0.f;
    } else {
        // reproject_image case 2: partial = orig.R @ inv(virt.R) @ inv(virt.K): the first product fp32 (both factors fp32),
        // the second fp64
        double inv_r[9], pm[9], qd[9];
        float inv_rf[9], qf[9];
        inv3(rd, inv_r);
#pragma unroll
        for (int e = 0; e < 9; ++e) inv_rf[e] = (float)inv_r[e];
        mm3_gemm(c.r, inv_rf, qf);
#pragma unroll
        for (int e = 0; e < 9; ++e) qd[e] = qf[e];
        mm3_gemm(qd, inv_k, pm);
        o.mode = METRO_WARP_DISTORTED;
#pragma unroll
        for (int e = 0; e < 9; ++e) { o.partial[e] = pm[e]; o.homography[e] = 0.f; }
        o.intrinsics[0] = K[0]; o.intrinsics[1] = K[1]; o.intrinsics[2] = K[2];
        o.intrinsics[3] = K[3]; o.intrinsics[4] = K[4]; o.intrinsics[5] = K[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) o.distortion[e] = c.distortion[e];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = i * 3 + j;
            o.old_matrix[e] = c.old_matrix[e];
            o.orig_r[e] = c.r[e];
            o.virt_k[e] = k[e];
            o.virt_r[e] = rd[e];
            o.inv_intrinsics[e] = (float)inv_k[e];
            o.rot_to_orig_cam[e] = back[e];
            o.rot_to_world[e] = r[j * 3 + i];
        }
#pragma unroll
    for (int e = 0; e < 3; ++e) o.cam_loc[e] = c.t[e];
}

__global__ __launch_bounds__(64) void look_at_boxes_kernel(const double* __restrict__ boxes, const int32_t* __restrict__ frame_index,
                                                           int n, int n_frames, const MetroFrameCamera* __restrict__ cameras,
                                                           int n_cameras, int side, MetroViewBase* __restrict__ out,
                                                           int32_t* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int f = frame_index[i];
    if ((unsigned)f >= (unsigned)n_frames) {              // clamped, so that no table is read outside; the caller raises
        atomicAdd(status, 1);
        f = f < 0 ? 0 : n_frames - 1;
    }
    const double box[4] = {boxes[(size_t)i * 4 + 0], boxes[(size_t)i * 4 + 1], boxes[(size_t)i * 4 + 2], boxes[(size_t)i * 4 + 3]};
    MetroViewBase& o = out[i];
    o.frame = f;
    o.reserved = 0;
    if (!cameras)
        square_crop_record(box, side, o);
    else
        camera_record(box, cameras[n_cameras == 1 ? 0 : f], side, o);
}

}  // namespace

int launch_look_at_boxes(const double* boxes, const int32_t* frame_index, int n, int n_frames, const MetroFrameCamera* cameras,
                         int n_cameras, int side, MetroViewBase* out, int32_t* status, hipStream_t stream) {
    if (note_kernel("look_at_boxes")) return METRO_OK;
    METRO_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(look_at_boxes_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, boxes, frame_index, n, n_frames, cameras,
                       n_cameras, side, out, status);
    return launch_status("look_at_boxes");
}

}  // namespace metro
