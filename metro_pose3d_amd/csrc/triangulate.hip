// World positions of the joints of persons seen by several calibrated cameras, in ONE launch (metro_triangulate_joints,
// include/metro_hip.h).  Nothing in the reference to restate: its examples have one camera each.  The inputs are what the
// frames chain holds on the device after the forward: coords01 [m][J_head][3], the MetroPlacement record of every crop (the
// undistorted, square-pixel virtual camera: inv_intrinsics, rot_to_world, cam_loc -- no undistortion is needed) and, for the
// covariance weights, cov01 [m][J_head][6] of the MOMENTS forward.  The crop rows of person p are rows[starts[p] : starts[p+1]].
// Per (person, output joint r), every row i of the group gives one ray:
//   * the head joint is perm[mirrored ? mirror[r] : r] with mirrored = !(det rot_to_world > 0), metro_place_poses' rule: a
//     flipped test-time view reports the left joint where the right one is;
//   * (u, v) = heatmap_to_image(coords01) (crop_pixel), d = rot_to_world . (inv_intrinsics . (u, v, 1)) normalised, o = cam_loc;
//   * a ray with a non-finite component, or a row index outside [0, m), is skipped.
// The point nearest to the rays in the least-squares sense solves  (sum w (I - d d^T)) X = sum w (I - d d^T) o:
//   pass 1   w = 1;
//   pass 2   (METRO_TRI_COVARIANCE) w = 1 / (sigma^2 z^2) with z = d . (X0 - o) the ray's depth at the pass-1 point and
//            sigma^2 = (cov01_xx + cov01_yy) / 2 . lrc^2 . inv_intrinsics[0]^2 the isotropic variance of the ray in normalised
//            image units (floored at 1e-12 lrc^2 inv_intrinsics[0]^2: a one-hot heat-map gets a large finite weight): w is the
//            inverse variance of the ray's lateral position at the joint, in mm^-2.  z <= 0 or a non-finite w drops the ray.
// The 3x3 system is solved by its cofactors.  With A~ = A / sum w (eigenvalues in [0, 1]) a joint is undetermined when fewer
// than 2 rays remain or det A~ < min_det: two rays at angle t have det A~ = sin^2 t / 4, and rays from one optical centre
// have det A~ -> 0 however many they are.  Undetermined: point and residual NaN, n_rays the count of usable rays.
// residual = sqrt(sum w |(I - d d^T)(X - o)|^2 / sum w): the weighted RMS distance of the point from its rays, mm.
// metro_triangulate_joints_cov also writes the covariance of the point, mm^2, row-major symmetric 3x3, from the final solve's
// cofactors: METRO_TRI_COVARIANCE  Cov = A^-1 = cof(A~) / det A~ / sum w (w is an inverse variance in mm^-2);  METRO_TRI_UNIFORM
// Cov = s^2 A^-1 with s^2 = sum |p|^2 / (2 k - 3), |p| the distances the residual sums and k the rays (two constraints per ray,
// three unknowns); NaN where the joint is undetermined.  The plain kernel is compiled without the write.
// One thread per (person, output joint); rays are recomputed in each pass rather than stored (a group has no upper size).
// fp64 arithmetic on the fp32 inputs, no FMA contraction, one rounding to fp32 per output.
#include "metro_common.h"
#include "tri_ray.h"

#pragma clang fp contract(off)

namespace metro {

struct TriArgs {
    const float* coords01;            // [m][nj][3] head order
    const float* cov01;               // [m][nj][6] (METRO_TRI_COVARIANCE)
    const MetroPlacement* rec;        // [m]
    const int* rows;                  // [n_rows] indices into the m crop rows
    const int* starts;                // [n_persons + 1]
    const int* mirror;                // [n_out] output-order mirror joints
    float* points;                    // [n_persons][n_out][3]
    int* n_rays;                      // [n_persons][n_out]
    float* residual;                  // [n_persons][n_out]
    float* cov;                       // [n_persons][n_out][9] mm^2 (triangulate_joints_cov_kernel only)
    int m, n_rows, n_persons, nj, n_out, weights;
    double min_det;
    float lrc, half_off;
    int perm[METRO_MAX_JOINTS];
};

struct TriSystem { double a[6], b[3], sw; int cnt; };       // a: xx, yy, zz, xy, xz, yz of sum w (I - d d^T)

// pass-2 weight of a ray given the pass-1 point; < 0: the ray is dropped
__host__ __device__ inline double tri_weight(const TriRay& ray, const double* x0) {
    const double z = (ray.d[0] * (x0[0] - ray.o[0]) + ray.d[1] * (x0[1] - ray.o[1])) + ray.d[2] * (x0[2] - ray.o[2]);
    if (!(z > 0.0)) return -1.0;
    const double w = 1.0 / (ray.sigma2 * (z * z));
    return __builtin_isfinite(w) ? w : -1.0;
}

__host__ __device__ inline void tri_add(TriSystem& s, const TriRay& ray, double w) {
    const double* d = ray.d;
    const double* o = ray.o;
    const double m[6] = {1.0 - d[0] * d[0], 1.0 - d[1] * d[1], 1.0 - d[2] * d[2], -(d[0] * d[1]), -(d[0] * d[2]), -(d[1] * d[2])};
    for (int k = 0; k < 6; ++k) s.a[k] += w * m[k];
    s.b[0] += w * ((m[0] * o[0] + m[3] * o[1]) + m[4] * o[2]);
    s.b[1] += w * ((m[3] * o[0] + m[1] * o[1]) + m[5] * o[2]);
    s.b[2] += w * ((m[4] * o[0] + m[5] * o[1]) + m[2] * o[2]);
    s.sw += w;
    ++s.cnt;
}

// X = A~^-1 b~ by the cofactors of the symmetric A~ = A / sum w; false: undetermined.  inv (if given): A~^-1 as xx, yy, zz, xy,
// xz, yz
__host__ __device__ inline bool tri_solve(const TriSystem& s, double min_det, double* x, double* inv = nullptr) {
    if (s.cnt < 2) return false;
    const double xx = s.a[0] / s.sw, yy = s.a[1] / s.sw, zz = s.a[2] / s.sw, xy = s.a[3] / s.sw, xz = s.a[4] / s.sw, yz = s.a[5] / s.sw;
    const double b0 = s.b[0] / s.sw, b1 = s.b[1] / s.sw, b2 = s.b[2] / s.sw;
    const double c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
    const double det = (xx * c00 + xy * c01) + xz * c02;
    if (!(det >= min_det)) return false;
    const double c11 = xx * zz - xz * xz, c12 = xy * xz - xx * yz, c22 = xx * yy - xy * xy;
    x[0] = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
    x[1] = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
    x[2] = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
    if (inv) {
        inv[0] = c00 / det; inv[1] = c11 / det; inv[2] = c22 / det;
        inv[3] = c01 / det; inv[4] = c02 / det; inv[5] = c12 / det;
    }
    return true;
}

// one (person, output joint): what a thread of the kernel runs, and what tests/test_triangulation.py runs on the host
template <bool COV>
__host__ __device__ inline void triangulate_joint_t(const TriArgs& a, int idx) {
    const int person = idx / a.n_out, r = idx - person * a.n_out;
    int first = a.starts[person], last = a.starts[person + 1];
    if (first < 0) first = 0;
    if (last > a.n_rows) last = a.n_rows;
    const bool weighted = a.weights == METRO_TRI_COVARIANCE;
    TriRay ray;
    TriSystem sys = {{0, 0, 0, 0, 0, 0}, {0, 0, 0}, 0.0, 0};
    for (int k = first; k < last; ++k)
        if (tri_ray(a, a.rows[k], r, ray)) tri_add(sys, ray, 1.0);
    double x0[3] = {0, 0, 0}, x[3] = {0, 0, 0}, inv[6];
    bool ok = tri_solve(sys, a.min_det, x0, COV ? inv : nullptr);
    if (ok && weighted) {
        sys = {{0, 0, 0, 0, 0, 0}, {0, 0, 0}, 0.0, 0};
        for (int k = first; k < last; ++k) {
            if (!tri_ray(a, a.rows[k], r, ray)) continue;
            const double w = tri_weight(ray, x0);
            if (w > 0.0) tri_add(sys, ray, w);
        }
        ok = tri_solve(sys, a.min_det, x, COV ? inv : nullptr);
    } else {
        for (int t = 0; t < 3; ++t) x[t] = x0[t];
    }
    float* out = a.points + (size_t)idx * 3;
    a.n_rays[idx] = sys.cnt;
    if (!ok) {
        const float nan = __builtin_nanf("");
        out[0] = out[1] = out[2] = nan;
        a.residual[idx] = nan;
        if (COV)
            for (int t = 0; t < 9; ++t) a.cov[(size_t)idx * 9 + t] = nan;
        return;
    }
    double acc = 0.0;
    for (int k = first; k < last; ++k) {
        if (!tri_ray(a, a.rows[k], r, ray)) continue;
        const double w = weighted ? tri_weight(ray, x0) : 1.0;
        if (!(w > 0.0)) continue;
        const double v[3] = {x[0] - ray.o[0], x[1] - ray.o[1], x[2] - ray.o[2]};
        const double along = (ray.d[0] * v[0] + ray.d[1] * v[1]) + ray.d[2] * v[2];
        const double p[3] = {v[0] - ray.d[0] * along, v[1] - ray.d[1] * along, v[2] - ray.d[2] * along};
        acc += w * ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    }
    for (int t = 0; t < 3; ++t) out[t] = (float)x[t];
    a.residual[idx] = (float)sqrt(acc / sys.sw);
    if (COV) {
        // inv = (A / sum w)^-1, so A^-1 = inv / sum w; uniform weights: times the variance of a ray's distance from the point
        const double s2 = weighted ? 1.0 : acc / (double)(2 * sys.cnt - 3);
        float c6[6];
        for (int t = 0; t < 6; ++t) c6[t] = (float)(s2 * (inv[t] / sys.sw));
        float* c9 = a.cov + (size_t)idx * 9;
        c9[0] = c6[0]; c9[1] = c6[3]; c9[2] = c6[4];
        c9[3] = c6[3]; c9[4] = c6[1]; c9[5] = c6[5];
        c9[6] = c6[4]; c9[7] = c6[5]; c9[8] = c6[2];
    }
}

__host__ __device__ inline void triangulate_joint(const TriArgs& a, int idx) { triangulate_joint_t<false>(a, idx); }

__global__ __launch_bounds__(64) void triangulate_joints_kernel(TriArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < a.n_persons * a.n_out) triangulate_joint(a, idx);
}

__global__ __launch_bounds__(64) void triangulate_joints_cov_kernel(TriArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < a.n_persons * a.n_out) triangulate_joint_t<true>(a, idx);
}

// the launch's arguments from the entry's
inline TriArgs make_tri_args(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const int* rows,
                             int n_rows, const int* starts, int n_persons, const MetroSpec& spec, const int* mirror, int weights,
                             double min_det, float* points, int* n_rays, float* residual) {
    TriArgs a;
    a.coords01 = coords01; a.cov01 = cov01; a.rec = rec; a.rows = rows; a.starts = starts; a.mirror = mirror;
    a.points = points; a.n_rays = n_rays; a.residual = residual; a.cov = nullptr;
    a.m = m; a.n_rows = n_rows; a.n_persons = n_persons;
    a.weights = weights; a.min_det = min_det;
    tri_ray_fields(a, spec);
    return a;
}

int launch_triangulate_joints(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const int* rows,
                              int n_rows, const int* starts, int n_persons, const MetroSpec& spec, const int* mirror, int weights,
                              double min_det, float* points, int* n_rays, float* residual, float* cov, hipStream_t stream) {
    if (note_kernel("%s", cov ? "triangulate_joints_cov" : "triangulate_joints")) return METRO_OK;
    TriArgs a = make_tri_args(coords01, cov01, rec, m, rows, n_rows, starts, n_persons, spec, mirror, weights, min_det, points,
                                    n_rays, residual);
    const int total = n_persons * spec.n_joints_out;
    a.cov = cov;
    if (cov) {
        hipLaunchKernelGGL(triangulate_joints_cov_kernel, dim3((total + 63) / 64), dim3(64), 0, stream, a);
        return launch_status("triangulate_joints_cov");
    }
    hipLaunchKernelGGL(triangulate_joints_kernel, dim3((total + 63) / 64), dim3(64), 0, stream, a);
    return launch_status("triangulate_joints");
}

}  // namespace metro
