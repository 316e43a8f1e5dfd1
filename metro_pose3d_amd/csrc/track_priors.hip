// Heat-map priors from the track table, on the device (metro_plan_bind_track_prior, include/metro_hip.h, which is the
// specification).  Nothing in the reference to restate: it has no tracker.  Between a forward's finalize launch and its
// heat_posterior launch, every (crop row, output joint) turns the constant-velocity state of the row's track slot into the nine
// prior words heat_posterior.hip reads: the slot's joint is advanced to the row's time by smooth_predict (smooth_step.h, the
// function the association and the box prediction advance it with), taken into the crop's virtual camera with the row's
// MetroPlacement, projected to a crop pixel with the 2x3 Jacobian of that map, and brought to heat-map units by the inverse of
// heatmap_to_image; the 2x2 pixel covariance is inverted by cofactors into the xy precision.  z, which the model pins only
// relative to the root, is anchored at the root's coords01 z of the same forward (METRO_TRACK_PRIOR_DEPTH_ROOT), which is why the
// launch sits behind the finalize launch.
//   track_priors_kernel   one thread per (row, output joint), 64 per block: prior [n][Jout][9] and reason [n][Jout]
// The per-joint step is a __host__ __device__ function of one index, so tests/test_track_prior.py runs the same code on the host.
// Every matrix is in scalar registers and every loop has constant bounds: nothing is indexed dynamically but global memory (no
// scratch).  fp64 on the stored inputs, each output rounded to fp32 once.  No FMA contraction.
#include "metro_common.h"
#include "camera_math.h"
#include "smooth_step.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int TRACK_PRIOR_THREADS = 64;

// reason words
constexpr int TP_GIVEN = 0, TP_NO_SLOT = 1, TP_NO_STATE = 2, TP_TOO_OLD = 3, TP_NEAR = 4, TP_SINGULAR = 5, TP_NONFINITE = 6;

struct TrackPriorArgs {
    const double* state;          // [T][Jout][28], read only
    const int* slot;              // [n]
    const double* times;          // [n] s
    const MetroPlacement* rec;    // [n]
    const int* mirror;            // [Jout]
    const float* coords01;        // [n][J_head][3] of the same forward (DEPTH_ROOT), else not read
    float* prior;                 // [n][Jout][9]
    int* reason;                  // [n][Jout]
    int n, n_tracks, n_out, nj, coords, depth;
    int root_out;                 // the output joint of head joint J_head - 1, -1: the output order does not carry it
    double q, max_age, near, floor2, cov_scale;
    double lrc, half_off, box;    // heatmap_to_image's constants and box_size_mm
};

// The source joint `src` of slot s at time t in the crop's virtual camera: c [3] and C_c (xx, xy, xz, yy, yz, zz).
// Returns the reason word (TP_GIVEN: c and cc are set).
__host__ __device__ inline int track_prior_camera_point(const TrackPriorArgs& a, const MetroPlacement& rec, int s, int src, double t,
                                                        double* c, double* cc) {
    SmoothKf st, m;
    double t_last;
    if (src < 0 || src >= a.n_out) return TP_NO_STATE;           // a mirror table that points outside the skeleton
    if (!smooth_state_load(a.state + ((size_t)s * a.n_out + src) * SMOOTH_STATE_DOUBLES, st, t_last)) return TP_NO_STATE;
    if (!__builtin_isfinite(t)) return TP_NONFINITE;
    double dt = t - t_last;
    if (dt > a.max_age) return TP_TOO_OLD;
    if (!(dt > 0.0)) dt = 0.0;
    smooth_predict(st, dt, a.q, m);
    // C = cov_scale P_pos + sigma_floor^2 I
    double cw[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) cw[i][j] = a.cov_scale * SMOOTH_P(m.p, i, j) + (i == j ? a.floor2 : 0.0);
    // world: c = R^T (x - cam_loc), R = rot_to_world; camera: c = R^T x, R = rot_to_orig_cam.  C_c = R^T C R.
    const float* rf = a.coords == METRO_COORDS_WORLD ? rec.rot_to_world : rec.rot_to_orig_cam;
    double r[3][3], d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) r[i][j] = (double)rf[i * 3 + j];
        d[i] = a.coords == METRO_COORDS_WORLD ? m.x[i] - (double)rec.cam_loc[i] : m.x[i];
    }
    double cr[3][3];                                   // C R
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = (r[0][i] * d[0] + r[1][i] * d[1]) + r[2][i] * d[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) cr[i][j] = (cw[i][0] * r[0][j] + cw[i][1] * r[1][j]) + cw[i][2] * r[2][j];
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) cc[e++] = (r[0][i] * cr[0][j] + r[1][i] * cr[1][j]) + r[2][i] * cr[2][j];
    if (!(__builtin_isfinite(c[0]) && __builtin_isfinite(c[1]) && __builtin_isfinite(c[2]))) return TP_NONFINITE;
    if (!(c[2] >= a.near)) return TP_NEAR;
    return TP_GIVEN;
}

// item idx = i Jout + r
__host__ __device__ inline void track_prior_one(const TrackPriorArgs& a, int idx) {
    const int i = idx / a.n_out, r = idx - i * a.n_out;
    float* out = a.prior + (size_t)idx * 9;
    double w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = 0.0;
    int why = TP_GIVEN;
    const int s = a.slot[i];
    if (s < 0 || s >= a.n_tracks) why = TP_NO_SLOT;
    if (why == TP_GIVEN) {
        const MetroPlacement& rec = a.rec[i];
        const double t = a.times[i];
        const bool flipped = mirrored(a.coords == METRO_COORDS_WORLD ? rec.rot_to_world : rec.rot_to_orig_cam);
        const int src = flipped ? a.mirror[r] : r;
        double c[3], cc[6];
        why = track_prior_camera_point(a, rec, s, src, t, c, cc);
        if (why == TP_GIVEN) {
            // K = inv(inv_intrinsics); the pixel is its first two rows on (x / z, y / z, 1): a camera matrix ends in (0, 0, 1)
            double ki[9], k[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) ki[e] = (double)rec.inv_intrinsics[e];
            inv3(ki, k);
            const double nx = c[0] / c[2], ny = c[1] / c[2];
            const double u = (k[0] * nx + k[1] * ny) + k[2], v = (k[3] * nx + k[4] * ny) + k[5];
            // d(nx, ny) / dc = [1/z 0 -nx/z; 0 1/z -ny/z], times K's 2x2, times 1 / lrc
            const double iz = 1.0 / c[2];
            const double n0[3] = {iz, 0.0, -(nx * iz)}, n1[3] = {0.0, iz, -(ny * iz)};
            double j0[3], j1[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                j0[e] = (k[0] * n0[e] + k[1] * n1[e]) / a.lrc;
                j1[e] = (k[3] * n0[e] + k[4] * n1[e]) / a.lrc;
            }
            const double mx = (u - a.half_off) / a.lrc, my = (v - a.half_off) / a.lrc;
            // Sigma = J C_c J^T
            const double s3[3][3] = {{cc[0], cc[1], cc[2]}, {cc[1], cc[3], cc[4]}, {cc[2], cc[4], cc[5]}};
            double t0[3], t1[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                t0[e] = (s3[e][0] * j0[0] + s3[e][1] * j0[1]) + s3[e][2] * j0[2];
                t1[e] = (s3[e][0] * j1[0] + s3[e][1] * j1[1]) + s3[e][2] * j1[2];
            }
            const double sxx = (j0[0] * t0[0] + j0[1] * t0[1]) + j0[2] * t0[2];
            const double sxy = (j0[0] * t1[0] + j0[1] * t1[1]) + j0[2] * t1[2];
            const double syy = (j1[0] * t1[0] + j1[1] * t1[1]) + j1[2] * t1[2];
            const double det = sxx * syy - sxy * sxy;
            if (!(__builtin_isfinite(mx) && __builtin_isfinite(my))) {
                why = TP_NONFINITE;
            } else if (!(__builtin_isfinite(det) && det > 0.0)) {
                why = TP_SINGULAR;
            } else {
                w[0] = mx; w[1] = my;
                w[3] = syy / det; w[4] = sxx / det; w[6] = -sxy / det;
                if (a.depth == METRO_TRACK_PRIOR_DEPTH_ROOT && a.root_out >= 0 && r != a.root_out) {
                    double c0[3], cc0[6];
                    const int src0 = flipped ? a.mirror[a.root_out] : a.root_out;
                    // the root of the same slot at the same time; one that gives no point (its own reason word is not 0)
                    // leaves z without knowledge
                    if (track_prior_camera_point(a, rec, s, src0, t, c0, cc0) == TP_GIVEN) {
                        const double mz = (double)a.coords01[((size_t)i * a.nj + (a.nj - 1)) * 3 + 2] + (c[2] - c0[2]) / a.box;
                        const double lzz = (a.box * a.box) / (cc[5] + cc0[5]);
                        if (__builtin_isfinite(mz) && __builtin_isfinite(lzz) && lzz > 0.0) {
                            w[2] = mz; w[5] = lzz;
                        }
                    }
                }
            }
        }
    }
    if (why != TP_GIVEN) {
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = (float)w[k];
    a.reason[idx] = why;
}

__global__ __launch_bounds__(TRACK_PRIOR_THREADS) void track_priors_kernel(TrackPriorArgs a) {
    const int idx = blockIdx.x * TRACK_PRIOR_THREADS + threadIdx.x;
    if (idx < a.n * a.n_out) track_prior_one(a, idx);
}

// the output joint that is head joint J_head - 1 (the root the model's z is relative to), -1 if the output order has none
int track_prior_root_out(const MetroSpec& spec) {
    for (int r = 0; r < spec.n_joints_out && r < METRO_MAX_JOINTS; ++r)
        if (spec.permutation[r] == spec.n_joints_head - 1) return r;
    return -1;
}

TrackPriorArgs make_track_prior_args(const double* state, int capacity, const int* slot, const double* times, const MetroPlacement* rec,
                                     const int* mirror, const MetroTrackPrior& params, const float* coords01, int n,
                                     const MetroSpec& spec, float* prior_out, int* reason_out) {
    TrackPriorArgs a;
    a.state = state; a.slot = slot; a.times = times; a.rec = rec; a.mirror = mirror; a.coords01 = coords01;
    a.prior = prior_out; a.reason = reason_out;
    a.n = n; a.n_tracks = capacity; a.n_out = spec.n_joints_out; a.nj = spec.n_joints_head;
    a.coords = params.coords; a.depth = params.depth; a.root_out = track_prior_root_out(spec);
    a.q = params.accel_psd; a.max_age = params.max_age_s; a.near = params.near_mm;
    a.floor2 = params.sigma_floor_mm * params.sigma_floor_mm; a.cov_scale = params.cov_scale;
    const HeadPixelScale px = head_pixel_scale(spec);
    a.lrc = (double)px.lrc; a.half_off = (double)px.half_off; a.box = (double)spec.box_size_mm;
    return a;
}

int launch_track_priors(const double* state, int capacity, const int* slot, const double* times, const MetroPlacement* rec,
                        const int* mirror, const MetroTrackPrior& params, const float* coords01, int n, const MetroSpec& spec,
                        float* prior_out, int* reason_out, hipStream_t stream) {
    if (note_kernel("track_priors")) return METRO_OK;
    const TrackPriorArgs a = make_track_prior_args(state, capacity, slot, times, rec, mirror, params, coords01, n, spec, prior_out,
                                                   reason_out);
    const int items = a.n * a.n_out;
    hipLaunchKernelGGL(track_priors_kernel, dim3((items + TRACK_PRIOR_THREADS - 1) / TRACK_PRIOR_THREADS), dim3(TRACK_PRIOR_THREADS), 0,
                       stream, a);
    return launch_status("track_priors");
}

}  // namespace metro
