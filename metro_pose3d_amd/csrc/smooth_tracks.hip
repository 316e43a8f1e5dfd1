// Poses of tracked persons smoothed over time, in ONE launch (metro_smooth_tracks, include/metro_hip.h, which is the
// specification).  Nothing in the reference to restate: one example is one image.  Per (track, output joint) a
// constant-velocity Kalman filter runs over the track's rows in time order, the state x = (p, v) in mm and mm/s with the
// symmetric 6x6 covariance P, each row's pose the measurement of p with noise R (the row's heat-map covariance from
// metro_place_covariances, or isotropic); METRO_SMOOTH_RTS then runs the Rauch-Tung-Striebel backward pass over what the
// forward pass stored in the caller's workspace.  The rows of track t are rows[starts[t] : starts[t+1]] (CSR, built and
// time-sorted on the host, frames.track_groups).
//   predict   dt = t_k - t_prev (0 unless positive); x- = F x, P- = F P F^T + Q with F = [[I, dt I], [0, I]] and
//             Q = q [[dt^3/3 I, dt^2/2 I], [dt^2/2 I, dt I]]
//   measure   z missing (non-finite, or R non-finite / not positive definite) or gated (nu^T S^-1 nu > gate > 0): x = x-, P = P-
//   update    S = P-_pp + R (inverted by cofactors), K = P- H^T S^-1, x = x- + K nu, P = (I - KH) P- (I - KH)^T + K R K^T
//   start     without a carried state the first usable measurement gives x = (z, 0), P = diag(R, v0^2 I); rows before it
//             are NaN
//   smooth    C = P_k F^T (P-_{k+1})^-1 by an unpivoted LDL^T of P-_{k+1}; x^s_k = x_k + C (x^s_{k+1} - x-_{k+1}),
//             P^s_k = P_k + C (P^s_{k+1} - P-_{k+1}) C^T; a pivot that is not positive leaves the row at its filtered value
// P is kept as its 21 upper-triangle entries (row-major) and every loop over them has constant bounds and is unrolled, so
// the indices are compile-time constants and P lives in registers: the code object reports no scratch.
// One thread per (track, output joint); fp64 arithmetic on the fp32 inputs, no FMA contraction, one rounding to fp32 per output.
#include "metro_common.h"
#include "smooth_step.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int SMOOTH_WS_DOUBLES = 54;     // per (group row, joint): x 6, P 21, x- 6, P- 21

struct SmoothArgs {
    const float* poses;      // [n][J][3] mm
    const float* cov;        // [n][J][9] mm^2 (METRO_SMOOTH_COVARIANCE)
    const double* times;     // [n] s
    const int* rows;         // [n_rows] indices into the n pose rows, time-sorted within a group
    const int* starts;       // [n_tracks + 1]
    double* state;           // [n_tracks][J][28] or NULL
    double* ws;              // [54][n_rows][J] (METRO_SMOOTH_RTS)
    float* poses_out;        // [n][J][3]
    float* velocity_out;     // [n][J][3] or NULL
    float* cov_out;          // [n][J][9] or NULL
    unsigned char* used_out; // [n][J] or NULL
    int n, n_rows, n_tracks, n_out, mode, measurement;
    double q, r2, cov_scale, v02, gate;
};

// one RTS step: (xs, ps) = smoothed k+1 on entry, smoothed k on return.  f = filtered k, m = predicted k+1, dt = t_{k+1} - t_k.
// false: a pivot of P-_{k+1} was not positive, (xs, ps) = f
__host__ __device__ inline bool smooth_rts_step(const SmoothKf& f, const SmoothKf& m, double dt, SmoothKf& sm) {
    double l[6][6], d[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = SMOOTH_P(m.p, j, j);
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= (l[j][k] * l[j][k]) * d[k];
        ok = ok && dj > 0.0;
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = SMOOTH_P(m.p, i, j);
#pragma unroll
            for (int k = 0; k < j; ++k) v -= (l[i][k] * l[j][k]) * d[k];
            l[i][j] = v / dj;
        }
    }
    if (!ok) {
        sm = f;
        return false;
    }
    double dx[6], dp[21], c[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) dx[i] = sm.x[i] - m.x[i];
#pragma unroll
    for (int e = 0; e < 21; ++e) dp[e] = sm.p[e] - m.p[e];
    // row i of C solves P-_{k+1} c = (P_k F^T)(i, :)^T
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double y[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) y[j] = j < 3 ? SMOOTH_P(f.p, i, j) + dt * SMOOTH_P(f.p, i, 3 + (j % 3)) : SMOOTH_P(f.p, i, j);
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int k = 0; k < j; ++k) y[j] -= l[j][k] * y[k];
#pragma unroll
        for (int j = 0; j < 6; ++j) y[j] = y[j] / d[j];
#pragma unroll
        for (int j = 5; j >= 0; --j)
#pragma unroll
            for (int k = j + 1; k < 6; ++k) y[j] -= l[k][j] * y[k];
#pragma unroll
        for (int j = 0; j < 6; ++j) c[i][j] = y[j];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) acc += c[i][j] * dx[j];
        sm.x[i] = f.x[i] + acc;
    }
    double w[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc += c[i][k] * SMOOTH_P(dp, k, j);
            w[i][j] = acc;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc += w[i][k] * c[j][k];
            SMOOTH_P(sm.p, i, j) = SMOOTH_P(f.p, i, j) + acc;
        }
    return true;
}

__host__ __device__ inline void smooth_write(const SmoothArgs& a, size_t at, const SmoothKf& s) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        a.poses_out[at * 3 + t] = (float)s.x[t];
        if (a.velocity_out) a.velocity_out[at * 3 + t] = (float)s.x[3 + t];
    }
    if (a.cov_out) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) a.cov_out[at * 9 + i * 3 + j] = (float)SMOOTH_P(s.p, i, j);
    }
}

__host__ __device__ inline void smooth_write_nan(const SmoothArgs& a, size_t at) {
    const float nan = __builtin_nanf("");
    for (int t = 0; t < 3; ++t) {
        a.poses_out[at * 3 + t] = nan;
        if (a.velocity_out) a.velocity_out[at * 3 + t] = nan;
    }
    if (a.cov_out)
        for (int t = 0; t < 9; ++t) a.cov_out[at * 9 + t] = nan;
}

// workspace element e of (group row k, joint j): element-major, so the joints of a track, which are adjacent threads, are adjacent
__host__ __device__ inline size_t smooth_ws_at(const SmoothArgs& a, int e, int k, int j) {
    return ((size_t)e * a.n_rows + k) * a.n_out + j;
}
__host__ __device__ inline void smooth_ws_store(const SmoothArgs& a, int e0, int k, int j, const SmoothKf& s) {
#pragma unroll
    for (int e = 0; e < 6; ++e) a.ws[smooth_ws_at(a, e0 + e, k, j)] = s.x[e];
#pragma unroll
    for (int e = 0; e < 21; ++e) a.ws[smooth_ws_at(a, e0 + 6 + e, k, j)] = s.p[e];
}
__host__ __device__ inline void smooth_ws_load(const SmoothArgs& a, int e0, int k, int j, SmoothKf& s) {
#pragma unroll
    for (int e = 0; e < 6; ++e) s.x[e] = a.ws[smooth_ws_at(a, e0 + e, k, j)];
#pragma unroll
    for (int e = 0; e < 21; ++e) s.p[e] = a.ws[smooth_ws_at(a, e0 + 6 + e, k, j)];
}

// one (track, output joint): what a thread of the kernel runs, and what tests/test_track_smoothing.py runs on the host
__host__ __device__ inline void smooth_track_joint(const SmoothArgs& a, int idx) {
    const int track = idx / a.n_out, j = idx - track * a.n_out;
    int first = a.starts[track], last = a.starts[track + 1];
    if (first < 0) first = 0;
    if (last > a.n_rows) last = a.n_rows;
    const bool rts = a.mode == METRO_SMOOTH_RTS;
    SmoothKf s, m;
    double t_prev = 0.0;
    bool have = false;
    double* st = a.state ? a.state + (size_t)idx * SMOOTH_STATE_DOUBLES : nullptr;
    if (st) have = smooth_state_load(st, s, t_prev);
    int k_first = -1, k_last = -1;            // the first and the last group row with a filter state
    for (int k = first; k < last; ++k) {
        const int row = a.rows[k];
        if ((unsigned)row >= (unsigned)a.n) continue;
        const size_t at = (size_t)row * a.n_out + j;
        const double t = a.times[row];
        bool used;
        if (!smooth_filter_row(a, at, t, s, m, t_prev, have, used)) {
            smooth_write_nan(a, at);
            if (a.used_out) a.used_out[at] = 0;
            continue;
        }
        if (rts) {
            smooth_ws_store(a, 0, k, j, s);
            smooth_ws_store(a, 27, k, j, m);
        }
        smooth_write(a, at, s);
        if (a.used_out) a.used_out[at] = used ? 1 : 0;
        if (k_first < 0) k_first = k;
        k_last = k;
    }
    if (k_last < 0) return;
    if (st) smooth_state_store(st, s, t_prev);
    if (!rts) return;
    // backward: s holds the smoothed row k_next (the last row's smoothed value is its filtered one)
    int k_next = k_last;
    double t_next = t_prev;
    for (int k = k_last - 1; k >= k_first; --k) {
        const int row = a.rows[k];
        if ((unsigned)row >= (unsigned)a.n) continue;
        const double t = a.times[row];
        double dt = t_next - t;
        if (!(dt > 0.0)) dt = 0.0;
        SmoothKf f;
        smooth_ws_load(a, 0, k, j, f);
        smooth_ws_load(a, 27, k_next, j, m);
        if (smooth_rts_step(f, m, dt, s)) smooth_write(a, (size_t)row * a.n_out + j, s);
        k_next = k;
        t_next = t;
    }
}

__global__ __launch_bounds__(256) void smooth_tracks_kernel(SmoothArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < a.n_tracks * a.n_out) smooth_track_joint(a, idx);
}

inline SmoothArgs make_smooth_args(const float* poses, const float* cov, const double* times, int n, const int* rows, int n_rows,
                                   const int* starts, int n_tracks, int n_out, int mode, int measurement, double q, double r_floor,
                                   double cov_scale, double v0, double gate, double* state, double* ws, float* poses_out,
                                   float* velocity_out, float* cov_out, unsigned char* used_out) {
    SmoothArgs a;
    a.poses = poses; a.cov = cov; a.times = times; a.rows = rows; a.starts = starts; a.state = state; a.ws = ws;
    a.poses_out = poses_out; a.velocity_out = velocity_out; a.cov_out = cov_out; a.used_out = used_out;
    a.n = n; a.n_rows = n_rows; a.n_tracks = n_tracks; a.n_out = n_out; a.mode = mode; a.measurement = measurement;
    a.q = q; a.r2 = r_floor * r_floor; a.cov_scale = cov_scale; a.v02 = v0 * v0; a.gate = gate;
    return a;
}

size_t smooth_tracks_workspace_bytes(int n_rows, int n_out) {
    return (size_t)(n_rows > 0 ? n_rows : 0) * (size_t)(n_out > 0 ? n_out : 0) * SMOOTH_WS_DOUBLES * sizeof(double);
}

int launch_smooth_tracks(const float* poses, const float* cov, const double* times, int n, const int* rows, int n_rows,
                         const int* starts, int n_tracks, int n_out, int mode, int measurement, double q, double r_floor,
                         double cov_scale, double v0, double gate, double* state, void* workspace, float* poses_out,
                         float* velocity_out, float* cov_out, unsigned char* used_out, hipStream_t stream) {
    if (note_kernel("smooth_tracks")) return METRO_OK;
    const SmoothArgs a = make_smooth_args(poses, cov, times, n, rows, n_rows, starts, n_tracks, n_out, mode, measurement, q, r_floor,
                                          cov_scale, v0, gate, state, static_cast<double*>(workspace), poses_out, velocity_out,
                                          cov_out, used_out);
    const int total = n_tracks * n_out;
    hipLaunchKernelGGL(smooth_tracks_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, a);
    return launch_status("smooth_tracks");
}

}  // namespace metro
