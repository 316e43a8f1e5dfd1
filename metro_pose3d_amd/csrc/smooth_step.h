// The per-row step of the constant-velocity Kalman filter of one (track, output joint), shared by smooth_tracks.hip (the
// filter over a track's rows, then the RTS pass) and associate_tracks.hip (the working state that decides which box continues
// which track) so that both advance a state by the same operations in the same order: a state the association launch has
// advanced equals, bit for bit, what the smoothing launch writes for the same rows.  The model is metro_smooth_tracks'
// (include/metro_hip.h).  `Args` is the launch's argument struct; smooth_filter_row reads its fields poses [n][J][3],
// cov [n][J][9] (METRO_SMOOTH_COVARIANCE only), measurement, q, r2 = r_floor^2, cov_scale, v02 = v0^2 and gate.
// P is kept as its 21 upper-triangle entries (row-major) and every loop over them has constant bounds and is unrolled, so
// the indices are compile-time constants and P lives in registers.
#pragma once

#include "metro_common.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int SMOOTH_STATE_DOUBLES = 28;  // per (track, joint): x 6, P 21, t_last

// index of P(i, j) in the packed upper triangle
__host__ __device__ constexpr int smooth_tri(int i, int j) {
    return i <= j ? i * (13 - i) / 2 + (j - i) : j * (13 - j) / 2 + (i - j);
}
#define SMOOTH_P(p, i, j) (p)[smooth_tri((i), (j))]

struct SmoothKf { double x[6], p[21]; };

__host__ __device__ inline void smooth_predict(const SmoothKf& s, double dt, double q, SmoothKf& m) {
    const double dt2 = dt * dt, qa = q * (dt2 * dt / 3.0), qb = q * (dt2 / 2.0), qd = q * dt;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        m.x[a] = s.x[a] + dt * s.x[3 + a];
        m.x[3 + a] = s.x[3 + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double pv = SMOOTH_P(s.p, a, 3 + b), vv = SMOOTH_P(s.p, 3 + a, 3 + b);
            if (a <= b) {
                SMOOTH_P(m.p, a, b) = ((SMOOTH_P(s.p, a, b) + dt * (pv + SMOOTH_P(s.p, b, 3 + a))) + dt2 * vv) + (a == b ? qa : 0.0);
                SMOOTH_P(m.p, 3 + a, 3 + b) = vv + (a == b ? qd : 0.0);
            }
            SMOOTH_P(m.p, a, 3 + b) = (pv + dt * vv) + (a == b ? qb : 0.0);
        }
    }
}

// r: xx, xy, xz, yy, yz, zz.  Positive definite by its leading minors, all entries finite.
__host__ __device__ inline bool smooth_pd3(const double* r) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) fin = fin && __builtin_isfinite(r[k]);
    const double m2 = r[0] * r[3] - r[1] * r[1];
    const double det = (r[0] * (r[3] * r[5] - r[4] * r[4]) - r[1] * (r[1] * r[5] - r[4] * r[2])) + r[2] * (r[1] * r[4] - r[3] * r[2]);
    return fin && r[0] > 0.0 && m2 > 0.0 && det > 0.0;
}

// the measurement update of (m = x-, P-) with z and R (sym6) into s; false: gated, s untouched
__host__ __device__ inline bool smooth_update(const SmoothKf& m, const double* z, const double* r, double gate, SmoothKf& s) {
    const double sxx = m.p[smooth_tri(0, 0)] + r[0], sxy = m.p[smooth_tri(0, 1)] + r[1], sxz = m.p[smooth_tri(0, 2)] + r[2];
    const double syy = m.p[smooth_tri(1, 1)] + r[3], syz = m.p[smooth_tri(1, 2)] + r[4], szz = m.p[smooth_tri(2, 2)] + r[5];
    const double c00 = syy * szz - syz * syz, c01 = sxz * syz - sxy * szz, c02 = sxy * syz - sxz * syy;
    const double c11 = sxx * szz - sxz * sxz, c12 = sxy * sxz - sxx * syz, c22 = sxx * syy - sxy * sxy;
    const double det = (sxx * c00 + sxy * c01) + sxz * c02;
    const double si[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
    const double nu[3] = {z[0] - m.x[0], z[1] - m.x[1], z[2] - m.x[2]};
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = (si[a][0] * nu[0] + si[a][1] * nu[1]) + si[a][2] * nu[2];
    const double d2 = (nu[0] * t[0] + nu[1] * t[1]) + nu[2] * t[2];
    if (gate > 0.0 && d2 > gate) return false;
    const double rr[3][3] = {{r[0], r[1], r[2]}, {r[1], r[3], r[4]}, {r[2], r[4], r[5]}};
    double k[6][3], kr[6][3], tm[6][3];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            k[i][a] = (SMOOTH_P(m.p, i, 0) * si[0][a] + SMOOTH_P(m.p, i, 1) * si[1][a]) + SMOOTH_P(m.p, i, 2) * si[2][a];
        s.x[i] = m.x[i] + ((k[i][0] * nu[0] + k[i][1] * nu[1]) + k[i][2] * nu[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) kr[i][a] = (k[i][0] * rr[0][a] + k[i][1] * rr[1][a]) + k[i][2] * rr[2][a];
    }
    // T = (I - KH) P-: T(i, j) = P-(i, j) - sum_l K(i, l) P-(l, j); only its first three columns meet (I - KH)^T's K
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            tm[i][a] = SMOOTH_P(m.p, i, a) - ((k[i][0] * SMOOTH_P(m.p, 0, a) + k[i][1] * SMOOTH_P(m.p, 1, a)) + k[i][2] * SMOOTH_P(m.p, 2, a));
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double tij = SMOOTH_P(m.p, i, j) - ((k[i][0] * SMOOTH_P(m.p, 0, j) + k[i][1] * SMOOTH_P(m.p, 1, j)) + k[i][2] * SMOOTH_P(m.p, 2, j));
            const double tk = (tm[i][0] * k[j][0] + tm[i][1] * k[j][1]) + tm[i][2] * k[j][2];
            const double krk = (kr[i][0] * k[j][0] + kr[i][1] * k[j][1]) + kr[i][2] * k[j][2];
            SMOOTH_P(s.p, i, j) = (tij - tk) + krk;
        }
    return true;
}

// a carried state slot st[28] into (s, t_prev); false: the slot holds none (t_last NaN)
__host__ __device__ inline bool smooth_state_load(const double* st, SmoothKf& s, double& t_prev) {
    if (st[27] != st[27]) return false;
#pragma unroll
    for (int e = 0; e < 6; ++e) s.x[e] = st[e];
#pragma unroll
    for (int e = 0; e < 21; ++e) s.p[e] = st[6 + e];
    t_prev = st[27];
    return true;
}

__host__ __device__ inline void smooth_state_store(double* st, const SmoothKf& s, double t_last) {
#pragma unroll
    for (int e = 0; e < 6; ++e) st[e] = s.x[e];
#pragma unroll
    for (int e = 0; e < 21; ++e) st[6 + e] = s.p[e];
    st[27] = t_last;
}

// One row of one (track, joint): `at` = row * J + joint, t the row's time.  On entry (s, t_prev, have) is the state after the
// previous row (have false: none yet).  Start, or predict and then update / missing / gated, as the header has it; on return
// s is the row's filter state, m its prediction (the state itself on the starting row), t_prev = t, `used` whether the
// measurement entered.  false: no state yet and the measurement is unusable -- nothing changed, the row has no estimate.
template <class Args>
__host__ __device__ inline bool smooth_filter_row(const Args& a, size_t at, double t, SmoothKf& s, SmoothKf& m, double& t_prev,
                                                  bool& have, bool& used) {
    const double z[3] = {(double)a.poses[at * 3], (double)a.poses[at * 3 + 1], (double)a.poses[at * 3 + 2]};
    double r[6] = {a.r2, 0.0, 0.0, a.r2, 0.0, a.r2};
    bool usable = __builtin_isfinite(z[0]) && __builtin_isfinite(z[1]) && __builtin_isfinite(z[2]);
    if (a.measurement == METRO_SMOOTH_COVARIANCE) {
        const float* c9 = a.cov + at * 9;
        r[0] = a.cov_scale * (double)c9[0] + a.r2;
        r[1] = a.cov_scale * (double)c9[1];
        r[2] = a.cov_scale * (double)c9[2];
        r[3] = a.cov_scale * (double)c9[4] + a.r2;
        r[4] = a.cov_scale * (double)c9[5];
        r[5] = a.cov_scale * (double)c9[8] + a.r2;
        usable = usable && smooth_pd3(r);
    }
    used = false;
    if (!have) {
        if (!usable) return false;
#pragma unroll
        for (int e = 0; e < 21; ++e) s.p[e] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s.x[c] = z[c];
            s.x[3 + c] = 0.0;
            SMOOTH_P(s.p, 3 + c, 3 + c) = a.v02;
        }
        SMOOTH_P(s.p, 0, 0) = r[0]; SMOOTH_P(s.p, 0, 1) = r[1]; SMOOTH_P(s.p, 0, 2) = r[2];
        SMOOTH_P(s.p, 1, 1) = r[3]; SMOOTH_P(s.p, 1, 2) = r[4]; SMOOTH_P(s.p, 2, 2) = r[5];
        m = s;
        have = used = true;
    } else {
        double dt = t - t_prev;
        if (!(dt > 0.0)) dt = 0.0;
        smooth_predict(s, dt, a.q, m);
        used = usable && smooth_update(m, z, r, a.gate, s);
        if (!used) s = m;
    }
    t_prev = t;
    return true;
}

}  // namespace metro
