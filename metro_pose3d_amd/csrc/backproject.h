// Device pieces of the reference's metric back-projection, shared by heads.hip (backproject_kernel) and place_poses.hip
// (place_poses_kernel) so that both run the same operations in the same order:
//   * rays_and_delta_z: the rays of every head joint (crop_pixel and ray_through, camera_math.h) and
//     delta_z = (z - z_root) * box_size (volumetric.py:175-177);
//   * z_offset_by_bones: optimize_z_offset_by_bones_single (src/model/bone_length_based_backproj.py:38-62), whose
//     scipy.optimize.least_squares(method='lm') is MINPACK lmder; `lmder1` restates lmder / qrfac / lmpar / qrsolv for one
//     unknown in fp64, operation by operation (mode 2, diag = 1, ftol = xtol = gtol = 1e-8, factor = 100, maxfev = 100;
//     scipy/optimize/_lsq/least_squares.py call_minpack).  Its Jacobian is NOT the derivative of the residual
//     ((z*c+d)/len instead of (z*c+d/2)/len, :55-56): where it stops depends on MINPACK's step-acceptance history.
// The fp32 part mirrors NumPy on the fp32 tensors TF hands to the py_func: no FMA contraction anywhere (the pragma below
// holds for the rest of every file that includes this header).
#pragma once

#include "metro_common.h"
#include "camera_math.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int HEAD_MAX = METRO_MAX_JOINTS;      // what check_head_args (entries.cpp) admits: joints and edges per pose

struct LmProblem {
    const double* c; const double* d; const double* e; const double* t; int m;
};

__device__ inline void lm_fn(const LmProblem& p, double z, double* f) {
    for (int i = 0; i < p.m; ++i) f[i] = sqrt(z * z * p.c[i] + z * p.d[i] + p.e[i]) - p.t[i];
}
__device__ inline void lm_jac(const LmProblem& p, double z, double* j) {
    for (int i = 0; i < p.m; ++i) j[i] = (z * p.c[i] + p.d[i]) / sqrt(z * z * p.c[i] + z * p.d[i] + p.e[i]);
}
__device__ inline double lm_enorm(const double* v, int m) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += v[i] * v[i];
    return sqrt(s);
}

// MINPACK lmder, n = 1, mode = 2, diag = 1 (see oracle/lm1.py for the same sequence in Python)
__device__ static double lmder1(const LmProblem& prob, double x0) {
    const double ftol = 1e-8, xtol = 1e-8, gtol = 1e-8, factor = 100.0, diag = 1.0;
    const double epsmch = 2.220446049250313e-16, dwarf = 2.2250738585072014e-308;
    const int maxfev = 100, m = prob.m;
    double fvec[HEAD_MAX], f2[HEAD_MAX], fjac[HEAD_MAX], wa4[HEAD_MAX];
    double x = x0;
    lm_fn(prob, x, fvec);
    int nfev = 1, it = 1, info = 0;
    double fnorm = lm_enorm(fvec, m);
    double par = 0.0, delta = 0.0, xnorm = 0.0;
    while (true) {
        lm_jac(prob, x, fjac);
        const double acnorm = lm_enorm(fjac, m);          // qrfac
        double ajnorm = acnorm;
        if (ajnorm != 0.0) {
            if (fjac[0] < 0.0) ajnorm = -ajnorm;
            for (int i = 0; i < m; ++i) fjac[i] = fjac[i] / ajnorm;
            fjac[0] += 1.0;
        }
        const double r = -ajnorm;
        if (it == 1) {
            xnorm = sqrt((diag * x) * (diag * x));
            delta = factor * xnorm;
            if (delta == 0.0) delta = factor;
        }
        for (int i = 0; i < m; ++i) wa4[i] = fvec[i];
        if (fjac[0] != 0.0) {
            double s = 0.0;
            for (int i = 0; i < m; ++i) s += fjac[i] * wa4[i];
            const double temp = -s / fjac[0];
            for (int i = 0; i < m; ++i) wa4[i] += fjac[i] * temp;
        }
        const double qtf = wa4[0];
        double gnorm = 0.0;
        if (fnorm != 0.0 && acnorm != 0.0) {
            const double s = r * (qtf / fnorm);
            gnorm = fmax(gnorm, fabs(s / acnorm));
        }
        if (gnorm <= gtol) { info = 4; break; }
        while (true) {
            // ---- lmpar ----
            double p = r == 0.0 ? 0.0 : qtf / r;
            int liter = 0;
            double wa2 = diag * p;
            double dxnorm = sqrt(wa2 * wa2);
            double fp = dxnorm - delta;
            double par_out;
            if (fp <= 0.1 * delta) {
                par_out = 0.0;
            } else {
                double parl = 0.0;
                if (r != 0.0) {
                    double w = diag * (wa2 / dxnorm);
                    w = w / r;
                    const double temp = sqrt(w * w);
                    parl = ((fp / delta) / temp) / temp;
                }
                const double gw = (r * qtf) / diag;
                const double gn = sqrt(gw * gw);
                double paru = gn / delta;
                if (paru == 0.0) paru = dwarf / fmin(delta, 0.1);
                double pl = fmax(par, parl);
                pl = fmin(pl, paru);
                if (pl == 0.0) pl = gn / dxnorm;
                double sdiag = 0.0;
                while (true) {
                    ++liter;
                    if (pl == 0.0) pl = fmax(dwarf, 0.001 * paru);
                    const double sd = sqrt(pl) * diag;
                    double rr = r, wa = qtf, qtbpj = 0.0;          // qrsolv
                    if (sd != 0.0) {
                        double sn, cs;
                        if (fabs(rr) < fabs(sd)) {
                            const double cotan = rr / sd;
                            sn = 0.5 / sqrt(0.25 + 0.25 * cotan * cotan);
                            cs = sn * cotan;
                        } else {
                            const double tn = sd / rr;
                            cs = 0.5 / sqrt(0.25 + 0.25 * tn * tn);
                            sn = cs * tn;
                        }
                        rr = cs * rr + sn * sd;
                        const double t2 = cs * wa + sn * qtbpj;
                        qtbpj = -sn * wa + cs * qtbpj;
                        wa = t2;
                    }
                    sdiag = rr;
                    p = sdiag != 0.0 ? wa / sdiag : 0.0;
                    wa2 = diag * p;
                    dxnorm = sqrt(wa2 * wa2);
                    const double temp = fp;
                    fp = dxnorm - delta;
                    if (fabs(fp) <= 0.1 * delta || (parl == 0.0 && fp <= temp && temp < 0.0) || liter == 10) break;
                    double w = diag * (wa2 / dxnorm);
                    w = w / sdiag;
                    const double tw = sqrt(w * w);
                    const double parc = ((fp / delta) / tw) / tw;
                    if (fp > 0.0) parl = fmax(parl, pl);
                    if (fp < 0.0) paru = fmin(paru, pl);
                    pl = fmax(parl, pl + parc);
                }
                par_out = liter == 0 ? 0.0 : pl;
            }
            par = par_out;
            // ---- back in lmder ----
            const double wa1 = -p;
            const double x2 = x + wa1;
            const double wa3 = diag * wa1;
            const double pnorm = sqrt(wa3 * wa3);
            if (it == 1) delta = fmin(delta, pnorm);
            lm_fn(prob, x2, f2);
            ++nfev;
            const double fnorm1 = lm_enorm(f2, m);
            double actred = -1.0;
            if (0.1 * fnorm1 < fnorm) { const double q = fnorm1 / fnorm; actred = 1.0 - q * q; }
            const double w3 = r * wa1;
            const double temp1 = sqrt(w3 * w3) / fnorm;
            const double temp2 = (sqrt(par) * pnorm) / fnorm;
            const double prered = temp1 * temp1 + temp2 * temp2 / 0.5;
            const double dirder = -(temp1 * temp1 + temp2 * temp2);
            double ratio = 0.0;
            if (prered != 0.0) ratio = actred / prered;
            if (ratio <= 0.25) {
                double temp;
                if (actred >= 0.0) temp = 0.5;
                else temp = 0.5 * dirder / (dirder + 0.5 * actred);
                if (0.1 * fnorm1 >= fnorm || temp < 0.1) temp = 0.1;
                delta = temp * fmin(delta, pnorm / 0.1);
                par = par / temp;
            } else if (par == 0.0 || ratio >= 0.75) {
                delta = pnorm / 0.5;
                par = 0.5 * par;
            }
            if (ratio >= 1e-4) {
                x = x2;
                for (int i = 0; i < m; ++i) fvec[i] = f2[i];
                xnorm = sqrt((diag * x) * (diag * x));
                fnorm = fnorm1;
                ++it;
            }
            if (fabs(actred) <= ftol && prered <= ftol && 0.5 * ratio <= 1.0) info = 1;
            if (delta <= xtol * xnorm) info = 2;
            if (fabs(actred) <= ftol && prered <= ftol && 0.5 * ratio <= 1.0 && info == 2) info = 3;
            if (info != 0) break;
            if (nfev >= maxfev) info = 5;
            if (fabs(actred) <= epsmch && prered <= epsmch && 0.5 * ratio <= 1.0) info = 6;
            if (delta <= epsmch * xnorm) info = 7;
            if (gnorm <= epsmch) info = 8;
            if (info != 0) break;
            if (ratio >= 1e-4) break;
        }
        if (info != 0) break;
    }
    return x;
}

// rays of the nj head joints of one pose through its virtual camera's K^-1 and delta_z (volumetric.py:173-177)
__device__ inline void rays_and_delta_z(const float* c01, const float* k, int nj, float lrc, float half_off, float box,
                                        float (*cam)[3], float* dz) {
    const float zroot = c01[(nj - 1) * 3 + 2];
    for (int j = 0; j < nj; ++j) {
        float u, v;
        crop_pixel(c01 + j * 3, lrc, half_off, u, v);
        ray_through(k, u, v, cam[j]);
        dz[j] = (c01[j * 3 + 2] - zroot) * box;
    }
}

// optimize_z_offset_by_bones_single (bone_length_based_backproj.py:38-62): the edge coefficients in fp32 as NumPy forms them,
// the solve in fp64 from initial_guess = 2000, the result cast to np.float32
__device__ inline float z_offset_by_bones(const float (*cam)[3], const float* dz, const int* edges, int ne, const double* targets) {
    double c[HEAD_MAX], d[HEAD_MAX], e[HEAD_MAX];
    for (int q = 0; q < ne; ++q) {
        const int i = edges[q * 2], j = edges[q * 2 + 1];
        float av[3], bv[3];
        for (int t = 0; t < 3; ++t) {
            av[t] = cam[i][t] - cam[j][t];
            bv[t] = cam[i][t] * dz[i] - cam[j][t] * dz[j];
        }
        // np.sum over 3 fp32 elements: sequential
        const float cf = (av[0] * av[0] + av[1] * av[1]) + av[2] * av[2];
        const float df = ((2.0f * av[0]) * bv[0] + (2.0f * av[1]) * bv[1]) + (2.0f * av[2]) * bv[2];
        const float ef = (bv[0] * bv[0] + bv[1] * bv[1]) + bv[2] * bv[2];
        c[q] = (double)cf; d[q] = (double)df; e[q] = (double)ef;
    }
    LmProblem prob;
    prob.c = c; prob.d = d; prob.e = e; prob.m = ne;
    prob.t = targets;
    return (float)lmder1(prob, 2000.0);
}

}  // namespace metro
