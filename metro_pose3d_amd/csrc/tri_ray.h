// The ray of one (crop row, output joint) through the crop's virtual camera, shared by triangulate.hip (the point nearest to
// a person's rays) and match_views.hip (how close the rays of two boxes pass) so that both build it by the same operations in
// the same order.  `Args` is the launch's argument struct; tri_ray reads its fields coords01 [m][nj][3], cov01 [m][nj][6]
// (METRO_TRI_COVARIANCE only), rec [m], mirror [n_out], m, nj, n_out, weights, lrc, half_off and perm[METRO_MAX_JOINTS], which
// tri_ray_fields fills from the spec.
#pragma once

#include "metro_common.h"
#include "camera_math.h"

#pragma clang fp contract(off)

namespace metro {

struct TriRay { double d[3], o[3], sigma2; };

__host__ __device__ inline bool tri_finite3(const double* v) {
    return __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]);
}

// the ray of output joint r in crop row `row`; false: no usable ray
template <class Args>
__host__ __device__ inline bool tri_ray(const Args& a, int row, int r, TriRay& ray) {
    if ((unsigned)row >= (unsigned)a.m) return false;
    const MetroPlacement& rec = a.rec[row];
    const int ro = mirrored(rec.rot_to_world) ? a.mirror[r] : r;
    if ((unsigned)ro >= (unsigned)a.n_out) return false;
    const int j = a.perm[ro];
    if ((unsigned)j >= (unsigned)a.nj) return false;
    double u, v, cam[3];
    crop_pixel_f64(a.coords01 + ((size_t)row * a.nj + j) * 3, a.lrc, a.half_off, u, v);
    ray_through_f64(rec.inv_intrinsics, u, v, cam);
    rotate3_f64(rec.rot_to_world, cam, ray.d);
    const double len = sqrt(dot3_rounded(ray.d, ray.d));
    for (int t = 0; t < 3; ++t) {
        ray.d[t] = ray.d[t] / len;
        ray.o[t] = (double)rec.cam_loc[t];
    }
    ray.sigma2 = 0.0;
    if (a.weights == METRO_TRI_COVARIANCE) {
        const float* c6 = a.cov01 + ((size_t)row * a.nj + j) * 6;
        const double k0 = (double)rec.inv_intrinsics[0];
        const double scale = ((double)a.lrc * (double)a.lrc) * (k0 * k0);
        const double floor2 = 1e-12 * scale;
        ray.sigma2 = (0.5 * ((double)c6[0] + (double)c6[1])) * scale;
        if (ray.sigma2 < floor2) ray.sigma2 = floor2;          // a NaN covariance stays NaN: the ray drops where it is weighted
    }
    return tri_finite3(ray.d) && tri_finite3(ray.o);
}

// the spec's part of the ray arguments
template <class Args>
inline void tri_ray_fields(Args& a, const MetroSpec& spec) {
    a.nj = spec.n_joints_head; a.n_out = spec.n_joints_out;
    const HeadPixelScale px = head_pixel_scale(spec);
    a.lrc = (float)px.lrc; a.half_off = (float)px.half_off;
    head_permutation(spec, a.perm);
}

}  // namespace metro
