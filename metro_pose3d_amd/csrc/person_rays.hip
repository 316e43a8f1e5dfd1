// The ray of every joint of a person that ONE camera sees, in ONE launch (metro_person_rays, include/metro_hip.h, which is the
// specification).  Nothing in the reference to restate: its examples have one camera each and no world.  Such a person has no
// triangulated joints (one optical centre: no depth), but its box still pins every joint in the two directions across the ray;
// metro_associate_tracks_rays measures a track against these rays and feeds them to the smoother.
// Inputs as metro_triangulate_joints reads them (tri_ray.h builds the per-view ray: the mirror joint of a flipped view, sigma^2
// the ray's lateral variance), m = n * n_views crop rows, box-major, and single_box [n] of metro_person_steps_labels.
// Per (person p, output joint r) with b = single_box[p] >= 0, over the usable rays of the rows b * n_views + v:
//   w_v = 1 (METRO_TRI_UNIFORM) or 1 / sigma2_v (METRO_TRI_COVARIANCE; a view whose w_v is not finite and positive is dropped)
//   d = normalise(sum w_v d_v), o = that of the first usable view (all views of a box share the optical centre),
//   sigma2 = 1 / sum (1 / sigma2_v) (covariance weights) or 0 (uniform)
// rays_out [n][n_out][8] = o (3), d (3), sigma2, the number of views used; all eight NaN where there is no ray: b < 0, no usable
// view, or a sum of zero or non-finite length.  One thread per (person, output joint); fp64 arithmetic on the fp32 inputs, no
// FMA contraction.
#include "metro_common.h"
#include "tri_ray.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int PERSON_RAY_DOUBLES = 8;

struct PersonRaysArgs {
    const float* coords01;            // [m][nj][3] head order
    const float* cov01;               // [m][nj][6] (METRO_TRI_COVARIANCE)
    const MetroPlacement* rec;        // [m]
    const int* mirror;                // [n_out] output-order mirror joints
    const int* single_box;            // [n] the one box of a person, -1: none
    double* rays;                     // [n][n_out][8]
    int m, n, n_views, nj, n_out, weights;
    float lrc, half_off;
    int perm[METRO_MAX_JOINTS];
};

// one (person, output joint): what a thread of the kernel runs, and what tests/test_single_view.py runs on the host
__host__ __device__ inline void person_ray(const PersonRaysArgs& a, int idx) {
    const int person = idx / a.n_out, r = idx - person * a.n_out;
    const int b = a.single_box[person];
    const bool weighted = a.weights == METRO_TRI_COVARIANCE;
    double sum[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0}, sw = 0.0;
    int cnt = 0;
    if ((unsigned)b < (unsigned)a.n) {
        for (int v = 0; v < a.n_views; ++v) {
            TriRay ray;
            if (!tri_ray(a, b * a.n_views + v, r, ray)) continue;
            const double w = weighted ? 1.0 / ray.sigma2 : 1.0;
            if (!(__builtin_isfinite(w) && w > 0.0)) continue;
            if (cnt == 0)
                for (int t = 0; t < 3; ++t) o[t] = ray.o[t];
            for (int t = 0; t < 3; ++t) sum[t] += w * ray.d[t];
            sw += w;
            ++cnt;
        }
    }
    const double len = sqrt((sum[0] * sum[0] + sum[1] * sum[1]) + sum[2] * sum[2]);
    double* out = a.rays + (size_t)idx * PERSON_RAY_DOUBLES;
    if (cnt == 0 || !(len > 0.0) || !__builtin_isfinite(len)) {
        for (int t = 0; t < PERSON_RAY_DOUBLES; ++t) out[t] = __builtin_nan("");
        return;
    }
    for (int t = 0; t < 3; ++t) {
        out[t] = o[t];
        out[3 + t] = sum[t] / len;
    }
    out[6] = weighted ? 1.0 / sw : 0.0;
    out[7] = (double)cnt;
}

__global__ __launch_bounds__(64) void person_rays_kernel(PersonRaysArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < a.n * a.n_out) person_ray(a, idx);
}

// the launch's arguments from the entry's
inline PersonRaysArgs make_person_rays_args(const float* coords01, const float* cov01, const MetroPlacement* rec, int m,
                                            const MetroSpec& spec, const int* mirror, int weights, const int* single_box, int n,
                                            int n_views, double* rays) {
    PersonRaysArgs a;
    a.coords01 = coords01; a.cov01 = cov01; a.rec = rec; a.mirror = mirror; a.single_box = single_box; a.rays = rays;
    a.m = m; a.n = n; a.n_views = n_views; a.weights = weights;
    tri_ray_fields(a, spec);
    return a;
}

int launch_person_rays(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const MetroSpec& spec,
                       const int* mirror, int weights, const int* single_box, int n, int n_views, double* rays, hipStream_t stream) {
    if (note_kernel("person_rays")) return METRO_OK;
    const PersonRaysArgs a = make_person_rays_args(coords01, cov01, rec, m, spec, mirror, weights, single_box, n, n_views, rays);
    const int total = n * spec.n_joints_out;
    hipLaunchKernelGGL(person_rays_kernel, dim3((total + 63) / 64), dim3(64), 0, stream, a);
    return launch_status("person_rays");
}

}  // namespace metro
