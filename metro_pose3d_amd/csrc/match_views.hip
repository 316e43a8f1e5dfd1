// Which boxes of several calibrated cameras show the same person, decided on the device between the forward and
// metro_triangulate_joints (metro_view_affinity and metro_cluster_views, include/metro_hip.h).  Nothing in the reference to
// restate: its examples have one camera each.
//
// metro_view_affinity: cost[a][b], the weighted RMS distance in mm at which the per-joint rays of boxes a and b pass each
// other.  The rays are triangulate.hip's (tri_ray.h): crop row i * n_views + v of box i, the mirror joint for a flipped view,
// non-finite rays skipped, sigma2 the ray's variance in normalised image units.  Per view v and output joint r, with the
// unit directions da, db and w0 = oa - ob:  c = da . db;  the pair is skipped when 1 - c^2 < min_sin2 (near-parallel);
//   ta = (c (db . w0) - da . w0) / (1 - c^2),  tb = (db . w0 - c (da . w0)) / (1 - c^2),  dist = |w0 + ta da - tb db|;
// ta <= 0 or tb <= 0 (the rays meet behind a camera) counts with dist = clip_mm, else with min(dist, clip_mm).
// METRO_TRI_UNIFORM: w = 1.  METRO_TRI_COVARIANCE: w = 1 / (sigma_a^2 ta^2 + sigma_b^2 tb^2), the inverse variance of the
// rays' lateral positions where they pass, mm^-2; a pair whose w is not finite and positive is skipped.
// cost = sqrt(sum w dist^2 / sum w) over the counted pairs, n_pairs their number; +inf with fewer than min_pairs, for two
// boxes on one frame (a person appears once per camera; n_pairs 0) and on the diagonal.
// metro_view_affinity_steps: the same with step_index [n], the exposure of the rig each box belongs to: two boxes of different
// steps are +inf with n_pairs 0 as two boxes of one frame are, every other pair is computed as above (step_index NULL: no gate).
// Threads over the n x n index space: the one with a < b runs the serial loop over (v, r) and writes [a][b] and [b][a], the
// ones with a == b write the diagonal.  fp64 arithmetic on the fp32 inputs, no FMA contraction, one rounding per output.
//
// metro_cluster_views: constrained complete-linkage clustering of the n <= METRO_MATCH_MAX_BOXES boxes in ONE workgroup.
// The working matrix C = max(cost, cost^T) (NaN read as +inf) lives in LDS: 128 rows of 129 floats (64.5 KiB of the CU's
// 160 KiB; the odd row stride keeps the column walk of the merge off a single bank).  Every cluster is named by its lowest
// box.  Per round: every thread scans its share of the entries a < b for the smallest (value, a, b), the waves reduce by
// shuffles and the workgroup through LDS; unless that value is < max_cost the loop ends; else b merges into a:
// C[a][k] = C[k][a] = max(C[a][k], C[b][k]) for all k, and row and column b become +inf, which is how b is deactivated (an
// entry of +inf is never < max_cost, so it is never merged).  Same-frame pairs are +inf and max propagates it: no person gets
// two boxes of one camera.  Persons are numbered by their lowest box; a person with one box has an empty group (one optical
// centre fixes no depth, as frames.person_groups); the others own the crop rows i * n_views + v of their boxes in ascending
// box order.  starts has n + 1 entries (persons >= n_persons: empty), rows n * n_views, those past starts[n] are -1.
#include "metro_common.h"
#include "tri_ray.h"

#pragma clang fp contract(off)

namespace metro {

// ---- pairwise ray distance ---------------------------------------------------------------------------------------------

struct MatchArgs {
    const float* coords01;            // [m][nj][3] head order, m = n * n_views
    const float* cov01;               // [m][nj][6] (METRO_TRI_COVARIANCE)
    const MetroPlacement* rec;        // [m]
    const int* mirror;                // [n_out] output-order mirror joints
    const int* frame_index;           // [n]
    const int* step_index;            // [n] or NULL: pairs across two steps are not compared
    float* cost;                      // [n][n]
    int* n_pairs;                     // [n][n]
    int m, n, n_views, nj, n_out, weights, min_pairs;
    double min_sin2, clip;
    float lrc, half_off;
    int perm[METRO_MAX_JOINTS];
};

// one unordered pair of boxes ia < ib: what a thread of the kernel runs, and what tests/test_match_views.py runs on the host
__host__ __device__ inline void view_affinity_pair(const MatchArgs& a, int ia, int ib) {
    float cost = __builtin_inff();
    int cnt = 0;
    const bool same_step = !a.step_index || a.step_index[ia] == a.step_index[ib];
    if (same_step && a.frame_index[ia] != a.frame_index[ib]) {
        const bool weighted = a.weights == METRO_TRI_COVARIANCE;
        double sw = 0.0, swd = 0.0;
        TriRay ra, rb;
        for (int v = 0; v < a.n_views; ++v) {
            for (int r = 0; r < a.n_out; ++r) {
                if (!tri_ray(a, ia * a.n_views + v, r, ra) || !tri_ray(a, ib * a.n_views + v, r, rb)) continue;
                const double c = dot3_rounded(ra.d, rb.d);
                const double sin2 = 1.0 - c * c;
                if (!(sin2 >= a.min_sin2)) continue;
                const double w0[3] = {ra.o[0] - rb.o[0], ra.o[1] - rb.o[1], ra.o[2] - rb.o[2]};
                const double da = dot3_rounded(ra.d, w0), db = dot3_rounded(rb.d, w0);
                const double ta = (c * db - da) / sin2, tb = (db - c * da) / sin2;
                double dist = a.clip;
                if (ta > 0.0 && tb > 0.0) {
                    const double p[3] = {(w0[0] + ta * ra.d[0]) - tb * rb.d[0], (w0[1] + ta * ra.d[1]) - tb * rb.d[1],
                                         (w0[2] + ta * ra.d[2]) - tb * rb.d[2]};
                    dist = sqrt(dot3_rounded(p, p));
                    if (!(dist <= a.clip)) dist = a.clip;
                }
                double w = 1.0;
                if (weighted) {
                    w = 1.0 / (ra.sigma2 * (ta * ta) + rb.sigma2 * (tb * tb));
                    if (!(__builtin_isfinite(w) && w > 0.0)) continue;
                }
                sw += w;
                swd += w * (dist * dist);
                ++cnt;
            }
        }
        if (cnt >= a.min_pairs) cost = (float)sqrt(swd / sw);
    }
    a.cost[(size_t)ia * a.n + ib] = a.cost[(size_t)ib * a.n + ia] = cost;
    a.n_pairs[(size_t)ia * a.n + ib] = a.n_pairs[(size_t)ib * a.n + ia] = cnt;
}

__host__ __device__ inline void view_affinity_entry(const MatchArgs& a, int idx) {
    const int ia = idx / a.n, ib = idx - ia * a.n;
    if (ia < ib) {
        view_affinity_pair(a, ia, ib);
    } else if (ia == ib) {
        a.cost[idx] = __builtin_inff();
        a.n_pairs[idx] = 0;
    }
}

__global__ __launch_bounds__(64) void view_affinity_kernel(MatchArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < a.n * a.n) view_affinity_entry(a, idx);
}

inline MatchArgs make_match_args(const float* coords01, const float* cov01, const MetroPlacement* rec, const MetroSpec& spec,
                                 const int* mirror, const int* frame_index, int n, int n_views, int weights, double min_sin2,
                                 double clip_mm, int min_pairs, float* cost, int* n_pairs) {
    MatchArgs a;
    a.coords01 = coords01; a.cov01 = cov01; a.rec = rec; a.mirror = mirror; a.frame_index = frame_index;
    a.step_index = nullptr;
    a.cost = cost; a.n_pairs = n_pairs;
    a.m = n * n_views; a.n = n; a.n_views = n_views; a.weights = weights; a.min_pairs = min_pairs;
    a.min_sin2 = min_sin2; a.clip = clip_mm;
    tri_ray_fields(a, spec);
    return a;
}

int launch_view_affinity(const float* coords01, const float* cov01, const MetroPlacement* rec, const MetroSpec& spec,
                         const int* mirror, const int* frame_index, const int* step_index, int n, int n_views, int weights,
                         double min_sin2, double clip_mm, int min_pairs, float* cost, int* n_pairs, hipStream_t stream) {
    if (note_kernel("view_affinity")) return METRO_OK;
    MatchArgs a = make_match_args(coords01, cov01, rec, spec, mirror, frame_index, n, n_views, weights, min_sin2, clip_mm,
                                        min_pairs, cost, n_pairs);
    a.step_index = step_index;
    hipLaunchKernelGGL(view_affinity_kernel, dim3((n * n + 63) / 64), dim3(64), 0, stream, a);
    return launch_status("view_affinity");
}

// ---- complete-linkage clustering ---------------------------------------------------------------------------------------
// The steps below take (tid, nt): thread tid of nt covers the items tid, tid + nt, ...  The kernel calls them with its 256
// threads and a workgroup barrier between steps; tests/test_match_views.py runs the same steps on the host with one thread.

constexpr int MATCH_LD = METRO_MATCH_MAX_BOXES + 1;      // row stride of the working matrix, in floats
constexpr int MATCH_THREADS = 256;

struct ClusterArgs {
    const float* cost;                // [n][n]
    int* person_index;                // [n]
    int* n_persons;                   // [1]
    int* rows;                        // [n * n_views]
    int* starts;                      // [n + 1]
    int n, n_views;
    float max_cost;
};

struct MatchCand { float v; int idx; };                  // idx = a * n + b: its order is (a, b)'s

__host__ __device__ inline bool match_cand_less(const MatchCand& x, const MatchCand& y) {
    return x.v < y.v || (x.v == y.v && x.idx < y.idx);
}

__host__ __device__ inline float match_clean(float v) { return v == v ? v : __builtin_inff(); }

// C = max(cost, cost^T) with NaN as +inf; every box its own cluster
__host__ __device__ inline void cluster_load(const ClusterArgs& a, float* c, int* label, int tid, int nt) {
    for (int i = tid; i < a.n * a.n; i += nt) {
        const int p = i / a.n, q = i - p * a.n;
        const float x = match_clean(a.cost[i]), y = match_clean(a.cost[q * a.n + p]);
        c[p * MATCH_LD + q] = x > y ? x : y;
    }
    for (int i = tid; i < a.n; i += nt) label[i] = i;
}

// this thread's smallest (value, a, b) among the entries a < b
__host__ __device__ inline MatchCand cluster_scan(const float* c, int n, int tid, int nt) {
    MatchCand best = {__builtin_inff(), 0x7fffffff};
    for (int i = tid; i < n * n; i += nt) {
        const int p = i / n, q = i - p * n;
        if (p >= q) continue;
        const MatchCand x = {c[p * MATCH_LD + q], i};
        if (match_cand_less(x, best)) best = x;
    }
    return best;
}

// cluster hi merges into cluster lo (lo < hi): the maxima into row and column lo, row and column hi to +inf
__host__ __device__ inline void cluster_merge(float* c, int* label, int n, int lo, int hi, int tid, int nt) {
    for (int k = tid; k < n; k += nt) {
        if (k != lo && k != hi) {
            const float x = c[lo * MATCH_LD + k], y = c[hi * MATCH_LD + k];
            c[lo * MATCH_LD + k] = c[k * MATCH_LD + lo] = x > y ? x : y;
        }
        c[hi * MATCH_LD + k] = c[k * MATCH_LD + hi] = __builtin_inff();
        if (label[k] == hi) label[k] = lo;
    }
}

// size[k]: the boxes of the cluster named k (0 unless k is its lowest box)
__host__ __device__ inline void cluster_sizes(const int* label, int* size, int n, int tid, int nt) {
    for (int k = tid; k < n; k += nt) {
        int s = 0;
        for (int j = 0; j < n; ++j) s += label[j] == k;
        size[k] = s;
    }
}

// persons numbered by their lowest box: pid[k] = the clusters named below label[k]
__host__ __device__ inline void cluster_persons(const ClusterArgs& a, const int* label, const int* size, int* pid, int tid, int nt) {
    for (int k = tid; k < a.n; k += nt) {
        int p = 0, total = 0;
        for (int j = 0; j < a.n; ++j) {
            p += size[j] > 0 && j < label[k];
            total += size[j] > 0;
        }
        pid[k] = p;
        a.person_index[k] = p;
        if (k == 0) a.n_persons[0] = total;
    }
}

// rows below person p in the CSR: the boxes of persons < p that have company, n_views rows each
__host__ __device__ inline int cluster_rows_below(const int* label, const int* size, const int* pid, int n, int n_views, int p) {
    int s = 0;
    for (int j = 0; j < n; ++j) s += size[label[j]] >= 2 && pid[j] < p;
    return s * n_views;
}

__host__ __device__ inline void cluster_groups(const ClusterArgs& a, const int* label, const int* size, const int* pid, int tid, int nt) {
    const int n = a.n, nv = a.n_views;
    for (int p = tid; p <= n; p += nt) a.starts[p] = cluster_rows_below(label, size, pid, n, nv, p);
    for (int k = tid; k < n; k += nt) {
        if (size[label[k]] < 2) continue;
        int before = 0;
        for (int j = 0; j < k; ++j) before += label[j] == label[k];
        const int base = cluster_rows_below(label, size, pid, n, nv, pid[k]) + before * nv;
        for (int v = 0; v < nv; ++v) a.rows[base + v] = k * nv + v;
    }
    const int used = cluster_rows_below(label, size, pid, n, nv, n);
    for (int i = used + tid; i < n * nv; i += nt) a.rows[i] = -1;
}

__global__ __launch_bounds__(MATCH_THREADS) void cluster_views_kernel(ClusterArgs a) {
    __shared__ float c[METRO_MATCH_MAX_BOXES * MATCH_LD];
    __shared__ int label[METRO_MATCH_MAX_BOXES], size[METRO_MATCH_MAX_BOXES], pid[METRO_MATCH_MAX_BOXES];
    __shared__ MatchCand wave_best[MATCH_THREADS / 64];
    const int tid = threadIdx.x, nt = MATCH_THREADS;
    cluster_load(a, c, label, tid, nt);
    __syncthreads();
    for (int round = 1; round < a.n; ++round) {            // n boxes merge at most n - 1 times
        MatchCand best = cluster_scan(c, a.n, tid, nt);
        for (int off = 32; off > 0; off >>= 1) {
            const MatchCand other = {__shfl_xor(best.v, off), __shfl_xor(best.idx, off)};
            if (match_cand_less(other, best)) best = other;
        }
        if ((tid & 63) == 0) wave_best[tid >> 6] = best;
        __syncthreads();
        best = wave_best[0];
        for (int w = 1; w < MATCH_THREADS / 64; ++w)
            if (match_cand_less(wave_best[w], best)) best = wave_best[w];
        if (!(best.v < a.max_cost)) break;                 // the same value in every thread
        cluster_merge(c, label, a.n, best.idx / a.n, best.idx % a.n, tid, nt);
        __syncthreads();                                   // also: wave_best is read before it is written again
    }
    cluster_sizes(label, size, a.n, tid, nt);
    __syncthreads();
    cluster_persons(a, label, size, pid, tid, nt);
    __syncthreads();
    cluster_groups(a, label, size, pid, tid, nt);
}

int launch_cluster_views(const float* cost, int n, int n_views, float max_cost, int* person_index, int* n_persons, int* rows,
                         int* starts, hipStream_t stream) {
    if (note_kernel("cluster_views")) return METRO_OK;
    ClusterArgs a;
    a.cost = cost; a.person_index = person_index; a.n_persons = n_persons; a.rows = rows; a.starts = starts;
    a.n = n; a.n_views = n_views; a.max_cost = max_cost;
    hipLaunchKernelGGL(cluster_views_kernel, dim3(1), dim3(MATCH_THREADS), 0, stream, a);
    return launch_status("cluster_views");
}

}  // namespace metro
