// The bone lengths of followed persons, learned per track slot on the device in ONE launch (metro_track_bone_lengths,
// include/metro_hip.h, which is the specification).  Nothing in the reference to restate: its bone-length tables come from its
// training data.  The rows of slot t are rows[starts[t] : starts[t + 1]], the CSR metro_associate_tracks* writes.
//   reset     bone_ids[t] != ids[t]: the slot's stats become 0 and bone_ids[t] = ids[t] (a freed or reused slot forgets)
//   row       e = (a, b): d = p_b - p_a, l = |d|, u = d / l; skipped if a component is non-finite or l < min_length
//             covariance: C = cov_scale (C_a + C_b), skipped if an entry is non-finite or a diagonal entry < 0;
//                         q = u^T C u, v = tr C / 3 + r_floor^2, l^ = l - (tr C - q) / (2 l) (debias), else l
//             isotropic:  v = r_floor^2, l^ = l
//             skipped unless l^ > 0; gated (rejected += 1) if gate > 0, count >= min_count and
//             (l^ - S1 / S0)^2 > gate (v + 1 / S0); else S0 += 1 / v, S1 += l^ / v, count += 1
//   read-out  after the workgroup barrier, from the slot's stats in LDS: each edge pooled with its mirror partner (symmetric);
//             countp >= min_count and S0p > 0: length = S1p / S0p, sigma = sqrt(1 / S0p), known = 1; else fallback / NaN, 0
// One workgroup of BONE_THREADS = 64 threads (one wave) per slot, lane e = edge e: a latency-bound fp64 walk like
// smooth_tracks_kernel.  fp64 arithmetic on the fp32 inputs, no FMA contraction.  An edge with a joint outside [0, J) is never
// measured and a row outside [0, n) is skipped: nothing is read out of bounds.
#include "metro_common.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int BONE_THREADS = METRO_MAX_JOINTS;   // the most edges check_head_args admits
constexpr int BONE_STAT_DOUBLES = 4;

struct BoneStat { double s0, s1, count, rejected; };

struct BoneArgs {
    const float* poses;          // [n][J][3] mm, absolute
    const float* cov;            // [n][J][9] mm^2 or NULL (isotropic)
    const int* rows;             // [n_rows]
    const int* starts;           // [n_tracks + 1]
    const int* ids;              // [n_tracks] the track table's ids
    const int* edges;            // [E][2] output joint indices
    const int* edge_mirror;      // [E]
    const double* fallback;      // [E] or NULL
    double* stats;               // [n_tracks][E][4]
    int* bone_ids;               // [n_tracks]
    double* lengths_out;         // [n_tracks][E]
    double* sigma_out;           // [n_tracks][E]
    unsigned char* known_out;    // [n_tracks][E]
    int n, n_rows, n_tracks, n_joints, n_edges, min_count, debias, symmetric;
    double gate, r2, cov_scale, min_length;
};

__host__ __device__ inline bool bone_finite(double x) { return x - x == 0.0; }

// one listed row of edge (ja, jb) into s
__host__ __device__ inline void bone_row(const BoneArgs& a, int row, int ja, int jb, BoneStat& s) {
    const float* pa = a.poses + ((size_t)row * a.n_joints + ja) * 3;
    const float* pb = a.poses + ((size_t)row * a.n_joints + jb) * 3;
    double d[3];
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const double x = (double)pa[t], y = (double)pb[t];
        ok = ok && bone_finite(x) && bone_finite(y);
        d[t] = y - x;
    }
    if (!ok) return;
    const double l = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(l >= a.min_length)) return;
    double v = a.r2, lh = l;
    if (a.cov) {
        const float* ca = a.cov + ((size_t)row * a.n_joints + ja) * 9;
        const float* cb = a.cov + ((size_t)row * a.n_joints + jb) * 9;
        const int at[6] = {0, 1, 2, 4, 5, 8};          // the upper triangle: xx xy xz yy yz zz
        double c[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            c[k] = a.cov_scale * ((double)ca[at[k]] + (double)cb[at[k]]);
            ok = ok && bone_finite(c[k]);
        }
        if (!ok || c[0] < 0.0 || c[3] < 0.0 || c[5] < 0.0) return;
        const double u0 = d[0] / l, u1 = d[1] / l, u2 = d[2] / l;
        const double tr = (c[0] + c[3]) + c[5];
        const double q = ((u0 * u0) * c[0] + (u1 * u1) * c[3] + (u2 * u2) * c[5]) +
                         2.0 * ((u0 * u1) * c[1] + (u0 * u2) * c[2] + (u1 * u2) * c[4]);
        v = tr / 3.0 + a.r2;
        if (a.debias) lh = l - (tr - q) / (2.0 * l);
    }
    if (!(lh > 0.0)) return;
    if (a.gate > 0.0 && s.count >= (double)a.min_count) {
        const double r = lh - s.s1 / s.s0;
        if (r * r > a.gate * (v + 1.0 / s.s0)) {
            s.rejected += 1.0;
            return;
        }
    }
    s.s0 += 1.0 / v;
    s.s1 += lh / v;
    s.count += 1.0;
}

// steps 0 and 1 of (slot t, edge e): what lane e of workgroup t runs.  fresh: bone_ids[t] != ids[t], read by the caller before
// anything of the slot is written
__host__ __device__ inline BoneStat bone_track_edge(const BoneArgs& a, int t, int e, bool fresh) {
    double* st = a.stats + ((size_t)t * a.n_edges + e) * BONE_STAT_DOUBLES;
    BoneStat s = {0.0, 0.0, 0.0, 0.0};
    if (!fresh) s = {st[0], st[1], st[2], st[3]};
    const int ja = a.edges[2 * e], jb = a.edges[2 * e + 1];
    if (a.n_rows > 0 && (unsigned)ja < (unsigned)a.n_joints && (unsigned)jb < (unsigned)a.n_joints) {
        int first = a.starts[t], last = a.starts[t + 1];
        if (first < 0) first = 0;
        if (last > a.n_rows) last = a.n_rows;
        for (int k = first; k < last; ++k) {
            const int row = a.rows[k];
            if ((unsigned)row >= (unsigned)a.n) continue;
            bone_row(a, row, ja, jb, s);
        }
    }
    st[0] = s.s0; st[1] = s.s1; st[2] = s.count; st[3] = s.rejected;
    return s;
}

// step 2 of (slot t, edge e) from the slot's stats slot[0 .. E)
__host__ __device__ inline void bone_read_out(const BoneArgs& a, const BoneStat* slot, int t, int e) {
    double s0 = slot[e].s0, s1 = slot[e].s1, count = slot[e].count;
    const int m = a.symmetric ? a.edge_mirror[e] : -1;
    if ((unsigned)m < (unsigned)a.n_edges && m != e) {
        s0 += slot[m].s0;
        s1 += slot[m].s1;
        count += slot[m].count;
    }
    const bool known = count >= (double)a.min_count && s0 > 0.0;
    const size_t at = (size_t)t * a.n_edges + e;
    a.lengths_out[at] = known ? s1 / s0 : a.fallback ? a.fallback[e] : __builtin_nan("");
    a.sigma_out[at] = known ? sqrt(1.0 / s0) : __builtin_nan("");
    a.known_out[at] = known ? 1 : 0;
}

__global__ __launch_bounds__(BONE_THREADS) void track_bone_lengths_kernel(BoneArgs a) {
    __shared__ BoneStat slot[BONE_THREADS];
    const int t = blockIdx.x, e = threadIdx.x;
    const bool fresh = a.bone_ids[t] != a.ids[t];
    if (e < a.n_edges) slot[e] = bone_track_edge(a, t, e, fresh);
    __syncthreads();                         // every lane has read bone_ids[t]; the slot's stats are in LDS
    if (e == 0 && fresh) a.bone_ids[t] = a.ids[t];
    if (e < a.n_edges) bone_read_out(a, slot, t, e);
}

inline BoneArgs make_bone_args(const float* poses, const float* cov, int n, const int* rows, int n_rows, const int* starts, int n_tracks,
                               const int* ids, int n_joints, const int* edges, const int* edge_mirror, int n_edges,
                               const double* fallback, int min_count, double gate, double r_floor, double cov_scale, double min_length,
                               int debias, int symmetric, double* stats, int* bone_ids, double* lengths_out, double* sigma_out,
                               unsigned char* known_out) {
    BoneArgs a;
    a.poses = poses; a.cov = cov; a.rows = rows; a.starts = starts; a.ids = ids; a.edges = edges; a.edge_mirror = edge_mirror;
    a.fallback = fallback; a.stats = stats; a.bone_ids = bone_ids; a.lengths_out = lengths_out; a.sigma_out = sigma_out;
    a.known_out = known_out;
    a.n = n; a.n_rows = n_rows; a.n_tracks = n_tracks; a.n_joints = n_joints; a.n_edges = n_edges; a.min_count = min_count;
    a.debias = debias; a.symmetric = symmetric;
    a.gate = gate; a.r2 = r_floor * r_floor; a.cov_scale = cov_scale; a.min_length = min_length;
    return a;
}

int launch_track_bone_lengths(const float* poses, const float* cov, int n, const int* rows, int n_rows, const int* starts, int n_tracks,
                              const int* ids, int n_joints, const int* edges, const int* edge_mirror, int n_edges,
                              const double* fallback, int min_count, double gate, double r_floor, double cov_scale, double min_length,
                              int debias, int symmetric, double* stats, int* bone_ids, double* lengths_out, double* sigma_out,
                              unsigned char* known_out, hipStream_t stream) {
    if (note_kernel("track_bone_lengths")) return METRO_OK;
    const BoneArgs a = make_bone_args(poses, cov, n, rows, n_rows, starts, n_tracks, ids, n_joints, edges, edge_mirror, n_edges, fallback,
                                      min_count, gate, r_floor, cov_scale, min_length, debias, symmetric, stats, bone_ids, lengths_out,
                                      sigma_out, known_out);
    hipLaunchKernelGGL(track_bone_lengths_kernel, dim3(n_tracks), dim3(BONE_THREADS), 0, stream, a);
    return launch_status("track_bone_lengths");
}

}  // namespace metro
