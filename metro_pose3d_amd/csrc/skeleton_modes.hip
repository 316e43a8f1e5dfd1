// Which heat-map mode every joint of a crop is in, decided by the person's bone lengths: exact inference over the skeleton tree of
// a forward whose plan has a skeleton binding (metro_plan_bind_skeleton_modes, include/metro_hip.h, which holds the definition).
// Per crop row: voxel int32 [J, K] and stats fp32 [J, K, 11] in metro_plan_bind_modes' layout, lengths fp64 [E] in mm; the
// variables are the output joints, their states the present modes, the unaries the modes' normalised masses, the pairwise terms a
// Gaussian likelihood of the bone length between two modes (ln psi <= 0).  Outputs: the marginal of every mode (sum-product in the
// log domain), the MAP assignment (max-product, back-tracked), ln of the evidence and of the MAP's probability per component, and
// coords01 with the chosen modes' means in place of the plain ones.
// One launch, one workgroup of 64 lanes per crop row.  skeleton_walk below is the whole body, written for a TEAM (tid of nt, sync):
// the kernel's team is the wave, the host tests' team is one thread, or 64 threads at a barrier (tests/test_skeleton_modes.py
// compiles this file for the host and walks it).  Nothing is reduced ACROSS lanes: every value is computed by one lane, its inner
// index (modes, children, joints) in a fixed serial order, so every team size gives the same bits.  Phases, a sync between them:
//   1  present modes; per joint the unaries ln w (lane = joint)
//   2  known edges (lane = edge), then ln psi of every pair of modes of every known edge into LDS (lane = (edge, ka, kb))
//   3  the row's forest (lane = joint): the host's rooted schedule with the unknown edges cut, every component re-rooted at its
//      lowest-numbered joint (the path from that joint to the old root is reversed), depths, and the order by (depth, joint)
//   4  leaves to roots, one DEPTH LEVEL per step: per joint of the level 2 K lanes, K the sum-product message to the parent, K the
//      max-product message and its argument (lowest index among equals); then per (joint of the level above, mode) one lane adds
//      its children's messages into its belief, in the level's order
//   5  the roots' choices, then roots to leaves, one depth level per step: the beliefs become the full marginals, the choice
//      follows the parent's through the stored arguments
//   6  outputs (lane = joint, lane = head joint for coords01_sel)
// fp64 throughout on the stored fp32 inputs, no atomics; each output is rounded to fp32 once.  One instantiation for all plans.
#include "metro_common.h"

#pragma clang fp contract(off)

namespace metro {

#define SK_HD __host__ __device__ __forceinline__

constexpr int SK_THREADS = 64;
constexpr int SK_STATS = 11;                 // mass, peak, coords01 (3), cov01 (6): heat_modes' record
constexpr int SK_MAX_EDGES = 63;
constexpr int SK_LDS_MAX = 64 * 1024;

struct SkeletonArgs {
    const int32_t* voxel;    // [max_n][J][K]
    const float* stats;      // [max_n][J][K][11]
    const double* lengths;   // [max_n][E]
    const float* coords01;   // [n][Jhead][3], read only where coords01_sel is written
    void* prob;              // [max_n][J][K] fp32 (the host tests also read the fp64 values before that rounding)
    int32_t* choice;         // [max_n][J]
    void* info;              // [max_n][J][2]
    float* coords01_sel;     // [max_n][Jhead][3] or NULL
    int J, K, E, Jhead;
    MetroSkeletonModes p;
    // the host's rooted schedule: every component of the forest rooted at its lowest-numbered joint
    signed char parent[METRO_MAX_JOINTS];        // -1: a root
    signed char parent_edge[METRO_MAX_JOINTS];   // the edge to the parent
    unsigned char edge[SK_MAX_EDGES + 1][2];
    unsigned char perm[METRO_MAX_JOINTS];        // the head joint of output joint r
};

// the workgroup's LDS, carved from one buffer
struct SkeletonLds {
    double* psi;             // [E][K][K]: ln psi[e][mode of edge[e][0]][mode of edge[e][1]]
    double* bs;              // [J][K]: sum-product belief (unary + children's messages; after phase 5 the full log marginal, unnormalised)
    double* bm;              // [J][K]: max-product belief
    double* ms;              // [J][K]: the sum-product message joint -> parent, per mode of the parent
    double* mm;              // [J][K]: the max-product message
    signed char* arg;        // [J][K]: the max-product message's argument, per mode of the parent
    unsigned char* pres;     // [J][K]
    unsigned char* known;    // [64]
    signed char *par, *pe, *sub, *root, *depth, *order, *pick, *level;   // [64] each
    unsigned char *alive, *size;                                     // [64] each
};
SK_HD size_t sk_lds_bytes(int J, int K, int E) {
    return (size_t)8 * ((size_t)E * K * K + 4 * (size_t)J * K) + 2 * (((size_t)J * K + 7) & ~(size_t)7) + 11 * 64;
}
SK_HD SkeletonLds sk_carve(char* lds, int J, int K, int E) {
    SkeletonLds s;
    const size_t jk = (size_t)J * K, jk8 = (jk + 7) & ~(size_t)7;
    s.psi = reinterpret_cast<double*>(lds);
    s.bs = s.psi + (size_t)E * K * K; s.bm = s.bs + jk; s.ms = s.bm + jk; s.mm = s.ms + jk;
    char* b = reinterpret_cast<char*>(s.mm + jk);
    s.arg = reinterpret_cast<signed char*>(b); b += jk8;
    s.pres = reinterpret_cast<unsigned char*>(b); b += jk8;
    s.known = reinterpret_cast<unsigned char*>(b); b += 64;
    signed char* t = reinterpret_cast<signed char*>(b);
    s.par = t; s.pe = t + 64; s.sub = t + 128; s.root = t + 192; s.depth = t + 256; s.order = t + 320; s.pick = t + 384;
    s.alive = reinterpret_cast<unsigned char*>(b) + 448;
    s.size = reinterpret_cast<unsigned char*>(b) + 512;
    s.level = t + 576;
    return s;
}

SK_HD bool sk_finite(double x) { return x > -INFINITY && x < INFINITY; }

// ln psi of modes ka of joint p and kb of joint q on an edge of length L
SK_HD double sk_log_psi(const float* sa, const float* sb, double L, const MetroSkeletonModes& P) {
    const double dx = P.scale_mm[0] * (double)sb[2] - P.scale_mm[0] * (double)sa[2];
    const double dy = P.scale_mm[1] * (double)sb[3] - P.scale_mm[1] * (double)sa[3];
    const double dz = P.scale_mm[2] * (double)sb[4] - P.scale_mm[2] * (double)sa[4];
    const double l = sqrt(dx * dx + dy * dy + dz * dz);
    const double sx = P.scale_mm[0], sy = P.scale_mm[1], sz = P.scale_mm[2];
    const double cxx = sx * sx * ((double)sa[5] + (double)sb[5]), cyy = sy * sy * ((double)sa[6] + (double)sb[6]);
    const double czz = sz * sz * ((double)sa[7] + (double)sb[7]), cxy = sx * sy * ((double)sa[8] + (double)sb[8]);
    const double cxz = sx * sz * ((double)sa[9] + (double)sb[9]), cyz = sy * sz * ((double)sa[10] + (double)sb[10]);
    double s;
    if (l < P.min_length_mm || !(l > 0.0)) {
        s = (cxx + cyy + czz) / 3.0;
    } else {
        const double ux = dx / l, uy = dy / l, uz = dz / l;
        s = (ux * ux * cxx + uy * uy * cyy + uz * uz * czz) + 2.0 * (ux * uy * cxy + ux * uz * cxz + uy * uz * cyz);
    }
    s = s > 0.0 ? s : 0.0;
    const double v0 = P.sigma_mm * P.sigma_mm + (P.sigma_rel * L) * (P.sigma_rel * L);
    const double v = v0 + P.cov_scale * s;
    return -((l - L) * (l - L)) / (2.0 * v) - 0.5 * log(v / v0);
}

template <typename OutT = float, class Team>
__host__ __device__ inline void skeleton_walk(const SkeletonArgs& a, int img, char* lds, Team& team) {
    const int J = a.J, K = a.K, E = a.E;
    const int tid = team.tid, nt = team.nt;
    const SkeletonLds s = sk_carve(lds, J, K, E);
    const int32_t* voxel = a.voxel + (size_t)img * J * K;
    const float* stats = a.stats + (size_t)img * J * K * SK_STATS;
    const double* lengths = a.lengths + (size_t)img * E;

    // ---- 1: present modes, unaries ----
    for (int u = tid; u < J * K; u += nt) {
        const float* st = stats + (size_t)u * SK_STATS;
        bool ok = voxel[u] >= 0 && sk_finite((double)st[0]) && st[0] > 0.0f;
        for (int i = 2; i < SK_STATS; ++i) ok = ok && sk_finite((double)st[i]);
        s.pres[u] = ok ? 1 : 0;
    }
    team.sync();
    for (int j = tid; j < J; j += nt) {
        double total = 0.0;
        int any = 0;
        for (int k = 0; k < K; ++k)
            if (s.pres[j * K + k]) { total += (double)stats[(size_t)(j * K + k) * SK_STATS]; any = 1; }
        s.alive[j] = (unsigned char)any;
        for (int k = 0; k < K; ++k) {
            const double lw = s.pres[j * K + k] ? log((double)stats[(size_t)(j * K + k) * SK_STATS] / total) : (double)-INFINITY;
            s.bs[j * K + k] = lw; s.bm[j * K + k] = lw;
        }
    }
    team.sync();

    // ---- 2: known edges, ln psi ----
    for (int e = tid; e < E; e += nt) {
        const double L = lengths[e];
        s.known[e] = sk_finite(L) && L > 0.0 && s.alive[a.edge[e][0]] && s.alive[a.edge[e][1]] ? 1 : 0;
    }
    team.sync();
    for (int u = tid; u < E * K * K; u += nt) {
        const int e = u / (K * K), ka = (u / K) % K, kb = u % K;
        const int p = a.edge[e][0], q = a.edge[e][1];
        double v = 0.0;
        if (s.known[e] && s.pres[p * K + ka] && s.pres[q * K + kb])
            v = sk_log_psi(stats + (size_t)(p * K + ka) * SK_STATS, stats + (size_t)(q * K + kb) * SK_STATS, lengths[e], a.p);
        s.psi[u] = v;
    }

    // ---- 3: the row's forest ----
    for (int j = tid; j < J; j += nt) {                     // the root of j's component in the host's schedule, the unknown edges cut
        int c = j;
        while (a.parent[c] >= 0 && s.known[a.parent_edge[c]]) c = a.parent[c];
        s.sub[j] = (signed char)c;
        const bool cut = a.parent[j] < 0 || !s.known[a.parent_edge[j]];
        s.par[j] = cut ? (signed char)-1 : a.parent[j];
        s.pe[j] = cut ? (signed char)-1 : a.parent_edge[j];
    }
    team.sync();
    for (int j = tid; j < J; j += nt) {                     // its lowest-numbered joint, and its size
        int first = -1, count = 0;
        for (int i = 0; i < J; ++i)
            if (s.sub[i] == s.sub[j]) { first = first < 0 ? i : first; ++count; }
        s.root[j] = (signed char)first;
        s.size[j] = (unsigned char)count;
    }
    team.sync();
    for (int j = tid; j < J; j += nt) {                     // re-root: reverse the path from the lowest-numbered joint to the old root
        if (s.root[j] != j || s.sub[j] == j) continue;
        int prev = j, prev_edge = a.parent_edge[j], cur = a.parent[j];
        for (;;) {
            const int up = a.parent[cur], up_edge = a.parent_edge[cur];
            s.par[cur] = (signed char)prev; s.pe[cur] = (signed char)prev_edge;
            if (cur == s.sub[j]) break;
            prev = cur; prev_edge = up_edge; cur = up;
        }
        s.par[j] = -1; s.pe[j] = -1;
    }
    team.sync();
    for (int j = tid; j < J; j += nt) {
        int d = 0;
        for (int c = j; s.par[c] >= 0; c = s.par[c]) ++d;
        s.depth[j] = (signed char)d;
    }
    team.sync();
    for (int j = tid; j < J; j += nt) {                     // parents before children: by (depth, joint)
        int rank = 0;
        for (int i = 0; i < J; ++i) rank += s.depth[i] < s.depth[j] || (s.depth[i] == s.depth[j] && i < j) ? 1 : 0;
        s.order[rank] = (signed char)j;
        int before = 0;                                      // level[d]: where depth d starts in the order (d = lane's joint index)
        for (int i = 0; i < J; ++i) before += s.depth[i] < j ? 1 : 0;
        s.level[j] = (signed char)before;
    }
    team.sync();

    // ---- 4: leaves to roots, one depth level per step ----
    int deepest = 0;
    for (int i = 0; i < J; ++i) deepest = s.depth[i] > deepest ? s.depth[i] : deepest;
    for (int d = deepest; d >= 1; --d) {
        const int t0 = s.level[d], t1 = d == deepest ? J : s.level[d + 1], p0 = s.level[d - 1];
        for (int u = tid; u < (t1 - t0) * 2 * K; u += nt) {  // the messages of the level's joints to their parents
            const int c = s.order[t0 + u / (2 * K)], r = u % (2 * K), ka = r < K ? r : r - K;
            const int e = s.pe[c];
            const bool child_first = a.edge[e][0] == c;      // psi[e] is indexed (mode of edge[e][0], mode of edge[e][1])
            const double* bel = r < K ? s.bs + c * K : s.bm + c * K;
            const double* ps = s.psi + (size_t)e * K * K;
            double mx = -INFINITY;
            int at = 0;
            for (int kb = 0; kb < K; ++kb) {
                const double v = bel[kb] + (child_first ? ps[kb * K + ka] : ps[ka * K + kb]);
                if (v > mx) { mx = v; at = kb; }
            }
            if (r < K) {
                double m = mx;
                if (mx > -INFINITY) {
                    double sum = 0.0;
                    for (int kb = 0; kb < K; ++kb) sum += exp((bel[kb] + (child_first ? ps[kb * K + ka] : ps[ka * K + kb])) - mx);
                    m = mx + log(sum);
                }
                s.ms[c * K + ka] = m;
            } else {
                s.arg[c * K + ka] = (signed char)at;
                s.mm[c * K + ka] = mx;
            }
        }
        team.sync();
        for (int u = tid; u < (t0 - p0) * 2 * K; u += nt) {  // added into the beliefs of the level above, children in the level's order
            const int p = s.order[p0 + u / (2 * K)], r = u % (2 * K), ka = r < K ? r : r - K;
            double* bel = r < K ? s.bs : s.bm;
            const double* msg = r < K ? s.ms : s.mm;
            double acc = bel[p * K + ka];
            for (int t = t0; t < t1; ++t) {
                const int c = s.order[t];
                if (s.par[c] == p) acc += msg[c * K + ka];
            }
            bel[p * K + ka] = acc;
        }
        team.sync();
    }

    // ---- 5: the roots' choices; roots to leaves, one depth level per step ----
    for (int j = tid; j < J; j += nt) {
        if (s.par[j] >= 0) continue;
        int at = -1;
        double mx = -INFINITY;
        for (int k = 0; k < K; ++k)
            if (s.bm[j * K + k] > mx) { mx = s.bm[j * K + k]; at = k; }
        s.pick[j] = (signed char)at;                         // -1: a dead joint
    }
    team.sync();
    for (int d = 1; d <= deepest; ++d) {
        const int t0 = s.level[d], t1 = d == deepest ? J : s.level[d + 1];
        for (int u = tid; u < (t1 - t0) * (K + 1); u += nt) {
            const int c = s.order[t0 + u / (K + 1)], kb = u % (K + 1), p = s.par[c];
            if (kb == K) { s.pick[c] = s.arg[c * K + s.pick[p]]; continue; }
            const int e = s.pe[c];
            const bool child_first = a.edge[e][0] == c;
            const double* ps = s.psi + (size_t)e * K * K;
            double mx = -INFINITY;
            for (int ka = 0; ka < K; ++ka) {
                if (!s.pres[p * K + ka]) continue;
                const double v = (s.bs[p * K + ka] - s.ms[c * K + ka]) + (child_first ? ps[kb * K + ka] : ps[ka * K + kb]);
                mx = v > mx ? v : mx;
            }
            double sum = 0.0;
            for (int ka = 0; ka < K; ++ka) {
                if (!s.pres[p * K + ka]) continue;
                sum += exp(((s.bs[p * K + ka] - s.ms[c * K + ka]) + (child_first ? ps[kb * K + ka] : ps[ka * K + kb])) - mx);
            }
            s.bs[c * K + kb] += mx + log(sum);               // -Inf stays -Inf: an absent mode
        }
        team.sync();
    }

    // ---- 6: outputs ----
    OutT* prob = static_cast<OutT*>(a.prob) + (size_t)img * J * K;
    OutT* info = static_cast<OutT*>(a.info) + (size_t)img * J * 2;
    int32_t* choice = a.choice + (size_t)img * J;
    for (int j = tid; j < J; j += nt) {
        if (!s.alive[j]) {
            for (int k = 0; k < K; ++k) prob[j * K + k] = (OutT)NAN;
            choice[j] = -1; info[2 * j] = (OutT)NAN; info[2 * j + 1] = (OutT)NAN;
            continue;
        }
        const int r = s.root[j];
        if (s.size[j] == 1) {                                // no known edge: the unaries, and an evidence of exactly 1
            double total = 0.0;
            for (int k = 0; k < K; ++k)
                if (s.pres[j * K + k]) total += (double)stats[(size_t)(j * K + k) * SK_STATS];
            for (int k = 0; k < K; ++k)
                prob[j * K + k] = (OutT)(s.pres[j * K + k] ? (double)stats[(size_t)(j * K + k) * SK_STATS] / total : 0.0);
            choice[j] = s.pick[j]; info[2 * j] = (OutT)0.0; info[2 * j + 1] = (OutT)s.bm[j * K + s.pick[j]];
            continue;
        }
        double mx = -INFINITY, sum = 0.0;
        for (int k = 0; k < K; ++k) mx = s.bs[r * K + k] > mx ? s.bs[r * K + k] : mx;
        for (int k = 0; k < K; ++k) sum += exp(s.bs[r * K + k] - mx);
        const double log_z = mx + log(sum);
        for (int k = 0; k < K; ++k) prob[j * K + k] = (OutT)(s.pres[j * K + k] ? exp(s.bs[j * K + k] - log_z) : 0.0);
        choice[j] = s.pick[j];
        info[2 * j] = (OutT)(log_z < 0.0 ? log_z : 0.0);     // psi <= 1 and sum w = 1: above 0 by rounding only
        info[2 * j + 1] = (OutT)(s.bm[r * K + s.pick[r]] - log_z);
    }
    if (a.coords01_sel != nullptr) {
        const float* plain = a.coords01 + (size_t)img * a.Jhead * 3;
        float* sel = a.coords01_sel + (size_t)img * a.Jhead * 3;
        for (int h = tid; h < a.Jhead; h += nt) {            // one writer per head joint; of output joints that share it the last
            float x = plain[3 * h], y = plain[3 * h + 1], z = plain[3 * h + 2];
            for (int j = 0; j < J; ++j) {
                if (a.perm[j] != h || !s.alive[j]) continue;
                const float* st = stats + (size_t)(j * K + s.pick[j]) * SK_STATS;
                x = st[2]; y = st[3]; z = st[4];
            }
            sel[3 * h] = x; sel[3 * h + 1] = y; sel[3 * h + 2] = z;
        }
    }
}

// The kernel's team: one wave.
struct SkeletonWave {
    const int tid;
    static constexpr int nt = SK_THREADS;
    __device__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(SK_THREADS) void skeleton_modes_kernel(SkeletonArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    SkeletonWave team = {(int)threadIdx.x};
    skeleton_walk(a, blockIdx.x, sk_smem, team);
}

// The rooted schedule of a forest: every component rooted at its lowest-numbered joint.  Returns the index of the first edge that
// is out of range, a self-edge or closes a cycle (`why` says which), or -1.
int skeleton_schedule(const int32_t* edges, int n_edges, int n_joints, signed char* parent, signed char* parent_edge, const char** why) {
    int comp[METRO_MAX_JOINTS];
    for (int j = 0; j < n_joints; ++j) comp[j] = j;
    for (int e = 0; e < n_edges; ++e) {
        const int p = edges[2 * e], q = edges[2 * e + 1];
        if (p < 0 || p >= n_joints || q < 0 || q >= n_joints) { *why = "has a joint outside the output joints"; return e; }
        if (p == q) { *why = "joins a joint to itself"; return e; }
        if (comp[p] == comp[q]) { *why = "closes a cycle (the skeleton must be a forest)"; return e; }
        const int from = comp[q], to = comp[p];
        for (int j = 0; j < n_joints; ++j) comp[j] = comp[j] == from ? to : comp[j];
    }
    bool seen[METRO_MAX_JOINTS] = {};
    int queue[METRO_MAX_JOINTS];
    for (int r = 0; r < n_joints; ++r) {
        if (seen[r]) continue;
        int head = 0, tail = 0;
        queue[tail++] = r; seen[r] = true; parent[r] = -1; parent_edge[r] = -1;
        while (head < tail) {
            const int j = queue[head++];
            for (int e = 0; e < n_edges; ++e) {
                const int p = edges[2 * e], q = edges[2 * e + 1];
                const int other = p == j ? q : q == j ? p : -1;
                if (other < 0 || seen[other]) continue;
                seen[other] = true; parent[other] = (signed char)j; parent_edge[other] = (signed char)e;
                queue[tail++] = other;
            }
        }
    }
    return -1;
}

int launch_skeleton_modes(const int32_t* voxel, const float* stats, int k, const double* lengths, const int32_t* edges, int n_edges,
                          const signed char* parent, const signed char* parent_edge, const MetroSkeletonModes& params,
                          const float* coords01, int n, int max_n, const MetroSpec& spec, float* prob, int32_t* choice, float* info,
                          float* coords01_sel, hipStream_t stream) {
    const int J = spec.n_joints_out;
    if (J < 1 || J > METRO_MAX_JOINTS || spec.n_joints_head < 1 || spec.n_joints_head > METRO_MAX_JOINTS || k < 1 || k > METRO_MAX_MODES ||
        n_edges < 0 || n_edges > SK_MAX_EDGES || n < 1 || n > max_n || (coords01_sel != nullptr && coords01 == nullptr)) {
        set_error("skeleton_modes: unsupported call (%d output joints, %d head joints, k %d, %d edges, %d crops of %d)", J,
                  spec.n_joints_head, k, n_edges, n, max_n);
        return METRO_ERR_UNSUPPORTED;
    }
    SkeletonArgs a = {};
    a.voxel = voxel; a.stats = stats; a.lengths = lengths; a.coords01 = coords01;
    a.prob = prob; a.choice = choice; a.info = info; a.coords01_sel = coords01_sel;
    a.J = J; a.K = k; a.E = n_edges; a.Jhead = spec.n_joints_head; a.p = params;
    for (int j = 0; j < J; ++j) {
        a.parent[j] = parent[j]; a.parent_edge[j] = parent_edge[j];
        a.perm[j] = (unsigned char)spec.permutation[j];
    }
    for (int e = 0; e < n_edges; ++e) { a.edge[e][0] = (unsigned char)edges[2 * e]; a.edge[e][1] = (unsigned char)edges[2 * e + 1]; }
    if (note_kernel("skeleton_modes")) return METRO_OK;
    static PerDeviceInt attr;
    const int st = ensure_dyn_lds(reinterpret_cast<const void*>(skeleton_modes_kernel), SK_LDS_MAX, attr, "skeleton_modes");
    if (st) return st;
    hipLaunchKernelGGL(skeleton_modes_kernel, dim3(n), dim3(SK_THREADS), sk_lds_bytes(J, k, n_edges), stream, a);
    return launch_status("skeleton_modes");
}

}  // namespace metro
