// Which box of a video continues which track, decided on the device between the forward and metro_smooth_tracks, in ONE launch
// of ONE workgroup (metro_associate_tracks, include/metro_hip.h, which is the specification).  Nothing in the reference to
// restate: one example is one image, and a person detector gives boxes per frame with no identity from frame to frame.
// The launch walks the call's boxes step by step (all boxes of one timestamp are one step, the CSR of the steps is built on
// the host, frames.time_steps) over a table of T <= 128 track slots whose filter state is the smoother's own [T][J][28]:
//   begin     a working copy of the state goes to the caller's workspace; a live slot last seen before
//             t_first - max_age is retired (t_last = NaN in the state and the copy, id -1), a slot that is not live is free
//   cost      per (slot, box of the step): the RMS over the joints of min(|z - (p + dt v)|, clip), one rounding to fp32;
//             +inf with fewer than min_joints joints or a slot last seen before t_step - max_age
//   assign    greedy one-to-one: the smallest remaining cost (ties: lowest slot, then lowest position in the step) while it
//             is < max_cost; its row and its column of the matrix become +inf.  metro_associate_tracks_optimal: the admissible
//             pairs of the largest total gain max_cost - cost instead, by shortest augmenting paths (further down)
//   births    the unassigned boxes with a finite joint, in step order, take the lowest free slots and the next ids
//   filter    every slot that received a box advances its working state by smooth_filter_row (smooth_step.h), the per-row
//             step of smooth_tracks.hip
// and then writes the CSR per slot that metro_smooth_tracks reads.  The cost matrix lives in LDS: 128 rows of 129 floats
// (64.5 KiB of the CU's 160 KiB; the odd row stride keeps the column walk of the strike off a single bank).  The working
// state lives in global memory and is exchanged only within the workgroup, across __syncthreads().
// The steps below take (tid, nt): thread tid of nt covers the items tid, tid + nt, ...  Their order and the barriers between
// them are written once, in assoc_walk at the end of the file, for both assignment rules, with and without ray rows, and for
// whoever executes it: the kernel's 256 threads (AssocWorkgroup) or one thread on the host (tests/assoc_host.py, where
// tests/test_follow_tracks.py, test_assign_tracks.py and test_single_view.py run this very walk).
// fp64 arithmetic on the fp32 inputs, no FMA contraction.
#include <type_traits>

#include "metro_common.h"
#include "smooth_step.h"

#pragma clang fp contract(off)

namespace metro {

constexpr int ASSOC_MAX = METRO_ASSOC_MAX;               // boxes per step, and track slots
constexpr int ASSOC_LD = ASSOC_MAX + 1;                  // row stride of the cost matrix, in floats
constexpr int ASSOC_THREADS = 256;

struct AssocCand { float v; int idx; };                  // idx = slot * ASSOC_LD + position: its order is (slot, position)'s

// what the workgroup keeps in LDS (the host test keeps it on its heap)
struct AssocLds {
    float c[ASSOC_MAX * ASSOC_LD];                       // cost[slot][position in the step]
    float box_cost[ASSOC_MAX];                           // the accepted cost of a matched box, else NaN
    int box_row[ASSOC_MAX];                              // the pose row of a position, -1: not in [0, n)
    int box_any[ASSOC_MAX];                              // the box has a finite joint
    int box_slot[ASSOC_MAX];                             // the slot of the box, -1: none (yet)
    int born_slot[ASSOC_MAX], born_id[ASSOC_MAX];        // births decided, not yet applied
    int ids[ASSOC_MAX], count[ASSOC_MAX], fill[ASSOC_MAX], start[ASSOC_MAX + 1];
    int next_id, n_new, n_dropped;
};

__host__ __device__ inline bool assoc_cand_less(const AssocCand& x, const AssocCand& y) {
    return x.v < y.v || (x.v == y.v && x.idx < y.idx);
}

// step s owns the positions lo .. lo + m - 1 of step_rows: the starts clamped to [0, n_step_rows], at most 128 positions
__host__ __device__ inline void assoc_step_range(const AssocArgs& a, int s, int& lo, int& m) {
    lo = a.step_starts[s];
    int hi = a.step_starts[s + 1];
    if (lo < 0) lo = 0;
    if (hi > a.n_step_rows) hi = a.n_step_rows;
    m = hi - lo;
    if (m < 0) m = 0;
    if (m > ASSOC_MAX) m = ASSOC_MAX;
}

// the time of a step is that of its first row in [0, n); false: it has none, the step is skipped
__host__ __device__ inline bool assoc_step_time(const AssocArgs& a, int lo, int m, double& t) {
    for (int k = 0; k < m; ++k) {
        const int row = a.step_rows[lo + k];
        if ((unsigned)row < (unsigned)a.n) {
            t = a.times[row];
            return true;
        }
    }
    return false;
}

__host__ __device__ inline bool assoc_first_time(const AssocArgs& a, double& t) {
    for (int s = 0; s < a.n_steps; ++s) {
        int lo, m;
        assoc_step_range(a, s, lo, m);
        if (assoc_step_time(a, lo, m, t)) return true;
    }
    return false;
}

__host__ __device__ inline double* assoc_slot_state(const AssocArgs& a, double* base, int slot, int j) {
    return base + ((size_t)slot * a.n_out + j) * SMOOTH_STATE_DOUBLES;
}

// the working copy of the state, every box untracked until a step says otherwise, the table into LDS
__host__ __device__ inline void assoc_begin(const AssocArgs& a, AssocLds& l, int tid, int nt) {
    const size_t total = (size_t)a.n_tracks * a.n_out * SMOOTH_STATE_DOUBLES;
    for (size_t i = tid; i < total; i += nt) a.ws[i] = a.state[i];
    for (int i = tid; i < a.n; i += nt) {
        a.track_index[i] = -1;
        a.track_id[i] = -1;
        a.cost_out[i] = __builtin_nanf("");
    }
    for (int t = tid; t < a.n_tracks; t += nt) {
        l.ids[t] = a.ids[t];
        l.count[t] = 0;
        l.fill[t] = 0;
    }
    if (tid == 0) {
        l.next_id = a.next_id[0];
        l.n_new = 0;
        l.n_dropped = 0;
    }
}

// a live slot last seen before t_first - max_age is retired; a slot that is not live is free
__host__ __device__ inline void assoc_retire(const AssocArgs& a, AssocLds& l, bool have_first, double t_first, int tid, int nt) {
    for (int t = tid; t < a.n_tracks; t += nt) {
        bool live = false;
        double seen = -__builtin_inf();
        for (int j = 0; j < a.n_out; ++j) {
            const double tl = assoc_slot_state(a, a.ws, t, j)[27];
            if (tl != tl) continue;
            live = true;
            if (tl > seen) seen = tl;
        }
        if (live && have_first && seen < t_first - a.max_age) {
            for (int j = 0; j < a.n_out; ++j)
                assoc_slot_state(a, a.ws, t, j)[27] = assoc_slot_state(a, a.state, t, j)[27] = __builtin_nan("");
            live = false;
        }
        if (!live) l.ids[t] = -1;
    }
}

// the boxes of the step: their rows, whether a joint is finite, nobody assigned
__host__ __device__ inline void assoc_step_boxes(const AssocArgs& a, AssocLds& l, int lo, int m, int tid, int nt) {
    for (int k = tid; k < m; k += nt) {
        const int row = a.step_rows[lo + k];
        const bool valid = (unsigned)row < (unsigned)a.n;
        int any = 0;
        if (valid) {
            const float* z = a.poses + (size_t)row * a.n_out * 3;
            for (int j = 0; j < a.n_out; ++j)
                any |= __builtin_isfinite(z[j * 3]) && __builtin_isfinite(z[j * 3 + 1]) && __builtin_isfinite(z[j * 3 + 2]);
        }
        l.box_row[k] = valid ? row : -1;
        l.box_any[k] = any;
        l.box_slot[k] = -1;
        l.box_cost[k] = __builtin_nanf("");
    }
}

// the cost of slot `slot` continuing in pose row `row` at the step's time
__host__ __device__ inline float assoc_pair_cost(const AssocArgs& a, int slot, int row, double t_step) {
    double sum = 0.0, seen = -__builtin_inf();
    int cnt = 0;
    for (int j = 0; j < a.n_out; ++j) {
        const double* st = assoc_slot_state(a, a.ws, slot, j);
        const double tl = st[27];
        if (tl != tl) continue;
        if (tl > seen) seen = tl;
        const float* z = a.poses + ((size_t)row * a.n_out + j) * 3;
        if (!(__builtin_isfinite(z[0]) && __builtin_isfinite(z[1]) && __builtin_isfinite(z[2]))) continue;
        double dt = t_step - tl;
        if (!(dt > 0.0)) dt = 0.0;
        const double e0 = (double)z[0] - (st[0] + dt * st[3]), e1 = (double)z[1] - (st[1] + dt * st[4]),
                     e2 = (double)z[2] - (st[2] + dt * st[5]);
        double d = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        if (!(d <= a.clip)) d = a.clip;
        sum += d * d;
        ++cnt;
    }
    if (cnt < a.min_joints || cnt < 1 || seen < t_step - a.max_age) return __builtin_inff();
    return (float)sqrt(sum / (double)cnt);
}

__host__ __device__ inline void assoc_costs(const AssocArgs& a, AssocLds& l, int m, double t_step, int tid, int nt) {
    const int dq = nt / m, dr = nt - dq * m;
    int t = tid / m, k = tid - t * m;
    while (t < a.n_tracks) {
        l.c[t * ASSOC_LD + k] = l.box_row[k] >= 0 ? assoc_pair_cost(a, t, l.box_row[k], t_step) : __builtin_inff();
        t += dq;
        k += dr;
        if (k >= m) { k -= m; ++t; }
    }
}

// this thread's smallest (value, slot, position)
__host__ __device__ inline AssocCand assoc_scan(const AssocLds& l, int n_tracks, int m, int tid, int nt) {
    AssocCand best = {__builtin_inff(), 0x7fffffff};
    const int dq = nt / m, dr = nt - dq * m;
    int t = tid / m, k = tid - t * m;
    while (t < n_tracks) {
        const AssocCand x = {l.c[t * ASSOC_LD + k], t * ASSOC_LD + k};
        if (assoc_cand_less(x, best)) best = x;
        t += dq;
        k += dr;
        if (k >= m) { k -= m; ++t; }
    }
    return best;
}

// the pick (slot t, position k): the box is the slot's, its row and its column leave the matrix
__host__ __device__ inline void assoc_strike(AssocLds& l, int n_tracks, int m, AssocCand best, int tid, int nt) {
    const int t = best.idx / ASSOC_LD, k = best.idx - t * ASSOC_LD;
    const int span = n_tracks > m ? n_tracks : m;
    for (int i = tid; i < span; i += nt) {
        if (i < m) l.c[t * ASSOC_LD + i] = __builtin_inff();
        if (i < n_tracks) l.c[i * ASSOC_LD + k] = __builtin_inff();
    }
    if (tid == 0) {
        l.box_slot[k] = t;
        l.box_cost[k] = best.v;
    }
}

// the r-th unassigned box with a finite joint takes the r-th free slot and the id next_id + r
__host__ __device__ inline void assoc_births(const AssocArgs& a, AssocLds& l, int m, int tid, int nt) {
    for (int k = tid; k < m; k += nt) {
        l.born_slot[k] = -1;
        l.born_id[k] = -1;
        if (l.box_row[k] < 0 || l.box_slot[k] >= 0 || !l.box_any[k]) continue;
        int r = 0;
        for (int i = 0; i < k; ++i) r += l.box_row[i] >= 0 && l.box_slot[i] < 0 && l.box_any[i];
        int free_seen = 0;
        for (int t = 0; t < a.n_tracks; ++t) {
            if (l.ids[t] >= 0) continue;
            if (free_seen == r) {
                l.born_slot[k] = t;
                l.born_id[k] = l.next_id + r;
                break;
            }
            ++free_seen;
        }
    }
}

// the births into the table, the counters, and the step's outputs per box
__host__ __device__ inline void assoc_apply(const AssocArgs& a, AssocLds& l, int m, int tid, int nt) {
    if (tid == 0) {                                        // reads only what this step no longer writes
        int born = 0, untracked = 0;
        for (int k = 0; k < m; ++k) {
            if (l.box_row[k] < 0) continue;
            const bool matched = l.box_cost[k] == l.box_cost[k];
            born += l.born_slot[k] >= 0;
            untracked += !matched && l.born_slot[k] < 0;
        }
        l.next_id += born;
        l.n_new += born;
        l.n_dropped += untracked;
    }
    for (int k = tid; k < m; k += nt) {
        const int row = l.box_row[k];
        if (row < 0) continue;
        int slot = l.box_slot[k];
        if (l.born_slot[k] >= 0) {
            slot = l.born_slot[k];
            l.box_slot[k] = slot;
            l.ids[slot] = l.born_id[k];
        }
        if (slot < 0) continue;                            // untracked: as assoc_begin left it
        a.track_index[row] = slot;
        a.track_id[row] = l.ids[slot];
        a.cost_out[row] = l.box_cost[k];
        l.count[slot] += 1;                                // one box per slot and step: no other thread is here
    }
}

// every slot that received a box advances its working state, one (box, joint) per item
__host__ __device__ inline void assoc_filter(const AssocArgs& a, const AssocLds& l, int m, int tid, int nt) {
    for (int i = tid; i < m * a.n_out; i += nt) {
        const int k = i / a.n_out, j = i - k * a.n_out;
        const int slot = l.box_slot[k], row = l.box_row[k];
        if (slot < 0 || row < 0) continue;
        double* st = assoc_slot_state(a, a.ws, slot, j);
        SmoothKf s, pred;
        double t_prev = 0.0;
        bool have = smooth_state_load(st, s, t_prev), used;
        if (smooth_filter_row(a, (size_t)row * a.n_out + j, a.times[row], s, pred, t_prev, have, used)) smooth_state_store(st, s, t_prev);
    }
}

// the CSR offsets from the boxes each slot received
__host__ __device__ inline void assoc_starts(const AssocArgs& a, AssocLds& l, int tid, int nt) {
    if (tid != 0) return;
    int at = 0;
    for (int t = 0; t < a.n_tracks; ++t) {
        l.start[t] = a.starts_out[t] = at;
        at += l.count[t];
    }
    l.start[a.n_tracks] = a.starts_out[a.n_tracks] = at;
}

// the step's tracked boxes into their slots' groups: steps come in time order, so every group is time-sorted
__host__ __device__ inline void assoc_group_step(const AssocArgs& a, AssocLds& l, int lo, int m, int tid, int nt) {
    for (int k = tid; k < m; k += nt) {
        const int row = a.step_rows[lo + k];
        if ((unsigned)row >= (unsigned)a.n) continue;
        const int slot = a.track_index[row];
        if ((unsigned)slot >= (unsigned)a.n_tracks) continue;
        const int at = l.start[slot] + l.fill[slot];
        if (at < l.start[slot + 1] && at < a.n) a.rows_out[at] = row;
        l.fill[slot] += 1;
    }
}

__host__ __device__ inline void assoc_finish(const AssocArgs& a, const AssocLds& l, int tid, int nt) {
    for (int i = l.start[a.n_tracks] + tid; i < a.n; i += nt) a.rows_out[i] = -1;
    for (int t = tid; t < a.n_tracks; t += nt) a.ids[t] = l.ids[t];
    if (tid == 0) {
        a.next_id[0] = l.next_id;
        a.n_new[0] = l.n_new;
        a.n_dropped[0] = l.n_dropped;
    }
}

// ---- the optimal assignment (metro_associate_tracks_optimal): the block between assoc_costs and assoc_births ----
// The one-to-one set of admissible pairs (c < max_cost) of the largest total gain sum (max_cost - c): the linear assignment
// problem with one extra column of unlimited capacity at cost max_cost that means "unmatched".  Shortest augmenting paths
// (Jonker-Volgenant): one Dijkstra per box, in step order, over the T slot columns and that sink, on the costs reduced by the
// dual potentials u (boxes) and v (slots; the sink's stays 0); potentials and path lengths in fp64 on the fp32 costs.  A visit
// relaxes the columns from the box of the column reached last and takes the nearest unvisited one (ties: the lowest slot; a
// slot before the sink).  The search ends at a free slot or at the sink; a box that went to the sink is never searched
// through again (its way out, the sink, stays the cheapest).  Every thread keeps its own copy of the search (AssocPath), equal
// in all of them; thread t owns column t of dist / way / used.  At most T + 1 visits per box, T steps back along a path.

struct AssocOptLds {
    double u[ASSOC_MAX];                                 // potential of the box at a position
    double v[ASSOC_MAX];                                 // potential of a slot, <= 0
    double dist[ASSOC_MAX];                              // length of the shortest path found so far to a slot
    int way[ASSOC_MAX];                                  // the slot before it on that path, -1: the searching box itself
    int used[ASSOC_MAX];                                 // the slot was visited in this search
    int slot_box[ASSOC_MAX];                             // the position matched to a slot, -1: free
};

struct AssocCandD { double v; int idx; };

struct AssocPath {
    int row;                                             // the box whose costs the next visit relaxes
    int col;                                             // the slot reached last, -1: none yet
    double base;                                         // its distance
    double sink;                                         // the shortest way into the sink so far
    int sink_from;                                       // the slot it leaves from, -1: the searching box itself
    int end;                                             // -2: searching, -1: ended in the sink, >= 0: ended in this free slot
};

__host__ __device__ inline bool assoc_cand_less(const AssocCandD& x, const AssocCandD& y) {
    return x.v < y.v || (x.v == y.v && x.idx < y.idx);
}

__host__ __device__ inline void assoc_opt_begin(const AssocArgs& a, AssocOptLds& o, int m, int tid, int nt) {
    const int span = a.n_tracks > m ? a.n_tracks : m;
    for (int i = tid; i < span; i += nt) {
        if (i < m) o.u[i] = 0.0;
        if (i < a.n_tracks) {
            o.v[i] = 0.0;
            o.slot_box[i] = -1;
        }
    }
}

// the search of box k starts: no column reached
__host__ __device__ inline AssocPath assoc_opt_root(const AssocArgs& a, AssocOptLds& o, int k, int tid, int nt) {
    for (int t = tid; t < a.n_tracks; t += nt) {
        o.dist[t] = __builtin_inf();
        o.way[t] = -1;
        o.used[t] = 0;
    }
    const AssocPath p = {k, -1, 0.0, __builtin_inf(), -1, -2};
    return p;
}

// one visit: the column reached last is marked, the others and the sink are relaxed from the path's box
// -> this thread's nearest unvisited column
__host__ __device__ inline AssocCandD assoc_opt_relax(const AssocArgs& a, const AssocLds& l, AssocOptLds& o, AssocPath& p, int tid, int nt) {
    const double ur = o.u[p.row];
    const double to_sink = (p.base + (double)a.max_cost) - ur;
    if (to_sink < p.sink) {
        p.sink = to_sink;
        p.sink_from = p.col;
    }
    AssocCandD best = {__builtin_inf(), 0x7fffffff};
    for (int t = tid; t < a.n_tracks; t += nt) {
        if (t == p.col) o.used[t] = 1;
        if (o.used[t]) continue;
        const float c = l.c[t * ASSOC_LD + p.row];
        if (c < a.max_cost) {
            const double nd = ((p.base + (double)c) - ur) - o.v[t];
            if (nd < o.dist[t]) {
                o.dist[t] = nd;
                o.way[t] = p.col;
            }
        }
        const AssocCandD x = {o.dist[t], t};
        if (assoc_cand_less(x, best)) best = x;
    }
    return best;
}

// the workgroup's nearest unvisited column against the sink; the same in every thread
__host__ __device__ inline void assoc_opt_advance(const AssocArgs& a, const AssocOptLds& o, AssocPath& p, AssocCandD best) {
    if (!((unsigned)best.idx < (unsigned)a.n_tracks) || !(best.v <= p.sink)) {
        p.end = -1;
        return;
    }
    p.col = best.idx;
    p.base = best.v;
    const int k = o.slot_box[best.idx];
    if ((unsigned)k < (unsigned)ASSOC_MAX) p.row = k;
    else p.end = best.idx;
}

// the potentials after a search that ended at distance p.end's: visited columns and their boxes move by what the path to
// them was shorter; a search that found no end (a matrix without sense) changes nothing
__host__ __device__ inline void assoc_opt_duals(const AssocArgs& a, AssocOptLds& o, const AssocPath& p, int k, int tid, int nt) {
    if (p.end == -2) return;
    const double d_end = p.end >= 0 ? p.base : p.sink;
    for (int t = tid; t < a.n_tracks; t += nt) {
        if (!o.used[t]) continue;
        const double d = d_end - o.dist[t];
        o.v[t] -= d;
        const int kb = o.slot_box[t];
        if ((unsigned)kb < (unsigned)ASSOC_MAX) o.u[kb] += d;
    }
    if (tid == 0) o.u[k] += d_end;
}

// the path back from its end to box k: every slot on it takes the box of the slot before it, the first one box k
__host__ __device__ inline void assoc_opt_augment(const AssocArgs& a, AssocOptLds& o, const AssocPath& p, int k, int tid) {
    if (tid != 0 || p.end == -2) return;
    int t = p.end >= 0 ? p.end : p.sink_from;
    for (int hop = 0; hop < a.n_tracks && (unsigned)t < (unsigned)a.n_tracks; ++hop) {
        const int before = o.way[t];
        o.slot_box[t] = (unsigned)before < (unsigned)a.n_tracks ? o.slot_box[before] : k;
        t = before;
    }
}

// box_slot and box_cost as assoc_strike leaves them
__host__ __device__ inline void assoc_opt_pairs(const AssocArgs& a, AssocLds& l, const AssocOptLds& o, int m, int tid, int nt) {
    for (int t = tid; t < a.n_tracks; t += nt) {
        const int k = o.slot_box[t];
        if ((unsigned)k >= (unsigned)m) continue;
        l.box_slot[k] = t;
        l.box_cost[k] = l.c[t * ASSOC_LD + k];
    }
}

// ---- the same walk with RAY rows among the point rows (metro_associate_tracks_rays) ----
// A row b with single_box[b] >= 0 is a person one camera sees: it has no point, but one ray per joint, rays[b][j] = o (3), d (3),
// sigma2, views (metro_person_rays).  Point rows go through the steps above unchanged; for a ray row
//   cost      per slot: the RMS over the joints of the distance of the predicted joint p^ = p + dt v from the ray, min(|w - tau d|,
//             clip) with w = p^ - o, tau = d . w, and clip itself behind the camera (!(tau > 0)).  The cost is BLIND ALONG THE RAY:
//             a track anywhere on the ray costs 0, so of two tracks in line with the camera either may be taken.
//   births    never: a ray has no depth to start a state from.  Unassigned, the row is untracked and counted in n_unplaced, not
//             in n_dropped.
//   place     (new, between apply and filter) per assigned ray row and joint whose slot joint has a state, whose ray is finite
//             and with tau > 0 from the same p^ on the working state before this step's filter: z = o + tau d, the foot of the
//             perpendicular from p^ onto the ray, and R = sigma2 tau^2 (I - d d^T) + depth_sigma^2 d d^T -- tight across the ray,
//             wide along it, the linearised (EKF) form of a bearing measurement -- each rounded once to fp32 into poses[b][j]
//             and cov[b][j]; tau goes to ray_depth.  A joint not placed keeps the NaN the triangulation left.
//   filter    unchanged: smooth_filter_row reads the fp32 arrays it always reads, so metro_smooth_tracks on the CSR and the
//             arrays this launch wrote leaves the working state, bit for bit.  A placed joint whose ROUNDED R fails smooth_pd3
//             is predict-only (used 0): the safe outcome.
// AssocLds, AssocArgs and AssocOptLds keep their layout; the additions live in AssocRayArgs (metro_common.h) and AssocRayLds, and
// a walk without ray rows (assoc_walk<.., false>) neither calls a step of this section nor touches an AssocRayLds.

constexpr int ASSOC_RAY_DOUBLES = 8;

struct AssocRayLds {
    int box_ray[ASSOC_MAX];                              // the position holds a ray row
    int n_unplaced;
};

__host__ __device__ inline void assoc_ray_begin(const AssocRayArgs& a, AssocRayLds& r, int tid, int nt) {
    const size_t total = (size_t)a.n * a.n_out;
    for (size_t i = tid; i < total; i += nt) a.ray_depth[i] = __builtin_nanf("");
    if (tid == 0) r.n_unplaced = 0;
}

// after assoc_step_boxes, by the same thread per position: which boxes are ray rows; such a row is never born
__host__ __device__ inline void assoc_ray_step_boxes(const AssocRayArgs& a, AssocLds& l, AssocRayLds& r, int m, int tid, int nt) {
    for (int k = tid; k < m; k += nt) {
        const int row = l.box_row[k];
        r.box_ray[k] = row >= 0 && a.single_box[row] >= 0;
        if (r.box_ray[k]) l.box_any[k] = 0;
    }
}

// false: no finite ray
__host__ __device__ inline bool assoc_ray_load(const AssocRayArgs& a, int row, int j, const double*& ray) {
    ray = a.rays + ((size_t)row * a.n_out + j) * ASSOC_RAY_DOUBLES;
    bool fin = true;
    for (int e = 0; e < 7; ++e) fin = fin && __builtin_isfinite(ray[e]);
    return fin;
}

// the predicted joint against the ray: tau = d . (p^ - o) and the distance of p^ from the line
__host__ __device__ inline void assoc_ray_foot(const double* st, const double* ray, double t_step, double& tau, double& dist) {
    double dt = t_step - st[27];
    if (!(dt > 0.0)) dt = 0.0;
    const double w0 = (st[0] + dt * st[3]) - ray[0], w1 = (st[1] + dt * st[4]) - ray[1], w2 = (st[2] + dt * st[5]) - ray[2];
    tau = (ray[3] * w0 + ray[4] * w1) + ray[5] * w2;
    const double e0 = w0 - tau * ray[3], e1 = w1 - tau * ray[4], e2 = w2 - tau * ray[5];
    dist = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
}

// the cost of slot `slot` continuing in ray row `row` at the step's time
__host__ __device__ inline float assoc_ray_pair_cost(const AssocRayArgs& a, int slot, int row, double t_step) {
    double sum = 0.0, seen = -__builtin_inf();
    int cnt = 0;
    for (int j = 0; j < a.n_out; ++j) {
        const double* st = assoc_slot_state(a, a.ws, slot, j);
        const double tl = st[27];
        if (tl != tl) continue;
        if (tl > seen) seen = tl;
        const double* ray;
        if (!assoc_ray_load(a, row, j, ray)) continue;
        double tau, d;
        assoc_ray_foot(st, ray, t_step, tau, d);
        if (!(tau > 0.0) || !(d <= a.clip)) d = a.clip;
        sum += d * d;
        ++cnt;
    }
    if (cnt < a.min_joints || cnt < 1 || seen < t_step - a.max_age) return __builtin_inff();
    return (float)sqrt(sum / (double)cnt);
}

// after assoc_costs, in its order (the same thread owns the same entry): the columns of the ray rows
__host__ __device__ inline void assoc_ray_costs(const AssocRayArgs& a, AssocLds& l, const AssocRayLds& r, int m, double t_step, int tid,
                                                int nt) {
    const int dq = nt / m, dr = nt - dq * m;
    int t = tid / m, k = tid - t * m;
    while (t < a.n_tracks) {
        if (r.box_ray[k]) l.c[t * ASSOC_LD + k] = assoc_ray_pair_cost(a, t, l.box_row[k], t_step);
        t += dq;
        k += dr;
        if (k >= m) { k -= m; ++t; }
    }
}

// after assoc_apply: an unassigned ray row is unplaced, not dropped
__host__ __device__ inline void assoc_ray_count(AssocLds& l, AssocRayLds& r, int m, int tid) {
    if (tid != 0) return;
    int unplaced = 0;
    for (int k = 0; k < m; ++k) unplaced += l.box_row[k] >= 0 && r.box_ray[k] && l.box_slot[k] < 0;
    r.n_unplaced += unplaced;
    l.n_dropped -= unplaced;
}

// every assigned ray row becomes a point measurement per joint, one (box, joint) per item
__host__ __device__ inline void assoc_ray_place(const AssocRayArgs& a, const AssocLds& l, const AssocRayLds& r, int m, double t_step,
                                                int tid, int nt) {
    for (int i = tid; i < m * a.n_out; i += nt) {
        const int k = i / a.n_out, j = i - k * a.n_out;
        const int slot = l.box_slot[k], row = l.box_row[k];
        if (!r.box_ray[k] || slot < 0 || row < 0) continue;
        const double* st = assoc_slot_state(a, a.ws, slot, j);
        if (st[27] != st[27]) continue;
        const double* ray;
        if (!assoc_ray_load(a, row, j, ray)) continue;
        double tau, dist;
        assoc_ray_foot(st, ray, t_step, tau, dist);
        if (!(tau > 0.0)) continue;
        const size_t at = (size_t)row * a.n_out + j;
        const double lateral = ray[6] * (tau * tau);
        for (int c = 0; c < 3; ++c) {
            a.poses_w[at * 3 + c] = (float)(ray[c] + tau * ray[3 + c]);
            for (int e = 0; e < 3; ++e) {
                const double dd = ray[3 + c] * ray[3 + e];
                a.cov_w[at * 9 + c * 3 + e] = (float)(lateral * ((c == e ? 1.0 : 0.0) - dd) + a.depth_var * dd);
            }
        }
        a.ray_depth[at] = (float)tau;
    }
}

__host__ __device__ inline void assoc_ray_finish(const AssocRayArgs& a, const AssocRayLds& r, int tid) {
    if (tid == 0) a.n_unplaced[0] = r.n_unplaced;
}

// ---- the walk: the order of the steps and the barriers between them, for every rule, with and without ray rows ----
// A TEAM executes it: `tid` of `nt` for the steps, sync() where every member must have finished the step before, and least(x),
// the smallest candidate any member holds (the same value in all of them).  search() marks where the search of one box starts;
// only a team that counts the visits of a search does anything there.

template <bool RAYS>
using AssocWalkArgs = std::conditional_t<RAYS, AssocRayArgs, AssocArgs>;

// `o` is touched under OPTIMAL only and `r` under RAYS only
template <bool OPTIMAL, bool RAYS, class Team>
__host__ __device__ inline void assoc_walk(const AssocWalkArgs<RAYS>& a, AssocLds& l, AssocOptLds& o, AssocRayLds& r, Team& team) {
    const int tid = team.tid, nt = team.nt;
    assoc_begin(a, l, tid, nt);
    if constexpr (RAYS) assoc_ray_begin(a, r, tid, nt);
    team.sync();
    double t_first = 0.0;
    const bool have_first = assoc_first_time(a, t_first);
    assoc_retire(a, l, have_first, t_first, tid, nt);
    team.sync();
    for (int s = 0; s < a.n_steps; ++s) {                  // every branch below is taken by all members or by none
        int lo, m;
        double t_step;
        assoc_step_range(a, s, lo, m);
        if (!assoc_step_time(a, lo, m, t_step)) continue;
        assoc_step_boxes(a, l, lo, m, tid, nt);
        if constexpr (RAYS) assoc_ray_step_boxes(a, l, r, m, tid, nt);
        if constexpr (OPTIMAL) assoc_opt_begin(a, o, m, tid, nt);
        team.sync();
        assoc_costs(a, l, m, t_step, tid, nt);
        if constexpr (RAYS) assoc_ray_costs(a, l, r, m, t_step, tid, nt);
        team.sync();
        if constexpr (OPTIMAL) {
            for (int k = 0; k < m; ++k) {
                team.search();
                AssocPath p = assoc_opt_root(a, o, k, tid, nt);
                for (int visit = 0; visit <= a.n_tracks && p.end == -2; ++visit) {
                    const AssocCandD best = team.least(assoc_opt_relax(a, l, o, p, tid, nt));
                    assoc_opt_advance(a, o, p, best);
                }
                assoc_opt_duals(a, o, p, k, tid, nt);
                team.sync();                               // the duals read slot_box before the path rewrites it
                assoc_opt_augment(a, o, p, k, tid);
                team.sync();
            }
            assoc_opt_pairs(a, l, o, m, tid, nt);
            team.sync();
        } else {
            const int rounds = a.n_tracks < m ? a.n_tracks : m;
            for (int round = 0; round < rounds; ++round) {
                const AssocCand best = team.least(assoc_scan(l, a.n_tracks, m, tid, nt));
                if (!(best.v < a.max_cost)) break;
                assoc_strike(l, a.n_tracks, m, best, tid, nt);
                team.sync();                               // also: least() may not be entered again before every member has read its result
            }
        }
        assoc_births(a, l, m, tid, nt);
        team.sync();
        assoc_apply(a, l, m, tid, nt);
        team.sync();
        if constexpr (RAYS) {
            assoc_ray_count(l, r, m, tid);
            assoc_ray_place(a, l, r, m, t_step, tid, nt);
            team.sync();
        }
        assoc_filter(a, l, m, tid, nt);
        team.sync();                                       // the working state and the box arrays, before the next step
    }
    assoc_starts(a, l, tid, nt);
    team.sync();
    for (int s = 0; s < a.n_steps; ++s) {
        int lo, m;
        assoc_step_range(a, s, lo, m);
        if (m == 0) continue;
        assoc_group_step(a, l, lo, m, tid, nt);
        team.sync();
    }
    assoc_finish(a, l, tid, nt);
    if constexpr (RAYS) assoc_ray_finish(a, r, tid);
}

// The kernel's team: the workgroup.  least() is a 64-lane __shfl_xor ladder, then one candidate per wave through LDS and ONE
// barrier.  The greedy rule has a single set of them: the barrier after assoc_strike is what keeps a wave from writing the next
// round's candidate while another still reads this round's.  A visit of the optimal search has no other barrier, so its
// candidates go through two sets in turn: a wave can be at most one visit ahead of the slowest, and writes the other set.
template <bool OPTIMAL>
struct AssocWaveBest { std::conditional_t<OPTIMAL, AssocCandD, AssocCand> of[OPTIMAL ? 2 : 1][ASSOC_THREADS / 64]; };

template <bool OPTIMAL>
struct AssocWorkgroup {
    AssocWaveBest<OPTIMAL>& wave_best;                     // in LDS
    const int tid;
    static constexpr int nt = ASSOC_THREADS;
    int turn = 0;

    __device__ void sync() const { __syncthreads(); }
    __device__ void search() const {}
    template <class Cand>
    __device__ Cand least(Cand best) {
        for (int off = 32; off > 0; off >>= 1) {
            const Cand other = {__shfl_xor(best.v, off), __shfl_xor(best.idx, off)};
            if (assoc_cand_less(other, best)) best = other;
        }
        if ((tid & 63) == 0) wave_best.of[turn][tid >> 6] = best;
        __syncthreads();
        best = wave_best.of[turn][0];
        for (int w = 1; w < ASSOC_THREADS / 64; ++w)
            if (assoc_cand_less(wave_best.of[turn][w], best)) best = wave_best.of[turn][w];
        if constexpr (OPTIMAL) turn ^= 1;
        return best;
    }
};

template <bool OPTIMAL, bool RAYS>
__global__ __launch_bounds__(ASSOC_THREADS) void associate_tracks_kernel(AssocWalkArgs<RAYS> a) {
    __shared__ AssocLds l;
    __shared__ AssocOptLds o;                              // allocated where the walk touches them only:
    __shared__ AssocRayLds r;                              // o with OPTIMAL, r with RAYS
    __shared__ AssocWaveBest<OPTIMAL> wave_best;
    AssocWorkgroup<OPTIMAL> team = {wave_best, (int)threadIdx.x};
    assoc_walk<OPTIMAL, RAYS>(a, l, o, r, team);
}

size_t associate_tracks_workspace_bytes(int n_tracks, int n_out) {
    return (size_t)(n_tracks > 0 ? n_tracks : 0) * (size_t)(n_out > 0 ? n_out : 0) * SMOOTH_STATE_DOUBLES * sizeof(double);
}

template <bool OPTIMAL, bool RAYS>
static int launch_assoc(const AssocWalkArgs<RAYS>& a, const char* id, hipStream_t stream) {
    if (note_kernel("%s", id)) return METRO_OK;
    hipLaunchKernelGGL((associate_tracks_kernel<OPTIMAL, RAYS>), dim3(1), dim3(ASSOC_THREADS), 0, stream, a);
    return launch_status(id);
}

int launch_associate_tracks(const AssocArgs& a, bool optimal, hipStream_t stream) {
    return optimal ? launch_assoc<true, false>(a, "associate_tracks_optimal", stream)
                   : launch_assoc<false, false>(a, "associate_tracks", stream);
}

int launch_associate_tracks_rays(const AssocRayArgs& a, bool optimal, hipStream_t stream) {
    return optimal ? launch_assoc<true, true>(a, "associate_tracks_rays_optimal", stream)
                   : launch_assoc<false, true>(a, "associate_tracks_rays", stream);
}

}  // namespace metro
