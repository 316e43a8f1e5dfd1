// Per-joint heat-map modes of a forward whose plan has mode buffers bound (metro_plan_bind_modes, include/metro_hip.h, which holds
// the definition).  logits NHWC [n, S, S, C = D*J], channel c = d*J + j; l[y, x, d] the logits of one (crop, head joint), v = (y*S + x)*D + d,
// p = exp(l - M) / sum exp(l - M).  Per (crop, OUTPUT joint r, head joint perm[r]) the K places the joint may be:
//   candidates   voxels with a finite logit that beat every neighbour (up to 26, clipped to the volume; an equal neighbour only if it
//                has the higher index: a plateau has one candidate, its lowest index)
//   selection    candidates by decreasing logit (ties: increasing v), skipping those within 2R (Chebyshev) of a selected mode
//   per mode     mass, peak, coords01 and cov01 of p over the window of radius R, clipped to the volume
// One launch, one workgroup of 256 threads per (crop, output joint), the joint index fastest in the grid.  modes_walk below is the
// whole body, written for a TEAM (tid of nt, sync, max / sum / best over the team, and groups of lanes with a sum of their own): the
// kernel's team is the workgroup (64-lane __shfl_xor ladders, one LDS record per wave), the host tests' team is one thread
// (tests/test_heat_modes.py compiles this file for the host and walks it).  Three phases:
//   1  the joint's maximum M and normaliser: thread t takes voxels t, t + nt, ...; ladder; the four waves' records in order.
//   2  one candidate flag per voxel (a byte in LDS) from the logits staged in LDS in y-slabs with one halo row on each side; a
//      volume that fits is staged whole, once, and phase 1 reads it there too.
//   3  K rounds of "largest unselected, unsuppressed candidate": a thread keeps the best of its own flag words and rescans them
//      only after a round that suppressed it (the flags are never rewritten: suppression is tested against the selected list);
//      then wave w sums the windows of modes w, w + 4: first mass and first moments, then the six central moments about the mean.
// Sums: AccT = fp32 on f16 plans, fp64 on f32 / f32m / f64 plans (LogitT fp64 on f64 plans); fixed order, no atomics; the
// comparisons are on the stored logits, so the selected voxels are the same in every precision.  Each output is rounded to fp32 once.
// Non-finite logits: NaN or +Inf makes the normaliser NaN -> all K modes of that joint are voxel -1 with NaN floats; -Inf is a
// voxel of weight zero that is never a candidate.
#include "metro_common.h"

#pragma clang fp contract(off)

namespace metro {

#define MD_HD __host__ __device__ __forceinline__

constexpr int MD_THREADS = 256;
constexpr int MD_NONE = 0x7fffffff;          // "no candidate": loses to every voxel index
constexpr int MD_STATS = 11;                 // mass, peak, coords01 (3), cov01 (6)
constexpr int MD_LDS_HEAD = 128;             // wave records (64 B), the selected voxels (32 B)
constexpr int MD_LDS_MAX = 64 * 1024;

MD_HD float md_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __expf(x);
#else
    return expf(x);
#endif
}
MD_HD double md_exp(double x) { return exp(x); }

// the soft-argmax's grid: fp32 linspace(0, 1, k), fp32 step and fp32 product (one point: 0)
MD_HD float md_grid(int i, int k) { return k > 1 ? (float)i * (1.0f / (float)(k - 1)) : 0.0f; }

template <typename LogitT>
struct ModeCand { LogitT l; int v; };
// the order of the selection: decreasing logit, ties by increasing voxel index
template <typename LogitT>
MD_HD bool md_before(const ModeCand<LogitT>& a, const ModeCand<LogitT>& b) { return a.l > b.l || (a.l == b.l && a.v < b.v); }

// `rows`: nrows consecutive y-rows [nrows][S][D] of one joint's volume, clipped to it (row 0 or row nrows - 1 is the volume's edge
// wherever no further row was staged); is voxel (ly, x, d) of them a candidate?
template <typename LogitT>
MD_HD bool md_candidate(const LogitT* rows, int ly, int nrows, int x, int d, int S, int D) {
    const LogitT c = rows[((size_t)ly * S + x) * D + d];
    if (!(c > (LogitT)-INFINITY && c < (LogitT)INFINITY)) return false;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = ly + dy;
        if (yy < 0 || yy >= nrows) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= S) continue;
            for (int dd = -1; dd <= 1; ++dd) {
                const int zz = d + dd;
                if (zz < 0 || zz >= D || (dy == 0 && dx == 0 && dd == 0)) continue;
                const LogitT u = rows[((size_t)yy * S + xx) * D + zz];
                const bool later = dy > 0 || (dy == 0 && (dx > 0 || (dx == 0 && dd > 0)));          // u > v in linear index
                if (!(u < c || (u == c && later))) return false;
            }
        }
    }
    return true;
}

MD_HD int md_abs(int a) { return a < 0 ? -a : a; }
// is voxel v within 2R (in every axis) of the selected voxel s?
MD_HD bool md_suppressed(int v, int s, int radius, int S, int D) {
    const int dy = md_abs(v / (S * D) - s / (S * D)), dx = md_abs(v / D % S - s / D % S), dd = md_abs(v % D - s % D);
    return dy <= 2 * radius && dx <= 2 * radius && dd <= 2 * radius;
}

// y-rows a slab holds besides its two halo rows: S when the whole volume fits (no halo then), 0 when not even one row does
MD_HD int md_flag_bytes(int S, int D) { return (S * S * D + 15) & ~15; }
MD_HD int md_slab_rows(int S, int D, int logit_bytes) {
    const long avail = (long)MD_LDS_MAX - MD_LDS_HEAD - md_flag_bytes(S, D);
    if (avail <= 0) return 0;
    const long fit = avail / ((long)S * D * logit_bytes);
    if (fit >= S) return S;
    return fit >= 3 ? (int)fit - 2 : 0;
}
MD_HD int md_staged_rows(int S, int slab_rows) { return slab_rows + 2 < S ? slab_rows + 2 : S; }
MD_HD size_t md_lds_bytes(int S, int D, int logit_bytes, int slab_rows) {
    return (size_t)MD_LDS_HEAD + md_flag_bytes(S, D) + (size_t)md_staged_rows(S, slab_rows) * S * D * logit_bytes;
}

struct ModesArgs {
    const void* logits;
    int32_t* voxel;      // [n][n_out][K]
    float* stats;        // [n][n_out][K][11]
    int side, J, D, n_out, K, radius, slab_rows;
    int perm[METRO_MAX_JOINTS];
};

// voxel v of the joint whose first logit is `lg`: from the staged volume where it is staged whole, else from memory
template <typename LogitT>
MD_HD LogitT md_at(const LogitT* whole, const LogitT* lg, int v, int D, int C, int J) {
    return whole != nullptr ? whole[v] : lg[(size_t)(v / D) * C + (v % D) * J];
}

template <typename AccT, typename LogitT, class Team>
__host__ __device__ inline void modes_walk(const ModesArgs& a, int img, int r, char* lds, Team& team) {
    const int S = a.side, D = a.D, J = a.J, C = D * J, K = a.K, R = a.radius, row = S * D, vol = S * row;
    const int tid = team.tid, nt = team.nt;
    const LogitT* lg = static_cast<const LogitT*>(a.logits) + (size_t)img * S * S * C + a.perm[r];
    int* sel = reinterpret_cast<int*>(lds + 64);                                   // [METRO_MAX_MODES]
    unsigned char* flag = reinterpret_cast<unsigned char*>(lds + MD_LDS_HEAD);
    LogitT* slab = reinterpret_cast<LogitT*>(lds + MD_LDS_HEAD + md_flag_bytes(S, D));
    int32_t* vox_out = a.voxel + ((size_t)img * a.n_out + r) * K;
    float* st_out = a.stats + ((size_t)img * a.n_out + r) * K * MD_STATS;
    const bool staged_whole = a.slab_rows >= S;
    const LogitT* whole = staged_whole ? slab : nullptr;
    if (staged_whole) {
        for (int v = tid; v < vol; v += nt) slab[v] = lg[(size_t)(v / D) * C + (v % D) * J];
        team.sync();
    }

    // ---- 1: maximum and normaliser ----
    AccT m = (AccT)-INFINITY;
    for (int v = tid; v < vol; v += nt) {
        const AccT x = (AccT)md_at(whole, lg, v, D, C, J);
        m = x > m ? x : m;
    }
    const AccT M = team.max(m);
    const AccT mr = M == (AccT)-INFINITY ? (AccT)0 : M;          // nothing but -Inf: exponents about 0, the sum is 0
    AccT s = 0;
    for (int v = tid; v < vol; v += nt) s += md_exp((AccT)md_at(whole, lg, v, D, C, J) - mr);
    const AccT total = team.sum(s);
    const AccT inv_s = (AccT)1 / total;
    if (total != total) {                                          // a NaN or +Inf logit: no distribution, no modes
        for (int i = tid; i < K * MD_STATS; i += nt) st_out[i] = NAN;
        for (int i = tid; i < K; i += nt) vox_out[i] = -1;
        return;
    }

    // ---- 2: candidate flags ----
    const int step = staged_whole ? S : a.slab_rows;
    for (int y0 = 0; y0 < S; y0 += step) {
        const int y1 = y0 + step < S ? y0 + step : S;
        const int ya = y0 > 0 ? y0 - 1 : 0, yb = y1 < S ? y1 + 1 : S;
        if (!staged_whole) {
            team.sync();                                           // the slab before has been read
            for (int i = tid; i < (yb - ya) * row; i += nt) {
                const int v = ya * row + i;
                slab[i] = lg[(size_t)(v / D) * C + (v % D) * J];
            }
            team.sync();
        }
        for (int i = tid; i < (y1 - y0) * row; i += nt) {
            const int ly = i / row, rem = i - ly * row, x = rem / D, d = rem - x * D;
            flag[y0 * row + i] = md_candidate<LogitT>(slab, ly + (y0 - ya), yb - ya, x, d, S, D) ? 1 : 0;
        }
    }
    for (int i = vol + tid; i < md_flag_bytes(S, D); i += nt) flag[i] = 0;
    team.sync();

    // ---- 3: selection ----
    const ModeCand<LogitT> none = {(LogitT)-INFINITY, MD_NONE};
    ModeCand<LogitT> mine = none;
    bool stale = true;
    int n_sel = 0;
    const unsigned* flag4 = reinterpret_cast<const unsigned*>(flag);
    for (int k = 0; k < K; ++k) {                                  // every branch on `win` is taken by all members or by none
        if (stale) {
            mine = none;
            for (int w = tid; w < md_flag_bytes(S, D) / 4; w += nt) {
                const unsigned f = flag4[w];
                if (f == 0) continue;
                for (int b = 0; b < 4; ++b) {
                    if (((f >> (8 * b)) & 0xffu) == 0) continue;
                    const int v = w * 4 + b;
                    bool skip = false;
                    for (int q = 0; q < k; ++q) skip = skip || md_suppressed(v, sel[q], R, S, D);
                    if (skip) continue;
                    const ModeCand<LogitT> c = {md_at(whole, lg, v, D, C, J), v};
                    if (md_before(c, mine)) mine = c;
                }
            }
            stale = false;
        }
        const ModeCand<LogitT> win = team.best(mine);
        if (win.v == MD_NONE) break;
        if (tid == 0) sel[k] = win.v;
        n_sel = k + 1;
        if (mine.v != MD_NONE && md_suppressed(mine.v, win.v, R, S, D)) stale = true;
        team.sync();                                               // sel[k] is written; best() may be entered again
    }

    // ---- the windows ----
    for (int k = team.group; k < K; k += team.n_groups) {
        float* st = st_out + k * MD_STATS;
        if (k >= n_sel) {
            if (team.lane == 0) {
                vox_out[k] = -1;
                st[0] = 0.0f;
                for (int i = 1; i < MD_STATS; ++i) st[i] = NAN;
            }
            continue;
        }
        const int v0 = sel[k], cy = v0 / row, cx = v0 / D % S, cd = v0 % D;
        const int ylo = cy - R > 0 ? cy - R : 0, yhi = cy + R < S - 1 ? cy + R : S - 1;
        const int xlo = cx - R > 0 ? cx - R : 0, xhi = cx + R < S - 1 ? cx + R : S - 1;
        const int dlo = cd - R > 0 ? cd - R : 0, dhi = cd + R < D - 1 ? cd + R : D - 1;
        const int wx = xhi - xlo + 1, wd = dhi - dlo + 1, count = (yhi - ylo + 1) * wx * wd;
        AccT s0 = 0, sx = 0, sy = 0, sz = 0;
        for (int i = team.lane; i < count; i += team.lanes) {
            const int y = ylo + i / (wx * wd), x = xlo + i / wd % wx, d = dlo + i % wd;
            const AccT p = md_exp((AccT)md_at(whole, lg, (y * S + x) * D + d, D, C, J) - mr) * inv_s;
            s0 += p; sx += p * (AccT)md_grid(x, S); sy += p * (AccT)md_grid(y, S); sz += p * (AccT)md_grid(d, D);
        }
        s0 = team.group_sum(s0); sx = team.group_sum(sx); sy = team.group_sum(sy); sz = team.group_sum(sz);
        const AccT mx = sx / s0, my = sy / s0, mz = sz / s0;
        AccT cxx = 0, cyy = 0, czz = 0, cxy = 0, cxz = 0, cyz = 0;
        for (int i = team.lane; i < count; i += team.lanes) {
            const int y = ylo + i / (wx * wd), x = xlo + i / wd % wx, d = dlo + i % wd;
            const AccT p = md_exp((AccT)md_at(whole, lg, (y * S + x) * D + d, D, C, J) - mr) * inv_s;
            const AccT ex = (AccT)md_grid(x, S) - mx, ey = (AccT)md_grid(y, S) - my, ez = (AccT)md_grid(d, D) - mz;
            cxx += p * ex * ex; cyy += p * ey * ey; czz += p * ez * ez;
            cxy += p * ex * ey; cxz += p * ex * ez; cyz += p * ey * ez;
        }
        cxx = team.group_sum(cxx); cyy = team.group_sum(cyy); czz = team.group_sum(czz);
        cxy = team.group_sum(cxy); cxz = team.group_sum(cxz); cyz = team.group_sum(cyz);
        if (team.lane == 0) {
            vox_out[k] = v0;
            st[0] = (float)s0;
            st[1] = (float)(md_exp((AccT)md_at(whole, lg, v0, D, C, J) - mr) * inv_s);
            st[2] = (float)mx; st[3] = (float)my; st[4] = (float)mz;
            st[5] = (float)(cxx / s0); st[6] = (float)(cyy / s0); st[7] = (float)(czz / s0);
            st[8] = (float)(cxy / s0); st[9] = (float)(cxz / s0); st[10] = (float)(cyz / s0);
        }
    }
}

// The kernel's team: the workgroup.  max / sum / best: a 64-lane __shfl_xor ladder (every lane ends with the same bits: each
// step adds or compares the same two values in both lanes), one record per wave through LDS, folded in wave order by every
// thread.  max and sum end in a second barrier, so the records can be written again; best leaves that to the caller's sync.
struct ModesWorkgroup {
    char* rec;                                       // LDS, 64 bytes
    const int tid;
    static constexpr int nt = MD_THREADS, n_groups = MD_THREADS / 64, lanes = 64;
    const int group, lane;

    __device__ void sync() const { __syncthreads(); }
    template <typename T>
    __device__ T max(T x) const {
        for (int off = 32; off > 0; off >>= 1) {
            const T o = __shfl_xor(x, off);
            x = o > x ? o : x;
        }
        T* w = reinterpret_cast<T*>(rec);
        if (lane == 0) w[group] = x;
        __syncthreads();
        x = w[0];
        for (int g = 1; g < n_groups; ++g) x = w[g] > x ? w[g] : x;
        __syncthreads();
        return x;
    }
    template <typename T>
    __device__ T group_sum(T x) const {
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        return x;
    }
    template <typename T>
    __device__ T sum(T x) const {
        x = group_sum(x);
        T* w = reinterpret_cast<T*>(rec);
        if (lane == 0) w[group] = x;
        __syncthreads();
        x = w[0];
        for (int g = 1; g < n_groups; ++g) x += w[g];
        __syncthreads();
        return x;
    }
    template <typename LogitT>
    __device__ ModeCand<LogitT> best(ModeCand<LogitT> c) const {
        for (int off = 32; off > 0; off >>= 1) {
            const ModeCand<LogitT> o = {__shfl_xor(c.l, off), __shfl_xor(c.v, off)};
            if (md_before(o, c)) c = o;
        }
        ModeCand<LogitT>* w = reinterpret_cast<ModeCand<LogitT>*>(rec);
        if (lane == 0) w[group] = c;
        __syncthreads();
        c = w[0];
        for (int g = 1; g < n_groups; ++g)
            if (md_before(w[g], c)) c = w[g];
        return c;
    }
};

template <typename AccT, typename LogitT>
__global__ __launch_bounds__(MD_THREADS) void heat_modes_kernel(ModesArgs a) {
    extern __shared__ __attribute__((aligned(16))) char md_smem[];
    ModesWorkgroup team = {md_smem, (int)threadIdx.x, (int)threadIdx.x >> 6, (int)threadIdx.x & 63};
    modes_walk<AccT, LogitT>(a, blockIdx.y, blockIdx.x, md_smem, team);
}

static size_t md_align(size_t v) { return (v + 255) & ~(size_t)255; }

// the fp32 logits of `with_logits` plans (the one-launch head keeps them on chip otherwise); the kernel itself needs none
int64_t heat_modes_scratch_bytes(int n, int side, int n_joints_head, int depth, bool with_logits) {
    return (int64_t)(with_logits ? md_align((size_t)n * side * side * depth * n_joints_head * sizeof(float)) : 256);
}

template <typename AccT, typename LogitT>
static int launch_heat_modes_t(ModesArgs& a, int n, hipStream_t stream) {
    a.slab_rows = md_slab_rows(a.side, a.D, (int)sizeof(LogitT));
    if (a.slab_rows == 0) {
        set_error("heat_modes: a %d x %d x %d volume of %d-byte logits does not fit the kernel's LDS (flags and three rows in 64 KB)",
                  a.side, a.side, a.D, (int)sizeof(LogitT));
        return METRO_ERR_UNSUPPORTED;
    }
    if (note_kernel("heat_modes<acc%d,logits%d>", (int)sizeof(AccT) * 8, (int)sizeof(LogitT) * 8)) return METRO_OK;
    static PerDeviceInt attr;
    const int st = ensure_dyn_lds(reinterpret_cast<const void*>(heat_modes_kernel<AccT, LogitT>), MD_LDS_MAX, attr, "heat_modes");
    if (st) return st;
    const size_t lds = md_lds_bytes(a.side, a.D, (int)sizeof(LogitT), a.slab_rows);
    hipLaunchKernelGGL((heat_modes_kernel<AccT, LogitT>), dim3(a.n_out, n), dim3(MD_THREADS), lds, stream, a);
    return launch_status("heat_modes");
}

int launch_heat_modes(const void* logits, int precise, int n, int max_n, const MetroSpec& spec, int k, int radius, int32_t* voxel_out,
                      float* stats_out, hipStream_t stream) {
    if (spec.n_joints_head > METRO_MAX_JOINTS || spec.n_joints_out > METRO_MAX_JOINTS || n > max_n || n > 65535 ||
        k < 1 || k > METRO_MAX_MODES || radius < 0 || radius > METRO_MAX_MODE_RADIUS) {
        set_error("heat_modes: unsupported call (%d head joints, %d crops of %d, %d modes, radius %d)", spec.n_joints_head, n, max_n, k, radius);
        return METRO_ERR_UNSUPPORTED;
    }
    ModesArgs a;
    a.logits = logits; a.voxel = voxel_out; a.stats = stats_out;
    a.side = spec.proc_side / spec.stride; a.J = spec.n_joints_head; a.D = spec.depth; a.n_out = spec.n_joints_out;
    a.K = k; a.radius = radius; a.slab_rows = 0;
    head_permutation(spec, a.perm);
    if (precise == 0) return launch_heat_modes_t<float, float>(a, n, stream);
    if (precise == 1) return launch_heat_modes_t<double, float>(a, n, stream);
    if (precise == 2) return launch_heat_modes_t<double, double>(a, n, stream);
    set_error("heat_modes: precise must be 0, 1 or 2 (got %d)", precise);
    return METRO_ERR_INVALID_ARG;
}

}  // namespace metro
