// Per-joint heat-map posterior under a Gaussian prior, of a forward whose plan has prior buffers bound (metro_plan_bind_prior,
// include/metro_hip.h, which holds the definition).  logits NHWC [n, S, S, C = D*J], channel c = d*J + j; l[v] the logits of one
// (crop, head joint) over voxels v = (y*S + x)*D + d, g(v) = (gx[x], gy[y], gz[d]) the soft-argmax's own fp32 grids.  Per (crop,
// OUTPUT joint r, head joint perm[r]) with the prior row (mu, L) of output joint r:
//   q(v) = -1/2 (g - mu)^T L (g - mu),  w = l + q,  p' = exp(w - M') / S'   (M' = max w, S' its normaliser; M, S those of l)
//   log_evidence = (M' - M) + ln(S' / S),  peak' = max p',  coords01' = sum p' g,  cov01' = sum p' (g - coords01')(g - coords01')^T
// One launch, one workgroup of 256 threads per (crop, output joint), the joint index fastest in the grid.  posterior_walk below is
// the whole body, written for a TEAM (tid of nt, sync, max and sums over the team): the kernel's team is the workgroup (64-lane
// __shfl_xor ladders, one LDS record per wave, folded in wave order by every thread), the host tests' team is one thread
// (tests/test_heat_posterior.py compiles this file for the host and walks it).  Three passes, thread t over voxels t, t + nt, ...:
//   1  the two maxima M and M'
//   2  the two normalisers -- one loop, one reduction: the same code in the same order, so a zero L gives S' == S in every bit and
//      log_evidence exactly 0 -- and the three first moments of exp(w - M')
//   3  the six central second moments about the posterior mean (never E[g^2] - E[g]^2)
// A volume that fits in LDS is staged there once and the three passes read it; a larger one is read from memory three times.
// q is recomputed per pass in the accumulator type (some twenty operations; staging w would round it to the logits' type).
// Sums: AccT = fp32 on f16 plans, fp64 on f32 / f32m / f64 plans (LogitT fp64 on f64 plans); fixed order, no atomics; each output
// is rounded to fp32 once.  A NaN in the prior row or in a logit, a +Inf logit (S or S' is NaN then) and a non-finite M' (nothing
// but -Inf logits) give NaN in all 11 values of that joint; a -Inf logit is a voxel of weight zero.
#include "metro_common.h"

#pragma clang fp contract(off)

namespace metro {

#define PO_HD __host__ __device__ __forceinline__

constexpr int PO_THREADS = 256;
constexpr int PO_STATS = 11;                 // log_evidence, peak', coords01' (3), cov01' (6)
constexpr int PO_PRIOR = 9;                  // mu (x, y, z), precision (xx, yy, zz, xy, xz, yz)
constexpr int PO_LDS_HEAD = 256;             // wave records: 4 waves x 6 values x 8 bytes
constexpr int PO_LDS_MAX = 64 * 1024;

PO_HD float po_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __expf(x);
#else
    return expf(x);
#endif
}
PO_HD double po_exp(double x) { return exp(x); }
PO_HD float po_log(float x) { return logf(x); }
PO_HD double po_log(double x) { return log(x); }

// the soft-argmax's grid: fp32 linspace(0, 1, k), fp32 step and fp32 product (one point: 0) -- md_grid of heat_modes.hip
PO_HD float po_grid(int i, int k) { return k > 1 ? (float)i * (1.0f / (float)(k - 1)) : 0.0f; }

// is the volume staged in LDS whole?
PO_HD bool po_fits(int S, int D, int logit_bytes) { return (long)S * S * D * logit_bytes + PO_LDS_HEAD <= (long)PO_LDS_MAX; }
PO_HD size_t po_lds_bytes(int S, int D, int logit_bytes, bool staged) {
    return (size_t)PO_LDS_HEAD + (staged ? (size_t)S * S * D * logit_bytes : 0);
}

struct PosteriorArgs {
    const void* logits;
    const float* prior;  // [n][n_out][9]
    void* post;          // [n][n_out][11], fp32 (the host tests also read the accumulators' values before that rounding)
    int side, J, D, n_out, staged;
    int perm[METRO_MAX_JOINTS];
};

template <typename AccT>
struct PoPrior { AccT mx, my, mz, xx, yy, zz, xy, xz, yz; };

// the energy of the voxel at grid point (gx, gy, gz)
template <typename AccT>
PO_HD AccT po_energy(const PoPrior<AccT>& P, AccT gx, AccT gy, AccT gz) {
    const AccT ex = gx - P.mx, ey = gy - P.my, ez = gz - P.mz;
    const AccT diag = P.xx * ex * ex + P.yy * ey * ey + P.zz * ez * ez;
    const AccT off = P.xy * ex * ey + P.xz * ex * ez + P.yz * ey * ez;
    return (AccT)-0.5 * (diag + (AccT)2 * off);
}

// voxel v of the joint whose first logit is `lg`: from the staged volume where there is one, else from memory
template <typename LogitT>
PO_HD LogitT po_at(const LogitT* whole, const LogitT* lg, int v, int D, int C, int J) {
    return whole != nullptr ? whole[v] : lg[(size_t)(v / D) * C + (v % D) * J];
}

template <typename AccT, typename LogitT, typename OutT = float, class Team>
__host__ __device__ inline void posterior_walk(const PosteriorArgs& a, int img, int r, char* lds, Team& team) {
    const int S = a.side, D = a.D, J = a.J, C = D * J, row = S * D, vol = S * row;
    const int tid = team.tid, nt = team.nt;
    const LogitT* lg = static_cast<const LogitT*>(a.logits) + (size_t)img * S * S * C + a.perm[r];
    const float* pr = a.prior + ((size_t)img * a.n_out + r) * PO_PRIOR;
    OutT* out = static_cast<OutT*>(a.post) + ((size_t)img * a.n_out + r) * PO_STATS;
    LogitT* slab = reinterpret_cast<LogitT*>(lds + PO_LDS_HEAD);
    const LogitT* whole = a.staged ? slab : nullptr;
    if (a.staged) {
        for (int v = tid; v < vol; v += nt) slab[v] = lg[(size_t)(v / D) * C + (v % D) * J];
        team.sync();
    }
    const PoPrior<AccT> P = {(AccT)pr[0], (AccT)pr[1], (AccT)pr[2], (AccT)pr[3], (AccT)pr[4], (AccT)pr[5], (AccT)pr[6], (AccT)pr[7], (AccT)pr[8]};

    // ---- 1: the maxima of l and of w = l + q ----
    AccT mm[2] = {(AccT)-INFINITY, (AccT)-INFINITY};
    for (int v = tid; v < vol; v += nt) {
        const int y = v / row, rem = v - y * row, x = rem / D, d = rem - x * D;
        const AccT l = (AccT)po_at(whole, lg, v, D, C, J);
        const AccT w = l + po_energy(P, (AccT)po_grid(x, S), (AccT)po_grid(y, S), (AccT)po_grid(d, D));
        mm[0] = l > mm[0] ? l : mm[0];
        mm[1] = w > mm[1] ? w : mm[1];
    }
    team.template maxes<2>(mm);
    const AccT M = mm[0], Mp = mm[1];
    if (!(Mp > (AccT)-INFINITY && Mp < (AccT)INFINITY)) {          // nothing but -Inf logits, or a +Inf one: no distribution
        for (int i = tid; i < PO_STATS; i += nt) out[i] = (OutT)NAN;
        return;
    }

    // ---- 2: the normalisers of l and of w, the first moments of exp(w - M') ----
    AccT s1[5] = {0, 0, 0, 0, 0};
    for (int v = tid; v < vol; v += nt) {
        const int y = v / row, rem = v - y * row, x = rem / D, d = rem - x * D;
        const AccT gx = (AccT)po_grid(x, S), gy = (AccT)po_grid(y, S), gz = (AccT)po_grid(d, D);
        const AccT l = (AccT)po_at(whole, lg, v, D, C, J);
        const AccT w = l + po_energy(P, gx, gy, gz);
        const AccT e = po_exp(w - Mp);
        s1[0] += po_exp(l - M); s1[1] += e;
        s1[2] += e * gx; s1[3] += e * gy; s1[4] += e * gz;
    }
    team.template sums<5>(s1);
    const AccT total = s1[0], total_p = s1[1];
    if (total != total || total_p != total_p) {                    // a NaN logit, a +Inf logit, a NaN in the prior row
        for (int i = tid; i < PO_STATS; i += nt) out[i] = (OutT)NAN;
        return;
    }
    const AccT inv = (AccT)1 / total_p;
    const AccT mx = s1[2] * inv, my = s1[3] * inv, mz = s1[4] * inv;

    // ---- 3: the central second moments about the posterior mean ----
    AccT s2[6] = {0, 0, 0, 0, 0, 0};
    for (int v = tid; v < vol; v += nt) {
        const int y = v / row, rem = v - y * row, x = rem / D, d = rem - x * D;
        const AccT gx = (AccT)po_grid(x, S), gy = (AccT)po_grid(y, S), gz = (AccT)po_grid(d, D);
        const AccT w = (AccT)po_at(whole, lg, v, D, C, J) + po_energy(P, gx, gy, gz);
        const AccT p = po_exp(w - Mp) * inv;
        const AccT ex = gx - mx, ey = gy - my, ez = gz - mz;
        s2[0] += p * ex * ex; s2[1] += p * ey * ey; s2[2] += p * ez * ez;
        s2[3] += p * ex * ey; s2[4] += p * ex * ez; s2[5] += p * ey * ez;
    }
    team.template sums<6>(s2);
    if (tid == 0) {
        out[0] = (OutT)((Mp - M) + po_log(total_p / total));
        out[1] = (OutT)inv;                                        // exp(M' - M') / S'
        out[2] = (OutT)mx; out[3] = (OutT)my; out[4] = (OutT)mz;
        for (int i = 0; i < 6; ++i) out[5 + i] = (OutT)s2[i];
    }
}

// The kernel's team: the workgroup.  A 64-lane __shfl_xor ladder per value (every lane ends with the same bits: each step adds or
// compares the same two values in both lanes), one record per wave and value through LDS, folded in wave order by every thread;
// a second barrier, so that the records can be written again.
struct PosteriorWorkgroup {
    char* rec;                                       // LDS, PO_LDS_HEAD bytes
    const int tid;
    static constexpr int nt = PO_THREADS, n_groups = PO_THREADS / 64;
    const int group, lane;

    __device__ void sync() const { __syncthreads(); }
    template <int N, typename T>
    __device__ void maxes(T (&x)[N]) const {
        static_assert(n_groups * N * sizeof(T) <= (size_t)PO_LDS_HEAD, "wave records");
        T* w = reinterpret_cast<T*>(rec);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            for (int off = 32; off > 0; off >>= 1) {
                const T o = __shfl_xor(x[i], off);
                x[i] = o > x[i] ? o : x[i];
            }
            if (lane == 0) w[group * N + i] = x[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x[i] = w[i];
            for (int g = 1; g < n_groups; ++g) x[i] = w[g * N + i] > x[i] ? w[g * N + i] : x[i];
        }
        __syncthreads();
    }
    template <int N, typename T>
    __device__ void sums(T (&x)[N]) const {
        static_assert(n_groups * N * sizeof(T) <= (size_t)PO_LDS_HEAD, "wave records");
        T* w = reinterpret_cast<T*>(rec);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            for (int off = 32; off > 0; off >>= 1) x[i] += __shfl_xor(x[i], off);
            if (lane == 0) w[group * N + i] = x[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x[i] = w[i];
            for (int g = 1; g < n_groups; ++g) x[i] += w[g * N + i];
        }
        __syncthreads();
    }
};

template <typename AccT, typename LogitT>
__global__ __launch_bounds__(PO_THREADS) void heat_posterior_kernel(PosteriorArgs a) {
    extern __shared__ __attribute__((aligned(16))) char po_smem[];
    PosteriorWorkgroup team = {po_smem, (int)threadIdx.x, (int)threadIdx.x >> 6, (int)threadIdx.x & 63};
    posterior_walk<AccT, LogitT>(a, blockIdx.y, blockIdx.x, po_smem, team);
}

static size_t po_align(size_t v) { return (v + 255) & ~(size_t)255; }

// the fp32 logits of `with_logits` plans (the one-launch head keeps them on chip otherwise); the kernel itself needs none
int64_t heat_posterior_scratch_bytes(int n, int side, int n_joints_head, int depth, bool with_logits) {
    return (int64_t)(with_logits ? po_align((size_t)n * side * side * depth * n_joints_head * sizeof(float)) : 256);
}

template <typename AccT, typename LogitT>
static int launch_heat_posterior_t(PosteriorArgs& a, int n, hipStream_t stream) {
    a.staged = po_fits(a.side, a.D, (int)sizeof(LogitT)) ? 1 : 0;
    if (note_kernel("heat_posterior<acc%d,logits%d>", (int)sizeof(AccT) * 8, (int)sizeof(LogitT) * 8)) return METRO_OK;
    static PerDeviceInt attr;
    const int st = ensure_dyn_lds(reinterpret_cast<const void*>(heat_posterior_kernel<AccT, LogitT>), PO_LDS_MAX, attr, "heat_posterior");
    if (st) return st;
    const size_t lds = po_lds_bytes(a.side, a.D, (int)sizeof(LogitT), a.staged != 0);
    hipLaunchKernelGGL((heat_posterior_kernel<AccT, LogitT>), dim3(a.n_out, n), dim3(PO_THREADS), lds, stream, a);
    return launch_status("heat_posterior");
}

int launch_heat_posterior(const void* logits, int precise, int n, int max_n, const MetroSpec& spec, const float* prior, float* post_out,
                          hipStream_t stream) {
    const int side = spec.stride > 0 ? spec.proc_side / spec.stride : 0;
    if (spec.n_joints_head > METRO_MAX_JOINTS || spec.n_joints_out > METRO_MAX_JOINTS || n > max_n || n > 65535 || side < 1 ||
        spec.depth < 1 || (int64_t)side * side * spec.depth > (int64_t)1 << 24) {
        set_error("heat_posterior: unsupported call (%d head joints, %d crops of %d, a %d x %d x %d volume)", spec.n_joints_head, n, max_n,
                  side, side, spec.depth);
        return METRO_ERR_UNSUPPORTED;
    }
    PosteriorArgs a;
    a.logits = logits; a.prior = prior; a.post = post_out;
    a.side = side; a.J = spec.n_joints_head; a.D = spec.depth; a.n_out = spec.n_joints_out; a.staged = 0;
    head_permutation(spec, a.perm);
    if (precise == 0) return launch_heat_posterior_t<float, float>(a, n, stream);
    if (precise == 1) return launch_heat_posterior_t<double, float>(a, n, stream);
    if (precise == 2) return launch_heat_posterior_t<double, double>(a, n, stream);
    set_error("heat_posterior: precise must be 0, 1 or 2 (got %d)", precise);
    return METRO_ERR_INVALID_ARG;
}

}  // namespace metro
