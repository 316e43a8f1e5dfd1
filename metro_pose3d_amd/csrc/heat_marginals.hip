// Per-joint heat-map marginals of a forward whose plan has output buffers bound (metro_plan_bind_heatmaps, include/metro_hip.h).
// logits NHWC [n, S, S, C = D*J], channel c = d*J + j (reference volumetric.py:230-232); p = softmax over the joint's S*S*D voxels
// (tfu.py:466-471, the distribution net_output_to_heatmap_and_coords returns next to the coordinates, volumetric.py:227-235):
//   xy[i, r, y, x] = sum_d p[y, x, d]        z[i, r, d] = sum_{y,x} p[y, x, d]        r: output joint, head joint j = perm[r]
// Three launches on the forward's stream, the first and the last with one block per (pixel tile, crop):
//   heat_partial  per (crop, tile, channel) the maximum m and sum exp(l - m) over the tile's pixels.  Thread c reads channel c of
//                 every pixel of the tile: a wave reads 64 consecutive channels, the block whole rows of C channels.
//   heat_fold     one block per crop folds the tiles per channel (M_c, S_c: the z sums, kept per channel), then the D channels of
//                 every joint (M_j, 1 / S_j -> `jst`), and writes z = S_c exp(M_c - M_j) / S_j in output joint order.
//   heat_xy       per (crop, tile): p = exp(l - M_j) / S_j for a chunk of the tile's pixels, whole rows of C channels, staged in
//                 LDS [pixel][C]; thread (pixel, j) sums its D values (stride J: consecutive lanes on consecutive banks) into the
//                 transposed LDS image [J][tile pixels], which is written out per OUTPUT joint as one run of tile-pixels consecutive
//                 floats (32 pixels: 128 bytes).
// Sums: AccT = fp32 on f16 plans (fp32 logits, as the head's own statistics), fp64 on f32 / f32m (fp32 logits) and f64 (fp64
// logits) plans; every output is rounded to fp32 once.  Fixed order everywhere (no atomics): a crop's maps have the same bits
// in every call and at every batch.
// Non-finite logits: a NaN or +Inf logit makes its tile's sum NaN (exp(NaN), exp(Inf - Inf)), which every fold carries into the
// joint's normaliser: that joint's rows of both outputs are NaN, no other joint's.  A -Inf logit is a voxel of weight zero, as
// in the soft-argmax.
// The per-item arithmetic is __host__ __device__: tests/test_heat_marginals.py compiles this file for the host and walks it.
#include "metro_common.h"

#pragma clang fp contract(off)

namespace metro {

#define HM_HD __host__ __device__ __forceinline__

HM_HD float hm_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __expf(x);
#else
    return expf(x);
#endif
}
HM_HD double hm_exp(double x) { return exp(x); }

// pixel tiles of one crop: 32 pixels, 64 once the map has more than 2048 (the fold walks a crop's tiles serially)
HM_HD int hm_tile_pixels(int pixels) { return pixels > 2048 ? 64 : 32; }
HM_HD int hm_tiles(int pixels) { return (pixels + hm_tile_pixels(pixels) - 1) / hm_tile_pixels(pixels); }
// pixels of a tile whose probabilities heat_xy stages at a time: [chunk][C] AccT in at most 32 KiB of LDS
HM_HD int hm_chunk_pixels(int pixels, int C, int acc_bytes) {
    const int fit = 32768 / (C * acc_bytes), tp = hm_tile_pixels(pixels);
    return fit < 1 ? 1 : fit < tp ? fit : tp;
}

// heat_partial's item: channel c over the `npix` pixels that start at `tile` (the tile's first pixel, channel 0)
template <typename AccT, typename LogitT>
HM_HD void hm_tile_channel(const LogitT* tile, int C, int npix, int c, AccT& m_out, AccT& s_out) {
    AccT m = (AccT)-INFINITY;
    // both walks unrolled: eight of a lane's loads in flight (one per pixel and nothing to hide it behind otherwise)
#pragma unroll 8
    for (int p = 0; p < npix; ++p) {
        const AccT v = (AccT)tile[(size_t)p * C + c];
        m = v > m ? v : m;
    }
    const AccT mr = m == (AccT)-INFINITY ? (AccT)0 : m;      // nothing but -Inf: exponents about 0 (-Inf - -Inf would be NaN), s = 0
    AccT s = 0;
#pragma unroll 8
    for (int p = 0; p < npix; ++p) s += hm_exp((AccT)tile[(size_t)p * C + c] - mr);
    m_out = m; s_out = s;
}

// fold of `count` records (m, s) that lie `stride` records apart; a NaN sum is never dropped
template <typename AccT>
HM_HD void hm_fold(const AccT* rec, int count, size_t stride, AccT& M_out, AccT& S_out) {
    AccT M = (AccT)-INFINITY;
    for (int i = 0; i < count; ++i) {
        const AccT mv = rec[i * stride * 2];
        M = mv > M ? mv : M;
    }
    AccT S = 0;
    for (int i = 0; i < count; ++i) {
        const AccT m = rec[i * stride * 2], s = rec[i * stride * 2 + 1];
        if (s > 0) S += s * hm_exp(m - M);
        else if (s != s) S = s;
    }
    M_out = M; S_out = S;
}

// heat_xy's items: one probability, and the D-sum of one (pixel, joint) from the pixel's staged row of C probabilities
template <typename AccT, typename LogitT>
HM_HD AccT hm_prob(LogitT l, AccT M, AccT inv_s) { return hm_exp((AccT)l - M) * inv_s; }
template <typename AccT>
HM_HD float hm_depth_sum(const AccT* row, int J, int D, int j) {
    AccT acc = 0;
    for (int d = 0; d < D; ++d) acc += row[d * J + j];
    return (float)acc;
}
// heat_fold's last item: z of (head joint j, depth d) from the channel records `chan` [C][2] and the joint records `jst` [J][2]
template <typename AccT>
HM_HD float hm_z(const AccT* chan, const AccT* jst, int J, int j, int d) {
    const AccT m = chan[(d * J + j) * 2], s = chan[(d * J + j) * 2 + 1];
    const AccT M = jst[j * 2], inv_s = jst[j * 2 + 1];
    if (s > 0) return (float)(s * hm_exp(m - M) * inv_s);
    return (float)(s * inv_s);          // 0 (a channel of -Inf only), or NaN with the joint's normaliser
}

struct HeatArgs {
    const void* logits;
    void* part;          // AccT [n][tiles][C][2]
    void* jst;           // AccT [n][J][2]: M_j, 1 / S_j
    float* xy;           // [n][n_out][pixels]
    float* z;            // [n][n_out][D]
    int pixels, J, D, n_out, tiles, chunk;
    int perm[METRO_MAX_JOINTS];
};

template <typename AccT, typename LogitT>
__global__ __launch_bounds__(256) void heat_partial_kernel(HeatArgs a) {
    const int C = a.D * a.J, tile = blockIdx.x, img = blockIdx.y;
    const int tp = hm_tile_pixels(a.pixels), p0 = tile * tp;
    const int npix = a.pixels - p0 < tp ? a.pixels - p0 : tp;
    const LogitT* base = static_cast<const LogitT*>(a.logits) + ((size_t)img * a.pixels + p0) * C;
    AccT* out = static_cast<AccT*>(a.part) + ((size_t)img * a.tiles + tile) * C * 2;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        AccT m, s;
        hm_tile_channel<AccT, LogitT>(base, C, npix, c, m, s);
        out[c * 2] = m; out[c * 2 + 1] = s;
    }
}

template <typename AccT>
__global__ __launch_bounds__(256) void heat_fold_kernel(HeatArgs a) {
    extern __shared__ __attribute__((aligned(16))) char hm_fold_smem[];
    const int C = a.D * a.J, img = blockIdx.x;
    AccT* chan = reinterpret_cast<AccT*>(hm_fold_smem);          // [C][2]
    AccT* jst = chan + (size_t)C * 2;                            // [J][2]
    const AccT* part = static_cast<const AccT*>(a.part) + (size_t)img * a.tiles * C * 2;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        AccT M, S;
        hm_fold<AccT>(part + c * 2, a.tiles, (size_t)C, M, S);
        chan[c * 2] = M; chan[c * 2 + 1] = S;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < a.J; j += blockDim.x) {
        AccT M, S;
        hm_fold<AccT>(chan + j * 2, a.D, (size_t)a.J, M, S);
        const AccT inv_s = (AccT)1 / S;
        jst[j * 2] = M; jst[j * 2 + 1] = inv_s;
        AccT* o = static_cast<AccT*>(a.jst) + ((size_t)img * a.J + j) * 2;
        o[0] = M; o[1] = inv_s;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.n_out * a.D; idx += blockDim.x) {
        const int r = idx / a.D, d = idx - r * a.D;
        a.z[(size_t)img * a.n_out * a.D + idx] = hm_z<AccT>(chan, jst, a.J, a.perm[r], d);
    }
}

template <typename AccT, typename LogitT>
__global__ __launch_bounds__(256) void heat_xy_kernel(HeatArgs a) {
    extern __shared__ __attribute__((aligned(16))) char hm_xy_smem[];
    const int C = a.D * a.J, tile = blockIdx.x, img = blockIdx.y;
    const int tp = hm_tile_pixels(a.pixels), p0 = tile * tp;
    const int npix = a.pixels - p0 < tp ? a.pixels - p0 : tp;
    AccT* jst = reinterpret_cast<AccT*>(hm_xy_smem);             // [J][2]
    AccT* prob = jst + (size_t)a.J * 2;                          // [chunk][C]
    float* sums = reinterpret_cast<float*>(prob + (size_t)a.chunk * C);      // [J][tp]
    const AccT* jst_g = static_cast<const AccT*>(a.jst) + (size_t)img * a.J * 2;
    for (int i = threadIdx.x; i < a.J * 2; i += blockDim.x) jst[i] = jst_g[i];
    __syncthreads();
    const LogitT* base = static_cast<const LogitT*>(a.logits) + ((size_t)img * a.pixels + p0) * C;
    for (int q0 = 0; q0 < npix; q0 += a.chunk) {
        const int nq = npix - q0 < a.chunk ? npix - q0 : a.chunk;
        // rows q0 .. q0 + nq of the tile are one contiguous range of nq * C logits
        for (int idx = threadIdx.x; idx < nq * C; idx += blockDim.x) {
            const int c = idx % C, j = c % a.J;
            prob[idx] = hm_prob<AccT, LogitT>(base[(size_t)q0 * C + idx], jst[j * 2], jst[j * 2 + 1]);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < nq * a.J; idx += blockDim.x) {
            const int q = idx / a.J, j = idx - q * a.J;
            sums[j * tp + q0 + q] = hm_depth_sum<AccT>(prob + (size_t)q * C, a.J, a.D, j);
        }
        __syncthreads();
    }
    float* out = a.xy + (size_t)img * a.n_out * a.pixels + p0;
    for (int idx = threadIdx.x; idx < a.n_out * npix; idx += blockDim.x) {
        const int r = idx / npix, q = idx - r * npix;
        out[(size_t)r * a.pixels + q] = sums[a.perm[r] * tp + q];
    }
}

static size_t hm_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t hm_part_bytes(int n, int pixels, int C) { return hm_align((size_t)n * hm_tiles(pixels) * C * 2 * sizeof(double)); }
static size_t hm_jst_bytes(int n, int J) { return hm_align((size_t)n * J * 2 * sizeof(double)); }

// records (sized for fp64 whatever the plan's precision), then the joint records, then the fp32 logits of `with_logits` plans
int64_t heat_marginals_scratch_bytes(int n, int side, int n_joints_head, int depth, bool with_logits) {
    const int pixels = side * side, C = depth * n_joints_head;
    return (int64_t)(hm_part_bytes(n, pixels, C) + hm_jst_bytes(n, n_joints_head) +
                     (with_logits ? hm_align((size_t)n * pixels * C * sizeof(float)) : 0));
}
float* heat_marginals_scratch_logits(void* scratch, int max_n, int side, int n_joints_head, int depth) {
    return reinterpret_cast<float*>(static_cast<char*>(scratch) + hm_part_bytes(max_n, side * side, depth * n_joints_head) +
                                    hm_jst_bytes(max_n, n_joints_head));
}

template <typename AccT, typename LogitT>
static int launch_heat_marginals_t(HeatArgs& a, int n, hipStream_t stream) {
    const int C = a.D * a.J;
    a.chunk = hm_chunk_pixels(a.pixels, C, (int)sizeof(AccT));
    const size_t fold_lds = ((size_t)C + a.J) * 2 * sizeof(AccT);
    const size_t xy_lds = ((size_t)a.J * 2 + (size_t)a.chunk * C) * sizeof(AccT) + (size_t)a.J * hm_tile_pixels(a.pixels) * sizeof(float);
    if (fold_lds > 64 * 1024 || xy_lds > 64 * 1024) {
        set_error("heat_marginals: %d channels exceed the kernels' LDS images", C);
        return METRO_ERR_UNSUPPORTED;
    }
    if (note_kernel("heat_partial<acc%d,logits%d> & heat_fold<acc%d> & heat_xy<acc%d,logits%d>", (int)sizeof(AccT) * 8,
                    (int)sizeof(LogitT) * 8, (int)sizeof(AccT) * 8, (int)sizeof(AccT) * 8, (int)sizeof(LogitT) * 8))
        return METRO_OK;
    const int nt = C >= 256 ? 256 : (C + 63) / 64 * 64;
    hipLaunchKernelGGL((heat_partial_kernel<AccT, LogitT>), dim3(a.tiles, n), dim3(nt), 0, stream, a);
    int st = launch_status("heat_partial");
    if (st) return st;
    hipLaunchKernelGGL((heat_fold_kernel<AccT>), dim3(n), dim3(256), fold_lds, stream, a);
    st = launch_status("heat_fold");
    if (st) return st;
    hipLaunchKernelGGL((heat_xy_kernel<AccT, LogitT>), dim3(a.tiles, n), dim3(256), xy_lds, stream, a);
    return launch_status("heat_xy");
}

int launch_heat_marginals(const void* logits, int precise, int n, int max_n, const MetroSpec& spec, void* scratch, float* xy_out,
                          float* z_out, hipStream_t stream) {
    const int side = spec.proc_side / spec.stride;
    if (spec.n_joints_head > METRO_MAX_JOINTS || spec.n_joints_out > METRO_MAX_JOINTS || n > max_n || n > 65535) {
        set_error("heat_marginals: unsupported call (%d head joints, %d crops of %d)", spec.n_joints_head, n, max_n);
        return METRO_ERR_UNSUPPORTED;
    }
    HeatArgs a;
    a.logits = logits; a.xy = xy_out; a.z = z_out;
    a.pixels = side * side; a.J = spec.n_joints_head; a.D = spec.depth; a.n_out = spec.n_joints_out;
    a.tiles = hm_tiles(a.pixels); a.chunk = 0;
    a.part = scratch;
    a.jst = static_cast<char*>(scratch) + hm_part_bytes(max_n, a.pixels, a.D * a.J);
    head_permutation(spec, a.perm);
    if (precise == 0) return launch_heat_marginals_t<float, float>(a, n, stream);
    if (precise == 1) return launch_heat_marginals_t<double, float>(a, n, stream);
    if (precise == 2) return launch_heat_marginals_t<double, double>(a, n, stream);
    set_error("heat_marginals: precise must be 0, 1 or 2 (got %d)", precise);
    return METRO_ERR_INVALID_ARG;
}

}  // namespace metro
