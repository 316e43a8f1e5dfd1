// HBM-bound kernels of the path: the zero-padded max-pool, and the softmax-over-volume + expectation soft-argmax with mm
// decode.  (Input preparation and the crop warps: warp_crops.hip.)
#include "metro_common.h"
#include "gfx950_prims.h"

namespace metro {

// ---------------------------------------------------------------------------------------------
// 3x3 stride-2 max-pool over an input ZERO-padded by (1,1) (reference resnet_utils.py:177-185:
// array_ops.pad then VALID pooling -> the pad value 0 takes part in the max).
// One thread per (output pixel, 16-byte channel chunk).
// ---------------------------------------------------------------------------------------------
template <typename VecT, int VEC>
__global__ __launch_bounds__(256) void maxpool3x3s2_zeropad_kernel(const VecT* __restrict__ in,
                                                                   VecT* __restrict__ out, int n,
                                                                   int h_in, int w_in, int cvec) {
    const int h_out = (h_in + 2 - 3) / 2 + 1, w_out = (w_in + 2 - 3) / 2 + 1;
    const long total = (long)n * h_out * w_out * cvec;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        const int cv = (int)(idx % cvec);
        long t = idx / cvec;
        const int wo = (int)(t % w_out);
        t /= w_out;
        const int ho = (int)(t % h_out);
        const int im = (int)(t / h_out);
        VecT best;
        bool first = true;
        bool touched_pad = false;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int hi = 2 * ho - 1 + r;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int wi = 2 * wo - 1 + s;
                if ((unsigned)hi < (unsigned)h_in && (unsigned)wi < (unsigned)w_in) {
                    const VecT v = in[((size_t)(im * h_in + hi) * w_in + wi) * cvec + cv];
                    if (first) { best = v; first = false; }
                    else {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) best[e] = v[e] > best[e] ? v[e] : best[e];
                    }
                } else {
                    touched_pad = true;
                }
            }
        }
        if (touched_pad) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) best[e] = best[e] > 0 ? best[e] : 0;
        }
        out[idx] = best;
    }
}

typedef double doublex2 __attribute__((ext_vector_type(2)));

int launch_maxpool(const void* in, void* out, int n, int h_in, int w_in, int c, int dtype,
                   hipStream_t stream) {
    const int h_out = (h_in + 2 - 3) / 2 + 1, w_out = (w_in + 2 - 3) / 2 + 1;
    if (dtype != METRO_F16 && dtype != METRO_F32 && dtype != METRO_F64) { set_error("maxpool: unsupported dtype %d", dtype); return METRO_ERR_INVALID_ARG; }
    if (note_kernel("maxpool3x3s2_zeropad<%s>", dtype == METRO_F16 ? "f16" : dtype == METRO_F32 ? "f32" : "f64")) return METRO_OK;
    if (dtype == METRO_F16) {
        if (c % 8) { set_error("maxpool f16: channels %d not a multiple of 8", c); return METRO_ERR_INVALID_ARG; }
        const long total = (long)n * h_out * w_out * (c / 8);
        const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
        hipLaunchKernelGGL((maxpool3x3s2_zeropad_kernel<half8_t, 8>), dim3(blocks), dim3(256), 0, stream,
                           static_cast<const half8_t*>(in), static_cast<half8_t*>(out), n, h_in, w_in, c / 8);
    } else if (dtype == METRO_F32) {
        if (c % 4) { set_error("maxpool f32: channels %d not a multiple of 4", c); return METRO_ERR_INVALID_ARG; }
        const long total = (long)n * h_out * w_out * (c / 4);
        const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
        hipLaunchKernelGGL((maxpool3x3s2_zeropad_kernel<floatx4, 4>), dim3(blocks), dim3(256), 0, stream,
                           static_cast<const floatx4*>(in), static_cast<floatx4*>(out), n, h_in, w_in, c / 4);
    } else if (dtype == METRO_F64) {
        if (c % 2) { set_error("maxpool f64: channels %d not a multiple of 2", c); return METRO_ERR_INVALID_ARG; }
        const long total = (long)n * h_out * w_out * (c / 2);
        const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
        hipLaunchKernelGGL((maxpool3x3s2_zeropad_kernel<doublex2, 2>), dim3(blocks), dim3(256), 0, stream,
                           static_cast<const doublex2*>(in), static_cast<doublex2*>(out), n, h_in, w_in, c / 2);
    } else {
        set_error("maxpool: unsupported dtype %d", dtype);
        return METRO_ERR_INVALID_ARG;
    }
    return launch_status("maxpool3x3s2_zeropad");
}

// ---------------------------------------------------------------------------------------------
// Soft-argmax.  logits fp32 NHWC [n, S, S, C = D*J], channel c = d*J + j (reference
// volumetric.py:230-232).  Per (image, joint): softmax over all S*S*D voxels (tfu.py:466-471),
// then expectation of linspace(0,1,.) coordinates along W (x), H (y), D (z) (tfu.py:474-499 with
// axes [3,2,4], volumetric.py:234).
//
// Kernel 1 (partials): grid (slabs, n).  A slab is a contiguous range of pixels; since NHWC
// keeps a pixel's C channels contiguous, the slab is one contiguous float range read with
// 16-byte loads.  Thread (pp, q) owns the channel quad q (4 consecutive channels) and walks
// pixels pp, pp+PPB, ... keeping an ONLINE softmax state (running max m, sum e, sum e*x,
// sum e*y) per channel: logits are read exactly once.  The block then folds the PPB pixel
// lanes and the D depth channels of each joint through LDS and emits
// (m, S, Sx, Sy, Sz) per (image, slab, joint).
// Kernel 2 (finalize): folds the slabs, divides, decodes to millimetres
// (volumetric.py:288-295,303-306), subtracts the root = last head joint (tfu3d.py:23-25) and
// gathers the exported joint order (main.py:119-127).
// ---------------------------------------------------------------------------------------------
constexpr int SA_NT = 256;

int softargmax_slabs(int n, int side) {
    // Slabs of >= 32 pixels, at most 64 per image.  Deliberately independent of the batch size: the fp32 partial
    // sums are folded slab by slab, so a crop's pose has the same bits whatever batch it arrives in (no op of the
    // path crosses the batch dimension).  Batch 64 at stride 16: 8 slabs x 64 images = 512 blocks.
    (void)n;
    const int pixels = side * side;
    int slabs = pixels / 32;
    if (slabs > 64) slabs = 64;
    if (slabs < 1) slabs = 1;
    return slabs;
}

int64_t softargmax_scratch_bytes(int n, int side, int n_joints_head) {
    return (int64_t)n * softargmax_slabs(n, side) * n_joints_head * 5 * sizeof(double);
}

template <typename AccT>
__device__ __forceinline__ AccT acc_exp(AccT x);
template <> __device__ __forceinline__ float acc_exp<float>(float x) { return __expf(x); }
template <> __device__ __forceinline__ double acc_exp<double>(double x) { return exp(x); }

// MOMENTS: every record is followed, in `moments` [n][slabs][J][6], by its six second central moments about ITS OWN mean
// (xx, yy, zz, xy, xz, yz, weighted like S).  Centred from the first step: a pixel lane takes its channel's (xx, yy, xy) about
// its own mean in a second walk over its pixels (the slab is L2-resident: it was streamed a moment ago) -- an online update of
// centred sums needs a division per logit, raw sums E[x^2] - E[x]^2 cancel on a sharp peak -- and the two folds merge with the
// parallel-axis update, rescaled by the same factor f as the sums: every diagonal term is a sum of non-negative numbers.
template <typename AccT, typename LogitT, bool MOMENTS>
__global__ __launch_bounds__(SA_NT) void softargmax_partial_kernel(
    const LogitT* __restrict__ logits, AccT* __restrict__ partials, int side, int depth, int nj,
    int slabs, AccT* __restrict__ moments) {
    extern __shared__ __attribute__((aligned(16))) char sa_smem[];
    constexpr int RS = MOMENTS ? 7 : 4;
    AccT* red = reinterpret_cast<AccT*>(sa_smem);   // [ppb][C][RS]: m, s, sx, sy (MOMENTS: + xx, yy, xy)

    const int C = depth * nj;
    const int quads = C / 4;
    const int ppb = SA_NT / quads;            // pixel lanes per block
    const int tid = threadIdx.x;
    const int pp = tid / quads;
    const int q = tid - pp * quads;
    const int img = blockIdx.y;
    const int slab = blockIdx.x;
    const int pixels = side * side;
    const int p_begin = (int)((long)pixels * slab / slabs);
    const int p_end = (int)((long)pixels * (slab + 1) / slabs);
    const float step_s = 1.0f / (float)(side - 1);   // tf.linspace step in fp32 (tfu.py:481)

    AccT m[4], s[4], sx[4], sy[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { m[e] = (AccT)-INFINITY; s[e] = 0; sx[e] = 0; sy[e] = 0; }

    if (pp < ppb) {
        const LogitT* base = logits + (size_t)img * pixels * C + q * 4;
        typedef LogitT logit4 __attribute__((ext_vector_type(4)));
        // The path is HBM bound and every pixel lane has ONE 16-byte load per pixel: UNR pixels are requested before the first
        // is consumed -- with one load in flight per thread the launch ran at 3.3 TB/s at the configs[4] volume (8 blocks x 238
        // lanes x 16 B = 30 KB in flight per CU).  The online softmax is BRANCH FREE: per channel the running maximum is raised to
        // the maximum of the UNR new logits first (one rescale exp per channel and iteration; exp(0) = 1 exactly when it did not
        // move), pixels past the slab enter as -inf and contribute exp(-inf) = 0; a per-element `if (x > m)` cost a compare, an
        // exec-mask save / restore and a branch per logit.  Pixel coordinates advance incrementally (no division in the loop).
#ifndef METRO_SA_UNR
#define METRO_SA_UNR 2     // measured at the configs[4] volume (285 MB): 2 -> 67.6 us, 4 -> 69.3, 8 -> 88.7 (registers cut the occupancy); 1 (round 3) -> 87
#endif
        constexpr int UNR = METRO_SA_UNR;
        int ph = (p_begin + pp) / side, pw = (p_begin + pp) - ph * side;       // pixel of this lane, advanced by ppb per slot
        for (int p0 = p_begin + pp; p0 < p_end; p0 += UNR * ppb) {
            logit4 v[UNR];
            AccT cx[UNR], cy[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int p = p0 + u * ppb;
                const bool ok = p < p_end;
                v[u] = *reinterpret_cast<const logit4*>(base + (size_t)(ok ? p : p0) * C);
                cx[u] = (AccT)((float)pw * step_s);
                cy[u] = (AccT)((float)ph * step_s);
                if (!ok) { v[u][0] = v[u][1] = v[u][2] = v[u][3] = (LogitT)-INFINITY; }
                pw += ppb;
                while (pw >= side) { pw -= side; ++ph; }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                AccT mx = m[e];
#pragma unroll
                for (int u = 0; u < UNR; ++u) mx = (AccT)v[u][e] > mx ? (AccT)v[u][e] : mx;
                // a channel that has held nothing but -Inf so far (a voxel of weight zero: a -Inf logits bias) keeps m = -Inf and
                // s = 0: the exponents are taken about 0 then, -Inf - -Inf would be NaN.  Any other mx is its own reference.
                const AccT mr = mx == (AccT)-INFINITY ? (AccT)0 : mx;
                const AccT f = acc_exp<AccT>(m[e] - mr);          // exp(-inf) = 0 on first touch
                AccT s_ = s[e] * f, sx_ = sx[e] * f, sy_ = sy[e] * f;
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const AccT ex = acc_exp<AccT>((AccT)v[u][e] - mr);
                    s_ += ex; sx_ += ex * cx[u]; sy_ += ex * cy[u];
                }
                m[e] = mx; s[e] = s_; sx[e] = sx_; sy[e] = sy_;
            }
        }
        AccT cxx[4] = {0, 0, 0, 0}, cyy[4] = {0, 0, 0, 0}, cxy[4] = {0, 0, 0, 0};
        if constexpr (MOMENTS) {
            AccT mux[4], muy[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const AccT so = opaque_copy(s[e]);
                mux[e] = so > 0 ? opaque_copy(sx[e]) / so : (AccT)0;
                muy[e] = so > 0 ? opaque_copy(sy[e]) / so : (AccT)0;
            }
            AccT mo[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) mo[e] = opaque_copy(m[e]);
            const float sso = opaque_copy(step_s);
            for (int p = p_begin + pp; p < p_end; p += ppb) {
                const logit4 v = *reinterpret_cast<const logit4*>(base + (size_t)p * C);
                const int qh = p / side, qw = p - qh * side;
                const AccT px = (AccT)opaque_copy((float)qw * sso), py = (AccT)opaque_copy((float)qh * sso);      // the ROUNDED coordinates of the first pass: no fma into dx
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const AccT ex = acc_exp<AccT>((AccT)v[e] - mo[e]);
                    const AccT dx = px - mux[e], dy = py - muy[e];
                    cxx[e] += ex * dx * dx; cyy[e] += ex * dy * dy; cxy[e] += ex * dx * dy;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            AccT* r = red + ((size_t)pp * C + q * 4 + e) * RS;
            r[0] = m[e]; r[1] = s[e]; r[2] = sx[e]; r[3] = sy[e];
            if constexpr (MOMENTS) { r[4] = cxx[e]; r[5] = cyy[e]; r[6] = cxy[e]; }
        }
    }
    __syncthreads();

    // fold, stage 1: one thread per CHANNEL folds the pixel lanes (a serial walk of one thread per joint over ppb * depth = 56
    // records was the tail of every block); the result replaces lane 0's record
    for (int c = tid; c < C; c += SA_NT) {               // C > 256 for the 53-joint head
        AccT M = (AccT)-INFINITY;
        for (int l = 0; l < ppb; ++l) {
            const AccT mv = red[((size_t)l * C + c) * RS];
            M = mv > M ? mv : M;
        }
        AccT S = 0, SX = 0, SY = 0;
        for (int l = 0; l < ppb; ++l) {
            const AccT* r = red + ((size_t)l * C + c) * RS;
            if (r[1] > 0) {
                const AccT f = acc_exp<AccT>(r[0] - M);
                S += r[1] * f; SX += r[2] * f; SY += r[3] * f;
            } else if (r[1] != r[1]) S = r[1];           // a NaN sum must reach the finalize launch's non-finite screen
        }
        AccT XX = 0, YY = 0, XY = 0;
        if constexpr (MOMENTS) {
            const AccT So = opaque_copy(S), Mo = opaque_copy(M);
            const AccT mux = opaque_copy(SX) / So, muy = opaque_copy(SY) / So;
            for (int l = 0; l < ppb; ++l) {
                const AccT* r = red + ((size_t)l * C + c) * RS;
                if (r[1] > 0) {
                    const AccT f = acc_exp<AccT>(opaque_copy(r[0]) - Mo);
                    const AccT w = r[1] * f, lx = r[2] / r[1] - mux, ly = r[3] / r[1] - muy;
                    XX += f * r[4] + w * lx * lx; YY += f * r[5] + w * ly * ly; XY += f * r[6] + w * lx * ly;
                }
            }
        }
        AccT* r0 = red + (size_t)c * RS;                 // lane 0's record of this channel: read above by this thread only
        r0[0] = M; r0[1] = S; r0[2] = SX; r0[3] = SY;
        if constexpr (MOMENTS) { r0[4] = XX; r0[5] = YY; r0[6] = XY; }
    }
    __syncthreads();
    // stage 2: one thread per joint folds its `depth` channels (c = d * nj + j, volumetric.py:231)
    if (tid < nj) {
        const int j = tid;
        const float step_d = 1.0f / (float)(depth - 1);
        AccT M = (AccT)-INFINITY;
        for (int d = 0; d < depth; ++d) {
            const AccT mv = red[(size_t)(d * nj + j) * RS];
            M = mv > M ? mv : M;
        }
        AccT S = 0, SX = 0, SY = 0, SZ = 0;
        for (int d = 0; d < depth; ++d) {
            const AccT* r = red + (size_t)(d * nj + j) * RS;
            if (r[1] > 0) {
                const AccT f = acc_exp<AccT>(r[0] - M);
                const AccT cz = (AccT)((float)d * step_d);
                S += r[1] * f; SX += r[2] * f; SY += r[3] * f; SZ += r[1] * f * cz;
            } else if (r[1] != r[1]) S = r[1];
        }
        AccT* o = partials + (((size_t)img * slabs + slab) * nj + j) * 5;
        o[0] = M; o[1] = S; o[2] = SX; o[3] = SY; o[4] = SZ;
        if constexpr (MOMENTS) {
            const AccT So = opaque_copy(S), Mo = opaque_copy(M);
            const AccT mux = opaque_copy(SX) / So, muy = opaque_copy(SY) / So, muz = opaque_copy(SZ) / So;
            const float sdo = opaque_copy(step_d);
            AccT c[6] = {0, 0, 0, 0, 0, 0};
            for (int d = 0; d < depth; ++d) {
                const AccT* r = red + (size_t)(d * nj + j) * RS;
                if (r[1] > 0) {
                    const AccT f = acc_exp<AccT>(opaque_copy(r[0]) - Mo);
                    const AccT w = r[1] * f, lx = r[2] / r[1] - mux, ly = r[3] / r[1] - muy;
                    const AccT lz = (AccT)opaque_copy((float)d * sdo) - muz;
                    c[0] += f * r[4] + w * lx * lx; c[1] += f * r[5] + w * ly * ly; c[2] += w * lz * lz;
                    c[3] += f * r[6] + w * lx * ly; c[4] += w * lx * lz; c[5] += w * ly * lz;
                }
            }
            AccT* om = moments + (((size_t)img * slabs + slab) * nj + j) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) om[k] = c[k];
        }
    }
}

// One block of four waves per image; wave w folds joints w, w + 4, ...: its lanes stride over the slabs (up to 128 records per
// joint behind the 256-pixel head), maximum and the four rescaled sums folded across the wave with xor shuffles in a fixed
// order -- a serial loop over the slabs by ONE thread per joint cost 20 us on a 64 x 64 heat map.
template <typename AccT>
__device__ __forceinline__ AccT sa_wave_sum(AccT v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// MOMENTS: also folds the records' second central moments (`moments` [n][slabs][J][6], each about its record's own mean
// mu_i = (SX_i, SY_i, SZ_i) / S_i) with the parallel-axis update, scaled by exp(m_i - M) as the sums are:
//   Cov01 = sum_i f_i (C_i + S_i (mu_i - mu)(mu_i - mu)^T) / S,   mu = the coords01 of the joint,
// into cov01 fp32 [n][J][6] (xx, yy, zz, xy, xz, yz; head order) and peak [n][J] = max p = exp(M - M) / S = 1 / S.
template <typename AccT, bool MOMENTS>
__global__ __launch_bounds__(1024) void softargmax_finalize_kernel(const AccT* __restrict__ partials,
                                                                  float* __restrict__ poses,
                                                                  SoftArgmaxArgs a, int slabs,
                                                                  float* __restrict__ coords01,
                                                                  int32_t* __restrict__ status,
                                                                  const AccT* __restrict__ moments,
                                                                  float* __restrict__ cov01, float* __restrict__ peak) {
    __shared__ AccT mm[METRO_MAX_JOINTS][3];
    // Non-finite screen (status[img] = 1): a record whose sum is NaN, a non-finite maximum or normaliser.  fp16 storage overflows
    // at 65 504 (reference tfu.py:426-440 keeps fp32 variables for the same reason).  What carries an overflow to this screen: the
    // identity shortcuts keep a +-Inf (or the NaN of Inf - Inf) in the residual stream, every ReLU of the library is the
    // NaN-propagating metro::relu (gfx950_prims.h: a maxNum ReLU turned the NaN pixels into zeros in the next pre-activation, and
    // a projection shortcut, which reads only the pre-activated stream, then made the stream finite again), so the head's
    // pre-activation hands NaN / +Inf to every logit of that pixel, whose exp(l - max) is NaN in its record's sum.  A -Inf that
    // a ReLU turns into 0 is the right value, not a lost flag.  A NaN record is never dropped from the sums: its joint (every
    // joint, if it is the root's) is returned as NaN, not as the finite, wrong pose of the other slabs.
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    const int img = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nj = a.n_joints_head;
    if (slabs <= 16) {
        // few records per joint (stride-16 / 32 heads: 4 or 1): one thread per joint walks them -- the shuffle folds of the wave
        // form cost more than they save here (8.3 vs 4.6 us at batch 64)
        const int j = threadIdx.x;
        if (j < nj) {
            // every field of every record is loaded unconditionally, eight records' loads in flight: as a chain of dependent loads
            // (a record at a time, the sum fields behind the test of the normaliser) eight records cost 8.5 us
            AccT M = (AccT)-INFINITY;
#pragma unroll 8
            for (int sl = 0; sl < slabs; ++sl) {
                const AccT mv = partials[(((size_t)img * slabs + sl) * nj + j) * 5];
                M = mv > M ? mv : M;
            }
            AccT S = 0, SX = 0, SY = 0, SZ = 0;
#pragma unroll 8
            for (int sl = 0; sl < slabs; ++sl) {
                const AccT* r = partials + (((size_t)img * slabs + sl) * nj + j) * 5;
                const AccT r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
                // a record that is not a sum of exponentials (NaN: a NaN or +Inf logit in its slab) is added like any other, so
                // its joint comes out NaN, as the exact soft-argmax of those logits does, and the image is flagged
                const AccT f = acc_exp<AccT>(r0 - M);
                S += r1 * f; SX += r2 * f; SY += r3 * f; SZ += r4 * f;
                if (!(r1 > 0)) bad = true;
            }
            bad = bad || !(M - M == (AccT)0) || !(S - S == (AccT)0) || !(SX - SX == (AccT)0) || !(SY - SY == (AccT)0) || !(SZ - SZ == (AccT)0);
            const AccT x01 = SX / S, y01 = SY / S, z01 = SZ / S;
            if (coords01 != nullptr) {
                float* c = coords01 + ((size_t)img * nj + j) * 3;
                c[0] = (float)x01; c[1] = (float)y01; c[2] = (float)z01;
            }
            mm[j][0] = (x01 * (AccT)a.lrc + (AccT)a.half_off) * (AccT)a.box_size_mm / (AccT)a.proc_side;
            mm[j][1] = (y01 * (AccT)a.lrc + (AccT)a.half_off) * (AccT)a.box_size_mm / (AccT)a.proc_side;
            mm[j][2] = z01 * (AccT)a.box_size_mm;
            if constexpr (MOMENTS) {
                const AccT Mo = opaque_copy(M), So = opaque_copy(S);
                const AccT xo = opaque_copy(x01), yo = opaque_copy(y01), zo = opaque_copy(z01);
                AccT c[6] = {0, 0, 0, 0, 0, 0};
                for (int sl = 0; sl < slabs; ++sl) {
                    const AccT* r = partials + (((size_t)img * slabs + sl) * nj + j) * 5;
                    const AccT* q = moments + (((size_t)img * slabs + sl) * nj + j) * 6;
                    const AccT r0 = opaque_copy(r[0]), r1 = opaque_copy(r[1]), r2 = opaque_copy(r[2]), r3 = opaque_copy(r[3]), r4 = opaque_copy(r[4]);
                    if (r1 > 0) {
                        const AccT f = acc_exp<AccT>(r0 - Mo);
                        const AccT w = r1 * f, lx = r2 / r1 - xo, ly = r3 / r1 - yo, lz = r4 / r1 - zo;
                        c[0] += f * q[0] + w * lx * lx; c[1] += f * q[1] + w * ly * ly; c[2] += f * q[2] + w * lz * lz;
                        c[3] += f * q[3] + w * lx * ly; c[4] += f * q[4] + w * lx * lz; c[5] += f * q[5] + w * ly * lz;
                    }
                }
                float* co = cov01 + ((size_t)img * nj + j) * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) co[k] = (float)(c[k] / So);
                peak[(size_t)img * nj + j] = (float)((AccT)1 / So);
            }
        }
    } else
    for (int j = wave; j < nj; j += (int)(blockDim.x >> 6)) {      // many records per joint: a wave per joint (16 waves: one or two rounds)
        AccT M = (AccT)-INFINITY;
        for (int sl = lane; sl < slabs; sl += 64) {
            const AccT mv = partials[(((size_t)img * slabs + sl) * nj + j) * 5];
            M = mv > M ? mv : M;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const AccT other = __shfl_xor(M, o, 64);
            M = other > M ? other : M;
        }
        AccT S = 0, SX = 0, SY = 0, SZ = 0;
#pragma unroll 2
        for (int sl = lane; sl < slabs; sl += 64) {
            const AccT* r = partials + (((size_t)img * slabs + sl) * nj + j) * 5;
            const AccT r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];      // all five before the test: one latency, not two
            const AccT f = acc_exp<AccT>(r0 - M);
            S += r1 * f; SX += r2 * f; SY += r3 * f; SZ += r4 * f;
            if (!(r1 > 0)) bad = true;
        }
        S = sa_wave_sum(S); SX = sa_wave_sum(SX); SY = sa_wave_sum(SY); SZ = sa_wave_sum(SZ);
        bad = bad || !(M - M == (AccT)0) || !(S - S == (AccT)0) || !(SX - SX == (AccT)0) || !(SY - SY == (AccT)0) || !(SZ - SZ == (AccT)0);
        if (lane == 0) {
            const AccT x01 = SX / S, y01 = SY / S, z01 = SZ / S;
            if (coords01 != nullptr) {            // net_output_to_heatmap_and_coords output (volumetric.py:234-235)
                float* c = coords01 + ((size_t)img * nj + j) * 3;
                c[0] = (float)x01; c[1] = (float)y01; c[2] = (float)z01;
            }
            // heatmap_to_metric: (c * lrc + half) * box / proc_side ; z * box  (volumetric.py:288-306)
            mm[j][0] = (x01 * (AccT)a.lrc + (AccT)a.half_off) * (AccT)a.box_size_mm / (AccT)a.proc_side;
            mm[j][1] = (y01 * (AccT)a.lrc + (AccT)a.half_off) * (AccT)a.box_size_mm / (AccT)a.proc_side;
            mm[j][2] = z01 * (AccT)a.box_size_mm;
        }
        if constexpr (MOMENTS) {
            const AccT So = opaque_copy(S), Mo = opaque_copy(M);      // every lane holds the folded sums
            const AccT x01 = opaque_copy(SX) / So, y01 = opaque_copy(SY) / So, z01 = opaque_copy(SZ) / So;
            AccT c[6] = {0, 0, 0, 0, 0, 0};
            for (int sl = lane; sl < slabs; sl += 64) {
                const AccT* r = partials + (((size_t)img * slabs + sl) * nj + j) * 5;
                const AccT* q = moments + (((size_t)img * slabs + sl) * nj + j) * 6;
                const AccT r0 = opaque_copy(r[0]), r1 = opaque_copy(r[1]), r2 = opaque_copy(r[2]), r3 = opaque_copy(r[3]), r4 = opaque_copy(r[4]);
                if (r1 > 0) {
                    const AccT f = acc_exp<AccT>(r0 - Mo);
                    const AccT w = r1 * f, lx = r2 / r1 - x01, ly = r3 / r1 - y01, lz = r4 / r1 - z01;
                    c[0] += f * q[0] + w * lx * lx; c[1] += f * q[1] + w * ly * ly; c[2] += f * q[2] + w * lz * lz;
                    c[3] += f * q[3] + w * lx * ly; c[4] += f * q[4] + w * lx * lz; c[5] += f * q[5] + w * ly * lz;
                }
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) c[k] = sa_wave_sum(c[k]);
            if (lane == 0) {
                float* co = cov01 + ((size_t)img * nj + j) * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) co[k] = (float)(c[k] / So);
                peak[(size_t)img * nj + j] = (float)((AccT)1 / So);
            }
        }
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (status != nullptr && threadIdx.x == 0) status[img] = s_bad;
    const int j = threadIdx.x;
    if (poses != nullptr && j < a.n_joints_out) {
        const int src = a.perm[j];
        float* o = poses + ((size_t)img * a.n_joints_out + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (float)(mm[src][c] - mm[nj - 1][c]);   // tfu3d.py:23-25
    }
}

SoftArgmaxArgs make_softargmax_args(const MetroSpec& spec, int n) {
    SoftArgmaxArgs a;
    a.n = n;
    a.side = spec.proc_side / spec.stride;
    a.depth = spec.depth;
    a.n_joints_head = spec.n_joints_head;
    a.n_joints_out = spec.n_joints_out;
    const HeadPixelScale px = head_pixel_scale(spec);
    a.lrc = px.lrc; a.half_off = px.half_off;
    a.box_size_mm = spec.box_size_mm;
    a.proc_side = spec.proc_side;
    head_permutation(spec, a.perm);
    return a;
}

int64_t moments_scratch_bytes(int n, int side, int n_joints_head) {
    // one record of six sums per (image, 32-pixel slab, joint): the most any head or soft-argmax launch writes, as fp64
    const int slabs = side * side / 32 > 0 ? side * side / 32 : 1;
    return (int64_t)n * slabs * n_joints_head * 6 * (int64_t)sizeof(double);
}

template <typename AccT, typename LogitT, bool MOMENTS>
static int launch_softargmax_t(const void* logits, const SoftArgmaxArgs& a, void* partials,
                               float* poses, float* coords01, hipStream_t stream, int32_t* status, const MomentsOut& mo) {
    const int C = a.depth * a.n_joints_head;
    const int quads = C / 4;
    const int ppb = SA_NT / quads;
    const int slabs = softargmax_slabs(a.n, a.side);
    const size_t lds = (size_t)ppb * C * (MOMENTS ? 7 : 4) * sizeof(AccT);
    if (note_kernel(MOMENTS ? "softargmax_partial<acc%d,logits%d,moments> & softargmax_finalize<acc%d,moments>"
                            : "softargmax_partial<acc%d,logits%d> & softargmax_finalize<acc%d>", (int)sizeof(AccT) * 8,
                    (int)sizeof(LogitT) * 8, (int)sizeof(AccT) * 8))
        return METRO_OK;
    auto kern = softargmax_partial_kernel<AccT, LogitT, MOMENTS>;
    if (lds > 64 * 1024) {
        static PerDeviceInt attr_done;
        if (const int st = ensure_dyn_lds(reinterpret_cast<const void*>(kern), 160 * 1024, attr_done, "softargmax_partial")) return st;
    }
    hipLaunchKernelGGL(kern, dim3(slabs, a.n), dim3(SA_NT), lds, stream, static_cast<const LogitT*>(logits),
                       static_cast<AccT*>(partials), a.side, a.depth, a.n_joints_head, slabs, static_cast<AccT*>(mo.scratch));
    int st = launch_status("softargmax_partial");
    if (st) return st;
    hipLaunchKernelGGL((softargmax_finalize_kernel<AccT, MOMENTS>), dim3(a.n), dim3(slabs > 16 ? 1024 : 256), 0, stream,
                       static_cast<const AccT*>(partials), poses, a, slabs, coords01, status,
                       static_cast<const AccT*>(mo.scratch), mo.cov01, mo.peak);
    return launch_status("softargmax_finalize");
}

int launch_softargmax_finalize(const float* partials, const SoftArgmaxArgs& a, int slabs, float* poses_out,
                               hipStream_t stream, float* coords01_out, int32_t* status, const MomentsOut& mo) {
    if (mo.scratch != nullptr) {
        if (note_kernel("softargmax_finalize<acc32,moments>")) return METRO_OK;
        hipLaunchKernelGGL((softargmax_finalize_kernel<float, true>), dim3(a.n), dim3(slabs > 16 ? 1024 : 256), 0, stream, partials,
                           poses_out, a, slabs, coords01_out, status, static_cast<const float*>(mo.scratch), mo.cov01, mo.peak);
        return launch_status("softargmax_finalize");
    }
    if (note_kernel("softargmax_finalize<acc32>")) return METRO_OK;
    hipLaunchKernelGGL((softargmax_finalize_kernel<float, false>), dim3(a.n), dim3(slabs > 16 ? 1024 : 256), 0, stream, partials,
                       poses_out, a, slabs, coords01_out, status, nullptr, nullptr, nullptr);
    return launch_status("softargmax_finalize");
}

int launch_softargmax(const void* logits, const SoftArgmaxArgs& a, int precise, void* partials,
                      float* poses_out, hipStream_t stream, float* coords01_out, int32_t* status, const MomentsOut& mo) {
    const int C = a.depth * a.n_joints_head;
    if (C % 4 || C / 4 > SA_NT || a.n_joints_head > METRO_MAX_JOINTS || a.n_joints_out > 64) {
        set_error("softargmax: unsupported head (depth %d, joints %d)", a.depth, a.n_joints_head);
        return METRO_ERR_UNSUPPORTED;
    }
    if (mo.scratch != nullptr) {
        if (precise == 0) return launch_softargmax_t<float, float, true>(logits, a, partials, poses_out, coords01_out, stream, status, mo);
        if (precise == 1) return launch_softargmax_t<double, float, true>(logits, a, partials, poses_out, coords01_out, stream, status, mo);
        if (precise == 2) return launch_softargmax_t<double, double, true>(logits, a, partials, poses_out, coords01_out, stream, status, mo);
    } else {
        if (precise == 0) return launch_softargmax_t<float, float, false>(logits, a, partials, poses_out, coords01_out, stream, status, mo);
        if (precise == 1) return launch_softargmax_t<double, float, false>(logits, a, partials, poses_out, coords01_out, stream, status, mo);
        if (precise == 2) return launch_softargmax_t<double, double, false>(logits, a, partials, poses_out, coords01_out, stream, status, mo);
    }
    set_error("softargmax: precise must be 0, 1 or 2 (got %d)", precise);
    return METRO_ERR_INVALID_ARG;
}

}  // namespace metro
