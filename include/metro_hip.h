/*
 * metro_hip.h -- C ABI of libmetro_hip.so: the MI355X (gfx950) implementation of the MeTRo
 * inference hot path (ResNet-v2 backbone -> 1x1 volumetric head -> soft-argmax -> mm decode).
 *
 * The reference (isarandi/metro-pose3d) is pure Python/TensorFlow and has NO native interface:
 * every FLOP of this path runs inside `sess.run` of a frozen GraphDef (reference
 * inference.py:25-27,31-43).  This header is therefore the boundary a binding would attach to
 * in place of `tf.import_graph_def` + `Session.run`; each entry point names the reference
 * code whose work it replaces.  Plain pointers and sizes only; no torch / TF types.
 *
 * Conventions:
 *   - every function returns 0 on success or a negative MetroStatus; metro_last_error()
 *     returns a thread-local message for the last failure on the calling thread;
 *   - all `void* d_*` pointers are DEVICE pointers owned by the caller; the library never
 *     allocates or frees device memory and never synchronises the stream;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - a plan is bound to the device current at creation and is not thread-safe.
 */
#ifndef METRO_HIP_H
#define METRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define METRO_ABI_VERSION 8

typedef enum MetroStatus {
    METRO_OK = 0,
    METRO_ERR_INVALID_ARG = -1,
    METRO_ERR_UNSUPPORTED = -2,
    METRO_ERR_HIP = -3,
    METRO_ERR_STATE = -4,
    METRO_ERR_NONFINITE = -5   /* metro_forward_status: non-finite activations reached the soft-argmax */
} MetroStatus;

/* Arithmetic mode of a plan.  Images are always fp32 in, poses fp32 out.
 * F16: activations/weights fp16, fp32 MFMA accumulation, fp32 soft-argmax -- the reference's
 *      default compute dtype (reference src/options.py:73, src/tfu.py:426-440).  Throughput mode.
 * F32: activations fp32 in HBM, every contraction accumulated with v_mfma_f64_16x16x4_f64
 *      from fp64-folded weights, fp64 soft-argmax; one rounding to fp32 per layer output.
 *      Sits at the fp32 storage noise floor (~1e-3 mm vs exact arithmetic).
 * F64: as F32 but activations and logits are stored as fp64 too: the parity mode, measured
 *      against the fp64 oracle (bar <= 1e-3 mm; lands orders of magnitude below).
 * F32M: the arithmetic of the reference's fp32 graph (--dtype=float32, reference src/options.py:73): fp32 activations, fp32
 *      (BN-folded) weights, every contraction on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation in ascending
 *      k), fp64 soft-argmax on the fp32 logits.  The parity mode at fp32 speed: sits AT the noise floor two correct fp32
 *      implementations have between them (1-5e-3 mm), not under the 1e-3 mm bar. */
typedef enum MetroPrecision { METRO_PREC_F16 = 0, METRO_PREC_F32 = 1, METRO_PREC_F64 = 2, METRO_PREC_F32M = 3 } MetroPrecision;

typedef enum MetroDType { METRO_F16 = 0, METRO_F32 = 1, METRO_F64 = 2 } MetroDType;

#define METRO_MAX_JOINTS 64

/* The constants a frozen graph of the reference bakes in from its flags
 * (reference src/options.py:41,73,96,109-119; src/main.py:106-128). */
typedef struct MetroSpec {
    int32_t arch;                 /* 50 | 101: resnet_v2_50 / resnet_v2_101 (resnet_v2.py:272-312) */
    int32_t stride;               /* 4 | 8 | 16 | 32: --stride-test (options.py:96)                */
    int32_t n_joints_head;        /* J_head: head emits depth * J_head channels (volumetric.py:158) */
    int32_t depth;                /* D = 8 (options.py:113)                                         */
    int32_t centered_stride;      /* 1 (options.py:118)                                             */
    int32_t proc_side;            /* 256 (options.py:41)                                            */
    float   box_size_mm;          /* 2200 (options.py:119)                                          */
    int32_t base_width;           /* 64 for ResNet-50/101; smaller values = toy specs for tests     */
    int32_t precision;            /* MetroPrecision                                                 */
    int32_t n_joints_out;         /* Jout: rows of `output` (main.py:127)                           */
    int32_t permutation[METRO_MAX_JOINTS]; /* output row i = head joint permutation[i] (main.py:119-125) */
} MetroSpec;

typedef struct MetroPlan MetroPlan;

typedef enum MetroParamKind {
    METRO_PARAM_CONV_W = 0,   /* conv kernel, packed [c_out][kh][kw_pad][c_in_pad], BN-folded if bn_var != "" */
    METRO_PARAM_BIAS = 1,     /* per-c_out bias: conv biases, or beta - mean*scale of the folded BN           */
    METRO_PARAM_PRO_SCALE = 2,/* pre-activation BN as prologue: gamma / sqrt(var + 1e-5), per c_in            */
    METRO_PARAM_PRO_SHIFT = 3 /* beta - mean * scale, per c_in                                                */
} MetroParamKind;

/* One tensor of the plan's parameter blob.  The caller fills the blob (host side, any language)
 * from a TF-slim style variable dictionary and uploads it; see INTEGRATION.md. */
typedef struct MetroParamInfo {
    char    name[96];      /* plan-local name, e.g. "block3/unit_2/conv2/W"                      */
    char    conv_var[160]; /* slim scope of the source conv ("" for prologue tensors)            */
    char    bn_var[160];   /* slim scope of the BatchNorm folded in / used as prologue, or ""    */
    int32_t kind;          /* MetroParamKind                                                     */
    int32_t dtype;         /* MetroDType of the packed tensor                                    */
    int32_t c_out, kh, kw, c_in;   /* logical conv dims (c_out = length for 1-D tensors)        */
    int32_t kw_pad, c_in_pad;      /* packed dims; padding is zero-filled                        */
    int64_t offset;        /* byte offset in the blob (256-byte aligned)                         */
    int64_t bytes;
} MetroParamInfo;

#define METRO_FUSED_CONV1_IN_FRONT 1      /* '<unit>/conv1+conv2': conv1 (1x1 on the pre-activated unit input, folded BN + ReLU,
                                           * reference resnet_v2.py:119,127-128) runs on the 3x3 layer's LDS-resident input slab;
                                           * the layer's input tensor is the unit's RAW input (c_in = its channels)          */
#define METRO_FUSED_PROJECTION_SHORTCUT 2 /* conv3 launch that computes the unit's projection shortcut (resnet_v2.py:122-125)
                                           * from the unit's raw input instead of reading a shortcut tensor: has_residual = 0 */
/* block1 without its 256-channel residual stream in HBM (round 5; reference resnet_v2.py:119-138 of block1's units): */
#define METRO_FUSED_OUT_ON_CHIP 4         /* the launch's primary output (the unit's sum) is NOT written by metro_forward -- it only
                                           * feeds the next unit's conv1 inside the launch; metro_forward_upto(last_layer = this
                                           * layer) runs the storing form of the same kernel and writes it at out_offset        */
#define METRO_FUSED_REBUILT_SHORTCUT 8    /* conv3 launch whose identity shortcut x_{u-1} is rebuilt in the launch from the
                                           * 64-channel tensors it is a function of (the previous unit's conv2 output and conv3
                                           * weights + the block's projection shortcut of the pooled stem output) instead of being
                                           * read: has_residual / res_stride / res_offset still state the reference's shortcut   */
#define METRO_FUSED_COMPACT_SHORTCUT 16   /* conv3 of a strided unit whose sub-sampled shortcut (resnet_v2.py:113-121) is read from
                                           * the compact [n, h_out, w_out, c] copy the previous launch wrote at its out_sub_offset;
                                           * has_residual / res_stride / res_offset still state the reference's gather            */

typedef struct MetroLayerInfo {
    char    name[96];
    int32_t kind;          /* 0 input-prep, 1 conv, 2 max-pool, 3 soft-argmax partial, 4 finalize */
    int32_t h_in, w_in, c_in, h_out, w_out, c_out, kh, kw, stride, dilation, pad_top, pad_left;
    int32_t has_prologue, relu, has_residual, res_stride, res_offset;
    int32_t out_dtype;     /* MetroDType of the layer output in the workspace                    */
    int64_t out_offset;    /* byte offset of the output tensor in the workspace.  The 'logits' layer of an f16 plan
                            * whose head runs as one launch (head_f16) NEVER writes this slot during metro_forward:
                            * the logits stay on chip; only metro_forward_upto(last_layer = logits) fills it       */
    int64_t out_bytes_per_image;
    double  flops_per_image; /* 2*MACs (convs only), SURVEY.md section 8d accounting              */
    int64_t out2_offset;   /* fused launches with a second output tensor (shortcut+conv1 pairs,  */
    int32_t out2_channels; /*   conv3+next conv1): its workspace offset / channels; -1 / 0 = none.
                            * METRO_FUSED_CONV1_IN_FRONT layers: conv1's output, which lives in LDS during
                            * metro_forward and is written here ONLY by metro_forward_upto(last_layer = this layer) */
    int32_t fused_flags;   /* METRO_FUSED_*: other layers of the unit computed inside this launch        */
    /* algorithmic HBM bytes of this launch, every tensor it touches counted once (bench.py: the minimum the measured
     * rocprofv3 FETCH_SIZE/WRITE_SIZE traffic is compared with): activations read + written per image (input, outputs,
     * shortcut), and the parameter tensors it reads (once per launch, batch independent). */
    int64_t algo_act_bytes_per_image;
    int64_t algo_param_bytes;
    int64_t out_sub_offset; /* >= 0: the launch also (or only: METRO_FUSED_OUT_ON_CHIP) writes pixels (out_sub_off + 2 i,
                             * out_sub_off + 2 j) of its primary output as a compact [n, out_sub_side, out_sub_side, c_out]
                             * tensor here -- what the next, strided unit's shortcut reads; -1 = none                       */
    int32_t out_sub_side, out_sub_off;
} MetroLayerInfo;

/* ---- plan life cycle: replaces tf.import_graph_def of the frozen graph
 *      (reference inference.py:31-43) and the graph construction of
 *      volumetric.build_inference_model (reference src/model/volumetric.py:152-216). ---- */
int  metro_plan_create(const MetroSpec* spec, int32_t max_batch, MetroPlan** out_plan);
int  metro_plan_destroy(MetroPlan* plan);
int64_t metro_plan_workspace_bytes(const MetroPlan* plan);
int64_t metro_plan_param_bytes(const MetroPlan* plan);
int32_t metro_plan_num_params(const MetroPlan* plan);
int  metro_plan_param_info(const MetroPlan* plan, int32_t index, MetroParamInfo* out);
int32_t metro_plan_num_layers(const MetroPlan* plan);
int  metro_plan_layer_info(const MetroPlan* plan, int32_t index, MetroLayerInfo* out);
double metro_plan_flops_per_image(const MetroPlan* plan);
/* Which kernel instantiation layer `index` runs on at batch n (1 <= n <= max_batch): the choice depends on the layer's
 * shape AND on the batch (tile counts against the 256 CUs), so parity established at one batch does not transfer to another
 * unless the id is the same.  Writes a NUL-terminated id such as "conv3x3_f16_slab<128x256,rows384,bufs2,tps1,kc64,ws3>" or
 * "conv_igemm_f16_dma<128x128,bk64,s4,pro>+pair" ("a & b" when the layer launches two kernels).  A dry run of the layer's
 * dispatch code: nothing is launched and no device is needed.  tests/test_kernel_coverage.py requires every id the
 * BASELINE configurations dispatch at their per-GPU batch to be the id of a single-kernel test that compares with the oracle. */
int  metro_plan_layer_kernel(const MetroPlan* plan, int32_t index, int32_t n, char* buf, int32_t buf_len);
/* Test instrumentation for the single-kernel entry points below (thread-local): mode 0 off (default); 1 every launch on this
 * thread appends its kernel id to the string metro_last_kernel_id() returns; 2 DRY RUN -- entry points record the id and
 * return METRO_OK without launching.  Setting a mode clears the string, which holds 4 KiB -- every launch of a whole forward;
 * one that did not fit ends in " ...". */
int  metro_kernel_notes(int32_t mode);
const char* metro_last_kernel_id(void);
/* The tile-walk schedule of the last PERSISTENT launch on this thread since metro_kernel_notes(1 | 2) -- a kernel whose grid is
 * capped at CUs x resident blocks per CU and whose blocks walk several tiles (conv_pw64, conv_pws, conv_b1_chain, conv3x3_c64,
 * stem_pool_f16<split*>):  out[0] the grid launched, out[1] the work items (pixel tiles x halves, or patches), out[2] the grid
 * cap the launcher used, out[3] `halves` (blocks that share a pixel tile, one per slab of output channels; else 1).  All zero
 * when no such launch was noted.  In a dry run (mode 2) no device is asked: out[0] is the uncapped grid and out[2] is 0. */
int  metro_last_launch_schedule(int32_t out[4]);
/* Binds the uploaded parameter blob (device pointer, metro_plan_param_bytes() long). */
int  metro_plan_bind_params(MetroPlan* plan, const void* d_param_blob);

/* ---- the hot path: replaces sess.run(poses_tensor) (reference inference.py:25-27), i.e.
 *      architectures.resnet (architectures.py:24-35) -> net_output_to_heatmap_and_coords
 *      (volumetric.py:227-235) -> heatmap_to_metric (volumetric.py:303-306) -> root_relative
 *      (tfu3d.py:23-25) -> tf.gather(permutation) (main.py:127).
 *      d_images_nhwc: fp32 [n,256,256,3] in [0,1];  d_poses_out: fp32 [n,Jout,3] in mm.
 *      The launch contract, for this and EVERY entry with a `stream` parameter (tests/test_gpu_streams.py holds each one to it
 *      on a non-blocking side stream): all of the entry's work -- every kernel, every memset, the graph launch of a captured
 *      forward -- is enqueued on `stream` and on no other stream; no entry synchronises, except metro_forward_status and
 *      metro_forward_timed, which do so by contract.  A plan owns ONE workspace: consecutive calls on it that use different
 *      streams must be ordered by the caller (an event of the first stream waited for on the second), as calls from
 *      different threads must. ---- */
int  metro_forward(MetroPlan* plan, const float* d_images_nhwc, int32_t n, float* d_poses_out,
                   void* d_workspace, void* stream);
/* Small batches are launch-latency bound (45 dependent launches for ResNet-50 stride 16): forwards with
 * n <= max_batch_for_graphs are captured once per (n, buffers, stream) into a hipGraph and replayed.
 * 0 (default) = always plain launches.  The capture happens on the second call with a given key. */
int  metro_plan_set_graph_max_batch(MetroPlan* plan, int32_t max_batch_for_graphs);
/* Non-finite screen of the LAST metro_forward(n) on this workspace.  The reference keeps fp32 variables under fp16 compute
 * (reference src/tfu.py:426-440) and TensorFlow hands NaN poses back silently when an activation overflows fp16 (65 504); here
 * the finalize launch writes one int32 per image into the workspace (1 = a soft-argmax record, maximum or normaliser of that
 * image was not finite; a NaN record is never silently dropped) and this call copies the n words to the host -- it
 * SYNCHRONISES the stream, the only entry point of the path that does.  *n_nonfinite_out = number of flagged images; returns
 * METRO_ERR_NONFINITE (metro_last_error() names the remedy: precision f32m / f64) when it is not zero. */
int  metro_forward_status(const MetroPlan* plan, const void* d_workspace, int32_t n, void* stream, int32_t* n_nonfinite_out);
/* Byte offset, inside the workspace, of the int32[max_batch] non-finite words metro_forward_status reads: a caller that chains
 * several forwards (more crops than the plan's max_batch) can fold them on the device after each one and synchronise ONCE.  The
 * words are those of the LAST forward on this workspace: valid until the next metro_forward on it, on the same stream only. */
int64_t metro_plan_status_offset(const MetroPlan* plan);
/* ---- per-joint heat-map marginals, bound to the plan ----
 * Every joint's output is a softmax distribution p over its S x S x D volume (S = proc_side / stride; the heat-map
 * net_output_to_heatmap_and_coords returns next to the coordinates, reference volumetric.py:227-235).  With output buffers bound,
 * every forward entry -- metro_forward, metro_forward_coords01, metro_forward_u8, metro_forward_moments, in every precision;
 * metro_forward_timed and a metro_forward_upto that runs the whole plan too, outside the timed layers -- also writes, for crop i < n and OUTPUT joint r (head joint permutation[r]), on the stream it is given:
 *   d_xy_out fp32 [max_n, n_joints_out, S, S]:  xy[i, r, y, x] = sum_d p[y, x, d]
 *   d_z_out  fp32 [max_n, n_joints_out, D]:     z[i, r, d]     = sum_{y, x} p[y, x, d]
 * Their expectations on the soft-argmax grids (fp32 linspace(0,1,.)) are the coords01 of the same call.  Rows n .. max_n - 1 are
 * not touched.  Optional forward outputs are added this way: buffers bound to the plan, written by the existing entries -- no
 * new launching entry, neither function has a stream parameter.
 * Binding is HOST state: a forward reads the pointers when it enqueues, so rebinding (or unbinding: all three pointers NULL and
 * max_n 0) between two enqueues needs no synchronisation; the buffers must stay alive until the forwards enqueued while they
 * were bound have run.  Anything but the unbind call is checked in full: three non-NULL pointers, the scratch 16-byte aligned,
 * max_n in [1, the plan's max_batch].  d_scratch: metro_plan_heatmaps_scratch_bytes(plan, max_n) bytes (-1 for a bad argument);
 * on f16 plans whose head keeps the logits on chip it receives them as fp32 (the head kernels' layer-dump store), else the
 * logits are read from the workspace.
 * While bound: a forward with n > max_n returns METRO_ERR_INVALID_ARG before any launch; forwards make PLAIN launches -- the
 * hipGraph cache (metro_plan_set_graph_max_batch) does not serve them, as it does not serve metro_forward_u8; three launches
 * follow the finalize launch (heat_partial, heat_fold, heat_xy: csrc/heat_marginals.hip).  Poses, coords01, covariance, peak
 * and status words keep the bits of the unbound call.  Unbound, a forward enqueues exactly the kernels it always did.
 * Arithmetic: per-joint maximum and normaliser first, then p = exp(l - max) / sum.  All sums (tile sums of exponentials, their
 * folds, the sums over D and over pixels) are fp32 on f16 plans and fp64 on f32, f32m and f64 plans, in a fixed order; each
 * output is rounded to fp32 once.
 * Non-finite values: a joint one of whose logits is NaN or +Inf gets NaN in all its rows of both outputs (its normaliser is
 * NaN); the crop's other joints and every other crop are not affected by it, and the crop's pose, status word and
 * METRO_ERR_NONFINITE are those of the unbound call.  A -Inf logit is a voxel of weight zero, as in the soft-argmax. */
int64_t metro_plan_heatmaps_scratch_bytes(const MetroPlan* plan, int32_t max_n);
int  metro_plan_bind_heatmaps(MetroPlan* plan, float* d_xy_out, float* d_z_out, void* d_scratch, int32_t max_n);
/* ---- per-joint heat-map modes, bound to the plan ----
 * The mean and covariance of a two-peaked joint say only "between" and "wide", and the marginals above are a picture.  The modes
 * are numbers a consumer can act on: the K places the joint may be, how much probability each holds and how tight each is.  With
 * mode buffers bound, every forward entry (the list above) also writes them on the stream it is given, from the logits of the
 * same forward; the logits never pass through the host.  Definition, for crop i < n and head joint j:
 *   l[y, x, d] = logits[i, y, x, d * J + j], v = (y * S + x) * D + d the voxel's linear index, p = exp(l - M_j) / S_j the joint's
 *   softmax, as the marginals form it.  Parameters: k modes per joint, 1 <= k <= METRO_MAX_MODES, and the window radius,
 *   0 <= radius <= METRO_MAX_MODE_RADIUS.
 *   Neighbours of v: the voxels inside the volume that differ from it by at most 1 in each of y, x and d (up to 26).
 *   Candidates: v is one if l[v] is finite and, for every neighbour u, l[u] < l[v] or (l[u] == l[v] and u > v).  A plateau has one
 *   candidate, its lowest index; a -Inf voxel is never a candidate.
 *   Selection: the candidates in order of decreasing l, ties by increasing v; a candidate with max(|dy|, |dx|, |dd|) <= 2 radius to
 *   a mode already selected is skipped (so the windows of a joint's modes are disjoint and its masses sum to at most 1); stop at
 *   k modes.  The comparisons are on the logits as stored (fp32; fp64 on f64 plans), never on probabilities: the selected
 *   voxels are exact in every precision.
 *   Per mode, with W the voxels within `radius` of the mode in every axis, clipped to the volume:  mass = sum_W p;  peak = p[v];
 *   coords01 = sum_W p g / mass, g the soft-argmax's own grid (fp32 linspace(0,1,S) for x and y, linspace(0,1,D) for z, order
 *   x, y, z);  cov01 = the six central second moments of p over W about coords01, divided by mass, in the order (xx, yy, zz, xy,
 *   xz, yz) and units of metro_forward_moments' cov01.
 *   Fewer than k modes: the missing ones have voxel -1, mass 0, and NaN in peak, coords01 and cov01.
 *   Non-finite logits: a joint with a NaN or +Inf logit has, for all k modes, voxel -1 and NaN in every float; no other joint and no
 *   other crop is affected (the marginals' rule).
 *   Sums: fp32 on f16 plans, fp64 on f32, f32m and f64 plans, in a fixed order, no atomics; each output is rounded to fp32 once.
 * Outputs, in OUTPUT joint order (row r, head joint permutation[r]); rows n .. max_n - 1 are not touched:
 *   d_voxel_out int32 [max_n, n_joints_out, k]
 *   d_stats_out fp32  [max_n, n_joints_out, k, 11]: mass, peak, coords01 (3), cov01 (6)
 * Binding is HOST state: a forward reads the pointers when it enqueues, so rebinding (or unbinding: all three pointers NULL and
 * max_n = k = radius = 0) between two enqueues needs no synchronisation; the buffers must stay alive until the forwards enqueued
 * while they were bound have run.  Anything but the unbind call is checked in full: three non-NULL pointers, the scratch 16-byte
 * and the outputs 4-byte aligned, max_n in [1, the plan's max_batch], k and radius in their ranges.  d_scratch:
 * metro_plan_modes_scratch_bytes(plan, max_n) bytes (-1 for a bad argument); on f16 plans whose head keeps the logits on chip it
 * receives them as fp32 (the head kernels' layer-dump store), else the logits are read from the workspace.
 * While bound: a forward with n > max_n returns METRO_ERR_INVALID_ARG before any launch; forwards make PLAIN launches (the
 * hipGraph cache does not serve them); one launch (heat_modes: csrc/heat_modes.hip) follows the finalize launch, and the three
 * marginal launches when those are bound.  Heat-maps and modes may be bound together: the head's one fp32 logits store then goes
 * to the heat-map scratch and the modes read it there; each output is bit for bit what it is when bound alone.  A shape whose
 * volume does not fit the kernel's LDS (S * S * D flag bytes and three y-rows of logits in 64 KB) returns METRO_ERR_UNSUPPORTED.
 * Poses, coords01, covariance, peak and status words keep the bits of the unbound call.  Unbound, a forward enqueues exactly the
 * kernels it always did. */
#define METRO_MAX_MODES 8
#define METRO_MAX_MODE_RADIUS 3
int64_t metro_plan_modes_scratch_bytes(const MetroPlan* plan, int32_t max_n);
int  metro_plan_bind_modes(MetroPlan* plan, int32_t* d_voxel_out, float* d_stats_out, void* d_scratch,
                           int32_t max_n, int32_t k, int32_t radius);
/* ---- per-joint heat-map posterior under a Gaussian prior, bound to the plan ----
 * Moments, marginals and modes describe what the net believes on its own.  This lets the caller tell the forward what it already
 * knows (a tracker's prediction, the previous frame's pose, another camera's ray): a Gaussian prior is multiplied into the joint's
 * softmax before the expectation, so the posterior mean is taken from the peak that agrees with the prior, the posterior
 * covariance is that peak's, and the evidence is the probability the heat-map gives to the prior's region -- the quantity a
 * tracker gates a measurement with.  Exact over the whole S x S x D volume.  With prior buffers bound, every forward entry (the
 * list above) also writes the posterior on the stream it is given, from the logits of the same forward.  Definition, for crop
 * i < n, output joint r and head joint j = permutation[r]:
 *   l[v] = logits[i, y, x, d * J + j] over the voxels v = (y * S + x) * D + d;  g(v) = (gx[x], gy[y], gz[d]) the soft-argmax's own
 *   fp32 grids (fp32 linspace(0,1,S) for x and y, linspace(0,1,D) for z; a grid of one point is 0).
 *   Input   d_prior fp32 [max_n, n_joints_out, 9], OUTPUT joint order: per row mu (x, y, z, in coords01 units) and the precision
 *           L (xx, yy, zz, xy, xz, yz: the order of cov01, units of 1 / coords01^2).  L must be symmetric positive semi-definite
 *           and may be singular: a zero row and column means "no knowledge along that axis" (callers use this for z, whose absolute
 *           heat-map position the model does not pin).  The device does not check definiteness.
 *   Energy     q(v) = -1/2 (g(v) - mu)^T L (g(v) - mu)
 *   Posterior  w[v] = l[v] + q(v),  M' = max w,  p'[v] = exp(w[v] - M') / S',  S' = sum exp(w - M')
 *   Output  d_post_out fp32 [max_n, n_joints_out, 11], the layout of the mode stats with the mass slot replaced:
 *           log_evidence = (M' - M) + ln(S' / S), M and S the joint's plain maximum and normaliser, both sums formed by the same
 *             code in the same order (= ln sum_v p[v] exp(q(v)); <= 0 for a positive semi-definite L);
 *           peak' = max p';  coords01' = sum p' g (x, y, z);  cov01' = the six central second moments of p' about coords01', in the
 *           order (xx, yy, zz, xy, xz, yz).  Rows n .. max_n - 1 are not touched.
 *   Special rows: a zero L gives log_evidence exactly 0.0 and the plain distribution's statistics in the other ten values.  A NaN in
 *   the joint's mu or L, a NaN or +Inf logit, or a non-finite M' gives NaN in all 11 values of that joint only; a -Inf logit is a
 *   voxel of weight zero.  No other joint and no other crop is affected; the crop's pose, status word and METRO_ERR_NONFINITE are
 *   those of the unbound call.
 *   Sums: fp32 on f16 plans, fp64 on f32, f32m and f64 plans (the logits are read as fp64 on f64 plans); q is evaluated in the
 *   accumulator type; fixed order, no atomics; each output is rounded to fp32 once.  The central moments are formed about the
 *   posterior mean, not as E[g^2] - E[g]^2.
 * Binding is HOST state: a forward reads the pointers when it enqueues, so rebinding (or unbinding: all three pointers NULL and
 * max_n = 0) between two enqueues needs no synchronisation; the buffers must stay alive until the forwards enqueued while they
 * were bound have run.  Anything but the unbind call is checked in full: three non-NULL pointers, the scratch 16-byte and the
 * others 4-byte aligned, max_n in [1, the plan's max_batch].  d_scratch: metro_plan_prior_scratch_bytes(plan, max_n) bytes (-1 for
 * a bad argument); on f16 plans whose head keeps the logits on chip it receives them as fp32, else the logits are read from the
 * workspace.
 * While bound: a forward with n > max_n returns METRO_ERR_INVALID_ARG before any launch; forwards make PLAIN launches (the
 * hipGraph cache does not serve them); one launch (heat_posterior: csrc/heat_posterior.hip) follows the finalize launch, the three
 * marginal launches and the modes launch when those are bound.  All three may be bound together: the head's one fp32 logits
 * store goes to the heat-map scratch if heat-maps are bound, else to the modes scratch, else to this one, and the others read
 * the logits there; each output is bit for bit what it is when bound alone.  A shape the kernel cannot serve (more than 2^24
 * voxels a joint) returns METRO_ERR_UNSUPPORTED.  Poses, coords01, covariance, peak and status words keep the bits of the unbound
 * call.  Unbound, a forward enqueues exactly the kernels it always did. */
int64_t metro_plan_prior_scratch_bytes(const MetroPlan* plan, int32_t max_n);
int  metro_plan_bind_prior(MetroPlan* plan, const float* d_prior, float* d_post_out, void* d_scratch, int32_t max_n);
/* ---- the prior of the posterior above from the track table, bound to the plan ----
 * metro_plan_bind_prior takes prior rows in heat-map units of one particular crop, a frame no caller has a pose in.  A tracked
 * joint lives in the camera or the world, in mm, with a covariance (the [T, n_joints_out, 28] constant-velocity table of
 * metro_associate_tracks / metro_smooth_tracks).  While this is bound, every forward entry (the list above) first writes the
 * prior rows itself, one launch (track_priors: csrc/track_priors.hip) behind the finalize launch -- and behind the marginal and
 * modes launches when those are bound -- and then runs the heat_posterior launch of metro_plan_bind_prior on the rows it wrote.
 * No launching entry is added.  Definition, for crop row i < n and output joint r, fp64 on the stored inputs:
 *   1. Slot.  s = d_slot[i].  No prior (reason 1) if s is outside [0, capacity).
 *   2. Source joint.  q = r, or d_mirror[r] where the row's record has det(rot) <= 0 (a flipped test-time view; rot is
 *      rot_to_world for a world table, else rot_to_orig_cam; metro_merge_views' rule).  No prior (reason 2) if the state
 *      d_state[s, q] holds none (t_last NaN) or q lies outside the skeleton.
 *   3. Time.  t = d_times[i]; a non-finite t: no prior (reason 6).  t - t_last > max_age_s: no prior (reason 3).
 *   4. Prediction.  The constant-velocity prediction of metro_smooth_tracks over dt = max(t - t_last, 0) with q = accel_psd: x
 *      and P.  C = cov_scale P_pos + sigma_floor_mm^2 I.
 *   5. Into the crop's virtual camera.  World table: c = rot_to_world^T (x - cam_loc); camera table: c = rot_to_orig_cam^T x.
 *      C_c = R^T C R.  A non-finite c: no prior (reason 6).  c.z < near_mm: no prior (reason 4).
 *   6. Pixel.  K = inv(inv_intrinsics) in closed form, fp64 from the fp32 record; (u, v) = the first two rows of K on
 *      (c.x / c.z, c.y / c.z, 1) (a camera matrix ends in (0, 0, 1)), with the 2x3 Jacobian of that map.
 *   7. Heat-map units.  mu_xy = ((u, v) - half_stride) / last_receptive_center, the inverse of heatmap_to_image
 *      (volumetric.py:288-295); the Jacobian is divided by last_receptive_center.  A non-finite mu: no prior (reason 6).
 *   8. xy precision.  Sigma = J C_c J^T (2x2), L_xy = Sigma^-1 by cofactors.  A non-finite or non-positive determinant: no prior
 *      (reason 5).
 *   9. Depth.  The model pins z only relative to the root (volumetric.py:52-56).  METRO_TRACK_PRIOR_DEPTH_NONE: the z row and
 *      column of L are 0 and mu_z = 0.  METRO_TRACK_PRIOR_DEPTH_ROOT, for every output joint but the root's (head joint
 *      n_joints_head - 1), when steps 2 to 5 give a point c_root, C_c,root for the root joint of the same slot at the same t:
 *        mu_z = coords01[i, n_joints_head - 1, 2] + (c.z - c_root.z) / box_size_mm,   L_zz = box_size_mm^2 / (C_c[2,2] + C_c,root[2,2]),
 *      coords01 the plain soft-argmax output of the same forward; the xz and yz words are 0.  The root's own row, and a joint
 *      whose root gives no point, have the zero z block.  The z term ignores the correlation of z with the projected xy (a
 *      joint's depth error also moves its pixel) and the correlation between a joint and its root (the table keeps the joints
 *      as independent filters); it is anchored at the plain root mean, not at the root's posterior.
 *   Outputs, rows n .. max_n - 1 untouched:
 *     d_prior_out  fp32 [max_n, n_joints_out, 9]: mu x, y, z; L xx, yy, zz, xy, xz, yz -- metro_plan_bind_prior's layout, each
 *                  word rounded to fp32 once; nine zeros where there is no prior, for which the posterior has log_evidence
 *                  exactly 0 and the plain statistics (its special row);
 *     d_reason_out int32 [max_n, n_joints_out]: 0 prior given, 1 no slot, 2 no state, 3 too old, 4 behind or too near the
 *                  camera, 5 covariance not invertible, 6 non-finite input;
 *     d_post_out   fp32 [max_n, n_joints_out, 11]: metro_plan_bind_prior's output under d_prior_out.
 * Inputs, all DEVICE memory read when the forward runs: d_state fp64 [capacity, n_joints_out, 28]; d_slot int32 [max_n];
 * d_times fp64 [max_n]; d_records max_n MetroPlacement; d_mirror int32 [n_joints_out].  `params` is HOST memory, copied at bind
 * time.  d_scratch: metro_plan_prior_scratch_bytes(plan, max_n) bytes.
 * Binding is HOST state, as for the binds above; unbind with every pointer NULL and capacity = max_n = 0.  Anything else is
 * checked in full and returns METRO_ERR_INVALID_ARG: a NULL pointer, the scratch not 16-byte, d_state and d_times not 8-byte or
 * another pointer not 4-byte aligned, max_n outside [1, the plan's max_batch], capacity outside [1, METRO_ASSOC_MAX], coords
 * other than METRO_COORDS_CAMERA / METRO_COORDS_WORLD, depth other than the two modes, a negative or non-finite parameter,
 * DEPTH_ROOT on a skeleton whose output order does not carry head joint n_joints_head - 1, and binding while
 * metro_plan_bind_prior is bound (metro_plan_bind_prior likewise refuses while this is bound: one prior per forward).
 * While bound: a forward with n > max_n, or a forward entry called without a coords01 output while DEPTH_ROOT is bound, returns
 * METRO_ERR_INVALID_ARG before any launch; forwards make PLAIN launches; the head's one fp32 logits store goes to the heat-map
 * scratch, else to the modes', else to this one.  Poses, coords01, covariance, peak, status words, heat-maps and modes keep the
 * bits of the unbound call.  Unbound, a forward enqueues exactly the kernels it always did. */
#define METRO_TRACK_PRIOR_DEPTH_NONE 0
#define METRO_TRACK_PRIOR_DEPTH_ROOT 1
typedef struct MetroTrackPrior {
    int32_t coords;             /* METRO_COORDS_CAMERA or METRO_COORDS_WORLD: the frame of the track table                 */
    int32_t depth;              /* METRO_TRACK_PRIOR_DEPTH_*                                                                */
    double accel_psd;           /* q of the constant-velocity model, mm^2 / s^3 (metro_smooth_tracks)                      */
    double max_age_s;           /* a state older than this at the row's time gives no prior                                */
    double near_mm;             /* a joint nearer than this to the crop's camera plane gives no prior                      */
    double sigma_floor_mm;      /* added in quadrature to every axis of the predicted position                             */
    double cov_scale;           /* factor on the predicted position covariance                                             */
} MetroTrackPrior;              /* 48 bytes */
struct MetroPlacement;          /* defined below, with metro_place_poses */
int  metro_plan_bind_track_prior(MetroPlan* plan, const double* d_state, int32_t capacity, const int32_t* d_slot,
                                 const double* d_times, const struct MetroPlacement* d_records, const int32_t* d_mirror,
                                 const MetroTrackPrior* params, float* d_prior_out, int32_t* d_reason_out, float* d_post_out,
                                 void* d_scratch, int32_t max_n);
/* ---- a person's heat-maps from several cameras, fused on a grid of world points, bound to the plan ----
 * Nothing in the reference (its examples have one camera each).  metro_triangulate_joints reduces every crop to the mean of its
 * heat-map before the cameras meet; the mean of a two-peaked joint lies between the peaks and bends that camera's ray.  The
 * exact multi-view answer keeps the distributions: the product of the cameras' xy marginals along their rays, evaluated on a
 * grid of world points.  A wrong peak in one camera finds no partner in the others and vanishes from the product.  With TWO
 * cameras the wrong peak's ray still meets the other camera's ray and nothing resolves it: that is inherent, three views are
 * needed.  The bilinear probabilities are a coarser model than the soft-argmax, so on clean heat-maps the triangulated point
 * is the better one: the fusion is returned beside it and replaces nothing.
 * While this is bound, every forward entry (the list above) ends with the launch view_fusion (csrc/view_fusion.hip), one
 * workgroup per (person, output joint), behind the marginal launches (and every other bound launch) of the same forward, and
 * -- with d_centres NULL -- first with the launch of metro_triangulate_joints on the forward's own coords01 and cov01, the
 * bound CSR, records, mirror table, weights and min_det, whose points go to d_centres_out, bit for bit what that entry gives
 * on the same inputs (its n_rays and residual pass through d_info_out and d_stats_out, which view_fusion then overwrites).
 * With d_centres given (a track's prediction, say) those are copied to d_centres_out and no triangulation runs.  No launching
 * entry is added.  Definition, for person p < n_persons and output joint r, n the forward's crops; fp64 arithmetic on the
 * stored fp32 inputs, each output rounded to fp32 once:
 *   Grid.     X[a,b,c] = centre + (g[a], g[b], g[c]), g[i] = -extent_mm / 2 + i extent_mm / (G - 1), the axes world x, y, z; the
 *             point's index is v = (a G + b) G + c.  A centre that is not finite: NaN in every float output, rows used 0, edge 0.
 *   Rows.     The person's group is d_rows[d_starts[p] : d_starts[p + 1]] with metro_triangulate_joints' clamping.  Row i uses
 *             the map d_xy[i, flipped ? d_mirror[r] : r], flipped = !(det rot_to_world > 0) (metro_place_poses' rule).
 *   Skipped.  A row outside [0, n); a row whose record has a non-finite inv_intrinsics, rot_to_world or cam_loc entry; a row
 *             whose mirror joint lies outside the skeleton; a row whose map has a non-finite cell (the marginals' NaN rule
 *             for a bad joint).  Skipped rows are not counted.
 *   Project.  c = rot_to_world^T (X - cam_loc); K = inv(inv_intrinsics) in closed form; (u, v) = the first two rows of K on
 *             (c.x / c.z, c.y / c.z, 1); m = ((u, v) - half_stride) / last_receptive_center, the inverse of heatmap_to_image;
 *             f = m (S - 1).
 *   Sample.   If c.z > near_mm and 0 <= f.x, f.y <= S - 1: x0 = min(floor(f.x), S - 2), likewise y0, p the bilinear value of
 *             the four cells (never above the map's largest cell), l = ln max(p, floor).  Otherwise l = ln floor.
 *   Energy.   E[v] = (1 / n_views) sum over the used rows of l, in row order.
 *   Softmax.  M = max E at the lowest v among equals; w = exp(E - M) / sum exp(E - M).
 *   Outputs:
 *     d_points_out  fp32 [n_persons, n_joints_out, 3]: sum w X, world mm;
 *     d_cov_out     fp32 [n_persons, n_joints_out, 9]: the central second moments of X under w, mm^2, row-major symmetric 3x3
 *                   (the layout metro_smooth_tracks reads);
 *     d_stats_out   fp32 [n_persons, n_joints_out, 2]: max w, and agreement = M - (1 / n_views) sum over the used rows of
 *                   ln max(largest cell of the row's map, floor): <= 0, near 0 when all cameras' peaks meet in one point;
 *     d_info_out    int32 [n_persons, n_joints_out, 2]: the rows used, and edge = 1 when the point of M has an index 0 or G - 1
 *                   on some axis (the cube was too small);
 *     d_centres_out fp32 [n_persons, n_joints_out, 3]: the centres used.
 *   A group with no usable row has NaN in points, cov and stats, and (0, 0) in info.
 * Inputs, all DEVICE memory read when the forward runs: d_xy fp32 [max_n, n_joints_out, S, S], S the heat-map side -- in the
 * product the very buffer metro_plan_bind_heatmaps writes, but any buffer will do and the heat-map binding is not required;
 * d_records max_n MetroPlacement; d_rows int32 [n_rows]; d_starts int32 [n_persons + 1]; d_mirror int32 [n_joints_out];
 * d_centres fp32 [n_persons, n_joints_out, 3] or NULL.  `params` is HOST memory, copied at bind time.
 * Binding is HOST state, as for the binds above; unbind with every pointer NULL and n_rows = n_persons = max_n = 0.  Anything
 * else is checked in full and returns METRO_ERR_INVALID_ARG: a NULL pointer other than d_centres, a pointer not 4-byte
 * aligned, max_n outside [1, the plan's max_batch], n_rows or n_persons negative, grid outside [2, 16], n_views < 1, weights
 * other than METRO_TRI_UNIFORM / METRO_TRI_COVARIANCE, extent_mm not finite and > 0, floor outside (0, 1), near_mm not finite
 * and >= 0, min_det not finite, and a plan whose heat-map side is below 2.
 * While bound: a forward with n > max_n -- and, with d_centres NULL, a forward entry without a coords01 output, or under
 * METRO_TRI_COVARIANCE without a cov01 output -- returns METRO_ERR_INVALID_ARG before any launch; forwards make PLAIN launches
 * (the hipGraph cache does not serve them).  Every other output keeps the bits of the unbound call.  Unbound, a forward
 * enqueues exactly the kernels it always did. */
typedef struct MetroViewFusion {
    int32_t grid;               /* G points per axis, 2..16                                                                */
    int32_t n_views;            /* V >= 1: the rows per camera (test-time views); a row counts 1 / V                       */
    int32_t weights;            /* METRO_TRI_UNIFORM or METRO_TRI_COVARIANCE, of the internal triangulation                */
    double extent_mm;           /* the cube's side, > 0 (at offset 16)                                                     */
    double floor;               /* the least probability a row gives a point, in (0, 1)                                    */
    double near_mm;             /* a point nearer than this to a camera's plane takes the floor there, >= 0                */
    double min_det;             /* of the internal triangulation (metro_triangulate_joints)                                */
} MetroViewFusion;              /* 48 bytes; copied at bind */
int  metro_plan_bind_view_fusion(MetroPlan* plan, const float* d_xy, const struct MetroPlacement* d_records, const int32_t* d_rows,
                                 int32_t n_rows, const int32_t* d_starts, int32_t n_persons, const int32_t* d_mirror,
                                 const float* d_centres, const MetroViewFusion* params, float* d_points_out, float* d_cov_out,
                                 float* d_stats_out, int32_t* d_info_out, float* d_centres_out, int32_t max_n);
/* ---- which heat-map mode every joint is in, decided by the person's bone lengths: tree inference per crop, bound to the plan ----
 * Nothing in the reference (it reduces every heat-map to its mean, volumetric.py:227-235).  metro_plan_bind_modes gives per
 * joint the k places it may be; every entry above treats the joints of one person as independent.  The skeleton ties them
 * together: of a wrist's two peaks only one is a forearm's length from the elbow.  The skeletons of all three datasets are
 * trees, so "which mode of every joint" is exact inference on a tree per crop.
 * While this is bound, every forward entry (the list above) enqueues the launch skeleton_modes (csrc/skeleton_modes.hip), one
 * workgroup of 64 lanes per crop row, behind heat_modes of the same forward (behind the finalize launch where modes are not
 * bound).  No launching entry is added.  Definition, for crop row i < n, n the forward's crops; fp64 arithmetic on the stored
 * fp32 inputs in a fixed order, each output rounded to fp32 once:
 *   Present.    Mode k of output joint r is present if voxel[i, r, k] >= 0, its mass is finite and > 0 and its coords01 and
 *               cov01 are finite.  A joint with no present mode is DEAD; all of its edges are cut.
 *   Unary.      w[r, k] = mass / (the sum of the joint's present masses, in mode order).
 *   Geometry.   x[r, k] = scale_mm * coords01 (per axis), C[r, k] = diag(scale_mm) Cov01 diag(scale_mm).
 *   Known edge. Edge e = (p, q) is known for the row if lengths[i, e] = L is finite and > 0 and both joints are alive.
 *   Pair.       For present modes ka of p and kb of q on a known edge: d = x[q, kb] - x[p, ka], l = |d|, u = d / l,
 *               s = max(0, u^T (C[p, ka] + C[q, kb]) u) (a third of the trace where l < min_length_mm or l = 0),
 *               v0 = sigma_mm^2 + (sigma_rel L)^2, v = v0 + cov_scale s,
 *               ln psi = -(l - L)^2 / (2 v) - 1/2 ln(v / v0)  (<= 0: a Gaussian likelihood of the bone length, normalised so that
 *               a sharp, exact pair scores 0).
 *   Component.  A maximal set of alive joints joined by known edges.  Over its assignments k, P(k) ~ prod w prod psi.
 *   Outputs (rows n .. max_n - 1 are not touched):
 *     d_prob_out   fp32 [max_n, n_joints_out, k]: the exact marginal of every mode; 0 for an absent mode of an alive joint,
 *                  NaN for a dead joint; the unaries w themselves in a component of one joint;
 *     d_choice_out int32 [max_n, n_joints_out]: the MAP assignment, by max-product with back-tracking from the component's
 *                  lowest-numbered joint, the lowest index among equals at every step; -1 for a dead joint;
 *     d_info_out   fp32 [max_n, n_joints_out, 2]: log_evidence = ln sum_k prod w prod psi of the joint's component (<= 0,
 *                  exactly 0.0 for a component without a known edge) and log_map = ln P(the MAP assignment); NaN for a dead joint;
 *     d_coords01_sel_out fp32 [max_n, n_joints_head, 3] or NULL: the forward's coords01 with head joint permutation[r]
 *                  replaced by the chosen mode's coords01 for every alive output joint r (of output joints that share a head
 *                  joint the last); dead joints and head joints outside the output order keep the plain mean.
 *   No other crop, and no joint other than a dead one, is affected by a NaN.
 * It can only choose among the modes heat_modes found; lengths are compared in MeTRo's metric scale (heatmap_to_metric's linear
 * part, which `scale_mm` is); the covariance of a mode is its window's; a skeleton with a cycle is refused.  The defaults of
 * the host side -- sigma_mm 20, sigma_rel 0, cov_scale 1, min_length_mm 1 -- are design choices, not measurements.
 * Inputs, all DEVICE memory read when the forward runs: d_voxel int32 [max_n, n_joints_out, k] and d_stats fp32 [max_n,
 * n_joints_out, k, 11] in metro_plan_bind_modes' layout -- in the product the very buffers that binding writes, but any buffers
 * will do and the modes binding is not required; d_lengths fp64 [max_n, n_edges], mm.  h_edges int32 [n_edges, 2] (output-joint
 * indices) and `params` are HOST memory, copied at bind time with the rooted schedule derived from the edges.
 * Binding is HOST state, as for the binds above; there is no scratch; unbind with every pointer NULL and k = n_edges = max_n = 0.
 * Anything else is checked in full and returns METRO_ERR_INVALID_ARG: a NULL pointer other than d_coords01_sel_out (h_edges may
 * be NULL with n_edges 0), d_lengths not 8-byte or another pointer not 4-byte aligned, max_n outside [1, the plan's max_batch],
 * k outside [1, METRO_MAX_MODES], n_edges outside [0, 63], an edge with a joint outside [0, n_joints_out), a self-edge or an
 * edge that closes a cycle (the message names the edge), scale_mm or sigma_mm not finite and > 0, sigma_rel, cov_scale or
 * min_length_mm not finite and >= 0.
 * While bound: a forward with n > max_n, and a forward entry without a coords01 output while d_coords01_sel_out is bound,
 * return METRO_ERR_INVALID_ARG before any launch; forwards make PLAIN launches (the hipGraph cache does not serve them).  Every
 * other output keeps the bits of the unbound call.  Unbound, a forward enqueues exactly the kernels it always did. */
typedef struct MetroSkeletonModes {
    double scale_mm[3];         /* mm per coords01 unit (x, y, z): the linear part of heatmap_to_metric, > 0                */
    double sigma_mm;            /* sd of a bone's length, > 0                                                              */
    double sigma_rel;           /* and the part of it that grows with the length, >= 0                                     */
    double cov_scale;           /* how much of the modes' own covariance along the bone widens the likelihood, >= 0        */
    double min_length_mm;       /* below this distance the bone has no direction: a third of the trace is used, >= 0       */
} MetroSkeletonModes;           /* 56 bytes; copied at bind */
int  metro_plan_bind_skeleton_modes(MetroPlan* plan, const int32_t* d_voxel, const float* d_stats, int32_t k, const double* d_lengths,
                                    const int32_t* h_edges, int32_t n_edges, const MetroSkeletonModes* params, float* d_prob_out,
                                    int32_t* d_choice_out, float* d_info_out, float* d_coords01_sel_out, int32_t max_n);
/* Same, stopping after layer `last_layer` (inclusive) so tests can read that layer's output at
 * MetroLayerInfo.out_offset in the workspace.  d_poses_out may be NULL if the finalize layer
 * is not reached. */
int  metro_forward_upto(MetroPlan* plan, const float* d_images_nhwc, int32_t n,
                        float* d_poses_out, void* d_workspace, void* stream,
                        int32_t last_layer);

/* ---- per-layer timing on the launch stream (HIP events around every launch; this is what
 *      bench.py's roofline object is computed from).  ms_out[i] accumulates layer i's time. ---- */
int  metro_forward_timed(MetroPlan* plan, const float* d_images_nhwc, int32_t n,
                         float* d_poses_out, void* d_workspace, void* stream,
                         float* ms_out /* [num_layers] host */);

/* ---- single-kernel entry points (parity tests call these through ctypes) ---- */

/* Implicit-GEMM convolution over NHWC (replaces slim.conv2d / conv2d_same call sites:
 * reference resnet_v2.py:123-136,219-220,233-236; resnet_utils.py:82-135).  Generic over
 * kernel size, stride, dilation and asymmetric TF padding; optional per-input-channel
 * scale/shift+ReLU prologue (pre-activation BN, resnet_v2.py:119,229) and
 * bias / ReLU / strided-shifted residual epilogue (resnet_v2.py:113-121,138).
 *
 * Non-finite values.  Every ReLU of the library -- the `relu` epilogue, the prologue's, those inside the fused launches and the
 * head's, in every precision -- is IEEE-754-2019 maximum(v, 0): relu(NaN) = NaN, relu(+Inf) = +Inf, relu(-Inf) = 0 (the value
 * behind a -Inf is hugely negative: zero is its ReLU).  A store rounds to the output type as IEEE does: |y| past the largest
 * fp16 (65 504) is stored as +-Inf.  A non-finite input element therefore reaches exactly the outputs it is a term of, as IEEE
 * arithmetic on the fp64 restatement of the layer gives them, and no other element of the launch: nothing outside the tensors
 * the descriptor states is ever a term of an output, whatever its bits.  That is what lets the finalize launch's screen
 * (metro_forward_status) see an overflow that began several units in front of the head. */
typedef struct MetroConvDesc {
    int32_t n, h_in, w_in, c_in;
    int32_t in_pix_stride;      /* elements between consecutive input pixels (>= c_in)      */
    int32_t h_out, w_out, c_out;
    int32_t kh, kw, stride, dilation;
    int32_t pad_top, pad_left;  /* input row = ho*stride - pad_top + r*dilation             */
    int32_t has_prologue;       /* requires kh == kw == 1 and no padding                    */
    int32_t relu;
    int32_t has_residual;
    int32_t res_h, res_w;       /* spatial dims of the residual tensor [n,res_h,res_w,c_out] */
    int32_t res_stride, res_offset; /* residual pixel = (ho*res_stride+res_offset, wo*...)  */
    int32_t out_dtype;          /* MetroDType of output AND residual: F16/F32 (fast kernel; F32 without residual), F32/F64 (precise kernel) */
    int32_t in_dtype;           /* MetroDType of the input: F16 (fast kernel), F32/F64 (precise kernel) */
} MetroConvDesc;

/* fp16 operands, fp32 MFMA accumulate (v_mfma_f32_32x32x16_f16).  Weights [c_out][kh*kw*c_in]
 * fp16, bias fp32[c_out], prologue scale/shift fp16[c_in], residual fp16 (F16 output only: F32 output with a
 * residual is rejected).  c_in % 8 == 0, c_in <= 2048, c_out % 4 == 0 (% 8 with a residual). */
int  metro_conv_f16(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                    const void* d_pro_scale, const void* d_pro_shift, const void* d_residual,
                    void* d_out, void* stream);
/* Two 1x1 convolutions of a bottleneck unit on the SAME pre-activated input in one launch: the projection
 * shortcut (rows [0, split) of d_w / d_bias, no ReLU, -> d_out with `split` channels) and conv1 with its folded
 * BN + ReLU (rows [split, d->c_out) -> d_out2 with d->c_out - split channels).  Replaces the two
 * layers_lib.conv2d calls of reference src/model/resnet_v2.py:122-128.  d->has_prologue = 1, no residual. */
int  metro_conv_f16_pair(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                         const void* d_pro_scale, const void* d_pro_shift, void* d_out, int32_t split,
                         void* d_out2, void* stream);
/* conv3 (+bias, + shortcut) of unit u and conv1 (pre-activation BN+ReLU of unit u+1, folded BN + ReLU) of
 * unit u+1 in one launch (block1 shapes: c_in = c2 = 64, c_out = 256):
 *   d_out  = conv(d_in) + bias + residual                          (resnet_v2.py:134-138 of unit u)
 *   d_out2 = relu(W2 * relu(d_out * scale2 + shift2) + bias2)      (resnet_v2.py:119,127-128 of unit u+1)
 * W2 fp16 [c2][c_out], bias2 fp32 [c2], scale2/shift2 fp16 [c_out], d_out2 fp16 [.., c2]. */
int  metro_conv_f16_next(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                         const void* d_residual, void* d_out, const void* d_w2, const float* d_bias2,
                         const void* d_scale2, const void* d_shift2, void* d_out2, int32_t c2, void* stream);
/* block1/unit_1 in two launches (the unit's input has only 64 channels, so recomputing beats storing):
 * metro_conv_f16_conv1_conv2 -- conv1 (1x1, 64 -> 64, folded BN + ReLU) on relu(x * pro_scale + pro_shift), then conv2 (3x3, SAME,
 *   folded BN + ReLU; d = ITS descriptor, relu = 1) in one launch; conv1's output lives in LDS only (reference
 *   resnet_v2.py:119,127-132).  d_x fp16 [n,h,w,64], d_w1 fp16 [64][64], d_w2 fp16 [64][3][3][64], d_out fp16 [n,h,w,64].
 * metro_conv_f16_next_proj -- metro_conv_f16_next with the unit's PROJECTION shortcut computed in the launch:
 *   d_out = fp16(conv3(d_in) + bias) + fp16(Wsc * relu(d_x * pro_scale + pro_shift) + bias_sc)   (resnet_v2.py:119,122-125,134-138)
 *   d_out2 = relu(W2 * relu(d_out * scale2 + shift2) + bias2)                                    (unit u+1, :119,127-128)
 *   d->has_residual = 0; d_x fp16 [.., 64] the unit's raw input, d_w_sc fp16 [256][64], d_bias_sc fp32 [256].
 *   d_out == NULL: the sum is NOT stored (it only feeds the second GEMM): the form metro_forward runs for block1/unit_1 (round 5).
 * metro_conv_f16_next_rebuild -- the launch of block1/unit_2 (round 5): the unit's identity shortcut x_1 is REBUILT from the tensors
 *   it is a function of instead of being read as a 512-byte-per-pixel tensor:
 *   x_1    = fp16(W3_prev * d_t2_prev + bias3_prev) + fp16(Wsc * relu(d_x * pro_scale + pro_shift) + bias_sc)      (unit 1, :119-138)
 *   d_out  = fp16(conv3(d_in) + bias) + x_1                                                                        (unit 2, :120-121,134-138)
 *   d_out2 = relu(W2 * relu(d_out * scale2 + shift2) + bias2)                                                      (unit 3, :119,127-128)
 *   with the MFMAs, k order and fp16 roundings of the launches that would have stored x_1: the same bits.  Exactly one of d_out
 *   (the whole sum, fp16 [n,h,w,256]) and d_out_sub (pixels (sub_off + 2i, sub_off + 2j) of it as a compact
 *   [n, ceil((h - sub_off) / 2), ceil((w - sub_off) / 2), 256] tensor: what a strided unit 3's shortcut reads, resnet_v2.py:113-121)
 *   must be non-NULL.  w a power of two >= 16, h * w % 64 == 0. */
int  metro_conv_f16_conv1_conv2(const MetroConvDesc* d, const void* d_x, const void* d_w1, const float* d_bias1, const void* d_pro_scale,
                                const void* d_pro_shift, const void* d_w2, const float* d_bias2, void* d_out, void* stream);
int  metro_conv_f16_next_proj(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias, const void* d_x,
                              const void* d_w_sc, const float* d_bias_sc, const void* d_pro_scale, const void* d_pro_shift, void* d_out,
                              const void* d_w2, const float* d_bias2, const void* d_scale2, const void* d_shift2, void* d_out2,
                              int32_t c2, void* stream);
int  metro_conv_f16_next_rebuild(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias, const void* d_x,
                                 const void* d_w_sc, const float* d_bias_sc, const void* d_pro_scale, const void* d_pro_shift,
                                 const void* d_t2_prev, const void* d_w3_prev, const float* d_bias3_prev, void* d_out, void* d_out_sub,
                                 int32_t sub_off, const void* d_w2, const float* d_bias2, const void* d_scale2, const void* d_shift2,
                                 void* d_out2, int32_t c2, void* stream);
/* Test switch (thread-local) for the two entry points above when their sum stays on chip or is rebuilt: metro_forward runs them on
 * the producer / consumer kernel of conv_b1.hip ("conv_b1_chain<...>"); 1 = run the classic single-role kernel of conv_pw64.hip
 * instead (what metro_forward_upto stopping at such a layer runs): two independent forms that must give the same bits.
 * It also switches metro_conv_f16 between conv_pws.hip's skewed kernel (default; conv3 + shortcut of blocks 3-4) and
 * conv_pw64.hip's lock-step one (1), and metro_conv_f16_pair on block2's shapes (256 -> 512 + 128) between the weight-resident
 * kernel conv_pw64<k256,wm8,cb512,pro,pair> (default, round 5) and the ring kernel it replaced (1): again the same bits.
 * Round 6: and the dilated 3x3 layers whose halo exceeds the tap-reuse kernel's slab (rate 4 / 8 at stride 4 and 8) between that
 * kernel in sub-grid pixel order ("conv3x3_f16_slab<...>+subgrid", default) and the generic ring kernel (1): two fp32 summation
 * orders of the same products (chunk-major / tap-major), equal up to rounding flips of the fp16 result. */
int  metro_conv_b1_form(int32_t classic);
/* The same contract as metro_conv_f16 / metro_conv_f16_pair on the 256 x 256 x 64 GEMM kernel with four waves of 128 x 128
 * (conv_gemm4w.hip: register-staged operands, one barrier per K tile), which metro_forward picks for the pre-activated deep-K
 * 1x1 layers with at least one tile per CU (conv1, projection shortcut, shortcut+conv1 pair of blocks 3-4: reference
 * resnet_v2.py:122-128; >= 256 tiles of 256 x 256, K >= 1024 or >= 1024 tiles).
 * 1x1, stride 1, c_in % 128 == 0, c_out % 256 == 0, n*h*w % 256 == 0.  split > 0: fused pair (rows [0,split) ->
 * d_out, rows [split, c_out) with ReLU -> d_out2, (c_out - split) % 256 == 0); split == 0: plain layer, d_out2 ignored.
 * Same K order and one fp32 accumulator per output as every other fp16 conv kernel here: bit-identical to them.
 * Round 6: the entry picks the tile itself, as metro_forward does -- whole 256 x 256 tiles; HALF tiles (256 cout x 128 pixels) for
 * a layer with fewer than 256 whole but >= 224 half tiles and K >= 1024 (block4's conv1 at 64 crops); QUARTER tiles (256 x 64) for
 * K >= 2048 below that (32 crops); a pair whose first output fills whole rounds of 256 CUs while its second one has < 256 whole
 * tiles as whole + half tiles in one grid (block4's pair at 64 crops).  metro_last_kernel_id names the forms
 * ("conv_gemm4w<256x128,pro>", "...<256x256,pro>+pair & ...<256x128,pro>+pair").  Same bits whatever the tile.
 * (Two earlier forms of this GEMM that metro_forward never dispatches -- conv_gemm8p, conv_gemm4d -- are built into
 * libmetro_experimental.so: metro_pose3d_amd/csrc/experimental/metro_experimental.h.) */
int  metro_conv_f16_gemm4w(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                           const void* d_pro_scale, const void* d_pro_shift, const void* d_residual, void* d_out,
                           int32_t split, void* d_out2, void* stream);
/* Stem 7x7/2 convolution (+bias) and zero-padded 3x3/2 max-pool in one launch (reference resnet_v2.py:219-224,
 * resnet_utils.py:138-185).  d_prepped = metro_prep_input_f16 output [n,side+6,side+8,4] fp16, d_w packed
 * [64][7][8][4] fp16, d_out fp16 [n,side/4,side/4,64].  side % 32 == 0. */
int  metro_stem_pool_f16(const void* d_prepped, const void* d_w, const float* d_bias, void* d_out, int32_t n,
                         int32_t side, void* stream);
/* Same, reading the fp32 NHWC crops [n,side,side,3] directly: the fp32->fp16 cast (reference
 * src/model/architectures.py:29) and the stem's zero border happen on the way into LDS. */
int  metro_stem_pool_f32in(const float* d_images, const void* d_w, const float* d_bias, void* d_out, int32_t n,
                           int32_t side, void* stream);
/* The twin of metro_stem_pool_f32in for uint8 NHWC crops [n,side,side,3]: byte b stands for the fp32 value b / 255 (IEEE
 * divide; normalize01, reference src/improc.py:56-61 -- what metro_warp_crop_u8 writes), so d_out has the bits of
 * metro_stem_pool_f32in on float(b) / 255.  The same sides.  d_images must be 16-byte aligned (the 256-pixel kernel fetches
 * whole 768-byte crop rows by LDS-DMA; every crop is a multiple of 16 bytes): METRO_ERR_INVALID_ARG otherwise. */
int  metro_stem_pool_u8in(const uint8_t* d_images, const void* d_w, const float* d_bias, void* d_out, int32_t n,
                          int32_t side, void* stream);
/* fp32 or fp64 activations (in_dtype / out_dtype), fp64 weights/bias/prologue,
 * v_mfma_f64_16x16x4_f64 accumulate, one rounding to out_dtype. */
int  metro_conv_f64acc(const MetroConvDesc* d, const void* d_in, const double* d_w,
                       const double* d_bias, const double* d_pro_scale,
                       const double* d_pro_shift, const void* d_residual, void* d_out,
                       void* stream);

/* fp32 activations, fp32 weights / bias / prologue, v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation): the conv
 * kernel of the METRO_PREC_F32M mode.  in_dtype = out_dtype = METRO_F32; any c_in. */
int  metro_conv_f32m(const MetroConvDesc* d, const void* d_in, const float* d_w, const float* d_bias, const float* d_pro_scale,
                     const float* d_pro_shift, const void* d_residual, void* d_out, void* stream);

/* fp32 NHWC [n,side,side,3] -> zero-bordered fp16 [n,side+6,side+8,4] (the stem's explicit
 * pad-3 of reference resnet_utils.py:125-135 materialised once; channel 3 is zero). */
int  metro_prep_input_f16(const float* d_images, int32_t n, int32_t side, void* d_out, void* stream);
/* count uint8 image values -> fp32: d_out[i] = clip(float(d_in[i]) / 255, -1, 1) with an IEEE divide (normalize01, reference
 * src/improc.py:56-61), one elementwise launch.  The fp32 image metro_forward_u8 stands for; the way uint8 crops enter the
 * two parity precisions (f32m, f64), whose metro_forward takes fp32. */
int  metro_images_u8_to_f32(const uint8_t* d_in, int64_t count, float* d_out, void* stream);

/* Crop pre-processing, the step before the path: n crops of one uint8
 * HWC RGB frame [h, w, 3] (row_stride bytes per row), crop i sampled through the 3x3 homography
 * d_homographies[i] (row-major fp32, maps OUTPUT pixel (x, y, 1) to SOURCE pixel coordinates) with
 * OpenCV's 8-bit remap rule (coordinates rounded to 1/32 px, 15-bit weights, result rounded to uint8, constant-0 border: the
 * reference warps the uint8 frame), then /255 and clip -- reference src/cameralib.py:406-429 (reproject_image_fast ->
 * cv2.remap INTER_LINEAR) + src/improc.py:56-61 (normalize01).  Every output value is k/255 for the byte k cv2 produces.
 * h, w <= 32767 (OpenCV holds the integer coordinate in a short).
 * d_out: fp32 NHWC [n, side, side, 3], exactly the input contract of metro_forward. */
int  metro_warp_crop_u8(const uint8_t* d_image, int32_t h, int32_t w, int32_t row_stride,
                        const float* d_homographies, int32_t n, int32_t side, float* d_out, void* stream);

/* Crops from MANY uint8 HWC RGB frames in one launch, with or without lens distortion of the original camera (the full
 * camera path of reference src/cameralib.py:265-324 reproject_image + src/improc.py:56-61 normalize01).
 * frames: HOST array of n_frames <= METRO_MAX_FRAMES entries (copied into the kernel arguments); frames may differ in size and
 * be separate allocations; h, w <= 32767 (cv2.remap's short coordinates), row_stride >= 3 w.
 * d_crops: DEVICE array of n MetroCropWarp records.  Crop i samples frame d_crops[i].frame (a crop whose index is outside
 * [0, n_frames) comes out as the border value 0: the index is device data, the host binding checks it) in one of two modes:
 *   METRO_WARP_HOMOGRAPHY  reproject_image_fast (cameralib.py:406-429): fp32 homography, the coordinate chain of
 *                          metro_warp_crop_u8 (bit for bit the same bytes for the same homography);
 *   METRO_WARP_DISTORTED   reproject_image case 2 (cameralib.py:294-312) for an original camera WITH distortion coefficients:
 *                          ray = partial (x, y, 1) in fp64 (the fp32 grid against the fp64 partial_homography, :297-306,
 *                          evaluated rn(rn(rn(P0 x) + rn(P1 y)) + P2)), cast to fp32, then project_points' fp32 chain in its
 *                          statement order (cameralib.py:375-397: r2, r4, r6, the distorter k1 k2 k3 1 p2 p1, the in-place
 *                          multiply-adds, K[:2,:2] and K[:2,2]); a ray with z <= 0 (or NaN) samples nothing (the border
 *                          value 0) -- the reference would project it through the origin.
 * Both modes then sample with cv2.remap's 8-bit rule exactly like metro_warp_crop_u8.  d_out: fp32 NHWC [n, side, side, 3],
 * the input contract of metro_forward. */
#define METRO_MAX_FRAMES 64
#define METRO_WARP_HOMOGRAPHY 0
#define METRO_WARP_DISTORTED 1
typedef struct MetroFrame {
    const uint8_t* data;        /* device pointer to row 0, pixel 0 */
    int32_t h, w, row_stride;   /* row_stride in bytes */
    int32_t reserved;
} MetroFrame;                   /* 24 bytes */
typedef struct MetroCropWarp {
    int32_t frame;              /* index into the frame table */
    int32_t mode;               /* METRO_WARP_HOMOGRAPHY | METRO_WARP_DISTORTED */
    double partial[9];          /* DISTORTED: row-major fp64 partial_homography = old.R inv(new.R) inv(new.K) */
    float homography[9];        /* HOMOGRAPHY: row-major, maps output pixel (x, y, 1) to source pixel coordinates */
    float intrinsics[6];        /* DISTORTED: the original camera's K[0,0] K[0,1] K[0,2] K[1,0] K[1,1] K[1,2] */
    float distortion[5];        /* DISTORTED: k1 k2 p1 p2 k3 (OpenCV order) */
} MetroCropWarp;                /* 160 bytes */
int  metro_warp_crops_frames_u8(const MetroFrame* frames, int32_t n_frames, const MetroCropWarp* d_crops, int32_t n,
                                int32_t side, float* d_out, void* stream);
/* The same launch writing the remapped BYTE ((sum of taps * weights + 2^14) >> 15, before normalize01) instead of byte / 255:
 * d_out uint8 NHWC [n, side, side, 3], the input contract of metro_forward_u8; 0 for a frame index outside [0, n_frames).
 * float(d_out) / 255 is metro_warp_crops_frames_u8's output bit for bit, at a quarter of the bytes. */
int  metro_warp_crops_frames_u8_to_u8(const MetroFrame* frames, int32_t n_frames, const MetroCropWarp* d_crops, int32_t n,
                                      int32_t side, uint8_t* d_out, void* stream);

/* metro_warp_crops_frames_u8 for frames in other pixel formats, as a decoder leaves them; the same MetroCropWarp records, modes,
 * frame-index rule and output, and frames of different formats may share one launch.  The colour conversion happens per tap
 * as the warp reads it; no RGB frame is written.
 * frames: HOST array of n_frames <= METRO_MAX_FRAMES descriptors (copied into the kernel arguments):
 *   METRO_PIX_RGB   plane[0] packed uint8 HWC RGB, stride[0] >= 3 w: the bytes of metro_warp_crops_frames_u8;
 *   METRO_PIX_BGR   the same with the channels reversed (OpenCV's order);
 *   METRO_PIX_NV12  plane[0] Y (stride[0] >= w), plane[1] interleaved UV at half resolution (stride[1] >= w); h, w even;
 *   METRO_PIX_I420  plane[0] Y (stride[0] >= w), plane[1] U and plane[2] V at half resolution (stride[1] >= w / 2, one
 *                   stride for both); h, w even.
 * A YUV frame is the RGB image of OpenCV's integer cvtColor(COLOR_YUV2RGB_NV12 / _I420) rule (limited range, chroma of the
 * 2x2 block replicated, no interpolation): u = U - 128, v = V - 128, y = max(0, Y - 16) CY,
 *   R = clamp((y + 2^19 + CVR v) >> 20), G = clamp((y + 2^19 + CVG v + CUG u) >> 20), B = clamp((y + 2^19 + CUB u) >> 20)
 * (arithmetic shifts, clamp to [0, 255]) with round(c 2^20) of the three-decimal coefficients
 *   METRO_YUV_BT601 (OpenCV's, the default)  CY 1220542  CVR 1673527  CVG -852492  CUG -409993  CUB 2116026
 *   METRO_YUV_BT709                          CY 1220542  CVR 1880097  CVG -558891  CUG -223347  CUB 2214593
 * and the warp samples that image with the remap rule above; a tap outside the frame is the border value 0 in RGB (black,
 * not YUV (0, 0, 0)).  So every crop is byte for byte metro_warp_crops_frames_u8 of the converted RGB frame.  ffmpeg's
 * swscale conversion rounds differently and is not reproduced.  matrix is ignored for RGB and BGR.
 * Checks: known format and matrix, the planes the format needs non-NULL, 0 < h, w <= 32767, the stride bounds above. */
#define METRO_PIX_RGB  0
#define METRO_PIX_BGR  1
#define METRO_PIX_NV12 2
#define METRO_PIX_I420 3
#define METRO_YUV_BT601 0
#define METRO_YUV_BT709 1
typedef struct MetroFramePlanes {
    const uint8_t* plane[3];    /* device pointers to row 0; RGB/BGR: [0] packed HWC; NV12: [0] Y, [1] UV; I420: [0] Y, [1] U, [2] V */
    int32_t h, w;               /* pixels; NV12 / I420: both even */
    int32_t stride[2];          /* bytes per row: [0] of plane 0, [1] of the chroma plane(s) */
    int32_t format, matrix;     /* METRO_PIX_*, METRO_YUV_* */
} MetroFramePlanes;             /* 48 bytes */
int  metro_warp_crops_frames_planes(const MetroFramePlanes* frames, int32_t n_frames, const MetroCropWarp* d_crops,
                                    int32_t n, int32_t side, float* d_out, void* stream);
/* metro_warp_crops_frames_planes writing the remapped byte: uint8 crops as metro_warp_crops_frames_u8_to_u8 writes them. */
int  metro_warp_crops_frames_planes_to_u8(const MetroFramePlanes* frames, int32_t n_frames, const MetroCropWarp* d_crops,
                                          int32_t n, int32_t side, uint8_t* d_out, void* stream);

/* 3x3 stride-2 max-pool over a ZERO-padded (1,1) input (reference resnet_utils.py:177-185).
 * dtype METRO_F16 / METRO_F32 / METRO_F64; c % 8 == 0 (f16), c % 4 == 0 (f32), c % 2 == 0 (f64). */
int  metro_maxpool3x3s2_zeropad(const void* d_in, void* d_out, int32_t n, int32_t h_in,
                                int32_t w_in, int32_t c, int32_t dtype, void* stream);

/* Soft-argmax over the (H,W,D) volume per joint from fp32 NHWC logits [n,side,side,depth*J]
 * (channel = d*J + j), then mm decode, root-relative and joint permutation (reference
 * volumetric.py:227-235,288-306; tfu.py:466-499; tfu3d.py:23-25; main.py:127).
 * d_partials: scratch of metro_softargmax_scratch_bytes().  precise = 0: fp32 logits, fp32
 * accumulators; 1: fp32 logits, fp64 accumulators; 2: fp64 logits, fp64 accumulators. */
int64_t metro_softargmax_scratch_bytes(int32_t n, int32_t side, int32_t n_joints_head);
int  metro_softargmax(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise,
                      void* d_partials, float* d_poses_out, void* stream);

/* The volumetric head in ONE launch, as metro_forward runs it in f16 mode for heads of <= 160 channels (head_f16.hip):
 * postnorm BN + ReLU on the raw residual stream (reference resnet_v2.py:229), the 1x1 logits convolution + bias (:233-236,
 * fp32 accumulators, architectures.py:34), the per-joint softmax statistics of every 32-pixel slab from the on-chip logits
 * tile (volumetric.py:227-235, tfu.py:466-499), then the slab fold / mm decode / root-relative / gather of metro_softargmax.
 * The kernel (tile of 256 / 128 / 64 pixels, K-parts per wave group) is chosen from the batch: results are reproducible for a
 * given n, not bit-identical across n (the K-parts are added in a fixed order that depends on the tile).
 * d_x fp16 [n, side, side, c_in]; d_w fp16 [depth * J][c_in]; d_bias fp32; d_pro_scale / d_pro_shift fp16 [c_in];
 * d_partials: metro_head_f16_scratch_bytes(); d_logits_out: optional fp32 NHWC logits dump (NULL in the product path). */
int64_t metro_head_f16_scratch_bytes(int32_t n, int32_t side, int32_t n_joints_head);
int  metro_head_f16(const void* d_x, const void* d_w, const float* d_bias, const void* d_pro_scale, const void* d_pro_shift,
                    int32_t n, int32_t c_in, const MetroSpec* spec, void* d_partials, float* d_logits_out, float* d_poses_out,
                    void* stream);

/* Evaluation metrics, the step after the path (reference
 * src/main.py:339-359): per (pose, joint) root-relative distance in mm before and after rigid
 * alignment with scale (Procrustes without reflection: src/util3d.py:139-159,
 * src/eval/procrustes.py:6-107), and per-joint sums over the valid entries of
 * {count, dist, dist_aligned, max(0, 1 - dist/threshold), dist <= threshold} -> d_sums[J][5] (fp64).
 * d_pred / d_true: fp32 [n, J, 3] (root = last joint); d_valid: uint8 [n, J]. */
int  metro_eval_metrics(const float* d_pred, const float* d_true, const uint8_t* d_valid, int32_t n,
                        int32_t n_joints, float threshold_mm, float* d_dist, float* d_dist_aligned,
                        double* d_sums, void* stream);

/* ---- alternative decode heads, the step AFTER the path ---- */
/* Soft-argmax coordinates in [0,1], head joint order, (x,y,z): the `coords3d` that
 * net_output_to_heatmap_and_coords returns (reference src/model/volumetric.py:227-235), i.e. metro_softargmax
 * without heatmap_to_metric / root_relative / gather.  d_coords01_out fp32 [n, n_joints_head, 3]. */
int  metro_softargmax01(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, void* d_scratch,
                        float* d_coords01_out, void* stream);
/* `--scale-recovery=bone-lengths` / `bone-lengths-true` (volumetric.py:171-191): heatmap_to_image (:288-295),
 * rays = inv_intrinsics . [u,v,1] (:221-222), delta_z = (z - z_root) * box_size, per-pose z offset by the
 * reference's scipy Levenberg-Marquardt solve (src/model/bone_length_based_backproj.py:38-62; MINPACK lmder
 * restated for one unknown, fp64), back_project (:284-285).  d_bone_lengths fp64 [n_edges] (dataset means) or
 * [n, n_edges] when per_pose_lengths != 0; d_edges int32 [n_edges, 2] head joint indices.  root_relative != 0
 * subtracts the last head joint (tfu3d.py:23-25); permute != 0 gathers spec->permutation (main.py:119-127).
 * d_coords3d_out fp32 [n, J, 3]; d_z_offset_out fp32 [n] or NULL. */
int  metro_backproject_bone_lengths(const float* d_coords01, const float* d_inv_intrinsics, const double* d_bone_lengths,
                                    int32_t per_pose_lengths, const int32_t* d_edges, int32_t n_edges, int32_t n,
                                    const MetroSpec* spec, int32_t root_relative, int32_t permute,
                                    float* d_coords3d_out, float* d_z_offset_out, void* stream);
/* `--scale-recovery=true-root-depth` (volumetric.py:192-199): the same with a given root depth [n] fp32. */
int  metro_backproject_root_depth(const float* d_coords01, const float* d_inv_intrinsics, const float* d_root_z,
                                  int32_t n, const MetroSpec* spec, int32_t root_relative, int32_t permute,
                                  float* d_coords3d_out, void* stream);
/* heatmap_to_25d (volumetric.py:298-300): (x, y) in crop pixels via heatmap_to_image, z * box_size_mm; head order. */
int  metro_heatmap_to_25d(const float* d_coords01, int32_t n, const MetroSpec* spec, float* d_out, void* stream);
/* to_orig_cam (volumetric.py:277-281): x' = R x per joint, joints swapped with their mirror joint when
 * det(R) <= 0.  d_rot fp32 [n,9] row-major, d_mirror int32 [n_joints]. */
int  metro_to_orig_cam(const float* d_coords, const float* d_rot, const int32_t* d_mirror, float* d_out, int32_t n,
                       int32_t n_joints, void* stream);

/* ---- absolute poses and frame keypoints of crops cut from full frames (the reference's test path with a calibrated camera:
 *      src/data/data_loading.py:110-112 hands each crop's virtual camera to src/model/volumetric.py:171-216) ---- */
/* metro_forward that ALSO writes the soft-argmax coordinates in [0,1] (what metro_softargmax01 returns: head joint order,
 * (x, y, z); volumetric.py:234-235) to d_coords01_out fp32 [n, n_joints_head, 3], from the finalize launch the forward runs
 * anyway (every precision; no extra launch).  d_poses_out gets the bits metro_forward writes.  Captured forwards
 * (metro_plan_set_graph_max_batch) are keyed on d_coords01_out too. */
int  metro_forward_coords01(MetroPlan* plan, const float* d_images_nhwc, int32_t n, float* d_poses_out,
                            float* d_coords01_out, void* d_workspace, void* stream);
/* metro_forward / metro_forward_coords01 (d_coords01_out may be NULL) on uint8 crops: d_images_nhwc uint8 [n,side,side,3],
 * 16-byte aligned, byte b standing for the fp32 value b / 255 (IEEE divide, clipped to [-1, 1]: normalize01, reference
 * src/improc.py:56-61; what the crop warps write), which the stem rounds to fp16 as it rounds an fp32 image value
 * (architectures.py:29).  Poses, coords01 and status words have the bits of metro_forward_coords01 on float(b) / 255.
 * METRO_PREC_F16 plans only: uint8 is a property of the call, the plan, its layer table, parameter blob and workspace are
 * those of metro_forward; the first layer runs the uint8 form of its kernel (metro_stem_pool_u8in, or prep_input_f16 reading
 * bytes where that stem is not supported) and every later launch is the same.  A plan of another precision returns
 * METRO_ERR_INVALID_ARG: expand the crops with metro_images_u8_to_f32 and call metro_forward.  Always plain launches: the
 * hipGraph cache of metro_plan_set_graph_max_batch does not serve this entry. */
int  metro_forward_u8(MetroPlan* plan, const uint8_t* d_images_nhwc, int32_t n, float* d_poses_out,
                      float* d_coords01_out, void* d_workspace, void* stream);
/* One record per crop (host code: frames.placement_params): the crop's virtual camera and the way back to its frame. */
typedef struct MetroPlacement {
    int32_t keypoint_mode;      /* METRO_WARP_HOMOGRAPHY: keypoints through `homography`; METRO_WARP_DISTORTED: through
                                 * rot_to_orig_cam, intrinsics and distortion (an original camera with coefficients) */
    int32_t reserved;
    float inv_intrinsics[9];    /* row-major inverse K of the virtual camera, fp32 (data_loading.py:112)                   */
    float rot_to_orig_cam[9];   /* orig.R virt.R^T (data_loading.py:110)                                                   */
    float rot_to_world[9];      /* virt.R^T (data_loading.py:111)                                                          */
    float cam_loc[3];           /* the camera centre in world coordinates, virt.t = orig.t (volumetric.py:206-208)         */
    float homography[9];        /* HOMOGRAPHY: row-major, crop pixel (x, y, 1) -> frame pixel (the warp's matrix)           */
    float intrinsics[6];        /* DISTORTED: the original camera's K[0,0] K[0,1] K[0,2] K[1,0] K[1,1] K[1,2]              */
    float distortion[5];        /* DISTORTED: k1 k2 p1 p2 k3 (OpenCV order)                                                 */
} MetroPlacement;               /* 208 bytes */
#define METRO_SCALE_METRO 0             /* root-relative: the engine's poses (--scale-recovery=metro)                       */
#define METRO_SCALE_BONE_LENGTHS 1      /* --scale-recovery=bone-lengths (volumetric.py:171-191)                            */
#define METRO_SCALE_TRUE_ROOT_DEPTH 2   /* --scale-recovery=true-root-depth (volumetric.py:192-199)                         */
#define METRO_COORDS_CROP 0             /* the crop's virtual camera                                                        */
#define METRO_COORDS_CAMERA 1           /* the original camera: to_orig_cam(x, rot_to_orig_cam) (volumetric.py:204-205)     */
#define METRO_COORDS_WORLD 2            /* to_orig_cam(x, rot_to_world) (+ cam_loc for absolute poses, volumetric.py:206-208) */
/* n crops in one launch.  d_coords01 fp32 [n, n_joints_head, 3] (metro_forward_coords01); d_poses the engine's fp32
 * [n, n_joints_out, 3] (read in METRO_SCALE_METRO only, else may be NULL); d_records DEVICE array of n MetroPlacement.
 * scale_recovery METRO_SCALE_*:
 *   BONE_LENGTHS     d_bone_lengths fp64 [n_edges] or [n, n_edges] (per_pose_lengths != 0), d_edges int32 [n_edges, 2] head
 *                    joint indices; the z offset of metro_backproject_bone_lengths (same operations, same bits);
 *   TRUE_ROOT_DEPTH  d_root_depth fp32 [n]: the root's z in mm in the virtual camera;
 *   METRO            the engine's root-relative poses, rotated as metro_to_orig_cam does.
 * coords METRO_COORDS_*; d_mirror int32 [n_joints_out] output-order mirror joints (to_orig_cam when det R <= 0).
 * d_poses_out fp32 [n, n_joints_out, 3] (output joint order; BONE_LENGTHS in CROP coords = metro_backproject_bone_lengths
 * with root_relative 0, permute 1); d_keypoints_out fp32 [n, n_joints_out, 2] frame pixels of heatmap_to_image(coords01.xy)
 * (NaN where the ray lies behind the original camera) or NULL; d_z_offset_out fp32 [n] (absolute modes) or NULL. */
int  metro_place_poses(const float* d_coords01, const float* d_poses, const MetroPlacement* d_records, int32_t n,
                       const MetroSpec* spec, int32_t scale_recovery, const double* d_bone_lengths, int32_t per_pose_lengths,
                       const float* d_root_depth, const int32_t* d_edges, int32_t n_edges, const int32_t* d_mirror,
                       int32_t coords, float* d_poses_out, float* d_keypoints_out, float* d_z_offset_out, void* stream);

/* ---- test-time augmentation of frame crops: several views per person box (the reference's --test-aug geometry,
 *      src/data/data_loading.py:60-68, 77-79, 110-112) ---- */
/* One record per box (host code: frames.pack_view_bases; device: metro_look_at_boxes): the box's camera, its look_at_box camera and the records of the box
 * itself (what frames.crop_params / placement_params give it), from which metro_expand_views derives every view. */
typedef struct MetroViewBase {
    int32_t frame;              /* index into the frame table                                                             */
    int32_t mode;               /* METRO_WARP_HOMOGRAPHY | METRO_WARP_DISTORTED                                          */
    int32_t has_camera;         /* 0: cameras=None, the axis-aligned square crop of `homography`                         */
    int32_t reserved;
    double old_matrix[9];       /* HOMOGRAPHY with a camera: the original camera's K R as the host's fp32 product         */
    double orig_r[9];           /* the original camera's R (fp32 values)                                                 */
    double virt_k[9];           /* the look_at_box camera's K (fp64)                                                     */
    double virt_r[9];           /* the look_at_box camera's R (fp32 values)                                              */
    double partial[9];          /* the identity view's MetroCropWarp.partial                                              */
    float homography[9];        /* the identity view's homography (cameras=None: the square crop's, crop -> frame)        */
    float inv_intrinsics[9];    /* the identity view's MetroPlacement fields, and cam_loc = the original camera's t        */
    float rot_to_orig_cam[9];
    float rot_to_world[9];
    float cam_loc[3];
    float intrinsics[6];        /* the original camera's K[0,0] K[0,1] K[0,2] K[1,0] K[1,1] K[1,2]                        */
    float distortion[5];        /* k1 k2 p1 p2 k3 (OpenCV order)                                                          */
} MetroViewBase;                /* 576 bytes */
/* One view: the look_at_box camera zoomed by `zoom` about the principal point (cameralib.py:167-170), rolled about the optical
 * axis (R <- Rz(roll)^T R, cameralib.py:95-98; cos / sin computed on the host) and, if flip, mirrored (R[0] *= -1,
 * cameralib.py:191-192), in that order (data_loading.py:66-67, 77).  cos 1, sin 0, zoom 1, no flip is the identity view. */
#define METRO_MAX_VIEWS 32
typedef struct MetroView {
    double cos_roll, sin_roll, zoom;
    int32_t flip;
    int32_t reserved;
} MetroView;                    /* 32 bytes */
/* d_bases: DEVICE array of n MetroViewBase; views: HOST array of n_views <= METRO_MAX_VIEWS (copied into the kernel
 * arguments).  Writes n * n_views MetroCropWarp (metro_warp_crops_frames_u8's input) and MetroPlacement (metro_place_poses')
 * records, box-major (row i * n_views + v), one thread per (box, view) in fp64 with closed-form 3x3 inverses, following
 * frames._frame_params with the view camera in place of the look_at_box one (homography = old_matrix inv(K R) cast to fp32,
 * partial = orig.R inv(R) inv(K), rot_to_orig_cam = orig.R R^T, rot_to_world = R^T, inv_intrinsics = inv(K), all cast to
 * fp32).  cameras=None: the crop is a camera with principal point (side/2, side/2) whose frame is the square crop: the
 * view's homography is the square's times the image-plane similarity of the view, the rotations back are R^T of the view,
 * inv_intrinsics stays 0.  The identity view copies the box's own records: the bits of the call without views. */
int  metro_expand_views(const MetroViewBase* d_bases, int32_t n, const MetroView* views, int32_t n_views, int32_t side,
                        MetroCropWarp* d_crops_out, MetroPlacement* d_placements_out, void* stream);
/* One calibrated camera of a frame (host code: frames.pack_frame_cameras, column-wise from frames.Camera).  r_inv and
 * old_matrix are per-frame products the host takes once with NumPy (np.linalg.inv(R) as Camera.camera_to_world uses it, and
 * K R as pack_view_bases stores it), so that the device works from the host's own bits for them. */
typedef struct MetroFrameCamera {
    float intrinsics[9];        /* K, row-major fp32; fx K[0], fy K[4], cx K[2], cy K[5] (a skew K[1] rides along)         */
    float r[9];                 /* world -> camera rotation, row-major fp32                                                */
    float r_inv[9];             /* np.linalg.inv(R) in fp32 (camera_to_world's matrix)                                     */
    float t[3];                 /* optical centre in world coordinates, fp32                                               */
    float distortion[5];        /* k1 k2 p1 p2 k3 (OpenCV order); read when has_distortion                                 */
    int32_t has_distortion;     /* 0: distortion_coeffs None (homography mode); 1: any coefficient array, zeros included  */
    double world_up[3];         /* turn_towards' up vector                                                                 */
    double old_matrix[9];       /* K R as the host's fp32 product (MetroViewBase.old_matrix)                               */
} MetroFrameCamera;             /* 240 bytes */
/* The MetroViewBase of n person boxes on the device, one thread per box in fp64: frames.pack_view_bases without the host.
 * d_boxes fp64 [n, 4] (x, y, w, h); d_frame_index int32 [n], each in [0, n_frames) (n_frames <= METRO_MAX_FRAMES): the frame
 * of each box.  d_cameras: NULL (cameras=None: preprocess.box_homography's square crop, has_camera 0, rotations I,
 * inv_intrinsics 0; n_cameras 0) or a DEVICE table of n_cameras == 1 (one camera for every frame) or n_cameras == n_frames
 * entries (camera of frame f at f).  With a camera each record follows frames.look_at_box step by step in the host's dtypes
 * (side points and centre rounded to fp32, undistort_points' 5 fixed iterations in fp64, camera_to_world / world_to_camera
 * and the new R in fp32, square_pixels' K in fp64, zoom, centre_principal_point) and then _frame_params_and_cameras
 * (homography = old_matrix inv(K R) cast to fp32; partial = fp32(orig.R fp32(inv R)) inv(K); rot_to_orig_cam, rot_to_world,
 * inv_intrinsics = inv(K) cast to fp32; cam_loc = t), 3x3 inverses in closed form: within a few fp32 ulp of the host, not
 * its LAPACK bits.  A frame index outside [0, n_frames) is clamped into it (the record's `frame` too, so nothing downstream
 * reads outside the tables) and counted: d_status (one int32, overwritten) receives the number of such boxes, which the
 * caller must treat as an error. */
int  metro_look_at_boxes(const double* d_boxes, const int32_t* d_frame_index, int32_t n, int32_t n_frames,
                         const MetroFrameCamera* d_cameras, int32_t n_cameras, int32_t side, MetroViewBase* d_bases_out,
                         int32_t* d_status, void* stream);
/* Fuses the n_views rows of each of n boxes (box-major, row i * n_views + v).  d_poses fp32 [n * n_views, n_joints, 3] in the
 * requested coords with joints already mirrored (metro_place_poses / metro_to_orig_cam); d_keypoints fp32
 * [n * n_views, n_joints, 2] frame pixels (unmirrored, as metro_place_poses writes them) or NULL; d_z_offset fp32
 * [n * n_views] or NULL; d_records the views' MetroPlacement (a view with det(rot_to_orig_cam) <= 0 contributes its mirror
 * joint's keypoint; d_mirror int32 [n_joints] output order).  Outputs: d_poses_out [n, n_joints, 3] the mean over the views;
 * d_keypoints_out [n, n_joints, 2] the mean over the views whose keypoint is finite (NaN if none); d_z_offset_out [n] the
 * mean; d_spread_out [n, n_joints] (or NULL) the RMS 3D distance of the views from their mean.  fp64 sums in view order,
 * one rounding to fp32: n_views copies of one view give its bits and a spread of 0. */
int  metro_merge_views(const float* d_poses, const float* d_keypoints, const float* d_z_offset,
                       const MetroPlacement* d_records, const int32_t* d_mirror, int32_t n, int32_t n_views, int32_t n_joints,
                       float* d_poses_out, float* d_keypoints_out, float* d_z_offset_out, float* d_spread_out, void* stream);

/* ---- per-joint heat-map covariance and peak confidence ----
 * Every joint's output is a softmax distribution p over its S x S x D volume and the pose is only its mean.  With the voxel
 * coordinates c = (x01, y01, z01) the soft-argmax uses (fp32 linspace(0,1,.)) and mu = sum p c (= coords01):
 *   Cov01 = sum p (c - mu)(c - mu)^T     stored as six fp32 words xx, yy, zz, xy, xz, yz;      peak = max p.
 * This is the spread of the joint's OWN heat-map in the crop's virtual-camera axes -- not of the root-relative difference the
 * poses are.  The statistics are centred at every step (each record about its own mean, merged with the parallel-axis
 * update): variances are sums of non-negative terms and a one-hot heat-map gives exactly 0.
 * d_moments_scratch: caller's device buffer of metro_moments_scratch_bytes(spec, n) bytes, 16-byte aligned (the plan's
 * workspace is not touched by it: its size and layout are those of metro_forward). */
int64_t metro_moments_scratch_bytes(const MetroSpec* spec, int32_t n);
/* metro_forward_coords01 (images_u8 == 0: d_images_nhwc fp32) or metro_forward_u8 (images_u8 == 1: uint8, f16 plans only)
 * that ALSO writes d_cov01_out fp32 [n, n_joints_head, 6] and d_peak_out fp32 [n, n_joints_head] (head joint order), from the
 * MOMENTS instantiations of the same head / soft-argmax launches: same launch count; poses, coords01 and status words have
 * the bits of those entries on the same input.  d_coords01_out may be NULL; d_cov01_out, d_peak_out and d_moments_scratch go
 * together (all NULL: the plain forward, eagerly).  Always plain launches: the hipGraph cache does not serve this entry.
 * Non-finite values (this entry and the two kernel-level ones below): a crop that reaches the soft-argmax with a NaN or +Inf
 * logit is answered and flagged exactly as by the plain entries (poses, coords01 and status word keep those bits).  Its
 * covariance is not a statistic of anything: the six d_cov01_out words and d_peak_out of every joint that has such a logit are
 * NaN (the joint's normaliser is NaN and every word is divided by it) -- through the head a non-finite input element is a
 * term of every channel of its pixel, so of every joint of the crop; the crop's other joints, and every other crop of the
 * call, keep the bits of the call without the non-finite value (tests/test_gpu_heat_moments_closure.py). */
int  metro_forward_moments(MetroPlan* plan, const void* d_images_nhwc, int32_t images_u8, int32_t n, float* d_poses_out,
                           float* d_coords01_out, float* d_cov01_out, float* d_peak_out, void* d_moments_scratch,
                           void* d_workspace, void* stream);
/* metro_head_f16 with the moments: d_coords01_out (optional), d_cov01_out, d_peak_out as above; d_poses_out optional. */
int  metro_head_f16_moments(const void* d_x, const void* d_w, const float* d_bias, const void* d_pro_scale,
                            const void* d_pro_shift, int32_t n, int32_t c_in, const MetroSpec* spec, void* d_partials,
                            void* d_moments_scratch, float* d_logits_out, float* d_poses_out, float* d_coords01_out,
                            float* d_cov01_out, float* d_peak_out, void* stream);
/* metro_softargmax01 with the moments (precise 0 / 1 / 2 as there; the records are in the accumulator type). */
int  metro_softargmax01_moments(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, void* d_scratch,
                                void* d_moments_scratch, float* d_coords01_out, float* d_cov01_out, float* d_peak_out,
                                void* stream);
/* The kernels behind metro_plan_bind_heatmaps, metro_plan_bind_modes and metro_plan_bind_prior on the caller's own logits
 * (kernel-level entries for the tests and heads.marginals_from_logits / modes_from_logits / posterior_from_logits): the launchers
 * the bound forwards call, with max_n = n.  d_logits: device NHWC [n, S, S, D * J], S = proc_side / stride; precise 0: fp32
 * logits, fp32 sums (what f16 plans run); 1: fp32 logits, fp64 sums (f32, f32m); 2: fp64 logits and sums (f64).  Outputs,
 * definitions, arithmetic and non-finite rules are those of the bound forms above, word for word, in OUTPUT joint order
 * (spec->n_joints_out rows, head joint spec->permutation[r]); d_prior is the bound form's input [n, n_joints_out, 9].
 * d_scratch (marginals only): metro_heat_marginals_scratch_bytes(spec, n) bytes (-1 for a bad argument), 16-byte aligned -- the
 * tile and joint records alone, no copy of the logits.  Checked before any launch: non-NULL pointers, the logits aligned to
 * their element, the scratch to 16 and every other pointer to 4 bytes, 1 <= n <= 65535, both joint counts in
 * [1, METRO_MAX_JOINTS], depth >= 1, stride >= 1 and proc_side / stride >= 1, k and radius in the ranges of
 * metro_plan_bind_modes (METRO_ERR_INVALID_ARG); a shape the kernel cannot serve returns METRO_ERR_UNSUPPORTED as the bound
 * forward does.  All work is enqueued on `stream`. */
int64_t metro_heat_marginals_scratch_bytes(const MetroSpec* spec, int32_t n);
int  metro_heat_marginals(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, void* d_scratch,
                          float* d_xy_out, float* d_z_out, void* stream);
int  metro_heat_modes(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, int32_t k, int32_t radius,
                      int32_t* d_voxel_out, float* d_stats_out, void* stream);
int  metro_heat_posterior(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, const float* d_prior,
                          float* d_post_out, void* stream);
/* Covariances in mm^2, output joint order, requested coordinates, one launch, one thread per (box, output joint).
 * d_cov01 / d_peak: [n * n_views, n_joints_head, 6] / [n * n_views, n_joints_head] (box-major rows i * n_views + v).
 * Gathers spec->permutation; Cov_mm = diag(s) Cov01 diag(s) with the linear part of heatmap_to_metric,
 * s = (lrc box_size_mm / proc_side, the same, box_size_mm) (volumetric.py:288-306; the half stride does not enter);
 * coords CAMERA / WORLD: R Cov R^T with the row's rot_to_orig_cam / rot_to_world of d_records (n * n_views MetroPlacement),
 * taking the mirror joint's covariance (d_mirror int32 [n_joints_out]) when det R <= 0 as metro_to_orig_cam does; CROP reads
 * neither.  Views are averaged (covariances after rotation, and peaks).  MeTRo's metric scale, whatever scale recovery
 * placed the poses.  d_cov_out fp32 [n, n_joints_out, 9] (row-major symmetric 3x3); d_peak_out fp32 [n, n_joints_out]. */
int  metro_place_covariances(const float* d_cov01, const float* d_peak, const MetroPlacement* d_records, int32_t n,
                             int32_t n_views, const MetroSpec* spec, const int32_t* d_mirror, int32_t coords,
                             float* d_cov_out, float* d_peak_out, void* stream);

/* ---- world poses of persons seen by several calibrated cameras ----
 * Nothing in the reference: its examples have one camera each.  Every crop row that shows a person gives one ray per joint,
 * from the crop's undistorted virtual camera (MetroPlacement.inv_intrinsics, rot_to_world, cam_loc: no undistortion needed);
 * the joint is the point nearest to its rays, X = (sum w (I - d d^T))^-1 sum w (I - d d^T) o.  One launch, one thread per
 * (person, output joint), fp64 arithmetic on the fp32 inputs, one rounding to fp32 per output.
 * d_coords01 fp32 [m, n_joints_head, 3] (metro_forward_coords01); d_cov01 fp32 [m, n_joints_head, 6] (metro_forward_moments;
 * read by METRO_TRI_COVARIANCE only, else may be NULL); d_records DEVICE array of m MetroPlacement.
 * Grouping (CSR): person p owns the crop rows d_rows[d_starts[p] : d_starts[p + 1]], d_rows int32 [n_rows] indices into the m
 * rows, d_starts int32 [n_persons + 1] non-decreasing from 0 to n_rows.  A group may be empty.  An index of d_rows outside
 * [0, m) gives no ray and d_starts is clamped to [0, n_rows]: the kernel reads nothing out of bounds.  With n_rows == 0 the
 * four row inputs are not read and may be NULL.
 * Ray of row i and output joint r: head joint spec->permutation[mirrored ? d_mirror[r] : r], mirrored = !(det rot_to_world >
 * 0) (a flipped test-time view; metro_place_poses' rule); (u, v) = heatmap_to_image(coords01); d = rot_to_world .
 * (inv_intrinsics . (u, v, 1)) normalised; o = cam_loc.  A ray with a non-finite component is skipped.
 * weights METRO_TRI_UNIFORM: w = 1.  METRO_TRI_COVARIANCE: a second solve with w = 1 / (sigma^2 z^2), z = d . (X0 - o) the
 * ray's depth at the uniform solution X0 and sigma^2 = (cov01_xx + cov01_yy) / 2 . lrc^2 . inv_intrinsics[0]^2 (lrc: the
 * heat-map-to-pixel factor of heatmap_to_image), floored at 1e-12 lrc^2 inv_intrinsics[0]^2; a ray with z <= 0 or a
 * non-finite w is dropped.
 * Determinacy: with A~ = sum w (I - d d^T) / sum w, a joint with fewer than 2 rays or det A~ < min_det is undetermined:
 * point and residual NaN, n_rays the number of usable rays.  Two rays at angle t have det A~ = sin^2 t / 4, so
 * min_det = sin^2(min_angle) / 4 rejects (anti-)parallel rays, and any bundle of rays from one optical centre.
 * d_points_out fp32 [n_persons, n_joints_out, 3] world mm; d_n_rays_out int32 [n_persons, n_joints_out] rays in the final
 * solve; d_residual_out fp32 [n_persons, n_joints_out] = sqrt(sum w |(I - d d^T)(X - o)|^2 / sum w), the weighted RMS
 * distance of the point from its rays in mm.  n_persons == 0 launches nothing.
 * metro_triangulate_joints_cov: the same launch (points, n_rays and residual bit for bit those of the plain entry) that also
 * writes d_cov_out fp32 [n_persons, n_joints_out, 9], the covariance of the point in mm^2, row-major symmetric 3x3 (the layout
 * metro_smooth_tracks and metro_associate_tracks read), from the cofactors of the final solve.  METRO_TRI_COVARIANCE:
 * Cov = A^-1 with A = sum w (I - d d^T) of the second solve (w is an inverse variance in mm^-2).  METRO_TRI_UNIFORM:
 * Cov = s^2 A^-1 with A = sum (I - d d^T) and s^2 = sum |p|^2 / (2 k - 3), |p| the distances of the point from its k rays that
 * the residual sums (two constraints per ray, three unknowns; exactly meeting rays give Cov = 0).  An undetermined joint gets
 * a NaN block.  -1 also for a NULL d_cov_out. */
#define METRO_TRI_UNIFORM 0
#define METRO_TRI_COVARIANCE 1
int  metro_triangulate_joints(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, int32_t m,
                              const int32_t* d_rows, int32_t n_rows, const int32_t* d_starts, int32_t n_persons,
                              const MetroSpec* spec, const int32_t* d_mirror, int32_t weights, double min_det,
                              float* d_points_out, int32_t* d_n_rays_out, float* d_residual_out, void* stream);
int  metro_triangulate_joints_cov(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, int32_t m,
                                  const int32_t* d_rows, int32_t n_rows, const int32_t* d_starts, int32_t n_persons,
                                  const MetroSpec* spec, const int32_t* d_mirror, int32_t weights, double min_det,
                                  float* d_points_out, int32_t* d_n_rays_out, float* d_residual_out, float* d_cov_out,
                                  void* stream);

/* ---- which boxes of several calibrated cameras show the same person: cross-view association on the device ----
 * Nothing in the reference: its examples have one camera each, and a person detector gives boxes per camera with no shared
 * identity.  Two launches between the forward and metro_triangulate_joints, no host work in between.
 * metro_view_affinity: how close the per-joint rays of every two boxes pass.  Inputs as metro_triangulate_joints reads them:
 * d_coords01 fp32 [m, n_joints_head, 3], d_cov01 fp32 [m, n_joints_head, 6] (METRO_TRI_COVARIANCE only, else may be NULL),
 * d_records m MetroPlacement, d_mirror int32 [n_joints_out], with m = n * n_views crop rows, box-major (row i * n_views + v);
 * d_frame_index int32 [n], the frame (camera) of each box.  Rays as there: the mirror joint for a flipped view, a non-finite
 * ray skipped, sigma^2 the same variance.  Per pair of boxes a < b on different frames, per view v and output joint r, with
 * the unit directions da, db from oa, ob and c = da . db: the ray pair is skipped if a ray is unusable or
 * 1 - c^2 < min_sin2 (within min_angle of parallel, min_sin2 = sin^2(min_angle) in (0, 1]); the lines are closest at the
 * parameters ta, tb at the distance dist; with ta <= 0 or tb <= 0 (they meet behind a camera) the pair counts with
 * dist = clip_mm, else with min(dist, clip_mm).  weights METRO_TRI_UNIFORM: w = 1; METRO_TRI_COVARIANCE:
 * w = 1 / (sigma_a^2 ta^2 + sigma_b^2 tb^2), a pair whose w is not finite and positive is skipped.
 * d_cost_out fp32 [n, n] = sqrt(sum w dist^2 / sum w) in mm over the counted pairs, symmetric; d_n_pairs_out int32 [n, n]
 * their number.  +inf where n_pairs < min_pairs, for two boxes on one frame (n_pairs 0: a person appears once per camera)
 * and on the diagonal (n_pairs 0).  One thread per entry of the n x n index space, the one with a < b writes [a][b] and
 * [b][a]; fp64 arithmetic on the fp32 inputs, one rounding to fp32 per output.
 * metro_view_affinity_steps: the same kernel with d_step_index int32 [n], the time step (one exposure of the rig) of each box:
 * two boxes of different steps get +inf and n_pairs 0, as two boxes of one frame do, every other entry has the bits the plain
 * entry gives.  +inf survives the complete-linkage maximum, so no cluster of metro_cluster_views spans two steps.
 * metro_cluster_views: constrained complete-linkage clustering of the boxes, one workgroup, the working matrix in LDS.
 * d_cost fp32 [n, n] is read as C = max(cost, cost^T) with NaN as +inf.  Every box starts as its own cluster, named by its
 * lowest box.  Repeat: among the clusters a < b take the smallest C[a][b] (ties: the smallest a, then the smallest b); unless
 * it is < max_cost stop; else b merges into a, C[a][k] = C[k][a] = max(C[a][k], C[b][k]) for all k.  +inf propagates through
 * the max, so no person gets two boxes of one frame.  d_person_index_out int32 [n]: persons numbered by their lowest box (box
 * 0 is in person 0); d_n_persons_out int32 [1]; the CSR grouping metro_triangulate_joints reads with n as its person count:
 * d_starts_out int32 [n + 1], d_rows_out int32 [n * n_views].  A person with several boxes owns the crop rows
 * i * n_views + v of its boxes in ascending box order; a person with one box (one optical centre: no depth) and the persons
 * >= n_persons have empty groups; the entries of d_rows_out from d_starts_out[n] on are -1.
 * -1 before any launch for a NULL pointer (d_cov01 only with METRO_TRI_COVARIANCE), a negative n, n > METRO_MATCH_MAX_BOXES,
 * n_views outside [1, METRO_MAX_VIEWS], unknown weights, joint counts out of range, min_sin2 outside (0, 1], clip_mm or
 * max_cost not > 0 (or NaN) and min_pairs < 1.  n == 0 launches nothing and returns 0.
 * metro_person_steps: the time step of every person metro_cluster_views found and the persons as the time-step CSR
 * metro_associate_tracks reads, one workgroup of 128 threads (thread p = person p) between the triangulation and the association
 * launch.  Inputs: the cluster CSR d_rows int32 [n_rows], d_starts int32 [n + 1] and d_n_persons int32 [1] as
 * metro_cluster_views wrote them, n <= METRO_MATCH_MAX_BOXES the upper bound of the persons; d_box_step int32 [n_boxes], the
 * step of each box (box = crop row / n_views); d_step_times fp64 [n_steps] seconds, ascending.
 * d_person_step_out int32 [n]: the smallest step among the boxes of the person's group (a gated cluster has one; ungated
 * clusters take the earliest); -1 for the persons >= d_n_persons[0] and for an empty group (a person seen by one camera).  A
 * row outside [0, n_boxes n_views) and a step outside [0, n_steps) are skipped, never read; d_starts is clamped to [0, n_rows].
 * d_person_times_out fp64 [n]: d_step_times of that step, NaN where it is -1.  d_step_rows_out int32 [n]: the persons that
 * have a step sorted by (step, person), the entries past their number -1.  d_step_starts_out int32 [n_steps + 1]: step s owns
 * d_step_rows_out[d_step_starts_out[s] : d_step_starts_out[s + 1]]; d_step_starts_out[n_steps] is the number of persons that
 * have a step.  -1 before any launch for a negative size, n > METRO_MATCH_MAX_BOXES, n_views outside [1, METRO_MAX_VIEWS] and,
 * with n > 0, a NULL pointer (d_rows and d_box_step only with n_rows > 0, d_step_times only with n_steps > 0).  n == 0 launches
 * nothing and returns 0. */
#define METRO_MATCH_MAX_BOXES 128
int  metro_view_affinity(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, const MetroSpec* spec,
                         const int32_t* d_mirror, const int32_t* d_frame_index, int32_t n, int32_t n_views, int32_t weights,
                         double min_sin2, double clip_mm, int32_t min_pairs, float* d_cost_out, int32_t* d_n_pairs_out,
                         void* stream);
int  metro_view_affinity_steps(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records,
                               const MetroSpec* spec, const int32_t* d_mirror, const int32_t* d_frame_index,
                               const int32_t* d_step_index, int32_t n, int32_t n_views, int32_t weights, double min_sin2,
                               double clip_mm, int32_t min_pairs, float* d_cost_out, int32_t* d_n_pairs_out, void* stream);
int  metro_cluster_views(const float* d_cost, int32_t n, int32_t n_views, float max_cost, int32_t* d_person_index_out,
                         int32_t* d_n_persons_out, int32_t* d_rows_out, int32_t* d_starts_out, void* stream);
int  metro_person_steps(const int32_t* d_rows, int32_t n_rows, const int32_t* d_starts, const int32_t* d_n_persons, int32_t n,
                        int32_t n_views, const int32_t* d_box_step, int32_t n_boxes, const double* d_step_times, int32_t n_steps,
                        int32_t* d_person_step_out, double* d_person_times_out, int32_t* d_step_rows_out,
                        int32_t* d_step_starts_out, void* stream);

/* ---- persons that ONE camera sees: their time step, their box and the ray of every joint ----
 * Nothing in the reference: its examples have one camera each and no world.  metro_cluster_views gives a person with one box
 * an empty group, so metro_person_steps gives it no step and it never reaches the association.  These two launches bring it
 * there as a RAY row (metro_associate_tracks_rays, further down).  The ABI version is unchanged: the entries are additions.
 * metro_person_steps_labels: metro_person_steps without the cluster CSR, one workgroup of 128 threads, thread p = person p.
 * d_person_index int32 [n_boxes], the person of every box as metro_cluster_views wrote it; d_n_persons int32 [1];
 * n <= METRO_MATCH_MAX_BOXES the upper bound of the persons; d_box_step int32 [n_boxes]; d_step_times fp64 [n_steps] ascending.
 * The step of person p < d_n_persons[0] is the smallest d_box_step[b] in [0, n_steps) over the boxes b with
 * d_person_index[b] == p -- for a person with several boxes the value metro_person_steps gives, and a person with one box now
 * has a step too; -1 for a person with no such box and for the persons >= d_n_persons[0].  A label outside [0, n) belongs to no
 * person and a step outside [0, n_steps) is skipped: nothing is read through either.  d_person_step_out, d_person_times_out,
 * d_step_rows_out and d_step_starts_out are metro_person_steps' four outputs, built from these steps by the same code.
 * d_single_box_out int32 [n]: the box of a person that has exactly one box, whose step is valid; -1 for everyone else, the
 * persons >= d_n_persons[0] included.  -1 before any launch for a negative size, n > METRO_MATCH_MAX_BOXES and, with n > 0, a NULL
 * pointer (d_person_index and d_box_step only with n_boxes > 0, d_step_times only with n_steps > 0).  n == 0 launches nothing
 * and returns 0.
 * metro_person_rays: one thread per (person, output joint) in blocks of 64, fp64 arithmetic on the fp32 inputs.  d_coords01,
 * d_cov01 (METRO_TRI_COVARIANCE only, else may be NULL), d_records, spec, d_mirror and weights as metro_triangulate_joints
 * reads them, m = n * n_views crop rows, box-major; d_single_box int32 [n] as written above.  Per (p, r): with
 * b = d_single_box[p] outside [0, n) there is no ray.  Otherwise over the usable rays (d_v, o_v, sigma2_v) of the rows
 * b * n_views + v, built exactly as the triangulation builds them (the mirror joint of a flipped view; a non-finite ray is
 * skipped): w_v = 1 (METRO_TRI_UNIFORM) or 1 / sigma2_v (METRO_TRI_COVARIANCE; a view whose w_v is not finite and positive is
 * dropped); d = (sum w_v d_v) normalised; o = o_v of the first usable view (the views of a box share one optical centre);
 * sigma2 = 1 / sum (1 / sigma2_v) with covariance weights, 0 with uniform ones.  No ray if no view is usable or the sum has
 * zero or non-finite length.  d_rays_out fp64 [n, n_joints_out, 8]: o (3), d (3), sigma2, the number of views used; all eight
 * NaN where there is no ray.  -1 before any launch for a NULL spec, joint counts out of range, unknown weights, a negative size,
 * n > METRO_MATCH_MAX_BOXES, n_views outside [1, METRO_MAX_VIEWS], m != n * n_views and, with n > 0, a NULL pointer (d_cov01
 * only with METRO_TRI_COVARIANCE).  n == 0 launches nothing and returns 0. */
int  metro_person_steps_labels(const int32_t* d_person_index, const int32_t* d_n_persons, int32_t n, const int32_t* d_box_step,
                               int32_t n_boxes, const double* d_step_times, int32_t n_steps, int32_t* d_person_step_out,
                               double* d_person_times_out, int32_t* d_step_rows_out, int32_t* d_step_starts_out,
                               int32_t* d_single_box_out, void* stream);
int  metro_person_rays(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, int32_t m,
                       const MetroSpec* spec, const int32_t* d_mirror, int32_t weights, const int32_t* d_single_box, int32_t n,
                       int32_t n_views, double* d_rays_out, void* stream);

/* ---- poses of tracked persons smoothed over time: constant-velocity Kalman filter + Rauch-Tung-Striebel pass ----
 * Nothing in the reference: one example is one image.  One launch, one thread per (track, output joint), fp64 arithmetic on
 * the fp32 inputs, one rounding to fp32 per output.  J = spec->n_joints_out (nothing else of the spec is read).
 * d_poses fp32 [n, J, 3] mm, the measurements (metro_place_poses / metro_merge_views); d_cov fp32 [n, J, 9] mm^2, row-major
 * 3x3 per joint (metro_place_covariances), of which the upper triangle is read; read by METRO_SMOOTH_COVARIANCE only, else
 * may be NULL; d_times fp64 [n] seconds.
 * Grouping (CSR): track t owns the rows d_rows[d_starts[t] : d_starts[t + 1]] IN TIME ORDER (the host sorts them), d_rows
 * int32 [n_rows] indices into the n rows, d_starts int32 [n_tracks + 1] non-decreasing from 0 to n_rows.  A group may be
 * empty.  An index of d_rows outside [0, n) is skipped as if it were not listed, and d_starts is clamped to [0, n_rows]: the
 * kernel reads nothing out of bounds.
 * Per joint the state is x = (p, v) in R^6, mm and mm/s, with the symmetric 6x6 covariance P.
 * Measurement of row k: z = d_poses[row, joint], H = [I 0], R = r_floor^2 I (METRO_SMOOTH_ISOTROPIC) or
 * cov_scale Cov + r_floor^2 I (METRO_SMOOTH_COVARIANCE).  z is MISSING if a component is non-finite or, in covariance mode,
 * if R has a non-finite entry or is not positive definite (leading minors R00, R00 R11 - R01^2, det R all > 0).
 * Start: with d_state NULL or the slot's t_last NaN, rows before the track's first non-missing measurement get NaN in every
 * float output and used = 0; that measurement sets x = (z, 0), P = diag(R, v0^2 I), used = 1.
 * Every later row, and every row of a track with a carried state: dt = t_k - t_prev (t_prev the time of the previous listed
 * row, or t_last of the carried state), 0 unless dt > 0; F = [[I, dt I], [0, I]], Q = q [[dt^3/3 I, dt^2/2 I], [dt^2/2 I, dt I]]
 * (white-noise acceleration of spectral density q, mm^2/s^3); x- = F x, P- = F P F^T + Q.  Unless z is missing:
 * nu = z - H x-, S = P-_pp + R; with gate > 0 the measurement is GATED if nu^T S^-1 nu > gate (gate == 0: never); otherwise
 * K = P- H^T S^-1, x = x- + K nu, P = (I - K H) P- (I - K H)^T + K R K^T (Joseph form), used = 1.  A missing or gated
 * row is predict-only: x = x-, P = P-, used = 0.
 * mode METRO_SMOOTH_FILTER: the outputs of row k are x_k and P_k.  METRO_SMOOTH_RTS: from the track's last listed row of
 * this call (whose smoothed value is its filtered one) back to its first row with a state, C = P_k F_{k+1}^T (P-_{k+1})^-1,
 * x^s_k = x_k + C (x^s_{k+1} - x-_{k+1}), P^s_k = P_k + C (P^s_{k+1} - P-_{k+1}) C^T, the 6x6 system solved by an
 * unpivoted LDL^T; if a pivot is not > 0 row k keeps its filtered value, which the pass continues from.  The outputs of
 * row k are x^s_k and P^s_k.
 * d_workspace: metro_smooth_tracks_workspace_bytes(n_rows, J) bytes = n_rows J 54 fp64 (x_k, P_k, x-_k, P-_k per listed row
 * and joint); written and read by METRO_SMOOTH_RTS only, else may be NULL.
 * d_state fp64 [n_tracks, J, 28] or NULL: x (6), the upper triangle of P row by row (21), t_last.  A track with at least one
 * listed row in [0, n) and a state by its last row has the FILTER state of that row and the row's time written back, in both
 * modes (never smoothed values); every other slot is left untouched.
 * Outputs, written only for rows listed in some group: d_poses_out fp32 [n, J, 3] (p); optional (NULL: not written)
 * d_velocity_out fp32 [n, J, 3] mm/s (v), d_cov_out fp32 [n, J, 9] mm^2 (the position block of P, symmetric),
 * d_used_out uint8 [n, J].
 * -1 before any launch for a NULL spec, J outside [1, METRO_MAX_JOINTS], a bad mode or measurement, negative n / n_rows /
 * n_tracks, q <= 0, r_floor <= 0, v0 <= 0, cov_scale < 0, gate < 0 (or any of them NaN), and, with n_tracks > 0 and
 * n_rows > 0, NULL d_poses, d_times, d_rows, d_starts or d_poses_out, NULL d_cov in covariance mode, NULL d_workspace in RTS
 * mode.  n_tracks == 0 or n_rows == 0 launches nothing and returns 0. */
#define METRO_SMOOTH_FILTER 0
#define METRO_SMOOTH_RTS 1
#define METRO_SMOOTH_ISOTROPIC 0
#define METRO_SMOOTH_COVARIANCE 1
size_t metro_smooth_tracks_workspace_bytes(int32_t n_rows, int32_t n_joints_out);
int  metro_smooth_tracks(const float* d_poses, const float* d_cov, const double* d_times, int32_t n, const int32_t* d_rows,
                         int32_t n_rows, const int32_t* d_starts, int32_t n_tracks, const MetroSpec* spec, int32_t mode,
                         int32_t measurement, double q, double r_floor, double cov_scale, double v0, double gate,
                         double* d_state, void* d_workspace, float* d_poses_out, float* d_velocity_out, float* d_cov_out,
                         uint8_t* d_used_out, void* stream);

/* ---- which box of a video continues which track: frame-to-frame association on the device ----
 * Nothing in the reference: one example is one image, and a person detector gives boxes per frame, unordered, with no
 * identity from one frame to the next.  One launch of one workgroup (256 threads, the cost matrix in LDS) between the forward
 * and metro_smooth_tracks, no host work in between; fp64 arithmetic on the fp32 inputs.  J = spec->n_joints_out (nothing else
 * of the spec is read).
 * d_poses fp32 [n, J, 3] mm, ABSOLUTE (root-relative poses of different persons coincide); d_cov fp32 [n, J, 9] mm^2, read by
 * METRO_SMOOTH_COVARIANCE only, else may be NULL; d_times fp64 [n] seconds: metro_smooth_tracks' inputs.
 * Time steps (CSR, built on the host): step s owns the boxes d_step_rows[d_step_starts[s] : d_step_starts[s + 1]],
 * d_step_rows int32 [n_step_rows] indices into the n rows, d_step_starts int32 [n_steps + 1]; the steps are in ascending
 * time and all boxes of one timestamp form one step; every row is listed at most once.  The time t_s of a step is that of its
 * first listed row in [0, n); a step without one is skipped.  An index outside [0, n) is skipped as if it were not listed
 * (it keeps its position in the step), d_step_starts is clamped to [0, n_step_rows], and of a step with more than
 * METRO_ASSOC_MAX positions only the first METRO_ASSOC_MAX are read: the kernel reads and writes nothing out of bounds.  A
 * row in no step, or past that limit, is untracked and counted nowhere.
 * Track table, n_tracks = T <= METRO_ASSOC_MAX slots: d_state fp64 [T, J, 28], metro_smooth_tracks' carried state;
 * d_ids int32 [T], the persistent id of the track in each slot, -1: the slot is free; d_next_id int32 [1], the next id to
 * give.  A slot is LIVE iff some joint's t_last is not NaN; its last-seen time is the largest such t_last.
 * d_workspace: metro_associate_tracks_workspace_bytes(T, J) bytes = T J 28 fp64, the WORKING state: a copy of d_state made
 * at the start of the launch that the launch advances and leaves behind; it is exchanged only within the workgroup.
 * At the start: a live slot whose last-seen time is < t_first - max_age_s (t_first the time of the first step that has one)
 * is RETIRED: every joint's t_last becomes NaN in d_state and in the working state, and its id -1.  This is the only write
 * to d_state; it makes the smoothing launch that follows start a reborn slot afresh.  A slot that is not live is free: its
 * id becomes -1.  No slot is retired inside a call, so a slot never holds two tracks within one group of the CSR below.
 * Then per step, in order:
 * 1. cost[t][b] of slot t continuing in box b: over the joints j whose working t_last[j] is not NaN and whose measurement
 *    z = d_poses[b, j] is finite, with dt = max(t_s - t_last[j], 0) and the working x = (p, v):
 *    d_j = min(|z - (p + dt v)|, clip_mm); cost = sqrt(mean d_j^2), rounded once to fp32.  +inf with fewer than min_joints
 *    such joints, or if the slot's last-seen time is < t_s - max_age_s (a free slot has no such joint).
 * 2. Greedy one-to-one assignment on the fp32 costs: take the smallest remaining cost -- ties go to the lowest slot, then
 *    to the lowest position in the step -- and unless it is < max_cost_mm stop; else that box continues that slot, and the
 *    slot's row and the box's column are struck out.
 * 3. Births: the unassigned boxes that have at least one finite joint, in step order, take the free slots in ascending
 *    order, each with ids[slot] = next_id++.  A box for which no free slot is left, or without a finite joint, is UNTRACKED.
 * 4. Filter: every slot that received a box advances its working state, per joint, by exactly the per-row step of
 *    metro_smooth_tracks (start, predict, update, missing, gated; measurement, q, r_floor, cov_scale, v0 and gate as there;
 *    t_prev the joint's t_last, the row's time its d_times).  A joint with no state and an unusable measurement stays as it is.
 * Outputs: d_track_index_out int32 [n] the slot of each box, -1 untracked; d_track_id_out int32 [n] the id, -1 untracked;
 * d_cost_out fp32 [n] the accepted cost of a box that continues a track, NaN for births and untracked boxes; the CSR grouping
 * metro_smooth_tracks reads with T as its track count and n as its n_rows: d_starts_out int32 [T + 1], d_rows_out int32 [n],
 * slot t owning its boxes in time order, the entries from d_starts_out[T] on -1; d_n_new_out int32 [1] the births,
 * d_n_dropped_out int32 [1] the untracked boxes of the steps; d_ids and d_next_id updated in place.  Running
 * metro_smooth_tracks (either mode) on that CSR with d_state leaves in d_state, bit for bit, the working state.
 * -1 before any launch for a NULL spec, J outside [1, METRO_MAX_JOINTS], a bad measurement, negative n / n_step_rows /
 * n_steps, n_tracks outside [1, METRO_ASSOC_MAX], q <= 0, r_floor <= 0, v0 <= 0, cov_scale < 0, gate < 0, max_cost_mm <= 0,
 * clip_mm <= 0, max_age_s < 0 (or any of them NaN), min_joints outside [1, J], and, with n, n_step_rows and n_steps all > 0,
 * a NULL pointer (d_cov only in covariance mode).  n == 0, n_step_rows == 0 or n_steps == 0 launches nothing, writes nothing
 * and returns 0. */
#define METRO_ASSOC_MAX 128
size_t metro_associate_tracks_workspace_bytes(int32_t n_tracks, int32_t n_joints_out);
int  metro_associate_tracks(const float* d_poses, const float* d_cov, const double* d_times, int32_t n,
                            const int32_t* d_step_rows, int32_t n_step_rows, const int32_t* d_step_starts, int32_t n_steps,
                            const MetroSpec* spec, int32_t measurement, double q, double r_floor, double cov_scale, double v0,
                            double gate, float max_cost_mm, double clip_mm, int32_t min_joints, double max_age_s,
                            double* d_state, int32_t n_tracks, int32_t* d_ids, int32_t* d_next_id, void* d_workspace,
                            int32_t* d_track_index_out, int32_t* d_track_id_out, float* d_cost_out, int32_t* d_rows_out,
                            int32_t* d_starts_out, int32_t* d_n_new_out, int32_t* d_n_dropped_out, void* stream);

/* ---- the same walk with the OPTIMAL assignment of a step's boxes to the slots ----
 * metro_associate_tracks_optimal is metro_associate_tracks -- parameters, argument checks, workspace
 * (metro_associate_tracks_workspace_bytes), one launch of one workgroup, every step, output and return value -- except for step 2
 * of a time step, which becomes, with c = cost[t][b] as step 1 writes it (fp32) and g = max_cost_mm (fp32):
 * 2'. A pair is ADMISSIBLE if c < g.  The assignment is the one-to-one set M of admissible pairs that minimises
 *    sum over M of (c - g), i.e. maximises the total gain sum (g - c): the linear assignment problem on min(c, g) in which a
 *    pair at g means "unmatched" (the m x (T + m) problem with m dummy columns at cost g).  It is not a maximum-cardinality
 *    matching: one pair at 10 mm beats two pairs at 299 mm each (gains 290 against 1 + 1, with g = 300).  The greedy rule of
 *    step 2 can miss it: with slots A, B and boxes p, q at costs A-p 100, A-q 120, B-p 130, B-q 350 it takes A-p, after which
 *    B has no admissible box left (B bridges, q is born under a new id); the optimum A-q + B-p keeps both tracks.
 *    The sums (dual potentials, path lengths of the shortest augmenting paths) are fp64 over the fp32 costs.  The boxes are
 *    augmented in step order and every minimum takes the lowest index among equals (a slot before "unmatched"), so the result
 *    does not depend on the number of threads; which of several exactly equal optima is returned is otherwise not specified.
 *    Every loop is bounded by the sizes alone: one search per box, at most T + 1 column visits per search, at most T steps
 *    back along a path; a cost that is not a number is not admissible.
 * d_cost_out holds the cost c of each accepted pair, as there.  The ABI version is unchanged: the entry is an addition. */
int  metro_associate_tracks_optimal(const float* d_poses, const float* d_cov, const double* d_times, int32_t n,
                                    const int32_t* d_step_rows, int32_t n_step_rows, const int32_t* d_step_starts,
                                    int32_t n_steps, const MetroSpec* spec, int32_t measurement, double q, double r_floor,
                                    double cov_scale, double v0, double gate, float max_cost_mm, double clip_mm,
                                    int32_t min_joints, double max_age_s, double* d_state, int32_t n_tracks, int32_t* d_ids,
                                    int32_t* d_next_id, void* d_workspace, int32_t* d_track_index_out, int32_t* d_track_id_out,
                                    float* d_cost_out, int32_t* d_rows_out, int32_t* d_starts_out, int32_t* d_n_new_out,
                                    int32_t* d_n_dropped_out, void* stream);

/* ---- the same walk with RAY rows: a person one camera sees keeps feeding its track ----
 * metro_associate_tracks_rays is metro_associate_tracks (assignment 0: the greedy step 2) or metro_associate_tracks_optimal
 * (assignment 1: step 2') -- workspace, one launch of one workgroup, the cost matrix in LDS -- with these additions.
 * d_poses and d_cov are WRITABLE; d_single_box int32 [n]: >= 0 marks row b as a RAY row (metro_person_steps_labels; the value
 * itself is not read); d_rays fp64 [n, J, 8]: o (3), d (3, unit), sigma2, views per joint (metro_person_rays); depth_sigma_mm;
 * d_ray_depth_out fp32 [n, J]; d_n_unplaced_out int32 [1].  A row that is no ray row is a POINT row and behaves exactly as
 * there.  Of a ray row d_poses and d_cov are not read before the launch has written them; it differs as follows.
 * 1. cost[t][b]: over the joints j whose working t_last[j] is not NaN and whose ray is finite (o, d and sigma2), with
 *    p^ = p + dt v, dt as there: w = p^ - o, tau = d . w, dist_j = clip_mm if !(tau > 0) (behind the camera), else
 *    min(|w - tau d|, clip_mm); cost = sqrt(mean dist_j^2), rounded once to fp32; +inf under the conditions there (min_joints,
 *    max_age_s).  The cost is BLIND ALONG THE RAY: a slot anywhere on the rays costs 0, so of two tracks in line with the
 *    camera either may be taken; a cost that knows the depth is left to a later version.
 * 2. The assignment runs unchanged on the one matrix that holds both kinds of rows.
 * 3. A ray row is never born: it has no depth.  Unassigned it is untracked and counted in d_n_unplaced_out, not in
 *    d_n_dropped_out, which keeps its meaning.
 * 3a. Place (new, between the births and the filter): per assigned ray row b and joint j whose slot joint has a state, whose
 *    ray is finite and with tau > 0 -- tau from the same p^, on the working state before this step's filter:
 *    z = o + tau d, the foot of the perpendicular from p^ onto the ray, and, in fp64,
 *    R = sigma2 tau^2 (I - d d^T) + depth_sigma_mm^2 d d^T: tight across the ray, wide along it, the linearised (EKF) form of
 *    a bearing measurement.  z goes to d_poses[b, j] and all nine entries of R to d_cov[b, j], each rounded once to fp32; tau
 *    to d_ray_depth_out[b, j], which is NaN everywhere else.  A joint not placed keeps what d_poses and d_cov held (NaN from
 *    the triangulation): the filter bridges it.
 * 4. The filter is unchanged and reads the fp32 arrays it always reads.  So the contract survives: metro_smooth_tracks on
 *    d_rows_out / d_starts_out and the d_poses and d_cov this launch leaves writes into d_state the working state, bit for bit.
 *    A placed joint whose ROUNDED R (scaled and floored as there) is not positive definite is predict-only (used 0): the safe
 *    outcome.
 * -1 before any launch for whatever metro_associate_tracks refuses, a measurement other than METRO_SMOOTH_COVARIANCE (an
 * isotropic R would ignore the ray's shape and pin the depth), an assignment other than 0 and 1, depth_sigma_mm not finite and
 * > 0 and, with n, n_step_rows and n_steps all > 0, a NULL pointer, d_cov and the four new ones included.  The ABI version is
 * unchanged: the entry is an addition. */
int  metro_associate_tracks_rays(float* d_poses, float* d_cov, const double* d_times, int32_t n, const int32_t* d_step_rows,
                                 int32_t n_step_rows, const int32_t* d_step_starts, int32_t n_steps, const MetroSpec* spec,
                                 int32_t measurement, double q, double r_floor, double cov_scale, double v0, double gate,
                                 float max_cost_mm, double clip_mm, int32_t min_joints, double max_age_s, double* d_state,
                                 int32_t n_tracks, int32_t* d_ids, int32_t* d_next_id, void* d_workspace,
                                 int32_t* d_track_index_out, int32_t* d_track_id_out, float* d_cost_out, int32_t* d_rows_out,
                                 int32_t* d_starts_out, int32_t* d_n_new_out, int32_t* d_n_dropped_out, int32_t assignment,
                                 const int32_t* d_single_box, const double* d_rays, double depth_sigma_mm,
                                 float* d_ray_depth_out, int32_t* d_n_unplaced_out, void* stream);

/* ---- the bone lengths of followed persons, learned per track slot and skeleton edge ----
 * Nothing in the reference: its bone-length tables come from its training data, one average skeleton per dataset.  Here every
 * person a rig follows is measured: its triangulated joints give one length per skeleton edge and exposure.  One launch after
 * metro_associate_tracks* (and metro_smooth_tracks), one workgroup of 64 threads per track slot, lane e = edge e; fp64
 * arithmetic on the fp32 inputs; E = n_edges in [1, METRO_MAX_JOINTS], J = n_joints_out in [1, METRO_MAX_JOINTS], T = n_tracks
 * in [1, METRO_ASSOC_MAX].
 * d_poses fp32 [n, J, 3] mm, ABSOLUTE (the triangulation's own output: a joint it could not place is NaN); d_cov fp32
 * [n, J, 9] mm^2 of which the upper triangle is read, NULL: isotropic mode.  d_rows int32 [n_rows] / d_starts int32 [T + 1]: the
 * CSR metro_associate_tracks* writes, slot t owning d_rows[d_starts[t] : d_starts[t + 1]] in time order; an index outside
 * [0, n) is skipped and d_starts is clamped to [0, n_rows].  d_ids int32 [T]: the track table's ids AFTER the association.
 * d_edges int32 [E, 2] in OUTPUT joint indices (Skeleton.edges, which lists head_edges in the same order); an edge with a joint
 * outside [0, J) is never measured -- checked in the kernel, nothing is read through it.  d_edge_mirror int32 [E]: the edge made
 * of the two mirror joints, in either orientation (Skeleton.edge_mirror); -1, e itself or a value outside [0, E): no partner.
 * d_fallback fp64 [E] or NULL.
 * The bone table, read and written in place: d_stats fp64 [T, E, 4] = (S0, S1, count, rejected), d_bone_ids int32 [T].
 * 0. Reset: if d_bone_ids[t] != d_ids[t] the slot's stats become 0 and d_bone_ids[t] = d_ids[t]: a slot that was freed or
 *    reused forgets the previous person.
 * 1. Per listed row, in CSR order, with e = (a, b): d = p_b - p_a, l = |d|, u = d / l.  The row is skipped, and counted
 *    nowhere, if a component of p_a or p_b is non-finite or l < min_length_mm.  Covariance mode: C = cov_scale (C_a + C_b),
 *    skipped if an entry is non-finite or a diagonal entry is < 0; q = u^T C u, v = tr C / 3 + r_floor^2,
 *    l^ = l - (tr C - q) / (2 l) (debias != 0; else l^ = l).  Isotropic mode: v = r_floor^2, l^ = l.  Skipped unless l^ > 0.
 *    Gate: if gate > 0, count >= min_count and (l^ - S1 / S0)^2 > gate (v + 1 / S0) then rejected += 1; otherwise
 *    S0 += 1 / v, S1 += l^ / v, count += 1.
 * 2. Read-out, after the workgroup barrier, from the slot's stats in LDS: S0p, S1p, countp are the sums over the edge and its
 *    mirror partner (symmetric != 0; else the edge's own).  countp >= min_count and S0p > 0: length = S1p / S0p,
 *    sigma = sqrt(1 / S0p), known = 1; otherwise length = d_fallback[e] (NaN without one), sigma = NaN, known = 0.
 *    d_lengths_out fp64 [T, E] mm, d_sigma_out fp64 [T, E] mm, d_known_out uint8 [T, E].
 * n_rows == 0 (or n == 0) with T > 0 still launches: reset and read-out only.
 * Two choices, checked with fp64 NumPy on a 250 mm bone along (0.6, 0, 0.8), joint noise N(0, s^2 diag(8, 8, 30)^2) and
 * N(0, s^2 diag(10, 10, 35)^2) mm, s ~ U(0.5, 3) per row, 20 000 rows, seeds 0 to 4:
 *  - l^ corrects the first-order bias of a noisy length: with d = delta + eps, eps ~ N(0, C),
 *    E|d| ~ |delta| + (tr C - u^T C u) / (2 |delta|).
 *  - the weight is 1 / (tr C / 3 + r_floor^2), NOT 1 / (u^T C u + r_floor^2): u is the noisy direction, and a weight that depends
 *    on it correlates with the sample's own length.  Mean error over the five seeds: direction weights -8.2 to -8.8 mm
 *    uncorrected and -14.6 to -15.3 mm with l^; trace weights +3.3 to +3.9 mm uncorrected and -0.40 to +0.15 mm with l^; unit
 *    weights with l^ -1.5 to -0.3 mm.  The trace weight still down-weights a badly seen exposure and is independent of the
 *    sample's noise direction.
 * min_count = 8, gate = 9 (3 sigma, one degree of freedom), min_length_mm = 1, r_floor = 1 and cov_scale = 1 with symmetric
 * pooling are the callers' defaults: design choices, not measurements.
 * The estimator ignores the correlation between the two joints of one person and between consecutive exposures, and it is meant
 * for the RAW triangulated measurements, not the smoothed ones, whose rows are correlated in time.
 * -1 before any launch for T, E or J out of range, negative n / n_rows, min_count < 1, gate < 0, r_floor <= 0, cov_scale < 0,
 * min_length_mm < 0 (or any of them not finite), a NULL d_ids, d_edges, d_edge_mirror, d_stats, d_bone_ids or output pointer
 * and, with n > 0 and n_rows > 0, NULL d_poses, d_rows or d_starts.  The ABI version is unchanged: the entry is an addition. */
int  metro_track_bone_lengths(const float* d_poses, const float* d_cov, int32_t n, const int32_t* d_rows, int32_t n_rows,
                              const int32_t* d_starts, int32_t n_tracks, const int32_t* d_ids, int32_t n_joints_out,
                              const int32_t* d_edges, const int32_t* d_edge_mirror, int32_t n_edges, const double* d_fallback,
                              int32_t min_count, double gate, double r_floor, double cov_scale, double min_length_mm,
                              int32_t debias, int32_t symmetric, double* d_stats, int32_t* d_bone_ids, double* d_lengths_out,
                              double* d_sigma_out, uint8_t* d_known_out, void* stream);

/* ---- next-frame person boxes from the track table: crops between the key frames of a detector ----
 * Nothing in the reference: one example is one image and its box is given.  Two launches on `stream`, no host work in
 * between: one thread per (frame, slot) writes dense tables, one workgroup compacts them into rows and appends the
 * detector's boxes that no predicted box covers.  The table is READ, never written.
 * Track table as metro_associate_tracks has it: d_state fp64 [T, J, 28], d_ids int32 [T] (-1: free), T = n_tracks in
 * [1, METRO_ASSOC_MAX], J = n_joints_out in [1, METRO_MAX_JOINTS]; the positions are absolute mm in the frame's camera
 * (coords METRO_COORDS_CAMERA: r and t of the camera table are not read) or in the world (METRO_COORDS_WORLD).
 * d_cameras: DEVICE table of n_cameras == 1 (every frame) or n_cameras == n_frames entries; frame_sizes int32 [F, 2] (W, H)
 * and frame_times fp64 [F] seconds are HOST arrays, copied into the kernel arguments (F = n_frames in [1, METRO_MAX_FRAMES]).
 * Per (frame f, slot s):
 * 1. d_ids[s] < 0, no joint with a state (t_last NaN), or frame_times[f] - (the newest t_last of the slot) > max_age_s:
 *    no box, joint count -1.
 * 2. Every joint with a state is advanced by dt = max(frame_times[f] - t_last, 0) with the prediction step of
 *    metro_smooth_tracks (white-noise acceleration q): the position metro_associate_tracks compares a box against, and its P.
 * 3. Camera point: METRO_COORDS_WORLD R (p - t) (Camera.world_to_camera) from the fp32 entries, in fp64; else p itself.  The
 *    joint is VISIBLE iff the point is finite, z >= near_mm and, with has_distortion and r2 = (x/z)^2 + (y/z)^2,
 *    1 + 3 k1 r2 + 5 k2 r2^2 + 7 k3 r2^3 > 0 (the radial polynomial still grows: beyond, it folds a far joint back into the
 *    image), and its pixel is finite.
 * 4. Pixel (u, v): the point rounded to fp32, then project_points' fp32 chain in its statement order with has_distortion
 *    (metro_place_poses' keypoints), else K (x/z, y/z, 1) in fp32.
 * 5. Margin, fp64: sigma = min(sqrt(max(Pxx, Pyy, Pzz, 0)), max_sigma_mm), mg = n_sigma sigma sqrt(|fx fy|) / z; the joint
 *    contributes [u - mg, u + mg] x [v - mg, v + mg].
 * 6. Box, fp64: the union over the visible joints; their count goes to d_joints_dense; fewer than min_joints: no box.  The
 *    union is scaled about its centre by expand, intersected with [0, W_f] x [0, H_f] when clip != 0, and dropped if then
 *    narrower or lower than min_side_px.  d_boxes_dense fp64 [F, T, 4] (x, y, w, h), all NaN where there is no box;
 *    d_joints_dense int32 [F, T].
 * Rows, capacity F T + n_detections (d_boxes_out fp64 [., 4], d_frame_out, d_slot_out, d_id_out, d_detection_out,
 * d_n_joints_out int32 [.]): first the boxes present, frame-major then by slot, with their frame, slot, d_ids[slot],
 * detection -1 and joint count; then the detections (d_det_boxes fp64 [m, 4], d_det_frame int32 [m], both NULL with
 * n_detections == 0, m <= METRO_PREDICT_MAX_DETECTIONS) in their given order with slot -1, id -1, detection = their index and
 * joint count -1.  A detection whose frame lies outside [0, F) is dropped and counted in d_counts[4], which the caller must
 * treat as an error; else one with a non-finite coordinate or w <= 0 or h <= 0 is dropped and counted in d_counts[3]; else
 * one whose intersection over union with ANY predicted box of its frame is >= iou_max is suppressed and counted in
 * d_counts[2].  d_counts int32 [5]: rows written, predicted rows, suppressed, bad detections, bad frame indices; rows past
 * d_counts[0] are not written.
 * -1 before any launch for J, T, F or n_detections out of range, coords other than METRO_COORDS_CAMERA / _WORLD, a
 * non-finite or out-of-range q (> 0), max_age_s (>= 0), expand (>= 1), n_sigma (>= 0), max_sigma_mm (>= 0), near_mm (> 0),
 * min_side_px (>= 0) or iou_max (in (0, 1]), min_joints outside [1, J], n_cameras neither 1 nor F, a NULL pointer, a frame
 * size < 1 and a non-finite frame time.  With T F == 0 rows and no detections there is nothing to do: no launch, nothing
 * written, 0. */
#define METRO_PREDICT_MAX_DETECTIONS 4096
int  metro_predict_boxes(const double* d_state, const int32_t* d_ids, int32_t n_tracks, int32_t n_joints_out,
                         const MetroFrameCamera* d_cameras, int32_t n_cameras, const int32_t* frame_sizes,
                         const double* frame_times, int32_t n_frames, int32_t coords, double q, double max_age_s,
                         double expand, double n_sigma, double max_sigma_mm, double near_mm, double min_side_px,
                         int32_t min_joints, int32_t clip, const double* d_det_boxes, const int32_t* d_det_frame,
                         int32_t n_detections, double iou_max, double* d_boxes_dense, int32_t* d_joints_dense,
                         double* d_boxes_out, int32_t* d_frame_out, int32_t* d_slot_out, int32_t* d_id_out,
                         int32_t* d_detection_out, int32_t* d_n_joints_out, int32_t* d_counts, void* stream);

const char* metro_last_error(void);
int32_t metro_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* METRO_HIP_H */
