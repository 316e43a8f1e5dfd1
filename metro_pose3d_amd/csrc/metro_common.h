// Internal helpers shared by the HIP translation units of libmetro_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/metro_hip.h"

namespace metro {

// thread-local last-error message (metro_last_error)
void set_error(const char* fmt, ...);
const char* get_error();

#define METRO_CHECK_ARG(cond, ...)                  \
    do {                                            \
        if (!(cond)) {                              \
            ::metro::set_error(__VA_ARGS__);        \
            return METRO_ERR_INVALID_ARG;           \
        }                                           \
    } while (0)

#define METRO_HIP_CHECK(expr)                                                              \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            ::metro::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),      \
                               __FILE__, __LINE__);                                        \
            return METRO_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

// Tuning knobs: compile-time constants in the product build.  A build with -DMETRO_TUNING_KNOBS (tools/
// build_dbg_variants.sh, A/B timing runs) reads them from the environment instead; the product never calls getenv.
inline int tuning_knob(const char* name, int dflt) {
#ifdef METRO_TUNING_KNOBS
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// ---- dispatch notes ----------------------------------------------------------------------------------------
// Which kernel INSTANTIATION a layer runs on depends on its shape and on the batch (tile counts vs 256 CUs).  Every
// leaf launcher calls note_kernel() FIRST -- before any HIP call -- with the id of the instantiation it is about to
// launch.  Off (the default) it is one thread-local load; mode 1 appends the id to a thread-local string
// (metro_last_kernel_id); mode 2 is a DRY RUN: the id is recorded and the launcher returns METRO_OK without touching
// the device (metro_plan_layer_kernel, and the coverage test in tests/test_kernel_coverage.py, work without a GPU).
struct KernelNotes {
    int mode;
    char ids[4096];       // holds the ids of a whole forward; a string that did not fit ends in " ..." (tests assert against it)
    int32_t schedule[4];  // the last persistent launch's tile-walk schedule (note_schedule; metro_last_launch_schedule)
};
KernelNotes& kernel_notes();
bool note_kernel(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // true = dry run: skip the launch
// The schedule of a persistent launch -- a launcher that caps its grid with ensure_dyn_lds_and_grid_cap and lets a block walk several
// tiles -- recorded right after the launcher has computed its grid: the grid launched, the work items (tiles x halves, or
// patches), the grid cap (CUs x resident blocks per CU: known on the device only) and `halves` (blocks that share a tile, one per
// output-channel slab; 1 where a block owns its tiles).  What a block's tile loop does -- buffer parity, counted waits, ramp and
// drain -- follows from these four (tests/test_gpu_persistent_schedules.py: schedule_class).  Off (the default) this is one
// thread-local load, like note_kernel.  A dry run reaches no device: its launchers record the uncapped grid and a cap of 0.
inline void note_schedule(int grid, int work, int cap, int halves) {
    KernelNotes& kn = kernel_notes();
    if (kn.mode == 0) return;
    kn.schedule[0] = grid; kn.schedule[1] = work; kn.schedule[2] = cap; kn.schedule[3] = halves;
}

// ---- block -> tile maps of the grids that deal their blocks round-robin to the 8 XCDs (one L2 each) -------------------------------
// Integer arithmetic on blockIdx / gridDim only, __host__ __device__ so that tests/test_block_tile_maps.py walks them on the
// host for every grid a device could ask for.
// conv_pw64.hip / conv_pws.hip: `grid` = halves x G blocks serve G tile streams; block b works on the CB-channel slab `half` of the
// tiles first, first + G, ...  The `halves` blocks that share a tile are placed on the SAME XCD (b & 7) wherever the grid splits
// into eight equal runs of whole streams; otherwise consecutive blocks share a tile.
struct BlockStream { int half, first; };
// (block and grid keep the unsigned type of blockIdx.x / gridDim.x: the divisions by `halves` are the unsigned ones the kernels
// were built with)
__host__ __device__ __forceinline__ BlockStream block_stream_map(unsigned block, unsigned grid, int halves) {
    BlockStream s;
    if ((grid & 7) == 0 && ((grid >> 3) % halves) == 0) {
        const int xcd = block & 7, j = block >> 3;
        s.half = j % halves;
        s.first = xcd * ((grid >> 3) / halves) + j / halves;
    } else {
        s.half = block % halves;
        s.first = block / halves;
    }
    return s;
}
// conv_igemm_f16_dma.hip / conv3x3_f16_slab.hip: one tile per block; the blocks of one XCD get a contiguous run of tile ids
// (bijective for any nblk: the first nblk & 7 XCDs hold one block more)
__host__ __device__ __forceinline__ int xcd_block_lid(int block, int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = block & 7, idx = block >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// 16-byte activation store of an epilogue, in the form its translation unit chose with METRO_WT_STORES:
//   0  plain: the line stays DIRTY in the writing XCD's L2 (the eight L2s are not coherent), and the release at the end of the
//      launch writes every dirty line back, with no wave running, before the next launch may start.
//   1  write-through (sc1): the bytes go to memory while the kernel runs and the line is dropped from the L2, so the launch ends
//      clean.  The consumer loses nothing: every launch fetches its input from beyond the L2 anyway (profiles/*_pmc_layers.tsv).
// A kernel file that ships write-through defines METRO_WT_STORES 1 above its includes (unless the command line set it:
// tools/build_variant.sh <name> "-DMETRO_WT_STORES=0|1" <file>.hip flips one family); NOTES_dead_ends.md has the A/B per family.
// Inline asm, not __builtin_amdgcn_raw_buffer_store_b128(.., aux 16), which hipcc would count: the builtin wants a wave-uniform
// descriptor and a 32-bit offset, the 17 call sites hold per-lane 64-bit pointers into tensors of up to 16 GiB (block4's output
// at stride 4, crop side 512, 256 crops: 2^33 fp16 elements -- no 32-bit offset reaches across them), and a per-lane
// descriptor costs a waterfall loop.  hipcc does not model the asm: `s_nop 1` keeps the data registers from being rewritten while
// the store reads them, and the store is absent from the compiler's vmcnt bookkeeping -- compiler-placed waits count fewer
// younger operations than there are (longer waits, never shorter); A CALLER WITH A HAND-COUNTED WAIT COUNTS THESE STORES ITSELF
// (one instruction each, as before).  No "memory" clobber: no kernel reads back what it stores here; volatile asm keeps its order.
typedef unsigned int metro_u32x4 __attribute__((ext_vector_type(4)));
#ifndef METRO_WT_STORES
#define METRO_WT_STORES 0
#endif
__device__ __forceinline__ void store_out16(void* p, uint4 v) {
#if METRO_WT_STORES
    const metro_u32x4 w = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(w));
#else
    *reinterpret_cast<uint4*>(p) = v;
#endif
}

// ---- launch-resident weight fragments of the persistent (weight-stationary) kernels -------------------------------------------
// A wave keeps `rows32` x 32 weight rows [.][K] as v_mfma_f32_32x32x16_f16 A fragments: lane (r = lane & 31, h = lane >> 5) holds
// W[row][16 kk + 8 h .. + 7] for every k step kk.  Loading them straight from global memory asks the L2 for 32 rows x 32 bytes per
// wave instruction -- and the L2s answer a near-constant REQUEST rate (~120 G requests/s chip-wide, whatever the size):
// 256 blocks x 8 waves x K/4 instructions x 32 pieces is 2.1 M requests = 16-17 us at K = 512 (8 us at K = 256) before the first
// MFMA of the launch, measured as the batch-independent part of conv_pws / conv_pw64 (round 5).  Staged form: the wave copies 32
// rows x 256 bytes per step with 8 loads of 4 x 256 contiguous bytes (8x fewer, 8x larger requests) into a PRIVATE 8.5 KiB LDS
// scratch (rows padded to 272 bytes: conflict-free 16-byte reads of 32 rows) and reads its fragments back.  No barrier: LDS
// executes a wave's instructions in order; wave_barrier() only keeps hipcc from moving the reads above the writes.
constexpr int W_STAGE_ROW = 272;
constexpr int W_STAGE_BYTES = 32 * W_STAGE_ROW;            // per wave
template <int K, typename Frag>
__device__ __forceinline__ void load_w_frags_staged(const _Float16* __restrict__ rows /* the wave's first row */, Frag* wf /* [K / 16] */,
                                                    char* scratch /* wave-private, W_STAGE_BYTES */, int lane) {
    static_assert(K % 128 == 0 || K == 64, "whole 256-byte row pieces (K = 64: one 128-byte piece)");
    constexpr int PIECE = K >= 128 ? 128 : 64;             // channels per staged step
    constexpr int LPR = PIECE / 8;                         // lanes per row: 16 (or 8)
    constexpr int RPI = 64 / LPR;                          // rows per load instruction: 4 (or 8)
    const int lr = lane / LPR, lc = lane % LPR;
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int c = 0; c < K / PIECE; ++c) {
#pragma unroll
        for (int j = 0; j < 32 / RPI; ++j)
            *reinterpret_cast<uint4*>(scratch + (j * RPI + lr) * W_STAGE_ROW + lc * 16) =
                *reinterpret_cast<const uint4*>(rows + (size_t)(j * RPI + lr) * K + c * PIECE + lc * 8);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k8 = 0; k8 < PIECE / 16; ++k8)
            wf[c * (PIECE / 16) + k8] = *reinterpret_cast<const Frag*>(scratch + fr * W_STAGE_ROW + k8 * 32 + fh * 16);
        __builtin_amdgcn_wave_barrier();
    }
}

// The same for v_mfma_f32_16x16x32_f16 A fragments: 16 weight rows [.][K], lane (r = lane & 15, g = lane >> 4) holds
// W[row][32 ks + 8 g .. + 7] for every k step ks (K / 32 registers of 16 bytes).  Staged 128 channels (256-byte row pieces) at a time.
template <int K, typename Frag>
__device__ __forceinline__ void load_w_frags16_staged(const _Float16* __restrict__ rows, Frag* wf /* [K / 32] */, char* scratch, int lane) {
    static_assert(K % 128 == 0, "whole 256-byte row pieces");
    const int lr = lane >> 4, lc = lane & 15;
#pragma unroll
    for (int c = 0; c < K / 128; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<uint4*>(scratch + (j * 4 + lr) * W_STAGE_ROW + lc * 16) =
                *reinterpret_cast<const uint4*>(rows + (size_t)(j * 4 + lr) * K + c * 128 + lc * 8);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
            wf[c * 4 + k4] = *reinterpret_cast<const Frag*>(scratch + (lane & 15) * W_STAGE_ROW + k4 * 64 + (lane >> 4) * 16);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- per-device one-time kernel setup -----------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) and the occupancy query act on the CURRENT device's copy of a
// kernel: a process that drives several GPUs (inference.py caches one Engine per device) must do them once per
// device, not once per process.  Zero-initialised statics of this type replace `static bool attr_set`.
constexpr int METRO_MAX_DEVICES = 64;
struct PerDeviceInt { int v[METRO_MAX_DEVICES]; };

inline int current_device_slot(int* slot) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= METRO_MAX_DEVICES) {
        set_error("hipGetDevice: %s (device %d; at most %d devices per process)", hipGetErrorString(e), dev, METRO_MAX_DEVICES);
        return METRO_ERR_HIP;
    }
    *slot = dev;
    return METRO_OK;
}

// opts a kernel in to `bytes` of dynamic LDS on the current device (once per device)
inline int ensure_dyn_lds(const void* kern, int bytes, PerDeviceInt& done, const char* what) {
    int slot = 0;
    const int st = current_device_slot(&slot);
    if (st) return st;
    if (done.v[slot]) return METRO_OK;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute(%s, %d B of LDS, device %d): %s", what, bytes, slot, hipGetErrorString(e));
        return METRO_ERR_HIP;
    }
    done.v[slot] = 1;
    return METRO_OK;
}

// same, and returns CUs x resident blocks per CU of the kernel on the current device (persistent kernels' grid cap)
inline int ensure_dyn_lds_and_grid_cap(const void* kern, int threads, int bytes, PerDeviceInt& cap, const char* what,
                                       int max_blocks_per_cu, int* grid_cap) {
    int slot = 0;
    int st = current_device_slot(&slot);
    if (st) return st;
    if (cap.v[slot] == 0) {
        const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) {
            set_error("hipFuncSetAttribute(%s, %d B of LDS, device %d): %s", what, bytes, slot, hipGetErrorString(e));
            return METRO_ERR_HIP;
        }
        int cus = 0, occ = 0;
        METRO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, slot));
        if (const int lim = tuning_knob("METRO_CU_LIMIT", 0); lim > 0 && lim < cus) cus = lim;   // A/B builds: partitioned-GPU experiments
        METRO_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, threads, bytes));
        if (occ < 1) occ = 1;
        if (max_blocks_per_cu > 0 && occ > max_blocks_per_cu) occ = max_blocks_per_cu;
        cap.v[slot] = cus * occ;
    }
    *grid_cap = cap.v[slot];
    return METRO_OK;
}

inline int launch_status(const char* what) {
    if (kernel_notes().mode == 2) {     // a leaf launcher that did not call note_kernel() before touching the device
        set_error("internal: %s was launched during a dry run (note_kernel must come first)", what);
        return METRO_ERR_STATE;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("launch of %s failed: %s", what, hipGetErrorString(e));
        return METRO_ERR_HIP;
    }
    return METRO_OK;
}

// Two convolutions over the same input fused into one launch: weight/bias rows [0, split) belong
// to the first output (desc.c_out == split + c_out2 rows in total), rows [split, ...) to `out2`
// (NHWC with c_out2 channels, its own ReLU flag).  split must be a multiple of the cout tile.
struct ConvSplit {
    int split = 0;
    int c_out2 = 0;
    int relu2 = 0;
    void* out2 = nullptr;
};

// conv3 of a unit + conv1 of the NEXT unit in one launch (block1: full 256-channel rows per pixel tile):
// after the shortcut add, t1 = relu(W2 * relu(x_out * scale2 + shift2) + bias2) is computed from the
// LDS-resident output tile (reference resnet_v2.py:119,127-128 of unit u+1 on the output of :138 of unit u).
struct ConvFuse2 {
    const void* w2 = nullptr;       // fp16 [c2][c_out], BN-folded
    const float* bias2 = nullptr;   // [c2]
    const void* scale2 = nullptr;   // fp16 [c_out]  (pre-activation BN of unit u+1)
    const void* shift2 = nullptr;
    void* out2 = nullptr;           // fp16 NHWC [.., c2]
    int c2 = 0;
};

// conv1 of the SAME unit in front of a 64 -> 64 3x3 (conv3x3_c64.hip PRE1; block1/unit_1, whose input has 64 channels):
// t1 = relu(W1 * relu(x * scale + shift) + bias1) is computed on the LDS-resident slab (reference resnet_v2.py:119,127-128)
struct ConvPre1 {
    const void* w1 = nullptr;         // fp16 [64][64], BN-folded
    const float* bias1 = nullptr;     // [64]
    const void* pro_scale = nullptr;  // fp16 [64] pre-activation BN of the unit
    const void* pro_shift = nullptr;
    void* t1_dump = nullptr;          // optional: conv1's output fp16 [pixels][64] (layer dumps for the tests; NULL in the product path)
};

// Projection shortcut of the unit computed INSIDE its conv3 launch (conv_pw64.hip PSC; block1/unit_1): shortcut =
// fp16(Wsc * relu(x * scale + shift) + bias_sc) from the unit's 64-channel input x (reference resnet_v2.py:119,122-125),
// added to fp16(conv3 + bias) in fp16 like the reference graph (:138) -- the shortcut tensor never exists in HBM
struct ConvProjSc {
    const void* x = nullptr;          // fp16 [pixels][64]: the unit's raw input
    const void* w_sc = nullptr;       // fp16 [256][64]
    const float* bias_sc = nullptr;   // [256]
    const void* pro_scale = nullptr;  // fp16 [64]
    const void* pro_shift = nullptr;
};

// block1 without its 256-channel residual stream in HBM (conv_pw64.hip REB / OUTM, round 5).  The launch conv3(u) + conv1(u+1):
//   t2_prev != NULL  the unit's identity shortcut x_{u-1} is REBUILT in the launch from the previous unit's conv2 output and conv3
//                    parameters + the projection shortcut of ConvProjSc (x_{u-1} = fp16(W3_prev . t2_prev + b) + fp16(Wsc . pre(x0) + bsc)),
//                    reference resnet_v2.py:119-125,134-138 of unit u-1, instead of being read as a 512-byte-per-pixel tensor;
//   out_mode         0 = the launch's sum is stored in full, 1 = not at all (it only feeds the next unit's conv1 in the launch),
//                    2 = only the pixels (sub_off + 2 i, sub_off + 2 j) the next, strided unit's shortcut reads (resnet_v2.py:113-121;
//                    resnet_utils.py:64-79), as a compact [n, h_sub, w_sub, 256] tensor.
struct ConvRebuild {
    const void* t2_prev = nullptr;     // fp16 [pixels][64]
    const void* w3_prev = nullptr;     // fp16 [256][64]
    const float* bias3_prev = nullptr; // [256]
    int out_mode = 0;
    void* out_sub = nullptr;
    int sub_off = 0, h_sub = 0, w_sub = 0;
    int classic = 0;                   // 1 = the single-role kernel of conv_pw64.hip even where conv_b1.hip's producer / consumer form
                                       // would be dispatched (metro_forward_upto stopping at the layer: an independent second form)
};

// The shape of a fused conv launch (one launch that does more than one convolution), decided once -- by the planner or a C entry,
// checked with conv_form_supported -- and read by every launcher on the way to the kernel:
//   Plain        one convolution
//   Pair         the projection shortcut + conv1 of a unit over concatenated weight rows (`pair`)
//   Next         conv3 of a unit + conv1 of the next unit (`next`)
//   NextProj     Next with the unit's projection shortcut computed in the launch (`psc`; block1/unit_1); rb.out_mode 0 | 1
//   NextRebuild  NextProj on top of the unit's identity shortcut rebuilt in the launch (`rb`; block1/unit_2); rb.out_mode 0 | 2
// (ConvPre1, conv1 in front of the 64-channel 3x3, belongs to conv3x3_c64.hip's family and is not one of them.)
enum class ConvForm { Plain, Pair, Next, NextProj, NextRebuild };

struct ConvFused {
    ConvForm form = ConvForm::Plain;
    ConvSplit pair;
    ConvFuse2 next;
    ConvProjSc psc;
    ConvRebuild rb;    // out_mode and classic apply to NextProj too
};

// device-side view of MetroConvDesc plus derived values
struct ConvArgs {
    int split, c_out2, relu2;   // see ConvSplit (0 = plain convolution)
    int n, h_in, w_in, c_in, in_pix_stride;
    int h_out, w_out, c_out;
    int kh, kw, stride, dil, pad_top, pad_left;
    int res_h, res_w, res_stride, res_offset;
    int m_total;   // n * h_out * w_out
    int relu;
};

inline ConvArgs make_conv_args(const MetroConvDesc& d) {
    ConvArgs a;
    a.split = 0; a.c_out2 = 0; a.relu2 = 0;
    a.n = d.n; a.h_in = d.h_in; a.w_in = d.w_in; a.c_in = d.c_in; a.in_pix_stride = d.in_pix_stride;
    a.h_out = d.h_out; a.w_out = d.w_out; a.c_out = d.c_out;
    a.kh = d.kh; a.kw = d.kw; a.stride = d.stride; a.dil = d.dilation;
    a.pad_top = d.pad_top; a.pad_left = d.pad_left;
    a.res_h = d.res_h; a.res_w = d.res_w; a.res_stride = d.res_stride; a.res_offset = d.res_offset;
    a.m_total = d.n * d.h_out * d.w_out;
    a.relu = d.relu;
    return a;
}

int validate_conv_desc(const MetroConvDesc* d);

// the device tensors of one fp16 conv launch (a fused form's further tensors travel in its ConvFused)
struct ConvOperands {
    const void* in;
    const void* w;
    const float* bias;
    const void* pro_scale;
    const void* pro_shift;
    const void* residual;
    void* out;
};

// ---- fp16 convolution dispatch (conv_dispatch.cpp) ---------------------------------------------------------------------------
// The kernel families of the product, and the one ordered rule "form f.form of layer d runs on family K".  None: no family runs it.
enum class ConvKernel { C64, Slab, Pws, Pw64, B1Chain, Gemm4w, Fuse2, Ring, None };
ConvKernel choose_conv_kernel(const MetroConvDesc& d, const ConvFused& f);
// the dispatcher: one launch on the family choose_conv_kernel names (metro_conv_f16*, every fp16 conv layer of the plan);
// a fused `f` has passed conv_form_supported (the planner, the C entries)
int launch_conv_f16(const MetroConvDesc& d, const ConvOperands& o, hipStream_t stream, const ConvFused& f = ConvFused{});
// whether `d` with the parts of `f` can run as one launch of form f.form: the one shape rule of each form (the pair's split, the
// second GEMM's c2, the rebuilt residual's map and output mode), read by the planner, the C entries and the dispatch
bool conv_form_supported(const MetroConvDesc& d, const ConvFused& f);

// ---- kernel launchers implemented in the .hip files: each file launches its own kernels only ------------------------------------
// LDS-DMA ring kernel, coalesced epilogue (conv_igemm_f16_dma.hip); `split`: the two outputs of a Pair, else NULL
bool conv_f16_dma_supported(const MetroConvDesc& d);
int launch_conv_ring(const MetroConvDesc& d, const ConvOperands& o, hipStream_t stream, const ConvSplit* split);
// its one-K-step form with the next unit's conv1 as a second GEMM on the LDS-resident output tile (block1's Next launches)
bool conv_f16_fuse2_supported(const MetroConvDesc& d, int c2);
int launch_conv_fuse2(const MetroConvDesc& d, const ConvOperands& o, hipStream_t stream, const ConvFuse2& f);
// 256 x 256 x 64 GEMM, four waves of 128 x 128, register-staged operands (conv_gemm4w.hip): the pre-activated deep-K 1x1 layers
// (conv1, projection shortcut, shortcut + conv1 pair of blocks 3-4) with at least one tile per CU
bool conv_gemm4w_shape_ok(const MetroConvDesc& d, const ConvSplit* split);      // what the kernel can run
bool conv_gemm4w_supported(const MetroConvDesc& d, const ConvSplit* split);     // ... and when the dispatcher prefers it
int launch_conv_gemm4w(const MetroConvDesc& d, const ConvOperands& o, hipStream_t stream, const ConvSplit* split);
// persistent pipelined kernel for block1's 64-channel 1x1 convolutions and the conv3 layers of blocks 2-4 (conv_pw64.hip): whether it
// runs `d` in form f.form with f's parts
bool conv_pw64_supported(const MetroConvDesc& d, const ConvFused& f);
int launch_conv_pw64(const MetroConvDesc& d, const ConvOperands& o, hipStream_t stream, const ConvFused& f);
// the maps the rebuilt residual (conv_pw64.hip) and the producer / consumer form (conv_b1.hip) are built for: whole 64-pixel tiles,
// width a power of two >= 16 (the sub-sampled copy's pixel arithmetic)
inline bool b1_map_ok(const MetroConvDesc& d) {
    return (d.h_out * d.w_out) % 64 == 0 && d.w_out >= 16 && (d.w_out & (d.w_out - 1)) == 0;
}
// producer / consumer form of the NextProj / NextRebuild launches of block1 whose sum stays on chip or is rebuilt (conv_b1.hip):
// whether it is preferred for a launch that has passed conv_form_supported (the form, its output mode, rb.classic, the knob, the map)
bool conv_b1_chain_supported(const MetroConvDesc& d, const ConvFused& f);
void conv_b1_set_form(int classic);      // thread-local test switch: 1 = never dispatch it (nor conv_pws.hip's kernel)
bool classic_forms_forced();
// conv3 + shortcut of blocks 3-4 with the two waves of a SIMD half a tile apart (conv_pws.hip); same bits as conv_pw64's <k256|k512,wm8,res>
bool conv_pws_supported(const MetroConvDesc& d);
int launch_conv_pws(const MetroConvDesc& d, const void* in, const void* w, const float* bias, const void* res, void* out, hipStream_t stream);
int launch_conv_b1_chain(const MetroConvDesc& d, const void* in, const void* w, const float* bias, void* out, hipStream_t stream,
                         const ConvFused& f);
// stem 7x7/2 conv + zero-padded 3x3/2 max-pool in one persistent kernel (stem_pool_f16.hip); input is the
// bordered 4-channel fp16 image of launch_prep_input_f16, weights packed [64][7][8][4]
bool stem_pool_f16_supported(int side, int base_width);
int launch_stem_pool_f16(const void* prepped, const void* w, const float* bias, void* out, int n, int side,
                         hipStream_t stream);
// same, reading the fp32 NHWC3 crops directly (prep_input_f16 fused away)
bool stem_pool_f32in_supported(int side, int base_width);
int launch_stem_pool_f32in(const float* images, const void* w, const float* bias, void* out, int n, int side,
                           hipStream_t stream);
// same, reading uint8 NHWC3 crops (16-byte aligned; byte b = fp32 b / 255): where stem_pool_f32in_supported
int launch_stem_pool_u8in(const unsigned char* images, const void* w, const float* bias, void* out, int n, int side,
                          hipStream_t stream);
// persistent weight-resident 3x3 for the 64 -> 64 channel layers (conv3x3_c64.hip)
bool conv3x3_c64_supported(const MetroConvDesc& d);
int launch_conv3x3_c64(const MetroConvDesc& d, const void* in, const void* w, const float* bias, void* out, hipStream_t stream,
                       const ConvPre1* pre1 = nullptr);
// 3x3 stride-1 convs with tap reuse from an LDS-resident activation slab
bool conv3x3_slab_supported(const MetroConvDesc& d);
int launch_conv3x3_slab(const MetroConvDesc& d, const void* in, const void* w, const float* bias, void* out,
                        hipStream_t stream);
int launch_conv_f64acc(const MetroConvDesc& d, const void* in, const double* w, const double* bias,
                       const double* pro_scale, const double* pro_shift, const void* residual,
                       void* out, hipStream_t stream);
// fp32 conv on the fp32 matrix cores (conv_igemm_f32.hip): METRO_PREC_F32M
int launch_conv_f32m(const MetroConvDesc& d, const void* in, const float* w, const float* bias, const float* pro_scale,
                     const float* pro_shift, const void* residual, void* out, hipStream_t stream);
int launch_prep_input_f16(const float* images, int n, int side, void* out, hipStream_t stream);
int launch_prep_input_u8_f16(const unsigned char* images, int n, int side, void* out, hipStream_t stream);
int launch_images_u8_to_f32(const unsigned char* in, long count, float* out, hipStream_t stream);
// the warp launchers: OutT = float (crops in [0, 1]) or unsigned char (the remapped byte itself)
struct FrameTable { MetroFrame f[METRO_MAX_FRAMES]; };
template <typename OutT>
int launch_warp_crops_frames_u8(const FrameTable& frames, int n_frames, const MetroCropWarp* crops, int n, int side,
                                OutT* out, hipStream_t stream);
// 64 x 48 bytes: passed by value, inside the 4 KiB of kernel arguments
struct FramePlanesTable { MetroFramePlanes f[METRO_MAX_FRAMES]; };
template <typename OutT>
int launch_warp_crops_frames_planes(const FramePlanesTable& frames, int n_frames, const MetroCropWarp* crops, int n,
                                    int side, OutT* out, hipStream_t stream);
template <typename OutT>
int launch_warp_crop_u8(const unsigned char* img, int h, int w, int row_stride, const float* homs, OutT* out,
                        int n, int side, hipStream_t stream);
int launch_eval_metrics(const float* pred, const float* truth, const unsigned char* valid, int n, int nj,
                        float threshold, float* dist, float* dist_pa, double* sums, hipStream_t stream);
int launch_maxpool(const void* in, void* out, int n, int h_in, int w_in, int c, int dtype,
                   hipStream_t stream);

struct SoftArgmaxArgs {
    int n, side, depth, n_joints_head, n_joints_out;
    int lrc, half_off;           // decode constants (reference volumetric.py:288-295)
    float box_size_mm;
    int proc_side;
    int perm[METRO_MAX_JOINTS];
};
// What the spec fixes of a decode launch's arguments (host side).  The pixel scale of heatmap_to_image (reference
// volumetric.py:288-295), as integers; a kernel that takes them as fp32 casts them.
struct HeadPixelScale { int lrc, half_off; };
inline HeadPixelScale head_pixel_scale(const MetroSpec& spec) {
    const int last = spec.proc_side - 1;
    return {last - (last % spec.stride) - 1,                    // last_receptive_center (:290-291)
            spec.centered_stride ? spec.stride / 2 : 0};        // :293-294
}
// head joint of every exported joint (main.py:119-127), 0 behind n_joints_out
inline void head_permutation(const MetroSpec& spec, int (&perm)[METRO_MAX_JOINTS]) {
    for (int i = 0; i < METRO_MAX_JOINTS; ++i) perm[i] = i < spec.n_joints_out ? spec.permutation[i] : 0;
}
// Heat-map moments (metro_forward_moments and the kernel-level *_moments entries): `scratch` non-NULL selects the MOMENTS
// instantiations, which write one record of six second central moments per (image, slab, joint) there (moments_scratch_bytes;
// in the accumulator type of the launch) and fold them into cov01 fp32 [n][J_head][6] (xx, yy, zz, xy, xz, yz) and peak [n][J_head].
struct MomentsOut {
    void* scratch = nullptr;
    float* cov01 = nullptr;
    float* peak = nullptr;
};
int64_t moments_scratch_bytes(int n, int side, int n_joints_head);
int softargmax_slabs(int n, int side);
int64_t softargmax_scratch_bytes(int n, int side, int n_joints_head);
int launch_softargmax(const void* logits, const SoftArgmaxArgs& a, int precise, void* partials,
                      float* poses_out, hipStream_t stream, float* coords01_out = nullptr, int32_t* status = nullptr,
                      const MomentsOut& mo = MomentsOut{});
// `status` (optional, int32 [n]): 1 where an image's soft-argmax statistics were not finite (fp16 overflow upstream), else 0
// finalize only (slabs folded, mm decode, root-relative, permutation) on fp32 partials written by another kernel
int launch_softargmax_finalize(const float* partials, const SoftArgmaxArgs& a, int slabs, float* poses_out,
                               hipStream_t stream, float* coords01_out = nullptr, int32_t* status = nullptr,
                               const MomentsOut& mo = MomentsOut{});
// Heat-map marginals of a bound forward (heat_marginals.hip): xy [n][J_out][S][S] and z [n][J_out][D] from the logits
// (fp32, or fp64 with precise == 2; precise as launch_softargmax).  `scratch`: heat_marginals_scratch_bytes(max_n, ...) bytes;
// with_logits plans (the one-launch head) also keep the head's fp32 logits there, at heat_marginals_scratch_logits.
int64_t heat_marginals_scratch_bytes(int n, int side, int n_joints_head, int depth, bool with_logits);
float* heat_marginals_scratch_logits(void* scratch, int max_n, int side, int n_joints_head, int depth);
int launch_heat_marginals(const void* logits, int precise, int n, int max_n, const MetroSpec& spec, void* scratch, float* xy_out,
                          float* z_out, hipStream_t stream);
// Heat-map modes of a bound forward (heat_modes.hip): voxel [n][J_out][k] and stats [n][J_out][k][11] from the logits (as above).
// The kernel needs no scratch; with_logits plans keep the head's fp32 logits in the bound scratch, from its first byte.
int64_t heat_modes_scratch_bytes(int n, int side, int n_joints_head, int depth, bool with_logits);
int launch_heat_modes(const void* logits, int precise, int n, int max_n, const MetroSpec& spec, int k, int radius, int32_t* voxel_out,
                      float* stats_out, hipStream_t stream);
// Heat-map posterior under a Gaussian prior of a bound forward (heat_posterior.hip): post [n][J_out][11] from the logits (as above)
// and the prior rows [n][J_out][9].  The kernel needs no scratch; with_logits plans keep the head's fp32 logits in the bound
// scratch, from its first byte.
int64_t heat_posterior_scratch_bytes(int n, int side, int n_joints_head, int depth, bool with_logits);
int launch_heat_posterior(const void* logits, int precise, int n, int max_n, const MetroSpec& spec, const float* prior, float* post_out,
                          hipStream_t stream);
// The prior rows of a forward with a track table bound (track_priors.hip): prior [n][J_out][9] and reason [n][J_out] from the
// table's states, the rows' slots, times and placement records; coords01 is the forward's own (read with DEPTH_ROOT only).
int track_prior_root_out(const MetroSpec& spec);      // the output joint of head joint J_head - 1, -1: not in the output order
int launch_track_priors(const double* state, int capacity, const int* slot, const double* times, const MetroPlacement* rec,
                        const int* mirror, const MetroTrackPrior& params, const float* coords01, int n, const MetroSpec& spec,
                        float* prior_out, int* reason_out, hipStream_t stream);
// The fused world joints of a forward with a view fusion bound (view_fusion.hip): per (person, output joint) the softmax of the
// rows' log marginals over a cube of world points around centres (NULL: centres_out, as the triangulation launch wrote it).
int launch_view_fusion(const float* xy, const MetroPlacement* rec, const int* rows, int n_rows, const int* starts, int n_persons,
                       const int* mirror, const float* centres, const MetroViewFusion& params, int n, const MetroSpec& spec,
                       float* points, float* cov, float* stats, int* info, float* centres_out, hipStream_t stream);
// The mode of every joint chosen by bone lengths, of a forward with a skeleton bound (skeleton_modes.hip): per crop row exact
// inference on the forest `edges` rooted by skeleton_schedule (every component at its lowest-numbered joint; returns the first
// bad edge and says why, or -1).
int skeleton_schedule(const int32_t* edges, int n_edges, int n_joints, signed char* parent, signed char* parent_edge, const char** why);
int launch_skeleton_modes(const int32_t* voxel, const float* stats, int k, const double* lengths, const int32_t* edges, int n_edges,
                          const signed char* parent, const signed char* parent_edge, const MetroSkeletonModes& params,
                          const float* coords01, int n, int max_n, const MetroSpec& spec, float* prob, int32_t* choice, float* info,
                          float* coords01_sel, hipStream_t stream);
// the volumetric head in one launch (head_f16.hip): postnorm prologue + logits GEMM + per-joint softmax statistics
bool head_f16_supported(int c_in, int c_head, int n_joints, int depth, int side);
int head_f16_slabs(int side);               // records per image the partials slot must hold
int head_f16_records(int n, int c_in, int c_head, int side);      // records per image a launch at batch n writes
int launch_head_f16(const void* x, const void* w, const float* bias, const void* pro_scale, const void* pro_shift,
                    int n, int c_in, int c_head, int n_joints, int depth, int side, float* partials, float* logits_out,
                    hipStream_t stream, float* moments = nullptr);
// `moments` (optional, fp32 [n][records][J][6]): the MOMENTS instantiation of the same kernel also writes every record's second
// central moments (launch_softargmax_finalize folds them into cov01)
// alternative decode heads (heads.hip): root_z != NULL selects true-root-depth, else the bone-length solve
int launch_backproject(const float* coords01, const float* inv_k, const double* targets, int per_pose_targets,
                       const float* root_z, const int* edges, int n, int nj, int ne, const MetroSpec& spec,
                       int root_relative, int permute, float* out, float* z_out, hipStream_t stream);
int launch_heatmap_to_25d(const float* coords01, float* out, int n, const MetroSpec& spec, hipStream_t stream);
int launch_to_orig_cam(const float* x, const float* rot, const int* mirror, float* out, int n, int nj, hipStream_t stream);
// absolute poses + frame keypoints of frame crops (place_poses.hip)
int launch_place_poses(const float* coords01, const float* poses, const MetroPlacement* rec, int n, const MetroSpec& spec,
                       int scale, const double* targets, int per_pose_targets, const float* root_z, const int* edges, int ne,
                       const int* mirror, int coords, float* out, float* keypoints, float* z_out, hipStream_t stream);
SoftArgmaxArgs make_softargmax_args(const MetroSpec& spec, int n);
// test-time augmentation views of frame crops (views.hip)
int launch_expand_views(const MetroViewBase* bases, int n, const MetroView* views, int n_views, int side, MetroCropWarp* crops,
                        MetroPlacement* places, hipStream_t stream);
int launch_merge_views(const float* poses, const float* keypoints, const float* z, const MetroPlacement* rec, const int* mirror,
                       int n, int n_views, int nj, float* poses_out, float* keypoints_out, float* z_out, float* spread_out,
                       hipStream_t stream);
// per-joint covariances of frame crops in the requested coordinates (covariances.hip)
int launch_place_covariances(const float* cov01, const float* peak, const MetroPlacement* rec, int n, int n_views,
                             const MetroSpec& spec, const int* mirror, int coords, float* cov_out, float* peak_out,
                             hipStream_t stream);
// world joints of persons seen by several cameras, from the rays of their crop rows (triangulate.hip)
int launch_triangulate_joints(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const int* rows,
                              int n_rows, const int* starts, int n_persons, const MetroSpec& spec, const int* mirror, int weights,
                              double min_det, float* points, int* n_rays, float* residual, float* cov, hipStream_t stream);
// cross-view association: pairwise ray distance of boxes and their complete-linkage clustering (match_views.hip)
int launch_view_affinity(const float* coords01, const float* cov01, const MetroPlacement* rec, const MetroSpec& spec,
                         const int* mirror, const int* frame_index, const int* step_index, int n, int n_views, int weights,
                         double min_sin2, double clip_mm, int min_pairs, float* cost, int* n_pairs, hipStream_t stream);
int launch_cluster_views(const float* cost, int n, int n_views, float max_cost, int* person_index, int* n_persons, int* rows,
                         int* starts, hipStream_t stream);
// the time step of every person metro_cluster_views found and the time-step CSR of the persons (world_tracks.hip)
int launch_person_steps(const int* rows, int n_rows, const int* starts, const int* n_persons, int n, int n_views, const int* box_step,
                        int n_boxes, const double* step_times, int n_steps, int* person_step, double* person_times, int* step_rows,
                        int* step_starts, hipStream_t stream);
// the same from the persons' labels, with a step for the persons one camera sees and their box (world_tracks.hip)
int launch_person_steps_labels(const int* person_index, const int* n_persons, int n, const int* box_step, int n_boxes,
                               const double* step_times, int n_steps, int* person_step, double* person_times, int* step_rows,
                               int* step_starts, int* single_box, hipStream_t stream);
// the ray of every joint of a person seen by one camera (person_rays.hip)
int launch_person_rays(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const MetroSpec& spec,
                       const int* mirror, int weights, const int* single_box, int n, int n_views, double* rays, hipStream_t stream);
// tracked poses smoothed over time: Kalman filter + RTS pass per (track, joint) (smooth_tracks.hip)
size_t smooth_tracks_workspace_bytes(int n_rows, int n_out);
int launch_smooth_tracks(const float* poses, const float* cov, const double* times, int n, const int* rows, int n_rows,
                         const int* starts, int n_tracks, int n_out, int mode, int measurement, double q, double r_floor,
                         double cov_scale, double v0, double gate, double* state, void* workspace, float* poses_out,
                         float* velocity_out, float* cov_out, unsigned char* used_out, hipStream_t stream);
// which box of a video continues which track: one workgroup over the steps of the call (associate_tracks.hip).  The arguments
// travel as ONE record from the public entry to the kernel: the entry builds it (make_assoc_args), checks it and hands it on
struct AssocArgs {
    const float* poses;      // [n][J][3] mm, absolute
    const float* cov;        // [n][J][9] mm^2 (METRO_SMOOTH_COVARIANCE)
    const double* times;     // [n] s
    const int* step_rows;    // [n_step_rows] indices into the n pose rows
    const int* step_starts;  // [n_steps + 1]
    double* state;           // [T][J][28]: only the retirement writes it
    int* ids;                // [T]
    int* next_id;            // [1]
    double* ws;              // [T][J][28] working copy of the state
    int* track_index;        // [n]
    int* track_id;           // [n]
    float* cost_out;         // [n]
    int* rows_out;           // [n]
    int* starts_out;         // [T + 1]
    int* n_new;              // [1]
    int* n_dropped;          // [1]
    int n, n_step_rows, n_steps, n_tracks, n_out, measurement, min_joints;
    double q, r2, cov_scale, v02, gate, clip, max_age;
    float max_cost;
};

// the same walk with ray rows that are costed against the slots and placed as point measurements: what it reads and writes more
struct AssocRayArgs : AssocArgs {
    float* poses_w;          // poses and
    float* cov_w;            // cov, writable: the place step fills the ray rows
    const int* single_box;   // [n] >= 0: the row is a ray row
    const double* rays;      // [n][J][8]
    double depth_var;        // depth_sigma_mm^2
    float* ray_depth;        // [n][J]
    int* n_unplaced;         // [1]
};

// the records from the arguments of the public entries, in their order; r2, v02 and depth_var are formed here, once, in fp64
inline AssocArgs make_assoc_args(const float* poses, const float* cov, const double* times, int n, const int* step_rows, int n_step_rows,
                                 const int* step_starts, int n_steps, int n_out, int measurement, double q, double r_floor,
                                 double cov_scale, double v0, double gate, float max_cost_mm, double clip_mm, int min_joints,
                                 double max_age_s, double* state, int n_tracks, int* ids, int* next_id, void* workspace, int* track_index,
                                 int* track_id, float* cost_out, int* rows_out, int* starts_out, int* n_new, int* n_dropped) {
    AssocArgs a;
    a.poses = poses; a.cov = cov; a.times = times; a.step_rows = step_rows; a.step_starts = step_starts;
    a.state = state; a.ids = ids; a.next_id = next_id; a.ws = static_cast<double*>(workspace);
    a.track_index = track_index; a.track_id = track_id; a.cost_out = cost_out; a.rows_out = rows_out; a.starts_out = starts_out;
    a.n_new = n_new; a.n_dropped = n_dropped;
    a.n = n; a.n_step_rows = n_step_rows; a.n_steps = n_steps; a.n_tracks = n_tracks; a.n_out = n_out;
    a.measurement = measurement; a.min_joints = min_joints;
    a.q = q; a.r2 = r_floor * r_floor; a.cov_scale = cov_scale; a.v02 = v0 * v0; a.gate = gate;
    a.clip = clip_mm; a.max_age = max_age_s; a.max_cost = max_cost_mm;
    return a;
}

inline AssocRayArgs make_assoc_ray_args(const AssocArgs& base, float* poses, float* cov, const int* single_box, const double* rays,
                                        double depth_sigma_mm, float* ray_depth, int* n_unplaced) {
    AssocRayArgs a;
    static_cast<AssocArgs&>(a) = base;
    a.poses_w = poses; a.cov_w = cov; a.single_box = single_box; a.rays = rays;
    a.depth_var = depth_sigma_mm * depth_sigma_mm; a.ray_depth = ray_depth; a.n_unplaced = n_unplaced;
    return a;
}

size_t associate_tracks_workspace_bytes(int n_tracks, int n_out);
// the greedy assignment or the optimal one; kernel notes associate_tracks[_rays][_optimal]
int launch_associate_tracks(const AssocArgs& a, bool optimal, hipStream_t stream);
int launch_associate_tracks_rays(const AssocRayArgs& a, bool optimal, hipStream_t stream);
// the bone lengths of followed persons, accumulated per (track slot, skeleton edge) and read out (bone_lengths.hip)
int launch_track_bone_lengths(const float* poses, const float* cov, int n, const int* rows, int n_rows, const int* starts, int n_tracks,
                              const int* ids, int n_joints, const int* edges, const int* edge_mirror, int n_edges,
                              const double* fallback, int min_count, double gate, double r_floor, double cov_scale, double min_length,
                              int debias, int symmetric, double* stats, int* bone_ids, double* lengths_out, double* sigma_out,
                              unsigned char* known_out, hipStream_t stream);
// per-box crop geometry of full frames (look_at_boxes.hip)
int launch_look_at_boxes(const double* boxes, const int32_t* frame_index, int n, int n_frames, const MetroFrameCamera* cameras,
                         int n_cameras, int side, MetroViewBase* out, int32_t* status, hipStream_t stream);

}  // namespace metro
