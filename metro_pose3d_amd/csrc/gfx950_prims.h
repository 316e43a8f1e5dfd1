// Device primitives of the gfx950 kernels: vector types, the LDS-DMA wave-instruction, counted waits + barriers, the LDS
// chunk swizzle, the fp16(acc + bias) epilogue.  Every kernel source includes this header; each file-local helper that a
// kernel keeps differs from these in shape.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the metro kernels are written for gfx950 (CDNA4) only: build with --offload-arch=gfx950"
#endif

namespace metro {

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void_t;

__device__ __forceinline__ unsigned lds_offset_of(const void* p) {
    return (unsigned)(size_t)(lds_void_t*)p;
}

// 16 zero bytes: the LDS-DMA source of padding, ragged tile edges and channel tails (a lane cannot be masked out of an
// LDS-DMA without leaving stale bytes in its slot).  Static: there is no relocatable device code, so every translation
// unit keeps its own, and a non-static __device__ variable defined in several of them would collide at the host link.
static __device__ __attribute__((aligned(16))) unsigned int g_zero_page[4];   // zero-initialised

// One LDS-DMA wave-instruction: 64 lanes x 16 bytes, lane l lands at lds_addr + 16*l.
// Inline asm on purpose: hipcc tracks the builtin form as an LDS write that may alias every
// later ds_read and drains it with s_waitcnt vmcnt(0), which serialises the ring.  The asm form
// is invisible to its bookkeeping; completion is ordered by the counted waits below.
// lds_addr must be wave-uniform (it goes through M0).
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_addr) {
    // M0 is written in the same statement that consumes it and is not preserved: nothing else in
    // these kernels uses M0 (gfx9+ LDS instructions do not need it).  No "memory" clobber: the
    // ordering is carried by the wait and barrier asm.
    asm volatile(
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, off"
        :
        : "v"(gsrc), "s"(lds_addr));
}
// The same with source = wave-uniform base (SGPR pair) + per-lane 32-bit byte offset, destination (lds_base + LDS_IMM) + 16*l.
template <int LDS_IMM>
__device__ __forceinline__ void dma16s(const void* sbase, unsigned voff, unsigned lds_base) {
    asm volatile(
        "s_add_u32 m0, %2, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_base), "n"(LDS_IMM)
        : "scc");
}

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm_and_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
// a raw s_barrier: __syncthreads() would also drain the stores (vmcnt(0))
__device__ __forceinline__ void wait_lgkm_and_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// s_waitcnt lgkmcnt(n), n a compile-time value after unrolling (0 .. 6), tied to the register the wait is for
__device__ __forceinline__ void wait_lgkm_dyn(half8_t& r, int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r)); break;
        case 1: asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(r)); break;
        case 2: asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(r)); break;
        case 3: asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(r)); break;
        case 4: asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(r)); break;
        case 5: asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(r)); break;
        default: asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(r)); break;
    }
}

// 16-byte chunk swizzle of an LDS operand row of BK fp16, so that ds_read_b128 of 32 consecutive rows x one chunk, at any
// alignment, hits 16 distinct 16-byte slots per 16-lane group: BK = 64 (128-byte rows, 2 per bank row): (row >> 1) & 7;
// BK = 32 (64-byte rows): (row >> 2) & 3.  An LDS-DMA image is lane-linear, so a DMA applies it to the per-lane source address.
template <int BK>
__device__ __forceinline__ int swz(int row) {
    static_assert(BK == 64 || BK == 32, "128- or 64-byte rows");
    return BK == 64 ? (row >> 1) & 7 : (row >> 2) & 3;
}

// fp16(acc + bias) for the four accumulators 4q .. 4q + 3: two v_pk_add_f32 on the accumulator's own (even-aligned) register
// pairs, two v_cvt_pk_f16_f32 -- 4 issue slots per 4 outputs.  Written out because hipcc's SLP pass turns the element-wise form
// into v_pk_add_f32 on shuffled register pairs + single v_cvt_f16_f32 + v_pack_b32_f16 / v_alignbit_b32 (conv_b1, an
// instruction-issue-bound launch: 313 instructions per producer tile instead of ~200).
// The converts give the bits of the (half_t) casts only under the MODE register the kernels run with: fp32 round to nearest
// even, fp16 denormals kept (not flushed).  A kernel that changes either must not use this.
__device__ __forceinline__ half4_t bias_cvt(const floatx16& acc, int q, const floatx4& bv) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    f32x2 lo = {acc[4 * q], acc[4 * q + 1]}, hi = {acc[4 * q + 2], acc[4 * q + 3]};
    const f32x2 blo = {bv[0], bv[1]}, bhi = {bv[2], bv[3]};
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(lo), "v"(blo));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(hi), "v"(bhi));
    u32x2 r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r.x) : "v"(lo.x), "v"(lo.y));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r.y) : "v"(hi.x), "v"(hi.y));
    return __builtin_bit_cast(half4_t, r);
}

// The ReLU of every kernel, scalar or packed: IEEE-754-2019 maximum(v, 0), NOT fmaxf / __builtin_elementwise_max (maxNum, which
// answers max(NaN, 0) = 0).  NaN stays NaN and +Inf stays +Inf, so a value that overflowed fp16 storage keeps travelling down the
// residual stream to the soft-argmax screen (pool_softargmax.hip, finalize) instead of becoming a plausible zero; -Inf -> 0 is
// right, the true value behind it is hugely negative.  One instruction where the maxNum form was one: v_maximum3_f32 v, v, 0, 0 /
// v_pk_maximum3_f16 (fp64, the parity kernels only: v_max_f64 + a NaN select).
template <typename T>
__device__ __forceinline__ T relu(T v) {
    return __builtin_elementwise_maximum(v, T{});
}

// A copy of a register value the optimiser knows nothing about (no instruction).  The MOMENTS instantiations of the head and
// soft-argmax kernels take their inputs through it: code added behind the default path then shares no expression with it -- a
// product that gains a second use is no longer contracted into an fma with its sum, which moved the default results by an ulp.
template <typename T>
__device__ __forceinline__ T opaque_copy(T v) {
    asm volatile("" : "+v"(v));
    return v;
}

// f(integral_constant<0>) ... f(integral_constant<N - 1>), in that order
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

}  // namespace metro
