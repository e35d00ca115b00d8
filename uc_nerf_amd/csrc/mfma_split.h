// Device primitives of the MLP kernels (mlp.hip, mlp_bf16.hip, mlp_bwd.hip, mlp_bwd_chain.hip, mlp_wgrad.hip): vector types, MFMA
// wrappers, the split of fp32 values into (hi, lo) bf16 terms, empty-asm launderers and the inline-asm statements of the LDS weight rings.
//
// Split-bf16 products: a*w = a_hi*w_hi + a_hi*w_lo + a_lo*w_hi (x_hi + x_lo = x to 16 significant bits; the dropped lo*lo term is 2^-16
// relative), three v_mfma_f32_32x32x16_bf16 per product with fp32 accumulation.
#pragma once
#include <hip/hip_runtime.h>

namespace ucnerf {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define SB0 __builtin_amdgcn_sched_barrier(0)

// D = A * B + C on 32x32 tiles: fp32 operands (one k per lane), or eight bf16 / fp16 operands per lane (k16)
__device__ __forceinline__ f32x16 mfma_32x32x2(float a, float b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// D = A * B + C on a 16x16 tile, fp32 operands, four k per instruction: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15];
// register r of the result is row 4 (l >> 4) + r, column l & 15
__device__ __forceinline__ f32x4 mfma_16x16x4(float a, float b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma_32x32x16(const bf16x8& a, const bf16x8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma_32x32x16(const f16x8& a, const f16x8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// eight values of one lane as (hi, lo) operand fragments
template <class V> struct HiLo { V hi, lo; };
// A fragments of one half-step of a weight ring: (hi, lo) of a pair of 32-row tiles
template <class V> struct PairFrags { V h0, l0, h1, l1; };

// (hi, lo) split of eight values: hi = truncated bf16 (v_perm of the top halves), lo = bf16_rne(x - hi).  The backward's operands;
// the forward's split8 (mlp_bf16.hip) rounds hi to nearest since round 5 -- the renders answer to an absolute 1e-4 bar; the gradients' bar is
// relative and they keep the truncated hi, which measured 0.2 % faster in the forward kernel.
__device__ __forceinline__ HiLo<bf16x8> split8_trunc(const float (&x)[8]) {
    u32x4 hi;
    HiLo<bf16x8> f;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const unsigned b0 = __builtin_bit_cast(unsigned, x[j]), b1 = __builtin_bit_cast(unsigned, x[j + 1]);
        hi[j >> 1] = __builtin_amdgcn_perm(b1, b0, 0x07060302u);
        const f32x2 l = (f32x2){x[j], x[j + 1]} - (f32x2){__builtin_bit_cast(float, b0 & 0xffff0000u), __builtin_bit_cast(float, b1 & 0xffff0000u)};
        f.lo[j] = (__bf16)l.x;
        f.lo[j + 1] = (__bf16)l.y;
    }
    f.hi = __builtin_bit_cast(bf16x8, hi);
    return f;
}

// ---- empty asm: a value the compiler may no longer look through
// Results that are only needed much later would be sunk towards their use -- out of the MFMA shadow they were written for, with their
// operands kept live meanwhile.  pin() on the result keeps the arithmetic where it is written.
template <class T> __device__ __forceinline__ void pin(T& v) { asm volatile("" : "+v"(v)); }
// A value that does not change across a loop (a lane offset, a table index) would be hoisted out of it, and what depends on it -- loads
// of constants, addresses -- with it, to be kept in registers or spilled: laundered, everything derived from it is re-computed at its use.
template <class T> __device__ __forceinline__ T opaque(T v) { pin(v); return v; }
// the same for a wave-uniform value (kept in a scalar register); `on` = 0: identity (inside a GEMM phase's fill the asm form does not
// select: "illegal VGPR to SGPR copy")
template <class T> __device__ __forceinline__ T sopaque(T v, bool on = true) { if (on) asm volatile("" : "+s"(v)); return v; }

// ---- the weight rings' inline asm
// One 16-byte piece per lane from global memory into LDS (global_load_lds_dwordx4): lds_dst = the wave's LDS byte address (M0),
// OFFSET moves both addresses.  Issued from inline asm on purpose: the compiler models a global_load_lds as a FLAT access that may touch
// both memories and from then on degrades every counted wait of the kernel to vmcnt(0) / lgkmcnt(0), which serialises the fragment reads
// of the ring.  The asm names m0 as a clobber on purpose (it loads the LDS base into it); the copies' completion is counted by the callers
// (wait_vmcnt, wait_vmcnt_lgkmcnt).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
template <int OFFSET = 0>
__device__ __forceinline__ void lds_dma16(const char* src, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off offset:%2" ::"v"(src), "s"(lds_dst), "n"(OFFSET) : "memory", "m0");
}
#pragma clang diagnostic pop

// counted waits: all but the N youngest vector-memory operations of this wave have completed (+ all of its LDS operations)
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N>
__device__ __forceinline__ void wait_vmcnt_lgkmcnt() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }
// block barrier behind this wave's LDS traffic only: its global loads in flight stay in flight
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace ucnerf
