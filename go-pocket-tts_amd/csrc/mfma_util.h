// mfma_util.h -- what every matrix-core kernel of the library shares: the vector types of the MFMA builtins, the fragment union, the
// f32 -> bf16 hi + lo operand split that gives the bf16 matrix cores f32-grade accuracy, and the LDS-DMA wave instruction.
//
// Device-only text; every function is forced inline, so a kernel that includes this header compiles to the code it had with a copy of its own.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace ptts {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // (a uint4 copied out of global memory is a struct memcpy the optimiser leaves in scratch)

// One MFMA operand (eight bf16 = 16 bytes) under the names the kernels fill and read it by: the builtin's vector, a 16-byte load or
// store, four packed pairs, the scratch-free vector of u32x4.
union Frag {
    bf16x8 v;
    uint4 q;
    unsigned u[4];
    u32x4 w;
};

// v -> bf16 hi + bf16 lo with v = hi + lo to ~2^-17 (round to nearest even; a NaN stays a NaN)
__device__ __forceinline__ void split1(float v, unsigned short& hi, unsigned short& lo) {
    const __bf16 h = (__bf16)v;
    const __bf16 l = (__bf16)(v - (float)h);
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, l);
}
// (a, b) -> packed bf16 hi pair and bf16 lo pair, each value split as above (v_cvt_pk_bf16_f32)
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& lo) {
    f32x2 f = {a, b};
    bf16x2 h = __builtin_convertvector(f, bf16x2);
    f32x2 r = f - __builtin_convertvector(h, f32x2);
    bf16x2 l = __builtin_convertvector(r, bf16x2);
    hi = *reinterpret_cast<unsigned*>(&h);
    lo = *reinterpret_cast<unsigned*>(&l);
}
// four f32 (weights) that were fetched as one 16-byte piece
__device__ __forceinline__ float4 as_float4(const uint4& u) {
    return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
}
// four consecutive k -> their 8 bytes of a hi plane and of a lo plane
__device__ __forceinline__ void split4(float4 x, uint2& hi, uint2& lo) {
    unsigned h01, l01, h23, l23;
    split2(x.x, x.y, h01, l01);
    split2(x.z, x.w, h23, l23);
    hi = make_uint2(h01, h23);
    lo = make_uint2(l01, l23);
}
// eight consecutive k -> the hi and the lo operand of a 32-deep MFMA step
__device__ __forceinline__ void split8(float4 x0, float4 x1, Frag& hi, Frag& lo) {
    split2(x0.x, x0.y, hi.q.x, lo.q.x);
    split2(x0.z, x0.w, hi.q.y, lo.q.y);
    split2(x1.x, x1.y, hi.q.z, lo.q.z);
    split2(x1.z, x1.w, hi.q.w, lo.q.w);
}

// One LDS-DMA wave-instruction: lane l's 16 bytes at src_lane -> dst + 16 l (dst: wave-uniform).
// Inline assembly on purpose: told about an LDS-DMA write (the builtin), hipcc puts `s_waitcnt vmcnt(0)` in front of the next ds_read of ANY slot --
// it cannot tell the slots apart -- which is the copy waited for at once instead of an iteration later.  So the copies are invisible to its
// counters and ordered by hand: every wave waits vmcnt(0) where a slot changes hands, in front of the block's barrier (k_ffn_fused, k_tall).
// (The compiler's own vmcnt(N) waits stay right: loads return in issue order, so a wait that lets the N youngest VISIBLE loads stay in flight
// has also seen every older copy land; and no visible load is issued between a copy and that wait.)  m0 carries the LDS address; nothing else
// in these kernels uses it -- and the compiler keeps nothing in it across statements: m0 is a RESERVED register to LLVM (listing it as a clobber is rejected as
// "reserved registers on the clobber list"), written right in front of each of the compiler's own uses (s_sendmsg, GWS, v_movrel), none of which these kernels have.
// The wait state between the write of m0 and its use is written out because the compiler's hazard recognizer does not look inside inline assembly
// (ISA: SALU write of M0 -> LDS "direct" / GDS / sendmsg use needs one).
__device__ __forceinline__ void lds_dma1k(const char* src_lane, char* dst) {
    const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)dst;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(base), "v"(src_lane) : "memory");
}

}  // namespace ptts
