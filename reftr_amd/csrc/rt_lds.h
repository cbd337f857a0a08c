// The gfx950 LDS primitives every staged kernel here is built from: global -> LDS DMA through a raw buffer descriptor, the
// counted wait that tracks it, and the LDS transpose read that turns natural [row][channel] tiles into MFMA fragments.
// One definition each: the m0 / s_nop hazard sequence of the DMA must not drift between kernels.  Internal to the library.
#pragma once
#include "rt_common.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;          // a buffer resource descriptor (V#), held in SGPRs

__device__ __forceinline__ i32x4 rt_make_rsrc(const void* ptr, unsigned bytes) {
    const uint64_t a = (uint64_t)ptr;
    return i32x4{(int)(uint32_t)a, (int)(uint32_t)(a >> 32), (int)bytes, 0x00020000};   // stride 0, raw buffer
}
// the same descriptor built from values the compiler cannot prove wave-uniform: forces it into SGPRs
__device__ __forceinline__ i32x4 rt_make_rsrc_uniform(const void* ptr, unsigned bytes) {
    const uint64_t a = (uint64_t)ptr;
    return i32x4{__builtin_amdgcn_readfirstlane((int)(uint32_t)a), __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)),
                 __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000};
}

// One global -> LDS DMA per lane, never through VGPRs: lane l of the wave instruction lands at LDS byte address
// lds_base + 16*l (rt_dma16) or lds_base + 4*l (rt_dma4), lds_base wave-uniform -- the landing is lane-linear and cannot
// scatter, so any bank swizzle is applied on the SOURCE side (voff).  Offsets past the descriptor's size write zeros.
// Issued as inline asm so that the compiler's waitcnt pass does not turn every later ds_read into vmcnt(0): completion is
// tracked with explicit counted waits (rt_wait_vmcnt), the compiler cannot tell which stage a ds_read aliases.
__device__ __forceinline__ void rt_dma16(const i32x4 rsrc, unsigned lds_base, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 ::"s"(lds_base), "v"(voff), "s"(rsrc), "s"(soff)
                 : "memory", "m0");
}
__device__ __forceinline__ void rt_dma16(const i32x4 rsrc, unsigned lds_base, int voff) {        // scalar offset 0: no SGPR spent on it
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                 ::"s"(lds_base), "v"(voff), "s"(rsrc)
                 : "memory", "m0");
}
__device__ __forceinline__ void rt_dma4(const i32x4 rsrc, unsigned lds_base, int voff) {         // 4 B per lane: the L2 prefetch touch
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds"
                 ::"s"(lds_base), "v"(voff), "s"(rsrc)
                 : "memory", "m0");
}
// wait until at most N vector-memory operations of this wave are outstanding
template <int N> __device__ __forceinline__ void rt_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// One bf16x8 MFMA fragment from two LDS transpose reads (ds_read_b64_tr_b16): each 16-lane group hands the instruction a
// 4(row) x 16(column) block and lane i gets column i's 4 row values; p0 / p1 are this lane's addresses in the two blocks
// (rows 4g..4g+3 and 16+4g..16+4g+3 of a 32-row slab, g = lane >> 4).
__device__ __forceinline__ bf16x8 rt_tr_frag(const unsigned char* p0, const unsigned char* p1) {
    typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)p0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)p1);
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo; u.s.b = hi;
    return u.v;
}
