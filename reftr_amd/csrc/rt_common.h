// Shared device helpers for the RefTR gfx950 kernels (CDNA4, wave64).
// All kernels in this directory are written for MI355X only: 64-lane waves,
// MFMA 16x16x32 bf16 fragments, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/reftr_hip.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define RT_WAVE 64

// Tuning switches of the A/B sessions recorded in LAB_NOTES.md.  The product library fixes every one at its measured-best value
// (the second argument); the lab library (REFTR_LAB=1 at build and at import: -DRT_LAB, libreftr_hip_lab.so) reads them from the
// environment, once, at the first launch that consults them.
#ifdef RT_LAB
#include <stdlib.h>
#define RT_TUNE(name, dflt) (getenv(name) ? atoi(getenv(name)) : (dflt))
#define RT_TUNE_SET(name) (getenv(name) != nullptr)
#else
#define RT_TUNE(name, dflt) (dflt)
#define RT_TUNE_SET(name) false
#endif

__device__ __forceinline__ float rt_bf2f(bf16_t v) { return (float)v; }
__device__ __forceinline__ bf16_t rt_f2bf(float v) { return (bf16_t)v; }

// Counter-based dropout hash: keep element `idx` of site `seed` iff hash >= thresh
// (thresh = p * 2^32).  Forward and backward regenerate the same mask from
// (seed, idx); the oracle restates the same integer arithmetic in numpy.
__device__ __forceinline__ uint32_t rt_hash32(uint32_t seed, uint32_t idx) {
    uint32_t x = idx * 0x9E3779B1u ^ seed;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
// effective seed of a dropout site when the step seed lives in device memory (captured graphs)
__device__ __forceinline__ uint32_t rt_site_seed(const uint32_t* seed_dev, uint32_t site) {
    return seed_dev ? rt_hash32(*seed_dev, site) : site;
}
__device__ __forceinline__ uint32_t rt_drop_thresh(float p) {
    return (uint32_t)((double)p * 4294967296.0);
}
// dropout of one site: element `idx` is kept (and scaled by ks) iff keep(idx)
struct rt_drop {
    bool on;
    uint32_t thresh;
    float ks;
    uint32_t seed;
    __device__ __forceinline__ rt_drop(float drop_p, const uint32_t* seed_dev, uint32_t drop_seed)
        : on(drop_p > 0.f), thresh(rt_drop_thresh(drop_p)), ks(on ? 1.f / (1.f - drop_p) : 1.f), seed(rt_site_seed(seed_dev, drop_seed)) {}
    // `seed`: the site's effective seed, already resolved by the caller
    __device__ __forceinline__ rt_drop(float drop_p, uint32_t seed)
        : on(drop_p > 0.f), thresh(rt_drop_thresh(drop_p)), ks(on ? 1.f / (1.f - drop_p) : 1.f), seed(seed) {}
    // a site whose kernel does not touch *seed_dev while dropout is off
    static __device__ __forceinline__ rt_drop site(float drop_p, const uint32_t* seed_dev, uint32_t drop_seed) {
        return rt_drop(drop_p, drop_p > 0.f ? rt_site_seed(seed_dev, drop_seed) : 0u);
    }
    __device__ __forceinline__ bool keep(uint32_t idx) const { return rt_hash32(seed, idx) >= thresh; }
    // v behind the mask (unchanged while dropout is off); the four elements' indices are (idx0 + e) >> shift
    __device__ __forceinline__ float apply(float v, uint32_t idx) const { return !on ? v : keep(idx) ? v * ks : 0.f; }
    __device__ __forceinline__ f32x4 apply(f32x4 v, uint32_t idx0, int shift = 0) const {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = apply(v[e], (idx0 + e) >> shift);
        return v;
    }
};

__device__ __forceinline__ float rt_gelu(float x) {
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}
__device__ __forceinline__ float rt_gelu_grad(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

__device__ __forceinline__ float rt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float rt_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-wide sum for blockDim.x <= 1024 (multiple of 64); `sm` holds >= 16 floats.
__device__ __forceinline__ float rt_block_sum(float v, float* sm) {
    v = rt_wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) sm[wid] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += sm[i];
    return r;
}

// Ordered selection of one image's valid phrases, one pass of 64 phrase slots per call (rt_box_postprocess, rt_eval_metrics).
// `valid_b` is the image's [P, K] slice of phrase_mask; the reference masked_selects the (p, k) entries of [P, K, 4] whose mask is
// set and keeps prediction 0 of each selected phrase (post_process.py:62-70).  The K entries of a phrase are equal by construction
// (reftr_transformer.py:237-238), so a phrase is selected iff its entry 0 is set; rank = number of selected phrases in front of it.
// Called by ALL 64 lanes of one wave with ph = j0 + lane: ranks inside a pass come from a ballot + population count of the lower
// lanes (ordered, exact), `base` carries the count of the passes before and is advanced by this pass's.  Returns whether this
// lane's phrase is selected; `rank` is meaningful only then.
__device__ __forceinline__ bool rt_phrase_rank(const uint8_t* __restrict__ valid_b, int P, int K, int ph, int lane, int& base, int& rank) {
    const bool mine = ph < P && valid_b[(size_t)ph * K] != 0;
    const unsigned long long bal = __ballot(mine);
    rank = base + __popcll(bal & ((1ull << lane) - 1ull));
    base += __popcll(bal);
    return mine;
}

// Row map of the grouped / broadcast row layouts (norm and fused-add descriptors):
// grp_rows > 0: (r / g) * stride + off + r % g;  grp_rows < 0: broadcast (r / -g) * stride + off;  0: identity
__device__ __forceinline__ int rt_map_row(int r, int grp_rows, int grp_stride, int grp_off) {
    if (grp_rows > 0) return (r / grp_rows) * grp_stride + grp_off + (r % grp_rows);
    if (grp_rows < 0) return (r / (-grp_rows)) * grp_stride + grp_off;
    return r;
}

// "Last job whose first tile <= b" of a launch that serves several jobs: first[j] = the first workgroup of job j (ascending, n >= 1)
__device__ __forceinline__ int rt_job_of(const int* first, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= b) lo = mid; else hi = mid - 1; }
    return lo;
}
// ... of the int64 [njobs][8] job tables in device memory (rt_weight_prep_batched, rt_adamw_mat): word 7 of a row is its first tile
__device__ __forceinline__ int rt_job_of(const int64_t* table, int n, int64_t b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (table[mid * 8 + 7] <= b) lo = mid; else hi = mid - 1; }
    return lo;
}

// One workgroup of 256 threads over chunk blockIdx.x of a device table of {int64 element offset, int64 count}: vec4(e) for every four
// elements e .. e + 3 inside the chunk whose e is a multiple of 4 (16-byte accesses are allowed), one(e) for each of the others -- a
// ragged end, or the whole chunk when its offset is not a multiple of 4.  ALIGNED: the table promises multiples of 4 (one() is dead).
template <bool ALIGNED, class V, class S>
__device__ __forceinline__ void rt_chunk_walk(const int64_t* __restrict__ table, V vec4, S one) {
    const size_t off = (size_t)table[2 * blockIdx.x], cnt = (size_t)table[2 * blockIdx.x + 1];
    for (size_t i = threadIdx.x * 4; i < cnt; i += 1024) {
        if (ALIGNED || (i + 4 <= cnt && ((off + i) & 3) == 0)) vec4(off + i);
        else for (size_t k = i; k < cnt && k < i + 4; ++k) one(off + k);
    }
}

// Small fp32 workspaces are cleared with a KERNEL, not hipMemsetAsync: inside a captured hipGraph (ROCm 7.2) memset
// nodes were observed to race with the kernel nodes that follow them (intermittent garbage statistics / losses),
// while kernel -> kernel ordering on the captured stream is reliable.
static __global__ void rt_zero_f32_kernel(float* p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.f;
}
static inline hipError_t rt_zero_f32(float* p, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(rt_zero_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, (int)n);
    return hipGetLastError();
}

// XCD-aware workgroup -> work-item map.  Workgroups are handed to the 8 XCDs round-robin by linear id, and each XCD has
// its own L2: with the identity map, neighbouring tiles (which share operand rows) land on 8 different L2s and every
// shared row is fetched over the fabric up to 8 times.  This map gives XCD x the contiguous range of items
// [x*n/8, (x+1)*n/8), so tiles that share rows share an L2.  `xcd_on` = 0 keeps the identity map (A/B switch).
__device__ __forceinline__ int rt_xcd_remap(int b, int n, int xcd_on) {
    if (!xcd_on || n < 16) return b;
    const int xcd = b & 7, idx = b >> 3, per = n >> 3, rem = n & 7;
    return xcd * per + (xcd < rem ? xcd : rem) + idx;
}

// Gradient-norm accumulator (round 4): the squared L2 norm of the weight gradients is collected WHERE THEY ARE PRODUCED -- every
// epilogue that assigns or accumulates a piece of a weight gradient adds (new^2 - old^2) of that piece -- instead of by a second
// pass over the 607 MB gradient buffer (engine_vg.py:62-63's clip_grad_norm_).  Contributions go to one of RT_SQ_SLOTS fp32 words
// (a cache line apart, picked by workgroup / wave id) with fire-and-forget atomics; rt_sqnorm_finish adds the slots up.
__device__ __forceinline__ void rt_sq_add(float* slots, unsigned who, float v) {
    atomicAdd(slots + (size_t)(who & (RT_SQ_SLOTS - 1)) * RT_SQ_STRIDE, v);
}
__device__ __forceinline__ float rt_hsum(float v) { return v; }
__device__ __forceinline__ float rt_hsum(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ void rt_store_bf16(bf16_t* p, float v) { *p = (bf16_t)v; }
__device__ __forceinline__ void rt_store_bf16(bf16_t* p, f32x4 v) {
    *reinterpret_cast<bf16x4*>(p) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
}
// The commit step of a finished weight-gradient piece (T = float or f32x4).  `a` is the reduced value, ALREADY multiplied by
// scale[n]; `old` what *o holds (read only when `accumulate`: a kernel that keeps several pieces' loads in flight reads it itself).
// Overwrites or accumulates *o, writes the bf16 exchange twin of the FINAL value (`twin` may be null) and returns the piece's
// |after|^2 - |before|^2 for the accumulator slots: (old + a)^2 - old^2 = a (2 old + a).
template <class T>
__device__ __forceinline__ float rt_wg_commit(T a, T old, T* o, bf16_t* twin, bool accumulate) {
    T d = a * a;
    if (accumulate) { d = a * (old + old + a); a = old + a; }
    *o = a;
    if (twin) rt_store_bf16(twin, a);
    return rt_hsum(d);
}
template <class T>
__device__ __forceinline__ float rt_wg_commit(T a, T* o, bf16_t* twin, bool accumulate) {
    return rt_wg_commit(a, accumulate ? *o : a, o, twin, accumulate);
}
// sign * |buf|^2 of n <= 32 fp32 buffers into the slots, one launch (the producers without an in-kernel contribution: a pass with
// sign -1 in front of an accumulating launch, +1 behind every launch); more than 32: RT_ERR_BADARG, the caller batches; rt_optim.hip
int rt_sq_pass(float* const* bufs, const long long* counts, const float* signs, int n, float* slots, hipStream_t s);
// twin[i] = bf16(buf[i]) for n <= 32 fp32 buffers, one launch (the bf16 exchange twins of weight gradients whose producer has no
// in-kernel twin store); more than 32: RT_ERR_BADARG; rt_optim.hip
int rt_round_pass(float* const* bufs, void* const* twins, const long long* counts, int n, hipStream_t s);

#define RT_CHECK_LAUNCH() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)
