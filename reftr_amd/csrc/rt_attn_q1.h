// Attention of ONE query against the S <= 768 keys of one (batch, head), head size 32, by a 256-thread workgroup: thread t owns the keys
// t, t + 256, t + 512 (a 64-byte K row and V row each), the softmax is a block reduction and the output / dq a 32-wide reduction over
// the block.  Shared by attn_q1_fwd_kernel / attn_q1_bwd_kernel (rt_attention.hip) and the cross-attention stages of the cooperative
// decoder (rt_decoder.hip), so that both evaluate the same expression tree: the decoder is accepted because it is bit-identical to
// the chain of launches it replaces.
// Where the query, dout and out rows come from (plain loads, tagged polls) and where o / dq go stay with the callers; the K / V
// prefetch is a call of its own, so that a caller may issue it before it waits for its query.
#pragma once
#include "rt_common.h"

constexpr int Q1_MAXK = 3;            // keys per thread: S <= 768

struct Q1Row { bf16x8 c[4]; };        // one 32-feature bf16 row, as loaded
__device__ __forceinline__ Q1Row q1_raw(const bf16_t* row) {
    Q1Row r;
#pragma unroll
    for (int c = 0; c < 4; ++c) r.c[c] = *reinterpret_cast<const bf16x8*>(row + c * 8);
    return r;
}
__device__ __forceinline__ void q1_load_row(const bf16_t* row, float* out32) {
    const Q1Row r = q1_raw(row);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) out32[c * 8 + e] = (float)r.c[c][e];
}
__device__ __forceinline__ float q1_dot(const Q1Row& r, const float* x) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) a += (float)r.c[c][e] * x[c * 8 + e];
    return a;
}

// the K and V rows of this thread's keys and whether each key counts (inside S and not padded); every load is issued up front
struct Q1KV { Q1Row k[Q1_MAXK], v[Q1_MAXK]; bool ok[Q1_MAXK]; };
__device__ __forceinline__ void q1_prefetch(const bf16_t* k, int ldk, const bf16_t* v, int ldv, const uint8_t* kpm, int S, int b, int h, Q1KV& kv) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < Q1_MAXK; ++i) {
        const int j = t + i * 256;
        const int jj = j < S ? j : 0;
        kv.ok[i] = j < S && !(kpm && kpm[(size_t)b * S + jj]);
        kv.k[i] = q1_raw(k + ((size_t)b * S + jj) * ldk + h * 32);
        kv.v[i] = q1_raw(v + ((size_t)b * S + jj) * ldv + h * 32);
    }
}

// block-wide sum of a 32-vector held per thread: leaves the four waves' sums in sm (behind a barrier); feature d = q1_sum4(sm, d)
__device__ __forceinline__ void q1_block_sum32(float* v, float (*sm)[32]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < 32; ++d) v[d] = rt_wave_sum(v[d]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 32; ++d) sm[wave][d] = v[d];
    }
    __syncthreads();
}
__device__ __forceinline__ float q1_sum4(const float (*sm)[32], int d) { return sm[0][d] + sm[1][d] + sm[2][d] + sm[3][d]; }

// forward of (b, h) = bh: softmax(scale q K^T) behind the dropout mask, times V.  Returns the row's log-sum-exp (every thread) and
// leaves the output in sm32 for q1_sum4; red holds 8 floats.
__device__ __forceinline__ float q1_fwd(const Q1KV& kv, const float* q, float scale, int S, int bh, const rt_drop& drop, float* red,
                                        float (*sm32)[32]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float sc[Q1_MAXK];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < Q1_MAXK; ++i) {
        sc[i] = kv.ok[i] ? q1_dot(kv.k[i], q) * scale : -INFINITY;
        m = fmaxf(m, sc[i]);
    }
    m = rt_wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float ms = (m == -INFINITY) ? 0.f : m;
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < Q1_MAXK; ++i) { sc[i] = __expf(sc[i] - ms); l += sc[i]; }
    l = rt_wave_sum(l);
    if (lane == 0) red[4 + wave] = l;
    __syncthreads();
    l = red[4] + red[5] + red[6] + red[7];
    const float inv_l = 1.f / l;                 // fully masked row: NaN below, as the reference
    float o[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = 0.f;
#pragma unroll
    for (int i = 0; i < Q1_MAXK; ++i) {
        const int j = t + i * 256;
        if (j >= S) continue;
        const float pr = drop.apply(sc[i] * inv_l, (uint32_t)((size_t)bh * S + j));
        if (pr != 0.f || pr != pr) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int e = 0; e < 8; ++e) o[c * 8 + e] += pr * (float)kv.v[i].c[c][e];
        }
    }
    q1_block_sum32(o, sm32);
    return ms + __logf(l);
}

// backward of (b, h) = bh: q, go (= dout), ov (= out) are the three 32-feature rows, lse the forward's.  The dk / dv rows of key j go
// out in four 8-feature pieces through store(j, c, dk8, dv8); dq is left in sm32 for q1_sum4.
template <class Store>
__device__ __forceinline__ void q1_bwd(const Q1KV& kv, const float* q, const float* go, const float* ov, float lse, float scale, int S, int bh,
                                       const rt_drop& drop, float (*sm32)[32], Store store) {
    const int t = threadIdx.x;
    float delta = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) delta += go[d] * ov[d];
    float dq[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) dq[d] = 0.f;
#pragma unroll
    for (int i = 0; i < Q1_MAXK; ++i) {
        const int j = t + i * 256;
        if (j >= S) continue;
        const float pr = kv.ok[i] ? __expf(q1_dot(kv.k[i], q) * scale - lse) : 0.f;
        float mk = 1.f;
        if (drop.on) mk = drop.keep((uint32_t)((size_t)bh * S + j)) ? drop.ks : 0.f;
        const float dp = q1_dot(kv.v[i], go);
        const float ds = pr * (mk * dp - delta) * scale;
        const float pd = pr * mk;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bf16x8 a8, b8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a8[e] = (bf16_t)(ds * q[c * 8 + e]); b8[e] = (bf16_t)(pd * go[c * 8 + e]);
                dq[c * 8 + e] += ds * (float)kv.k[i].c[c][e];
            }
            store(j, c, a8, b8);
        }
    }
    q1_block_sum32(dq, sm32);
}
