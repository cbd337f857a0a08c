// Masked multi-head attention forward / backward on MFMA for the RefTR sequence lengths
// (VL encoder S = L + HW/32^2, dh = 32; BERT L <= 128, dh = 64; decoder cross-attention n_q*n_ph x S).
//
// One workgroup (8 waves) owns one (batch, head) and 128 rows of the "outer" axis, 16 per wave; the whole
// inner-axis operand pair of that head is staged once in LDS in its natural [row][dh] layout (row stride
// padded by 32 B, conflict-free for both access patterns below).  The score matrix never leaves registers:
//
//   forward / dQ : S^T tile [16 keys x 16 queries] = mfma(K rows, Q^T)  ("swapped" product): a lane then holds,
//     for ONE query (lane & 15), keys 4g..4g+3 of the tile (g = lane >> 4).  Two such tiles (32 keys) are exactly
//     the B-operand fragment of the next MFMA  O^T[d][q] += V^T[d][keys] P^T[keys][q]  — no cross-lane traffic for
//     P; V^T / K^T fragments come from the natural V / K rows through the gfx950 LDS transpose read
//     (rt_tr_frag, rt_lds.h), with the same key -> k-slot assignment on both operands.
//     Softmax: two streaming passes over the keys (pass 1: running max / sum, pass 2: normalised P and PV), so
//     any S fits without holding S scores in registers; row statistics are combined across the 4 lane groups
//     with two shuffles.
//   dK / dV      : the roles swap — a wave owns 16 keys, S tile [16 queries x 16 keys] = mfma(Q rows, K^T), and
//     dV^T[d][key] += dO^T[d][q] P[q][key],  dK^T[d][key] += Q^T[d][q] dS[q][key]  with dO^T / Q^T via transpose reads.
//
// Dropout acts on the probabilities with the shared counter hash (index ((b*H+h)*Sq + q)*Sk + key); a fully
// masked row gives NaN like the reference's softmax over -inf.
//
// Every inner loop of the two-pass forward and of the backward is ONE function over `rows` staged rows that start at row c0 of the
// inner axis: fwd_stats_chunk (pass 1), fwd_pv_chunk (pass 2), dq_chunk, dkv_chunk, with stage_kv_bias / stage_qdo_stats filling the
// LDS they read.  The three bodies (attn_fwd_body, attn_bwd_dq_body, attn_bwd_dkv_body) take LONG as a compile-time parameter: the
// whole-axis kernels stage the axis once and call each chunk function once (rows = the padded axis, c0 = 0), the long-axis kernels
// call it per staged chunk.  The arithmetic of the two forms is the same code, which is what makes their results the same bits.
// The register-kept forward (attn_fwd_reg_kernel) keeps its own fully unrolled loops, pass 2 included, and reads the descriptor
// fields directly: moving it onto pv-step, staging or store helpers, or handing its descriptor to a helper by reference, changes
// the instruction stream the compiler emits for it (measured 6 % slower at S = 440); as written it compiles to the code it had.
#include "rt_common.h"
#include "rt_attn_q1.h"
#include "rt_lds.h"
#include <stdlib.h>

namespace {

__device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (bf16_t)v[e];
    return o;
}

template <int DH> struct Geo {
    // LDS row stride (bytes): + 32 B, conflict-free for both access patterns (a 16-B pad for dh = 32 would fit two workgroups per CU at
    // S = 440; measured identical -- the kernels are bound by the CU's VALU work, profiles/r03_side_stream_probes.txt)
    static constexpr int RS = DH * 2 + 32;
    static constexpr int KH = DH / 32;         // MFMA k-steps over the head dim
    static constexpr int DT = DH / 16;         // 16-wide output tiles over the head dim
};

// rows [0, rows) of a [*, ld] bf16 matrix (head slice) -> LDS rows of stride RS; rows [rows, rows_pad) zeroed
template <int DH>
__device__ __forceinline__ void stage_rows(unsigned char* dst, const bf16_t* src, int rows, int rows_pad, int ld, int tid, int nthreads) {
    constexpr int RS = Geo<DH>::RS, CPR = DH / 8, U = 4;
    // U independent 16-B loads in flight per thread before the first LDS store: the copy is one or two memory round trips, not
    // one per 16 B (a load -> store loop serialises on the load latency: 4-8 us for a 28 KB head slice)
    const int total = rows_pad * CPR;
    for (int c0 = tid; c0 < total; c0 += nthreads * U) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * nthreads;
            const int r = c / CPR, cc = c % CPR;
            v[u] = make_uint4(0, 0, 0, 0);
            if (c < total && r < rows) v[u] = *reinterpret_cast<const uint4*>(src + (size_t)r * ld + cc * 8);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * nthreads;
            const int r = c / CPR, cc = c % CPR;
            if (c < total) *reinterpret_cast<uint4*>(dst + r * RS + cc * 16) = v[u];
        }
    }
}

// two matrices at once (K and V, or Q and dO): both sets of loads are in flight together
template <int DH>
__device__ __forceinline__ void stage_rows2(unsigned char* dst0, const bf16_t* src0, int ld0, unsigned char* dst1, const bf16_t* src1, int ld1,
                                            int rows, int rows_pad, int tid, int nthreads) {
    constexpr int RS = Geo<DH>::RS, CPR = DH / 8, U = 4;
    const int total = rows_pad * CPR;
    for (int c0 = tid; c0 < total; c0 += nthreads * U) {
        uint4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * nthreads;
            const int r = c / CPR, cc = c % CPR;
            a[u] = make_uint4(0, 0, 0, 0); b[u] = make_uint4(0, 0, 0, 0);
            if (c < total && r < rows) {
                a[u] = *reinterpret_cast<const uint4*>(src0 + (size_t)r * ld0 + cc * 8);
                b[u] = *reinterpret_cast<const uint4*>(src1 + (size_t)r * ld1 + cc * 8);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * nthreads;
            const int r = c / CPR, cc = c % CPR;
            if (c < total) {
                *reinterpret_cast<uint4*>(dst0 + r * RS + cc * 16) = a[u];
                *reinterpret_cast<uint4*>(dst1 + r * RS + cc * 16) = b[u];
            }
        }
    }
}

// fragment of a [rows][DH] global matrix used as MFMA B operand: lane (i, g) <- row (r0 + i), cols 32*kh + 8g..+7
template <int DH>
__device__ __forceinline__ void load_bfrag(const bf16_t* base, int row, int nrows, int ld, int lg, bf16x8 (&f)[Geo<DH>::KH]) {
#pragma unroll
    for (int kh = 0; kh < Geo<DH>::KH; ++kh) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < nrows) v = *reinterpret_cast<const uint4*>(base + (size_t)row * ld + kh * 32 + lg * 8);
        f[kh] = *reinterpret_cast<bf16x8*>(&v);
    }
}

// S tile = sum_kh mfma(A rows from LDS (row0 + li), B frag)
template <int DH>
__device__ __forceinline__ f32x4 tile_dot(const unsigned char* sA, int row0, int li, int lg, const bf16x8 (&bf)[Geo<DH>::KH]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < Geo<DH>::KH; ++kh) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(sA + (row0 + li) * Geo<DH>::RS + kh * 64 + lg * 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[kh], acc, 0, 0, 0);
    }
    return acc;
}

// ------------------------------------------------------------------------------------------------ shared pieces
// (batch, head) of the workgroup, the lane's place in its wave's 16 x 16 tiles (li, lg) and in the transpose reads (tr_r, tr_c)
struct Lanes { int bh, b, h, lane, wave, li, lg, tr_r, tr_c; };
__device__ __forceinline__ Lanes lanes(int H) {
    Lanes t;
    t.bh = blockIdx.x; t.b = t.bh / H; t.h = t.bh % H;
    t.lane = threadIdx.x & 63; t.wave = threadIdx.x >> 6;
    t.li = t.lane & 15; t.lg = t.lane >> 4;
    t.tr_r = 4 * t.lg + (t.li >> 2); t.tr_c = (t.li & 3) * 8;
    return t;
}
// row 0 of this head's slice of a [B][S][ld] operand
template <int DH>
__device__ __forceinline__ const bf16_t* head_rows(const void* base, const Lanes& t, int S, int ld) {
    return (const bf16_t*)base + (size_t)t.b * S * ld + t.h * DH;
}

// the dynamic LDS of every kernel here (smem_bytes): two [span][RS] operand slabs -- K, V or Q, dO -- and two rows of span floats
// (key bias, or lse and delta)
template <int DH> struct Lds {
    unsigned char *a, *b;
    float *f0, *f1;
    __device__ __forceinline__ explicit Lds(int span) {
        extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
        a = smem;
        b = a + (size_t)span * Geo<DH>::RS;
        f0 = reinterpret_cast<float*>(b + (size_t)span * Geo<DH>::RS);
        f1 = f0 + span;
    }
};

// sum / max over the 4 lane groups that share a query (or key) column
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
// the lane's running (m, l) of pass 1 -> the row's max M (Ms: 0 for a fully masked row), sum l and 1 / l
__device__ __forceinline__ void softmax_finish(float m, float& l, float& M, float& Ms, float& inv_l) {
    M = group_max(m);
    Ms = (M == -INFINITY) ? 0.f : M;
    l *= __expf(m - Ms);
    l = group_sum(l);
    inv_l = 1.f / l;                 // fully masked row: 0 * inf = NaN in pass 2, as the reference
}

// delta of one query row = sum_d dO[d] * O[d], from the row's DH values in memory
template <int DH>
__device__ __forceinline__ float row_delta(const bf16_t* orow, const bf16_t* drow) {
    float del = 0.f;
#pragma unroll
    for (int c = 0; c < DH; c += 8) {
        const bf16x8 ov = *reinterpret_cast<const bf16x8*>(orow + c), dv8 = *reinterpret_cast<const bf16x8*>(drow + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) del += (float)dv8[e] * (float)ov[e];
    }
    return del;
}

// the lane's 4 x DT accumulator values -> its row of a bf16 output (columns 16 t + 4 lg ..+3)
template <int DH>
__device__ __forceinline__ void store_rows(bf16_t* row, int lg, const f32x4 (&acc)[Geo<DH>::DT]) {
#pragma unroll
    for (int t = 0; t < Geo<DH>::DT; ++t) {
        bf16x4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = (bf16_t)acc[t][r];
        *reinterpret_cast<bf16x4*>(row + t * 16 + lg * 4) = ov;
    }
}
template <int DH>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[Geo<DH>::DT]) {
#pragma unroll
    for (int t = 0; t < Geo<DH>::DT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Rows c0 .. c0 + rows of the head's K (WITH_V: and V) -> LDS rows 0 .. rows (past Sk: zeros), and their additive key bias
// (0, or -inf for padded / masked keys)
struct KvSrc { const void *k, *v; const uint8_t* kpm; int Sk, ldk, ldv; };
template <int DH, int NW, bool WITH_V>
__device__ __forceinline__ void stage_kv_bias(const Lds<DH>& s, const KvSrc& p, const Lanes& t, int c0, int rows) {
    const int valid = (p.Sk - c0 < rows) ? p.Sk - c0 : rows;
    const bf16_t* k = head_rows<DH>(p.k, t, p.Sk, p.ldk) + (size_t)c0 * p.ldk;
    if (WITH_V) stage_rows2<DH>(s.a, k, p.ldk, s.b, head_rows<DH>(p.v, t, p.Sk, p.ldv) + (size_t)c0 * p.ldv, p.ldv, valid, rows, threadIdx.x, 64 * NW);
    else stage_rows<DH>(s.a, k, valid, rows, p.ldk, threadIdx.x, 64 * NW);
    for (int j = threadIdx.x; j < rows; j += 64 * NW)
        s.f0[j] = (c0 + j < p.Sk && !(p.kpm && p.kpm[(size_t)t.b * p.Sk + c0 + j])) ? 0.f : -INFINITY;
}

// Rows c0 .. c0 + rows of the head's Q and dO -> LDS, with their lse (f0) and delta (f1).
// OWN_DELTA: delta[i] = sum_d dO[i, d] * O[i, d] is recomputed here for the head's query rows (64-128 B of O and dO per row)
// instead of being read from the dQ kernel's output: the two halves of the backward then do not depend on each other and run
// as ONE launch (attn_bwd_fused_kernel) -- on the encoder's chain that is a 17 us kernel and a graph-node boundary less per layer.
template <int DH, int NW, bool OWN_DELTA>
__device__ __forceinline__ void stage_qdo_stats(const Lds<DH>& s, const rt_attn_bwd_desc& p, const Lanes& t, int c0, int rows) {
    const int valid = (p.Sq - c0 < rows) ? p.Sq - c0 : rows;
    const bf16_t* dbase = head_rows<DH>(p.dout, t, p.Sq, p.ldo);
    stage_rows2<DH>(s.a, head_rows<DH>(p.q, t, p.Sq, p.ldq) + (size_t)c0 * p.ldq, p.ldq, s.b, dbase + (size_t)c0 * p.ldo, p.ldo,
                    valid, rows, threadIdx.x, 64 * NW);
    for (int i = threadIdx.x; i < rows; i += 64 * NW) {
        const int qi = c0 + i;
        s.f0[i] = (qi < p.Sq) ? p.lse[(size_t)t.bh * p.Sq + qi] : INFINITY;       // padded query rows: p = exp(-inf) = 0
        float del = 0.f;
        if (qi < p.Sq) {
            if (OWN_DELTA) {
                const size_t row = ((size_t)t.b * p.Sq + qi) * p.ldo + t.h * DH;
                del = row_delta<DH>((const bf16_t*)p.out + row, (const bf16_t*)p.dout + row);
            }
            else del = p.delta[(size_t)t.bh * p.Sq + qi];
        }
        s.f1[i] = del;
    }
}

// ------------------------------------------------------------------------------------------------ forward
// pass 1 over `rows` staged keys: running max / sum over this lane's keys (4 per 16-key tile)
template <int DH>
__device__ __forceinline__ void fwd_stats_chunk(const Lds<DH>& s, int rows, const Lanes& t, const bf16x8 (&qf)[Geo<DH>::KH], float scale,
                                                float& m, float& l) {
    for (int blk = 0; blk < (rows >> 4); ++blk) {
        const f32x4 acc = tile_dot<DH>(s.a, blk * 16, t.li, t.lg, qf);
        const f32x4 bias = *reinterpret_cast<const f32x4*>(s.f0 + blk * 16 + t.lg * 4);
        float sc[4], mx = m;
#pragma unroll
        for (int r = 0; r < 4; ++r) { sc[r] = acc[r] * scale + bias[r]; mx = fmaxf(mx, sc[r]); }
        const float ms = (mx == -INFINITY) ? 0.f : mx;
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) add += __expf(sc[r] - ms);
        l = l * __expf(m - ms) + add;
        m = mx;
    }
}

// pass 2 over `rows` staged keys: normalised probabilities -> P^T fragments -> O^T += V^T P^T
template <int DH>
__device__ __forceinline__ void fwd_pv_chunk(const Lds<DH>& s, int rows, int c0, const Lanes& t, const bf16x8 (&qf)[Geo<DH>::KH], float scale,
                                             float Ms, float inv_l, const rt_drop& drop, uint32_t drop_row, f32x4 (&o)[Geo<DH>::DT]) {
    constexpr int RS = Geo<DH>::RS;
    for (int c = 0; c < (rows >> 5); ++c) {
        float pv[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int k0 = c * 32 + half * 16;
            const f32x4 acc = tile_dot<DH>(s.a, k0, t.li, t.lg, qf);
            const f32x4 bias = *reinterpret_cast<const f32x4*>(s.f0 + k0 + t.lg * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float pr = __expf(acc[r] * scale + bias[r] - Ms) * inv_l;
                if (drop.on) pr = drop.keep(drop_row + (uint32_t)(c0 + k0 + t.lg * 4 + r)) ? pr * drop.ks : 0.f;
                pv[half * 4 + r] = pr;
            }
        }
        const bf16x8 pf = pack8(pv);
        const unsigned char* v0 = s.b + (c * 32 + t.tr_r) * RS + t.tr_c;
#pragma unroll
        for (int d = 0; d < Geo<DH>::DT; ++d) {
            const bf16x8 vf = rt_tr_frag(v0 + d * 32, v0 + 16 * RS + d * 32);
            o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[d], 0, 0, 0);
        }
    }
}

template <int DH>
__device__ __forceinline__ void fwd_store(void* out, float* lse, int Sq, int ldo, const Lanes& t, int q, const f32x4 (&o)[Geo<DH>::DT], float M, float l) {
    if (q < Sq) {
        store_rows<DH>((bf16_t*)out + ((size_t)t.b * Sq + q) * ldo + t.h * DH, t.lg, o);
        if (t.lg == 0 && lse) lse[(size_t)t.bh * Sq + q] = M + __logf(l);
    }
}

// The two-pass forward.  LONG: rows past Sq carry zero fragments and are never stored (no early return: every wave meets the
// chunk barriers); pass 1 stages K only.
template <int DH, int NW, bool LONG>
__device__ __forceinline__ void attn_fwd_body(const rt_attn_desc& p, const int ch) {
    const Lanes t = lanes(p.H);
    const int Skp = (p.Sk + 31) & ~31;
    const Lds<DH> s(LONG ? ch : Skp);
    const KvSrc kv{p.k, p.v, p.kpm, p.Sk, p.ldk, p.ldv};
    if constexpr (!LONG) {
        stage_kv_bias<DH, NW, true>(s, kv, t, 0, Skp);
        __syncthreads();
    }
    const int q = blockIdx.y * (16 * NW) + t.wave * 16 + t.li;          // this lane's query
    if (!LONG && blockIdx.y * (16 * NW) + t.wave * 16 >= p.Sq) return;
    bf16x8 qf[Geo<DH>::KH];
    load_bfrag<DH>(head_rows<DH>(p.q, t, p.Sq, p.ldq), q, p.Sq, p.ldq, t.lg, qf);

    float m = -INFINITY, l = 0.f;
    if constexpr (!LONG) {
        fwd_stats_chunk<DH>(s, Skp, t, qf, p.scale, m, l);
    } else {
        for (int c0 = 0; c0 < Skp; c0 += ch) {          // one staged chunk at a time, behind a barrier
            const int rows = (Skp - c0 < ch) ? Skp - c0 : ch;
            __syncthreads();
            stage_kv_bias<DH, NW, false>(s, kv, t, c0, rows);
            __syncthreads();
            fwd_stats_chunk<DH>(s, rows, t, qf, p.scale, m, l);
        }
    }
    float M, Ms, inv_l;
    softmax_finish(m, l, M, Ms, inv_l);

    const rt_drop drop(p.drop_p, p.seed_dev, p.drop_seed);
    const uint32_t drop_row = (uint32_t)(((size_t)t.bh * p.Sq + q) * p.Sk);
    f32x4 o[Geo<DH>::DT];
    zero_acc<DH>(o);
    if constexpr (!LONG) {
        fwd_pv_chunk<DH>(s, Skp, 0, t, qf, p.scale, Ms, inv_l, drop, drop_row, o);
    } else {
        for (int c0 = 0; c0 < Skp; c0 += ch) {          // one staged chunk at a time, behind a barrier
            const int rows = (Skp - c0 < ch) ? Skp - c0 : ch;
            __syncthreads();
            stage_kv_bias<DH, NW, true>(s, kv, t, c0, rows);
            __syncthreads();
            fwd_pv_chunk<DH>(s, rows, c0, t, qf, p.scale, Ms, inv_l, drop, drop_row, o);
        }
    }
    fwd_store<DH>(p.out, p.lse, p.Sq, p.ldo, t, q, o, M, l);
}

template <int DH, int NW>
__global__ __launch_bounds__(64 * NW) void attn_fwd_kernel(const rt_attn_desc p) {
    attn_fwd_body<DH, NW, false>(p, 0);
}

// Forward with the score row kept in registers (NT 16-key tiles, fully unrolled): the NT score MFMAs of a wave are
// independent and issue back to back, the softmax runs over registers, and the scores are not recomputed for the P V pass.
// The two-pass kernel above walks 2 x NT dependent [LDS read -> MFMA -> exp] steps per wave and is latency-bound at one
// workgroup per CU (88 KB of LDS for S = 440).  Its loops index registers, so they stay its own (see the file header).
template <int DH, int NW, int NT>
__global__ __launch_bounds__(64 * NW) void attn_fwd_reg_kernel(const rt_attn_desc p) {
    constexpr int RS = Geo<DH>::RS, DT = Geo<DH>::DT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Skp = (p.Sk + 31) & ~31;
    unsigned char* sK = smem;
    unsigned char* sV = sK + (size_t)Skp * RS;
    float* sBias = reinterpret_cast<float*>(sV + (size_t)Skp * RS);
    const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lg = lane >> 4;
    stage_rows2<DH>(sK, (const bf16_t*)p.k + (size_t)b * p.Sk * p.ldk + h * DH, p.ldk,
                    sV, (const bf16_t*)p.v + (size_t)b * p.Sk * p.ldv + h * DH, p.ldv, p.Sk, Skp, threadIdx.x, 64 * NW);
    for (int j = threadIdx.x; j < Skp; j += 64 * NW)
        sBias[j] = (j < p.Sk && !(p.kpm && p.kpm[(size_t)b * p.Sk + j])) ? 0.f : -INFINITY;
    __syncthreads();

    const int q = blockIdx.y * (16 * NW) + wave * 16 + li;
    if (blockIdx.y * (16 * NW) + wave * 16 >= p.Sq) return;
    bf16x8 qf[Geo<DH>::KH];
    load_bfrag<DH>((const bf16_t*)p.q + (size_t)b * p.Sq * p.ldq + h * DH, q, p.Sq, p.ldq, lg, qf);
    const int nblk = Skp >> 4;                  // <= NT, even

    f32x4 sc[NT];
    float m = -INFINITY;
#pragma unroll
    for (int blk = 0; blk < NT; ++blk) {
        if (blk < nblk) {
            const f32x4 acc = tile_dot<DH>(sK, blk * 16, li, lg, qf);
            const f32x4 bias = *reinterpret_cast<const f32x4*>(sBias + blk * 16 + lg * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) { sc[blk][r] = acc[r] * p.scale + bias[r]; m = fmaxf(m, sc[blk][r]); }
        } else {
            sc[blk] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
    }
    const float M = group_max(m);
    const float Ms = (M == -INFINITY) ? 0.f : M;
    float l = 0.f;
#pragma unroll
    for (int blk = 0; blk < NT; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) { sc[blk][r] = __expf(sc[blk][r] - Ms); l += sc[blk][r]; }
    l = group_sum(l);
    const float inv_l = 1.f / l;                 // fully masked row: 0 * inf = NaN below, as the reference

    const rt_drop drop(p.drop_p, p.seed_dev, p.drop_seed);
    const uint32_t drop_row = (uint32_t)(((size_t)bh * p.Sq + q) * p.Sk);
    f32x4 o[DT];
    zero_acc<DH>(o);
    const int tr_r = 4 * lg + (li >> 2), tr_c = (li & 3) * 8;
#pragma unroll
    for (int c = 0; c < NT / 2; ++c) {
        if (2 * c < nblk) {
            float pv[8];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int k0 = c * 32 + half * 16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float pr = sc[2 * c + half][r] * inv_l;
                    if (drop.on) pr = drop.keep(drop_row + (uint32_t)(k0 + lg * 4 + r)) ? pr * drop.ks : 0.f;
                    pv[half * 4 + r] = pr;
                }
            }
            const bf16x8 pf = pack8(pv);
            const unsigned char* v0 = sV + (c * 32 + tr_r) * RS + tr_c;
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                const bf16x8 vf = rt_tr_frag(v0 + t * 32, v0 + 16 * RS + t * 32);
                o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[t], 0, 0, 0);
            }
        }
    }
    if (q < p.Sq) {
        bf16_t* orow = (bf16_t*)p.out + ((size_t)b * p.Sq + q) * p.ldo + h * DH;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            bf16x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = (bf16_t)o[t][r];
            *reinterpret_cast<bf16x4*>(orow + t * 16 + lg * 4) = ov;
        }
        if (lg == 0 && p.lse) p.lse[(size_t)bh * p.Sq + q] = M + __logf(l);
    }
}

// ------------------------------------------------------------------------------------------------ dQ (+ delta)
// `rows` staged keys: dS^T from the recomputed probabilities, dQ^T += K^T dS^T
template <int DH>
__device__ __forceinline__ void dq_chunk(const Lds<DH>& s, int rows, int c0, const Lanes& t, const bf16x8 (&qf)[Geo<DH>::KH],
                                         const bf16x8 (&dof)[Geo<DH>::KH], float lse, float delta, float scale, const rt_drop& drop,
                                         uint32_t drop_row, f32x4 (&dq)[Geo<DH>::DT]) {
    constexpr int RS = Geo<DH>::RS;
    for (int c = 0; c < (rows >> 5); ++c) {
        float dsv[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int k0 = c * 32 + half * 16;
            const f32x4 sc = tile_dot<DH>(s.a, k0, t.li, t.lg, qf);
            const f32x4 dp = tile_dot<DH>(s.b, k0, t.li, t.lg, dof);
            const f32x4 bias = *reinterpret_cast<const f32x4*>(s.f0 + k0 + t.lg * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pr = __expf(sc[r] * scale + bias[r] - lse);
                float d = dp[r];
                if (drop.on) d = drop.keep(drop_row + (uint32_t)(c0 + k0 + t.lg * 4 + r)) ? d * drop.ks : 0.f;
                dsv[half * 4 + r] = pr * (d - delta) * scale;
            }
        }
        const bf16x8 dsf = pack8(dsv);
        const unsigned char* k0p = s.a + (c * 32 + t.tr_r) * RS + t.tr_c;
#pragma unroll
        for (int d = 0; d < Geo<DH>::DT; ++d) {
            const bf16x8 kf = rt_tr_frag(k0p + d * 32, k0p + 16 * RS + d * 32);
            dq[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, dsf, dq[d], 0, 0, 0);
        }
    }
}

template <int DH, int NW, bool LONG>
__device__ __forceinline__ void attn_bwd_dq_body(const rt_attn_bwd_desc& p, const int by, const int ch) {
    constexpr int KH = Geo<DH>::KH;
    const Lanes t = lanes(p.H);
    const int Skp = (p.Sk + 31) & ~31;
    const Lds<DH> s(LONG ? ch : Skp);
    const KvSrc kv{p.k, p.v, p.kpm, p.Sk, p.ldk, p.ldv};
    if constexpr (!LONG) {
        stage_kv_bias<DH, NW, true>(s, kv, t, 0, Skp);
        __syncthreads();
    }
    const int q = by * (16 * NW) + t.wave * 16 + t.li;
    if (!LONG && by * (16 * NW) + t.wave * 16 >= p.Sq) return;
    bf16x8 qf[KH], dof[KH], of[KH];
    load_bfrag<DH>(head_rows<DH>(p.q, t, p.Sq, p.ldq), q, p.Sq, p.ldq, t.lg, qf);
    load_bfrag<DH>(head_rows<DH>(p.dout, t, p.Sq, p.ldo), q, p.Sq, p.ldo, t.lg, dof);
    load_bfrag<DH>(head_rows<DH>(p.out, t, p.Sq, p.ldo), q, p.Sq, p.ldo, t.lg, of);
    float delta = 0.f;                          // from the fragments: each lane group holds a quarter of the row
#pragma unroll
    for (int kh = 0; kh < KH; ++kh)
#pragma unroll
        for (int e = 0; e < 8; ++e) delta += (float)dof[kh][e] * (float)of[kh][e];
    delta = group_sum(delta);
    const float lse = (q < p.Sq) ? p.lse[(size_t)t.bh * p.Sq + q] : INFINITY;
    if (t.lg == 0 && q < p.Sq) p.delta[(size_t)t.bh * p.Sq + q] = delta;

    const rt_drop drop(p.drop_p, p.seed_dev, p.drop_seed);
    const uint32_t drop_row = (uint32_t)(((size_t)t.bh * p.Sq + q) * p.Sk);
    f32x4 dq[Geo<DH>::DT];
    zero_acc<DH>(dq);
    if constexpr (!LONG) {
        dq_chunk<DH>(s, Skp, 0, t, qf, dof, lse, delta, p.scale, drop, drop_row, dq);
    } else {
        for (int c0 = 0; c0 < Skp; c0 += ch) {          // one staged chunk at a time, behind a barrier
            const int rows = (Skp - c0 < ch) ? Skp - c0 : ch;
            __syncthreads();
            stage_kv_bias<DH, NW, true>(s, kv, t, c0, rows);
            __syncthreads();
            dq_chunk<DH>(s, rows, c0, t, qf, dof, lse, delta, p.scale, drop, drop_row, dq);
        }
    }
    if (q < p.Sq) store_rows<DH>((bf16_t*)p.dq + ((size_t)t.b * p.Sq + q) * p.lddq + t.h * DH, t.lg, dq);
}

// ------------------------------------------------------------------------------------------------ dK, dV
// `rows` staged queries: P and dS of [query 4g+r][key li], dV^T += dO^T P, dK^T += Q^T dS
template <int DH>
__device__ __forceinline__ void dkv_chunk(const Lds<DH>& s, int rows, int c0, const Lanes& t, const bf16x8 (&kf)[Geo<DH>::KH],
                                          const bf16x8 (&vf)[Geo<DH>::KH], float kbias, float scale, const rt_drop& drop, int Sq, int Sk, int key,
                                          f32x4 (&dk)[Geo<DH>::DT], f32x4 (&dv)[Geo<DH>::DT]) {
    constexpr int RS = Geo<DH>::RS;
    for (int c = 0; c < (rows >> 5); ++c) {
        float pv[8], dsv[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int q0 = c * 32 + half * 16;
            const f32x4 sc = tile_dot<DH>(s.a, q0, t.li, t.lg, kf);          // [query 4g+r][key li]
            const f32x4 dp = tile_dot<DH>(s.b, q0, t.li, t.lg, vf);
            const f32x4 lse = *reinterpret_cast<const f32x4*>(s.f0 + q0 + t.lg * 4);
            const f32x4 del = *reinterpret_cast<const f32x4*>(s.f1 + q0 + t.lg * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pr = __expf(sc[r] * scale + kbias - lse[r]);
                float d = dp[r], pd = pr;
                if (drop.on) {
                    const int qq = c0 + q0 + t.lg * 4 + r;
                    const bool keep = drop.keep((uint32_t)(((size_t)t.bh * Sq + qq) * Sk + key));
                    d = keep ? d * drop.ks : 0.f; pd = keep ? pr * drop.ks : 0.f;
                }
                pv[half * 4 + r] = pd;
                dsv[half * 4 + r] = pr * (d - del[r]) * scale;
            }
        }
        const bf16x8 pf = pack8(pv), dsf = pack8(dsv);
        const unsigned char* d0 = s.b + (c * 32 + t.tr_r) * RS + t.tr_c;
        const unsigned char* q0p = s.a + (c * 32 + t.tr_r) * RS + t.tr_c;
#pragma unroll
        for (int d = 0; d < Geo<DH>::DT; ++d) {
            const bf16x8 dof = rt_tr_frag(d0 + d * 32, d0 + 16 * RS + d * 32);
            dv[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof, pf, dv[d], 0, 0, 0);
            const bf16x8 qtf = rt_tr_frag(q0p + d * 32, q0p + 16 * RS + d * 32);
            dk[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qtf, dsf, dk[d], 0, 0, 0);
        }
    }
}

template <int DH, int NW, bool LONG, bool OWN_DELTA>
__device__ __forceinline__ void attn_bwd_dkv_body(const rt_attn_bwd_desc& p, const int by, const int ch) {
    constexpr int KH = Geo<DH>::KH;
    const Lanes t = lanes(p.H);
    const int Sqp = (p.Sq + 31) & ~31;
    const Lds<DH> s(LONG ? ch : Sqp);
    if constexpr (!LONG) {
        stage_qdo_stats<DH, NW, OWN_DELTA>(s, p, t, 0, Sqp);
        __syncthreads();
    }
    const int key = by * (16 * NW) + t.wave * 16 + t.li;         // this lane's key (MFMA column)
    if (!LONG && by * (16 * NW) + t.wave * 16 >= p.Sk) return;
    bf16x8 kf[KH], vf[KH];
    load_bfrag<DH>(head_rows<DH>(p.k, t, p.Sk, p.ldk), key, p.Sk, p.ldk, t.lg, kf);
    load_bfrag<DH>(head_rows<DH>(p.v, t, p.Sk, p.ldv), key, p.Sk, p.ldv, t.lg, vf);
    const float kbias = (key < p.Sk && !(p.kpm && p.kpm[(size_t)t.b * p.Sk + key])) ? 0.f : -INFINITY;

    const rt_drop drop(p.drop_p, p.seed_dev, p.drop_seed);
    f32x4 dk[Geo<DH>::DT], dv[Geo<DH>::DT];
    zero_acc<DH>(dk);
    zero_acc<DH>(dv);
    if constexpr (!LONG) {
        dkv_chunk<DH>(s, Sqp, 0, t, kf, vf, kbias, p.scale, drop, p.Sq, p.Sk, key, dk, dv);
    } else {
        for (int c0 = 0; c0 < Sqp; c0 += ch) {          // one staged chunk at a time, behind a barrier
            const int rows = (Sqp - c0 < ch) ? Sqp - c0 : ch;
            __syncthreads();
            stage_qdo_stats<DH, NW, OWN_DELTA>(s, p, t, c0, rows);
            __syncthreads();
            dkv_chunk<DH>(s, rows, c0, t, kf, vf, kbias, p.scale, drop, p.Sq, p.Sk, key, dk, dv);
        }
    }
    if (key < p.Sk) {
        store_rows<DH>((bf16_t*)p.dk + ((size_t)t.b * p.Sk + key) * p.lddk + t.h * DH, t.lg, dk);
        store_rows<DH>((bf16_t*)p.dv + ((size_t)t.b * p.Sk + key) * p.lddv + t.h * DH, t.lg, dv);
    }
}

template <int DH, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_dq_kernel(const rt_attn_bwd_desc p) {
    attn_bwd_dq_body<DH, NW, false>(p, (int)blockIdx.y, 0);
}
template <int DH, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_dkv_kernel(const rt_attn_bwd_desc p) {
    attn_bwd_dkv_body<DH, NW, false, false>(p, (int)blockIdx.y, 0);
}
// both halves in one launch: blockIdx.y < ny_dq -> the dQ row blocks, the rest -> the dK / dV key blocks
template <int DH, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_fused_kernel(const rt_attn_bwd_desc p, const int ny_dq) {
    if ((int)blockIdx.y < ny_dq) attn_bwd_dq_body<DH, NW, false>(p, (int)blockIdx.y, 0);
    else attn_bwd_dkv_body<DH, NW, false, true>(p, (int)blockIdx.y - ny_dq, 0);
}

// ------------------------------------------------------------------------------------------------ long inner axes
// Sequences whose K / V (forward, dQ) or Q / dO (dK, dV) rows do not fit the CU's 160 KB at once (--dilation at 640 x 640: c5 at
// stride 16, S = 1600 + L): the bodies above with LONG = true walk the inner axis in chunks of `ch` <= LongGeo::CH rows, each staged
// into the same LDS region behind a barrier, and hand every chunk to the SAME chunk functions the whole-axis kernels
// call once -- same lane <-> (query, key) assignment, same key order per lane, the chunk's offset c0 entering only the dropout
// index -- so the results are bit-identical to attn_fwd_kernel / the whole-axis dq / dkv bodies wherever both apply (tests force
// this path on short sequences with a small chunk).  The dK / dV half always recomputes its delta (OWN_DELTA).
template <int DH> struct LongGeo { static constexpr int CH = DH == 32 ? 768 : 448; };     // 2 * CH * RS + 8 * CH <= 160 KB

template <int DH, int NW>
__global__ __launch_bounds__(64 * NW) void attn_fwd_long_kernel(const rt_attn_desc p, const int ch) {
    attn_fwd_body<DH, NW, true>(p, ch);
}
// both halves in one launch, as attn_bwd_fused_kernel: blockIdx.y < ny_dq -> the dQ row blocks, the rest -> the dK / dV key blocks
template <int DH, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_long_kernel(const rt_attn_bwd_desc p, const int ny_dq, const int ch) {
    if ((int)blockIdx.y < ny_dq) attn_bwd_dq_body<DH, NW, true>(p, (int)blockIdx.y, ch);
    else attn_bwd_dkv_body<DH, NW, true, true>(p, (int)blockIdx.y - ny_dq, ch);
}

// Opt a kernel into the full 160 KiB of dynamic LDS once per kernel (not per launch: keeps launches capturable in a
// hipGraph).  Keyed by the function pointer (kernels of equal signature share a C++ type).
template <typename K>
int set_smem(K kernel, size_t bytes) {
    if (bytes > 160 * 1024) return RT_ERR_UNSUPPORTED;
    static const void* seen[16];
    static int nseen = 0;
    const void* fp = reinterpret_cast<const void*>(kernel);
    for (int i = 0; i < nseen; ++i) if (seen[i] == fp) return RT_OK;
    hipError_t e = hipFuncSetAttribute(fp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    if (nseen < 16) seen[nseen++] = fp;
    return RT_OK;
}

size_t smem_bytes(int inner, int dh) {
    const size_t ip = (size_t)((inner + 31) & ~31);
    return 2 * ip * (dh * 2 + 32) + 2 * sizeof(float) * ip;
}

// rows of the inner axis per LDS pass of the long-axis kernels; 0 = the whole-axis kernels apply.  REFTR_ATTN_CHUNK (a multiple of
// 32) forces the long-axis kernels with that chunk on every shape (tests: bit-identity with the whole-axis kernels)
int long_chunk(int inner, int dh) {
    static const int env = getenv("REFTR_ATTN_CHUNK") ? atoi(getenv("REFTR_ATTN_CHUNK")) : 0;
    const int cap = dh == 32 ? LongGeo<32>::CH : LongGeo<64>::CH;
    if (env >= 32) return ((env < cap ? env : cap) + 31) & ~31;
    return smem_bytes(inner, dh) > 160 * 1024 ? cap : 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// One query per (batch, head): the decoder's cross-attention with a single referring query per image (Sq = 1, Sk = L + h*w).
// The MFMA kernels above are built for 16-query tiles and spend ~15 us of latency on this case; here a 256-thread workgroup
// owns one (b, h): each thread takes keys t, t + 256, ... (a 64-B K row and V row per key), the softmax is a block
// reduction and the output / dq a 32-wide reduction over the block.  Same arithmetic order of the definition, fp32.
// Backward produces dq, dk and dv in the same launch.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_q1_fwd_kernel(const rt_attn_desc p) {
    __shared__ float sm32[4][32];
    __shared__ float red[8];
    const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H, t = threadIdx.x;
    Q1KV kv;
    q1_prefetch((const bf16_t*)p.k, p.ldk, (const bf16_t*)p.v, p.ldv, p.kpm, p.Sk, b, h, kv);
    float q[32];
    q1_load_row((const bf16_t*)p.q + (size_t)b * p.ldq + h * 32, q);
    const float lse = q1_fwd(kv, q, p.scale, p.Sk, bh, rt_drop(p.drop_p, p.seed_dev, p.drop_seed), red, sm32);
    if (t == 0 && p.lse) p.lse[bh] = lse;
    if (t < 32) ((bf16_t*)p.out)[(size_t)b * p.ldo + h * 32 + t] = (bf16_t)q1_sum4(sm32, t);
}

__global__ __launch_bounds__(256) void attn_q1_bwd_kernel(const rt_attn_bwd_desc p) {
    __shared__ float sm32[4][32];
    const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H, t = threadIdx.x;
    Q1KV kv;
    q1_prefetch((const bf16_t*)p.k, p.ldk, (const bf16_t*)p.v, p.ldv, p.kpm, p.Sk, b, h, kv);
    float q[32], go[32], ov[32];
    q1_load_row((const bf16_t*)p.q + (size_t)b * p.ldq + h * 32, q);
    q1_load_row((const bf16_t*)p.dout + (size_t)b * p.ldo + h * 32, go);
    q1_load_row((const bf16_t*)p.out + (size_t)b * p.ldo + h * 32, ov);
    q1_bwd(kv, q, go, ov, p.lse[bh], p.scale, p.Sk, bh, rt_drop(p.drop_p, p.seed_dev, p.drop_seed), sm32,
           [&](int j, int c, bf16x8 dk8, bf16x8 dv8) {
               *reinterpret_cast<bf16x8*>((bf16_t*)p.dk + ((size_t)b * p.Sk + j) * p.lddk + h * 32 + c * 8) = dk8;
               *reinterpret_cast<bf16x8*>((bf16_t*)p.dv + ((size_t)b * p.Sk + j) * p.lddv + h * 32 + c * 8) = dv8;
           });
    if (t < 32) ((bf16_t*)p.dq)[(size_t)b * p.lddq + h * 32 + t] = (bf16_t)q1_sum4(sm32, t);
}

extern "C" int rt_attn_fwd(const rt_attn_desc* d, rt_stream_t stream) {
    if (!d || !d->q || !d->k || !d->v || !d->out) return RT_ERR_BADARG;
    if ((d->dh != 32 && d->dh != 64) || d->Sk <= 0 || d->Sq <= 0) return RT_ERR_UNSUPPORTED;
    if ((d->ldq | d->ldk | d->ldv | d->ldo) & 7) return RT_ERR_UNSUPPORTED;
    static const int q1_env = RT_TUNE("REFTR_ATTN_Q1", 1);
    if (q1_env && d->Sq == 1 && d->dh == 32 && d->Sk <= 256 * Q1_MAXK) {
        hipLaunchKernelGGL(attn_q1_fwd_kernel, dim3(d->B * d->H), dim3(256), 0, (hipStream_t)stream, *d);
        RT_CHECK_LAUNCH();
        return RT_OK;
    }
    int rc;
    if (const int ch = long_chunk(d->Sk, d->dh)) {
        const size_t lsmem = smem_bytes(ch, d->dh);
        const dim3 lgrid(d->B * d->H, (d->Sq + 127) / 128);
#define RT_ATTN_FWD_LONG(DHV) do { if ((rc = set_smem(attn_fwd_long_kernel<DHV, 8>, lsmem)) != RT_OK) return rc; \
        hipLaunchKernelGGL((attn_fwd_long_kernel<DHV, 8>), lgrid, dim3(512), lsmem, (hipStream_t)stream, *d, ch); } while (0)
        if (d->dh == 32) RT_ATTN_FWD_LONG(32); else RT_ATTN_FWD_LONG(64);
#undef RT_ATTN_FWD_LONG
        RT_CHECK_LAUNCH();
        return RT_OK;
    }
    const size_t smem = smem_bytes(d->Sk, d->dh);
    static const int nw_env = RT_TUNE("REFTR_ATTN_NW", 8);
    const int nw = nw_env == 4 ? 4 : (nw_env == 16 ? 16 : 8);
    // (b, h) on grid.x: the row blocks of one head get ids bh, bh + B*H, ... -> the same XCD whenever B*H is a multiple of 8, so the
    // head's K / V rows cross the fabric once per XCD instead of once per block
    const dim3 grid(d->B * d->H, (d->Sq + 16 * nw - 1) / (16 * nw));
#define RT_ATTN_FWD(DHV, NWV) do { if ((rc = set_smem(attn_fwd_kernel<DHV, NWV>, smem)) != RT_OK) return rc; \
        hipLaunchKernelGGL((attn_fwd_kernel<DHV, NWV>), grid, dim3(64 * NWV), smem, (hipStream_t)stream, *d); } while (0)
    static const int reg_env = RT_TUNE("REFTR_ATTN_REG", 1);
    const int tiles = ((d->Sk + 31) & ~31) >> 4;
    if (reg_env && nw == 8 && tiles <= 28) {          // 28 tiles = 180 VGPRs; 48 would spill: longer rows keep the two-pass kernel
#define RT_ATTN_FWD_REG(DHV, NTV) do { if ((rc = set_smem(attn_fwd_reg_kernel<DHV, 8, NTV>, smem)) != RT_OK) return rc; \
        hipLaunchKernelGGL((attn_fwd_reg_kernel<DHV, 8, NTV>), grid, dim3(512), smem, (hipStream_t)stream, *d); } while (0)
        if (d->dh == 32) { if (tiles <= 8) RT_ATTN_FWD_REG(32, 8); else RT_ATTN_FWD_REG(32, 28); }
        else             { if (tiles <= 8) RT_ATTN_FWD_REG(64, 8); else RT_ATTN_FWD_REG(64, 28); }
#undef RT_ATTN_FWD_REG
        RT_CHECK_LAUNCH();
        return RT_OK;
    }
    if (d->dh == 32) { if (nw == 8) RT_ATTN_FWD(32, 8); else if (nw == 4) RT_ATTN_FWD(32, 4); else RT_ATTN_FWD(32, 16); }
    else             { if (nw == 8) RT_ATTN_FWD(64, 8); else if (nw == 4) RT_ATTN_FWD(64, 4); else RT_ATTN_FWD(64, 16); }
#undef RT_ATTN_FWD
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_attn_bwd(const rt_attn_bwd_desc* d, rt_stream_t stream) {
    if (!d || !d->q || !d->k || !d->v || !d->out || !d->dout || !d->lse || !d->delta || !d->dq || !d->dk || !d->dv)
        return RT_ERR_BADARG;
    if ((d->dh != 32 && d->dh != 64) || d->Sk <= 0 || d->Sq <= 0) return RT_ERR_UNSUPPORTED;
    if ((d->ldq | d->ldk | d->ldv | d->ldo | d->lddq | d->lddk | d->lddv) & 7) return RT_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    static const int q1_env = RT_TUNE("REFTR_ATTN_Q1", 1);
    if (q1_env && d->Sq == 1 && d->dh == 32 && d->Sk <= 256 * Q1_MAXK) {
        hipLaunchKernelGGL(attn_q1_bwd_kernel, dim3(d->B * d->H), dim3(256), 0, s, *d);
        RT_CHECK_LAUNCH();
        return RT_OK;
    }
    int rc;
    {
        const int ch1 = long_chunk(d->Sk, d->dh), ch2 = long_chunk(d->Sq, d->dh);
        if (ch1 || ch2) {          // either inner axis too long for one LDS pass: both halves walk their axis in chunks
            const int ch = ch1 > ch2 ? ch1 : ch2;
            const size_t lsmem = smem_bytes(ch, d->dh);
            const int ny_dq = (d->Sq + 127) / 128, ny_kv = (d->Sk + 127) / 128;
#define RT_ATTN_BWD_LONG(DHV) do { if ((rc = set_smem(attn_bwd_long_kernel<DHV, 8>, lsmem)) != RT_OK) return rc; \
            hipLaunchKernelGGL((attn_bwd_long_kernel<DHV, 8>), dim3(d->B * d->H, ny_dq + ny_kv), dim3(512), lsmem, s, *d, ny_dq, ch); } while (0)
            if (d->dh == 32) RT_ATTN_BWD_LONG(32); else RT_ATTN_BWD_LONG(64);
#undef RT_ATTN_BWD_LONG
            RT_CHECK_LAUNCH();
            return RT_OK;
        }
    }
    const size_t smem1 = smem_bytes(d->Sk, d->dh), smem2 = smem_bytes(d->Sq, d->dh);
    static const int nw_env = RT_TUNE("REFTR_ATTN_NW", 8);
    const int nw = nw_env == 4 ? 4 : (nw_env == 16 ? 16 : 8);
    const dim3 g1(d->B * d->H, (d->Sq + 16 * nw - 1) / (16 * nw)), g2(d->B * d->H, (d->Sk + 16 * nw - 1) / (16 * nw));
    static const int fused_env = RT_TUNE("REFTR_ATTN_BWD_FUSED", 1);
    if (fused_env && nw == 8) {
        const size_t smem = smem1 > smem2 ? smem1 : smem2;
        const dim3 g(d->B * d->H, g1.y + g2.y);
#define RT_ATTN_BWD_F(DHV) do { if ((rc = set_smem(attn_bwd_fused_kernel<DHV, 8>, smem)) != RT_OK) return rc; \
        hipLaunchKernelGGL((attn_bwd_fused_kernel<DHV, 8>), g, dim3(512), smem, s, *d, (int)g1.y); } while (0)
        if (d->dh == 32) RT_ATTN_BWD_F(32); else RT_ATTN_BWD_F(64);
#undef RT_ATTN_BWD_F
        RT_CHECK_LAUNCH();
        return RT_OK;
    }
#define RT_ATTN_BWD(DHV, NWV) do { if ((rc = set_smem(attn_bwd_dq_kernel<DHV, NWV>, smem1)) != RT_OK) return rc; \
        if ((rc = set_smem(attn_bwd_dkv_kernel<DHV, NWV>, smem2)) != RT_OK) return rc; \
        hipLaunchKernelGGL((attn_bwd_dq_kernel<DHV, NWV>), g1, dim3(64 * NWV), smem1, s, *d); \
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<DHV, NWV>), g2, dim3(64 * NWV), smem2, s, *d); } while (0)
    if (d->dh == 32) { if (nw == 8) RT_ATTN_BWD(32, 8); else if (nw == 4) RT_ATTN_BWD(32, 4); else RT_ATTN_BWD(32, 16); }
    else             { if (nw == 8) RT_ATTN_BWD(64, 8); else if (nw == 4) RT_ATTN_BWD(64, 4); else RT_ATTN_BWD(64, 16); }
#undef RT_ATTN_BWD
    RT_CHECK_LAUNCH();
    return RT_OK;
}
