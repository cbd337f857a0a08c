// The decoder's query chain as ONE cooperative launch (transformer.py:231-252 x dec_layers, one query per image).
//
// With a single referring query per image the decoder works on M = B rows: every Linear is a 16-column-tile GEMV whose cost
// as a launch is the launch itself (~5 us per link, ~66 links per forward).  Here DEC_G workgroups stay resident for the whole
// stack and hand the M x 256 row block from stage to stage through global memory:
//   * the hand-off carries its own validity: a producer writes its columns as 8-byte units {4 bytes of data, 4-byte tag} with
//     write-through stores (sc0 sc1) and moves on -- no store acknowledgement, no counter; a consumer reads the units with
//     cache-bypassing loads and simply re-reads until every tag is the one of (this launch, this layer, this stage).  One memory
//     round trip per hand-off instead of three (store ack -> counter -> poll -> data read: the first version of this kernel,
//     5.2 us per stage measured with the stage trace below; a counter-only barrier probes at 1.6-2.1 us,
//     benchmarks/probes/grid_barrier_probe.hip) against ~4-5 us per launched link.  The tag's launch part is a word in the
//     hand-off buffer that workgroup 0 advances at the very end, so the buffer never needs clearing;
//   * everything that does not depend on the row block -- the stage's weight fragments, biases, the (b, h) K / V rows of the
//     cross-attention -- is requested BEFORE the wait, so it arrives while the workgroup polls;
//   * LayerNorm is not a stage: each consumer recomputes it on the M <= 16 rows (one wave per row, the arithmetic of
//     layernorm_fwd_vec_kernel) and keeps the fp32 result in LDS as the residual of the stage after next;
//   * four waves per workgroup (one per SIMD: the whole 512-register file per lane, the K / V rows of an attention stage stay in
//     registers across the wait); thread 0 polls -- its first poll returns behind its own prefetches, which the stage needs anyway.
// Arithmetic is the launched chain's: the LayerNorm rows and the one-query attention are the chain's own code (rt_ln_row.h,
// rt_attn_q1.h), the dropout sites its site type (rt_drop) with the same indices; only dec_tile restates a schedule, the K split over
// four waves and the reduction order of skinny_gemm_kernel.  The outputs are bit-identical to the chain's and the launched backward
// consumes the saved tensors unchanged (tests/test_decoder_coop_gpu.py).
// Stage map of one layer:  S1 v-proj + head dropout -> S2 out_proj + residual -> [LN1] S3 q-proj -> S4 cross-attention ->
// S5 out_proj + residual -> [LN2] S6 linear1 + relu -> S7 linear2 + residual -> [LN3] next layer's S1.  The 256-wide products
// (S1-S3, S5, S7) run on the 16 "core" workgroups (one 16-column tile each); the cross-attention (one (b, h) per workgroup) and
// linear1 (F / 16 tiles) on the G - 16 "workers", which therefore hold their K / V rows and weight fragments long before the
// rows they wait for exist.
#include "rt_common.h"
#include "rt_attn_q1.h"
#include "rt_ln_row.h"
#include <stdlib.h>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr int DEC_E = 256;            // model width (16 column tiles: the "core" workgroups 0..15 own one each)
constexpr int DEC_CORE = DEC_E / 16;
constexpr int DEC_COH = 17;           // buffer cache policy sc0 | sc1
constexpr int DEC_NT = 4;             // linear1 column tiles per workgroup (F / 16 / G <= 4)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t dec_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ u32x4 dec_ld16(const void* base, int byte_off) {          // coherent (cache-bypassing) 16-B load
    return __builtin_amdgcn_raw_buffer_load_b128(dec_rsrc(base), byte_off, 0, DEC_COH);
}
__device__ __forceinline__ void dec_st16(void* base, int byte_off, u32x4 v) {        // write-through stores
    __builtin_amdgcn_raw_buffer_store_b128(v, dec_rsrc(base), byte_off, 0, DEC_COH);
}
__device__ __forceinline__ void dec_st8(void* base, int byte_off, u32x2 v) {
    __builtin_amdgcn_raw_buffer_store_b64(v, dec_rsrc(base), byte_off, 0, DEC_COH);
}

struct DecSmem {
    f32x4 red[4][64];
    float ln32[16][DEC_E];           // fp32 LayerNorm output of the stage before: the residual of the next product
    float sm32[4][32];
    float redf[8];
};

// ---- hand-off through tagged units --------------------------------------------------------------------------------------------
// Region layout (bytes from the buffer start; words 0 / 1 = launch epoch / failure flag):
constexpr int LL_HDR = 256;
constexpr int LL_O = LL_HDR, LL_U = LL_O + 16 * 256 * 4, LL_Q2 = LL_U + 16 * 256 * 8, LL_O2 = LL_Q2 + 16 * 256 * 4,
              LL_U2 = LL_O2 + 16 * 256 * 4, LL_U3 = LL_U2 + 16 * 256 * 8, LL_HDN = LL_U3 + 16 * 256 * 8;      // hdn: 16 * F * 4 bytes
__device__ __forceinline__ unsigned ll_tag(unsigned epoch, int layer, int stage) { return (epoch << 8) | (unsigned)(layer * 8 + stage + 1); }

// consumer side: N coherent 16-byte loads of `base` at the byte offsets off(j) (load j is left out where !pred(j)), issued together
// and re-issued until words 1 and 3 of every one carry `tag`, `spin` times at most; a poll that gives up raises *err and the caller
// goes on with whatever it read
template <int N, class Off, class Pred>
__device__ __forceinline__ void ll_poll(const unsigned char* base, unsigned tag, unsigned* err, int spin, u32x4 (&v)[N], Off off, Pred pred) {
    u32x4 w[N];                              // polled into a local: the barrier below would keep the caller's array in memory
    int guard = 0;
    bool ok;
    do {
        asm volatile("" ::: "memory");       // the loads below must be re-issued on every pass
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (pred(j)) w[j] = dec_ld16(base, off(j));
        ok = true;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (pred(j)) ok = ok && w[j][1] == tag && w[j][3] == tag;
    } while (!ok && ++guard < spin);
    if (!ok) *err = 1u;
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = w[j];
}
template <int N, class Off>
__device__ __forceinline__ void ll_poll(const unsigned char* base, unsigned tag, unsigned* err, int spin, u32x4 (&v)[N], Off off) {
    ll_poll(base, tag, err, spin, v, off, [](int) { return true; });
}
// producer side: 4 consecutive bf16 features of row m (one 16-byte store), 4 consecutive fp32 features (two)
__device__ __forceinline__ void ll_put_bf16x4(unsigned char* ll, int region, unsigned tag, int elem, u32x2 packed) {
    dec_st16(ll + region, elem * 4, u32x4{packed[0], tag, packed[1], tag});
}
__device__ __forceinline__ void ll_put_f32x4(unsigned char* ll, int region, unsigned tag, int elem, f32x4 v) {
    dec_st16(ll + region, elem * 8, u32x4{__float_as_uint(v[0]), tag, __float_as_uint(v[1]), tag});
    dec_st16(ll + region, elem * 8 + 16, u32x4{__float_as_uint(v[2]), tag, __float_as_uint(v[3]), tag});
}

// ---- what a workgroup of either kernel knows about itself and its launch ----------------------------------------------------------
struct DecCtx {
    DecSmem& sm;
    bf16_t* xa;                      // [16][K + 8] bf16 operand rows of the current product
    int spin, M, F;
    int wg, t, lane, lg, wave;
    bool core, writer;               // the 16 workgroups of the 256-wide products / workgroup 0, which also writes what the chain saves once
    int wk, NW;                      // worker id / count: attention and the F-wide products run on the workers
    int ldE, ldF;
    int n0;                          // a core workgroup's column tile of every 256-wide product
    int n_bh, f_tiles;
    float drop_p;
    const uint32_t* seed_dev;
    unsigned char* ll;
    unsigned* err;
    unsigned epoch;                  // advanced by workgroup 0 when the whole stack is done
    unsigned* tr;                    // REFTR_DEC_TRACE: workgroups 0 (core) and G - 1 stamp the 100 MHz wall clock at every stage boundary
    int tr_i;

    template <class Desc>
    __device__ __forceinline__ DecCtx(const Desc& p, int G, int spin, DecSmem& sm, bf16_t* xa, unsigned* trace)
        : sm(sm), xa(xa), spin(spin), M(p.M), F(p.F), wg(blockIdx.x), t(threadIdx.x), lane(t & 63), lg(lane >> 4), wave(t >> 6),
          core(wg < DEC_CORE), writer(wg == 0), wk(wg - DEC_CORE), NW(G - DEC_CORE), ldE(DEC_E + 8), ldF(p.F + 8), n0(wg * 16),
          n_bh(p.M * p.H), f_tiles(p.F >> 4), drop_p(p.drop_p), seed_dev(p.seed_dev), ll(reinterpret_cast<unsigned char*>(p.handoff)),
          err(p.handoff + 1), epoch(p.handoff[0]),
          tr((trace && t == 0 && (wg == 0 || wg == G - 1)) ? trace + (wg == 0 ? 0 : 512) : nullptr), tr_i(0) {}
    __device__ __forceinline__ unsigned tag(int layer, int stage) const { return ll_tag(epoch, layer, stage); }
    __device__ __forceinline__ rt_drop drop(uint32_t site) const { return rt_drop::site(drop_p, seed_dev, site); }
    __device__ __forceinline__ void stamp() { if (tr) tr[tr_i++] = (unsigned)wall_clock64(); }
    // wave 0's bias of the column tile at n (the epilogue's lanes), requested with the weights
    __device__ __forceinline__ f32x4 bias(const float* b, int n) const {
        return wave == 0 ? *reinterpret_cast<const f32x4*>(b + n + lg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
};

// 4 consecutive fp32 features (4 units), 32 consecutive bf16 features as floats (16 units: elem is a multiple of 4)
__device__ __forceinline__ f32x4 ll_get_f32x4(const DecCtx& c, int region, unsigned tag, int elem) {
    u32x4 v[2];
    ll_poll(c.ll + region, tag, c.err, c.spin, v, [&](int j) { return elem * 8 + j * 16; });
    return f32x4{__uint_as_float(v[0][0]), __uint_as_float(v[0][2]), __uint_as_float(v[1][0]), __uint_as_float(v[1][2])};
}
__device__ __forceinline__ void ll_get_bf16x32(const DecCtx& c, int region, unsigned tag, int elem, float (&out)[32]) {
    u32x4 raw[8];
    ll_poll(c.ll + region, tag, c.err, c.spin, raw, [&](int j) { return (elem + j * 4) * 4; });
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned w0 = raw[j][0], w1 = raw[j][2];
        const bf16x2 lo = *reinterpret_cast<const bf16x2*>(&w0), hi = *reinterpret_cast<const bf16x2*>(&w1);
        out[j * 4 + 0] = (float)lo[0]; out[j * 4 + 1] = (float)lo[1]; out[j * 4 + 2] = (float)hi[0]; out[j * 4 + 3] = (float)hi[1];
    }
}
// bf16 row block [M][K] (unit = 2 bf16 + tag) -> LDS operand rows; NL 16-byte loads per thread in flight per round trip
template <int NL>
__device__ __forceinline__ void ll_rows_to_lds(const DecCtx& c, int region, unsigned tag, int K) {
    const int per_row = K >> 2, pieces = c.M * per_row;          // 16-byte pieces: 2 units = 4 bf16
    for (int i0 = 0; i0 < pieces; i0 += 256 * NL) {
        u32x4 v[NL];
        ll_poll(c.ll + region, tag, c.err, c.spin, v, [&](int j) { return (i0 + j * 256 + c.t) * 16; },
                [&](int j) { return i0 + j * 256 + c.t < pieces; });
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int i = i0 + j * 256 + c.t;
            if (i < pieces) {
                const int r = i / per_row, col = i - r * per_row;
                *reinterpret_cast<u32x2*>(c.xa + r * (K + 8) + col * 4) = u32x2{v[j][0], v[j][2]};
            }
        }
    }
}

// ---- LayerNorm of the M rows (rt_ln_row.h, as layernorm_fwd_vec_kernel<1>): fp32 result -> ln32, bf16(y [+ pos]) -> xa ----------
struct DecLnOut { float* y_f32; bf16_t* y_bf16; bf16_t* ypos_bf16; float* mean; float* rstd; };
// the rows come from a tagged fp32 region (4 units per lane); `o` is written where `writer`
__device__ __forceinline__ void dec_ln_rows(const DecCtx& c, int region, unsigned tag, const float* gamma, const float* beta, const float* pos,
                                            float eps, bool writer, const DecLnOut& o) {
    const int col = c.lane * 4;
    const f32x4 gam = *reinterpret_cast<const f32x4*>(gamma + col), bet = *reinterpret_cast<const f32x4*>(beta + col);
    for (int row = c.wave; row < c.M; row += 4) {
        const f32x4 v = ll_get_f32x4(c, region, tag, row * DEC_E + col);
        const f32x4 ps = pos ? *reinterpret_cast<const f32x4*>(pos + (size_t)row * DEC_E + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        float mean, rstd;
        rt_ln_stats<1>(&v, eps, mean, rstd);
        const f32x4 y = rt_ln_affine(v, mean, rstd, gam, bet, false);
        bf16x4 yb, yp;
#pragma unroll
        for (int e = 0; e < 4; ++e) { yb[e] = (bf16_t)y[e]; yp[e] = (bf16_t)(y[e] + ps[e]); }
        *reinterpret_cast<f32x4*>(&c.sm.ln32[row][col]) = y;
        *reinterpret_cast<bf16x4*>(c.xa + row * c.ldE + col) = pos ? yp : yb;
        if (writer) {
            const size_t off = (size_t)row * DEC_E + col;
            if (c.lane == 0) { if (o.mean) o.mean[row] = mean; if (o.rstd) o.rstd[row] = rstd; }
            if (o.y_f32) *reinterpret_cast<f32x4*>(o.y_f32 + off) = y;
            if (o.y_bf16) *reinterpret_cast<bf16x4*>(o.y_bf16 + off) = yb;
            if (o.ypos_bf16) *reinterpret_cast<bf16x4*>(o.ypos_bf16 + off) = yp;
        }
    }
}

// ---- weight fragments of one 16-column tile: lane (li, lg) holds W[n0 + li][32 ks + 8 lg .. + 7] for its wave's K steps ------
template <int PER>
__device__ __forceinline__ void dec_load_w(const void* W, int K, int n0, u32x4 (&wv)[PER]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bf16_t* row = (const bf16_t*)W + (size_t)(n0 + (lane & 15)) * K + (lane >> 4) * 8 + wave * PER * 32;
#pragma unroll
    for (int j = 0; j < PER; ++j) wv[j] = *reinterpret_cast<const u32x4*>(row + j * 32);
}

// one tile: K split over the four compute waves (PER 32-wide steps each, ascending), partial sums added wave 0 + 1 + 2 + 3, the
// epilogue on wave 0: lane (li, lg) owns row m = li, features n0 + 4 lg .. + 3 -- skinny_gemm_kernel's schedule exactly.
template <int PER, class Epi>
__device__ __forceinline__ void dec_tile(const DecCtx& c, const u32x4 (&wv)[PER], int ld, int n0, Epi epi) {
    const int li = c.lane & 15;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const bf16_t* xr = c.xa + li * ld + c.lg * 8 + c.wave * PER * 32;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xr + j * 32);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&wv[j]), xv, acc, 0, 0, 0);
    }
    c.sm.red[c.wave][c.lane] = acc;
    __syncthreads();
    if (c.wave == 0 && li < c.M) epi(li, n0 + c.lg * 4, c.sm.red[0][c.lane] + c.sm.red[1][c.lane] + c.sm.red[2][c.lane] + c.sm.red[3][c.lane]);
    __syncthreads();
}

// ---- the two epilogues of a product (wave 0: row m, features n .. n + 3) ------------------------------------------------------------
__device__ __forceinline__ u32x2 dec_pack4(f32x4 v) {
    bf16x4 b;
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = (bf16_t)v[r];
    return *reinterpret_cast<u32x2*>(&b);
}
// what stands between the bias and the dropout: nothing, relu, or relu's backward -- * gate_scale where the forward's `gate` > 0, else 0
struct DecAct { bool relu = false; const void* gate = nullptr; float gate_scale = 0.f; };
// bf16(drop(act(v [+ bias]))), dropout index (e + r) >> shift, e = the element's index in its [M][ld] block -> the tagged units of
// `region` [+ the same four bf16 at plain + e]
__device__ __forceinline__ void dec_epi_bf16(const DecCtx& c, int region, unsigned tag, int e, f32x4 v, const f32x4* bias, const DecAct& act,
                                             const rt_drop& drop, int shift, void* plain) {
    if (bias) v += *bias;
    if (act.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
    }
    if (act.gate) {
        const bf16x4 gg = *reinterpret_cast<const bf16x4*>((const bf16_t*)act.gate + e);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = ((float)gg[r] > 0.f) ? v[r] * act.gate_scale : 0.f;
    }
    const u32x2 pk = dec_pack4(drop.apply(v, (uint32_t)e, shift));
    ll_put_bf16x4(c.ll, region, tag, e, pk);
    if (plain) *reinterpret_cast<u32x2*>((bf16_t*)plain + e) = pk;
}
// drop(v [+ bias]) + the residual row kept in ln32 -> the tagged fp32 units of `region` (< 0: none) [+ the same at plain]
__device__ __forceinline__ void dec_epi_res(const DecCtx& c, int region, unsigned tag, int m, int n, f32x4 v, const f32x4* bias,
                                            const rt_drop& drop, float* plain) {
    const int e = m * DEC_E + n;
    if (bias) v += *bias;
    v = drop.apply(v, (uint32_t)e);
    v += *reinterpret_cast<const f32x4*>(&c.sm.ln32[m][n]);
    if (region >= 0) ll_put_f32x4(c.ll, region, tag, e, v);
    if (plain) *reinterpret_cast<f32x4*>(plain + e) = v;
}

// one product of a core workgroup over K = 128 PER inputs, its column tile n0: the weight fragments and the bias (b: or none) are
// requested first, rows() then brings the operand rows into LDS -- it is what waits --, then the tile with epi(m, n, acc, bias or null)
template <int PER, class Rows, class Epi>
__device__ __forceinline__ void dec_product(DecCtx& c, const void* W, const float* b, Rows rows, Epi epi) {
    constexpr int K = PER * 128;
    u32x4 w[PER];
    dec_load_w<PER>(W, K, c.n0, w);
    const f32x4 bias = b ? c.bias(b, c.n0) : f32x4{0.f, 0.f, 0.f, 0.f};
    rows();
    c.stamp();
    __syncthreads();
    dec_tile<PER>(c, w, K + 8, c.n0, [&](int m, int n, f32x4 v) { epi(m, n, v, b ? &bias : nullptr); });
    c.stamp();
}

// ---- cross-attention of one (b, h) on a worker (rt_attn_q1.h: the code of attn_q1_fwd_kernel / attn_q1_bwd_kernel) ----------------
// the K / V rows are requested before the wait for the query / dout row
template <class Desc, class Layer>
__device__ __forceinline__ void dec_kv_prefetch(const Desc& p, const Layer& L, int bh, Q1KV& kv) {
    q1_prefetch((const bf16_t*)L.k2, p.ldkv, (const bf16_t*)L.v2, p.ldkv, p.kpm, p.S, bh / p.H, bh % p.H, kv);
}
// thread t < 16: features 2t, 2t + 1 of the head's reduced 32-vector -> one tagged unit + the saved bf16 pair
__device__ __forceinline__ void dec_put_head(const DecCtx& c, int region, unsigned tag, int elem, void* saved) {
    if (c.t < 16) {
        bf16x2 pr;
        pr[0] = (bf16_t)q1_sum4(c.sm.sm32, 2 * c.t);
        pr[1] = (bf16_t)q1_sum4(c.sm.sm32, 2 * c.t + 1);
        const int e = elem + 2 * c.t;
        const unsigned bits = *reinterpret_cast<const unsigned*>(&pr);
        dec_st8(c.ll + region, e * 4, u32x2{bits, tag});
        *reinterpret_cast<unsigned*>((bf16_t*)saved + e) = bits;
    }
}
__device__ __forceinline__ void dec_attn(const DecCtx& c, const rt_decoder_fwd_desc& p, const rt_decoder_layer_fwd& L, int l, int bh,
                                         const Q1KV& kv, const rt_drop& drop) {
    const int elem = (bh / p.H) * DEC_E + (bh % p.H) * 32;
    float q[32];
    ll_get_bf16x32(c, LL_Q2, c.tag(l, 2), elem, q);              // the 32 query features of (b, h): the same 128 bytes for every lane
    const float lse = q1_fwd(kv, q, p.scale, p.S, bh, drop, c.sm.redf, c.sm.sm32);
    if (c.t == 0) L.lse2[bh] = lse;
    dec_put_head(c, LL_O2, c.tag(l, 3), elem, L.o2);
}
// do2 arrives as 16 tagged units; the dK / dV rows go to memory [and to the packed second copy]
__device__ __forceinline__ void dec_attn_bwd(const DecCtx& c, const rt_decoder_bwd_desc& p, const rt_decoder_layer_bwd& L, int l, int bh,
                                             const Q1KV& kv, const rt_drop& drop) {
    const int b = bh / p.H, h = bh % p.H, elem = b * DEC_E + h * 32;
    float q[32], go[32], ov[32];
    q1_load_row((const bf16_t*)L.q2 + elem, q);
    q1_load_row((const bf16_t*)L.o2 + elem, ov);
    ll_get_bf16x32(c, LL_O2, c.tag(l, 2), elem, go);
    q1_bwd(kv, q, go, ov, L.lse2[bh], p.scale, p.S, bh, drop, c.sm.sm32, [&](int j, int piece, bf16x8 dk8, bf16x8 dv8) {
        const size_t row = (size_t)b * p.S + j;
        const int col = h * 32 + piece * 8;
        *reinterpret_cast<bf16x8*>((bf16_t*)L.dk2 + row * p.ldkv + col) = dk8;
        *reinterpret_cast<bf16x8*>((bf16_t*)L.dv2 + row * p.ldkv + col) = dv8;
        if (L.dk2p) {
            *reinterpret_cast<bf16x8*>((bf16_t*)L.dk2p + row * p.ldkvp + col) = dk8;
            *reinterpret_cast<bf16x8*>((bf16_t*)L.dv2p + row * p.ldkvp + col) = dv8;
        }
    });
    dec_put_head(c, LL_Q2, c.tag(l, 3), elem, L.dq2);
}

__global__ __launch_bounds__(256) void decoder_fwd_kernel(const rt_decoder_fwd_desc p, const int G, const int spin, unsigned* trace) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dec_smem_raw[];
    DecSmem& sm = *reinterpret_cast<DecSmem*>(dec_smem_raw);
    DecCtx c(p, G, spin, sm, reinterpret_cast<bf16_t*>(dec_smem_raw + sizeof(DecSmem)), trace);
    const rt_drop nodrop(0.f, 0u);
    const int F = c.F;

    c.stamp();
    u32x4 wv[2];            // S1's weights (K = 256: two 32-wide steps per wave) are requested a layer ahead
    if (c.core) dec_load_w<2>(p.layer[0].Wv, DEC_E, c.n0, wv);
    for (int l = 0; l < p.n_layers; ++l) {
        const rt_decoder_layer_fwd& L = p.layer[l];
        if (c.core) {
            // ================= S1: o = headdrop(t16 Wv^T + bv); t = LN3 of the layer before (or the stack's input)
            const f32x4 bv = c.bias(L.bv, c.n0);
            const rt_drop d_ad = c.drop(L.seed_ad), d1 = c.drop(L.seed_d1);
            if (l == 0) {          // the stack's input from plain memory: bf16 rows -> xa (16-byte pieces, 32 per row), fp32 rows -> ln32
                for (int i = c.t; i < c.M * (DEC_E / 8); i += 256)
                    *reinterpret_cast<u32x4*>(c.xa + (i >> 5) * c.ldE + (i & 31) * 8) = *reinterpret_cast<const u32x4*>((const bf16_t*)p.t16 + (size_t)i * 8);
                for (int i = c.t; i < c.M * (DEC_E / 4); i += 256)
                    *reinterpret_cast<f32x4*>(&sm.ln32[0][0] + i * 4) = *reinterpret_cast<const f32x4*>(p.t32 + (size_t)i * 4);
            } else {
                const rt_decoder_layer_fwd& Lp = p.layer[l - 1];
                const DecLnOut out{Lp.t3_f32, (bf16_t*)Lp.t3_16, nullptr, Lp.mean3, Lp.rstd3};
                dec_ln_rows(c, LL_U3, c.tag(l - 1, 6), Lp.g3, Lp.be3, nullptr, p.eps, c.writer, out);
            }
            c.stamp();
            __syncthreads();
            dec_tile<2>(c, wv, c.ldE, c.n0, [&](int m, int n, f32x4 v) {
                dec_epi_bf16(c, LL_O, c.tag(l, 0), m * DEC_E + n, v, &bv, DecAct{}, d_ad, 5, L.o);
            });
            c.stamp();
            // ================= S2: u = t + drop(o Wo^T + bo)
            dec_product<2>(c, L.Wo, L.bo, [&] { ll_rows_to_lds<4>(c, LL_O, c.tag(l, 0), DEC_E); },
                           [&](int m, int n, f32x4 v, const f32x4* bias) { dec_epi_res(c, LL_U, c.tag(l, 1), m, n, v, bias, d1, L.u); });
            // ================= S3: q2 = (LN1(u) + query_pos) Wq^T + bq
            dec_product<2>(c, L.Wq, L.bq, [&] {
                const DecLnOut out{nullptr, nullptr, (bf16_t*)L.t1q16, L.mean1, L.rstd1};
                dec_ln_rows(c, LL_U, c.tag(l, 1), L.g1, L.be1, p.qpos, p.eps, c.writer, out);
            }, [&](int m, int n, f32x4 v, const f32x4* bias) {
                dec_epi_bf16(c, LL_Q2, c.tag(l, 2), m * DEC_E + n, v, bias, DecAct{}, nodrop, 0, L.q2);
            });
        }
        // ================= S4: cross-attention, (b, h) = worker id, + number of workers, ...
        if (!c.core && c.wk < c.n_bh) {
            const rt_drop d_ad2 = c.drop(L.seed_ad2);
            Q1KV kv;
            for (int bh = c.wk; bh < c.n_bh; bh += c.NW) {
                dec_kv_prefetch(p, L, bh, kv);
                dec_attn(c, p, L, l, bh, kv, d_ad2);
                __syncthreads();
            }
            c.stamp();
        }
        if (c.core) {
            // ================= S5: u2 = t1 + drop(o2 Wo2^T + bo2)
            const rt_drop d2 = c.drop(L.seed_d2);
            dec_product<2>(c, L.Wo2, L.bo2, [&] { ll_rows_to_lds<4>(c, LL_O2, c.tag(l, 3), DEC_E); },
                           [&](int m, int n, f32x4 v, const f32x4* bias) { dec_epi_res(c, LL_U2, c.tag(l, 4), m, n, v, bias, d2, L.u2); });
        }
        // ================= S6: hdn = drop(relu(LN2(u2) W1^T + b1)), column tiles worker id, + number of workers, ...
        if (!c.core && c.wk < c.f_tiles) {
            u32x4 w1[DEC_NT][2];
            f32x4 b1[DEC_NT];
#pragma unroll
            for (int i = 0; i < DEC_NT; ++i) {
                const int tile = c.wk + i * c.NW;
                if (tile < c.f_tiles) {
                    dec_load_w<2>(L.W1, DEC_E, tile * 16, w1[i]);
                    b1[i] = c.bias(L.b1, tile * 16);
                }
            }
            const rt_drop d_h = c.drop(L.seed_dh);
            {
                const DecLnOut out{nullptr, (bf16_t*)L.t2_16, nullptr, L.mean2, L.rstd2};
                dec_ln_rows(c, LL_U2, c.tag(l, 4), L.g2, L.be2, nullptr, p.eps, c.wk == 0, out);
            }
            c.stamp();
            __syncthreads();
#pragma unroll
            for (int i = 0; i < DEC_NT; ++i) {
                const int tile = c.wk + i * c.NW;
                if (tile < c.f_tiles) {
                    const f32x4 bb = b1[i];
                    dec_tile<2>(c, w1[i], c.ldE, tile * 16, [&](int m, int n, f32x4 v) {
                        dec_epi_bf16(c, LL_HDN, c.tag(l, 5), m * F + n, v, &bb, DecAct{true}, d_h, 0, L.hdn);
                    });
                }
            }
            c.stamp();
        }
        if (c.core) {
            // ================= S7: u3 = t2 + drop(hdn W2^T + b2)      (K = F: 16 steps per wave at F = 2048)
            const rt_drop d3 = c.drop(L.seed_d3);
            dec_product<16>(c, L.W2, L.b2, [&] {
                // t2 = LN2(u2): this product's residual (the workers recompute it as linear1's operand)
                const DecLnOut none{nullptr, nullptr, nullptr, nullptr, nullptr};
                dec_ln_rows(c, LL_U2, c.tag(l, 4), L.g2, L.be2, nullptr, p.eps, false, none);
                __syncthreads();         // xa is reused for the hdn rows below
                ll_rows_to_lds<16>(c, LL_HDN, c.tag(l, 5), F);
            }, [&](int m, int n, f32x4 v, const f32x4* bias) { dec_epi_res(c, LL_U3, c.tag(l, 6), m, n, v, bias, d3, L.u3); });
            if (l + 1 < p.n_layers) dec_load_w<2>(p.layer[l + 1].Wv, DEC_E, c.n0, wv);
        }
    }
    // ---- the last layer's norm3 (statistics, bf16 rows, the fp32 rows the shared decoder norm reads); then the launch epoch moves on:
    // every workgroup read it at its start, and nothing of this launch is in flight once the last u3 is complete
    if (c.writer && p.n_layers > 0) {
        const rt_decoder_layer_fwd& Lp = p.layer[p.n_layers - 1];
        const DecLnOut out{Lp.t3_f32, (bf16_t*)Lp.t3_16, nullptr, Lp.mean3, Lp.rstd3};
        dec_ln_rows(c, LL_U3, c.tag(p.n_layers - 1, 6), Lp.g3, Lp.be3, nullptr, p.eps, true, out);
        if (c.t == 0) p.handoff[0] = c.epoch + 1;
        c.stamp();
    }
}

// =====================================================================================================================================
// Backward of the stack, same machinery.  Per layer (last to first), hand-offs in brackets:
//   B1 LayerNorm3 backward of (dnorm + dta of the layer above) -> du3 (fp32, kept in LDS) / du3b     [every workgroup recomputes it]
//   B2 workers: dhdn = relu-gate(du3b W2) * 1/(1-p)                                                  [dhdn]
//   B3 core:    dt2 = du3 + dhdn W1                                                                  [dt2]
//   B4 LayerNorm2 backward -> du2 (LDS, until B9) / du2b       B5 core: do2 = du2b Wo2              [do2]
//   B6 workers: one-query attention backward of (b, h): dK, dV rows to memory, dq                    [dq2]
//   B8 core:    dt1q = dq2 Wq (+= into d query_pos)                                                  [dt1q]
//   B9 LayerNorm1 backward of (du2 + dt1q) -> du (LDS) / dub   B10 core: dv = head-mask(dub Wo)      [dv]
//   B11 core:   dta = du + dv Wv                                                                     [dta -> B1 of the layer below]
// Everything the launched chain leaves for the launches that stay outside is written in the chain's format and values.
struct DecSmemB {
    DecSmem a;
    float res2[16][DEC_E];           // du2: LayerNorm2's input gradient waits here for LayerNorm1's backward
    float pstage[4][2][DEC_E];       // one block of LayerNorm parameter-gradient partials (4 rows = 4 waves)
};

struct DecLnbSrc { const float* plain; const float* lds; int region; unsigned tag; };      // region < 0: no tagged part

// LayerNorm backward of the M rows (rt_ln_row.h, as layernorm_bwd_vec_kernel<1>: one wave per row; block b of that kernel = rows 4b..4b+3 =
// waves 0..3 here, so the parameter-gradient partials are the same sums in the same order).  dy = the sum of src's parts; dx -> res
// (fp32), bf16(drop2(dx)) -> xa [and dxb_plain, with the partials, on the writer]
__device__ __forceinline__ void dec_lnb_rows(const DecCtx& c, const DecLnbSrc& src, const float* x, const float* mean_p, const float* rstd_p,
                                             const float* gamma, const rt_drop& drop2, float (*res)[DEC_E], bf16_t* dxb_plain, float* partials,
                                             float (*pstage)[2][DEC_E]) {
    const int col = c.lane * 4;
    const f32x4 gam = *reinterpret_cast<const f32x4*>(gamma + col);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dg[4], db[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) { dg[b] = f32x4{0.f, 0.f, 0.f, 0.f}; db[b] = dg[b]; }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int row = b * 4 + c.wave;
        if (row >= c.M) continue;
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        bool have = false;
        if (src.plain) { d = *reinterpret_cast<const f32x4*>(src.plain + (size_t)row * DEC_E + col); have = true; }
        if (src.lds) { d = *reinterpret_cast<const f32x4*>(src.lds + row * DEC_E + col); have = true; }
        if (src.region >= 0) {
            const f32x4 v = ll_get_f32x4(c, src.region, src.tag, row * DEC_E + col);
            d = have ? d + v : v;
        }
        const float rstd = rstd_p[row];
        f32x4 xh, g;
        float s1 = 0.f, s2 = 0.f;
        rt_ln_bwd_group(d, *reinterpret_cast<const f32x4*>(x + (size_t)row * DEC_E + col), mean_p[row], rstd, gam, zero, false, xh, g, s1, s2, dg[b], db[b]);
        rt_ln_bwd_means<1>(s1, s2);
        const f32x4 dx = rt_ln_bwd_dx(g, xh, rstd, s1, s2);
        const int o = row * DEC_E + col;
        const f32x4 d2 = drop2.apply(dx, (uint32_t)o);
        bf16x4 bb;
#pragma unroll
        for (int e = 0; e < 4; ++e) bb[e] = (bf16_t)d2[e];
        *reinterpret_cast<f32x4*>(&res[row][col]) = dx;
        *reinterpret_cast<bf16x4*>(c.xa + row * c.ldE + col) = bb;
        if (c.writer && dxb_plain) *reinterpret_cast<bf16x4*>(dxb_plain + o) = bb;
    }
    if (c.writer && partials) {                    // uniform per workgroup
        const int nb = (c.M + 3) >> 2;
        for (int b = 0; b < nb; ++b) {
            f32x4 a = dg[0], q = db[0];
            if (b == 1) { a = dg[1]; q = db[1]; } else if (b == 2) { a = dg[2]; q = db[2]; } else if (b == 3) { a = dg[3]; q = db[3]; }
            *reinterpret_cast<f32x4*>(&pstage[c.wave][0][col]) = a;
            *reinterpret_cast<f32x4*>(&pstage[c.wave][1][col]) = q;
            __syncthreads();
            const int cc = c.t;
            partials[((size_t)b * 2) * DEC_E + cc] = pstage[0][0][cc] + pstage[1][0][cc] + pstage[2][0][cc] + pstage[3][0][cc];
            partials[((size_t)b * 2 + 1) * DEC_E + cc] = pstage[0][1][cc] + pstage[1][1][cc] + pstage[2][1][cc] + pstage[3][1][cc];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void decoder_bwd_kernel(const rt_decoder_bwd_desc p, const int G, const int spin) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dec_smem_raw[];
    DecSmemB& smb = *reinterpret_cast<DecSmemB*>(dec_smem_raw);
    DecSmem& sm = smb.a;
    DecCtx c(p, G, spin, sm, reinterpret_cast<bf16_t*>(dec_smem_raw + sizeof(DecSmemB)), nullptr);
    const rt_drop nodrop(0.f, 0u);
    const int F = c.F, NL = p.n_layers;

    for (int l = NL - 1; l >= 0; --l) {
        const rt_decoder_layer_bwd& L = p.layer[l];
        // ---- requests that depend on nothing computed here
        u32x4 wA[DEC_NT][2];          // workers: linear2^T tiles
        u32x4 wf[16];                 // core: linear1^T
        if (!c.core) {
#pragma unroll
            for (int i = 0; i < DEC_NT; ++i) {
                const int tile = c.wk + i * c.NW;
                if (tile < c.f_tiles) dec_load_w<2>(L.WT2, DEC_E, tile * 16, wA[i]);
            }
        } else {
            dec_load_w<16>(L.WT1, F, c.n0, wf);
        }
        // ================= B1: LayerNorm3 backward
        {
            const DecLnbSrc src{L.dnorm, nullptr, l + 1 < NL ? LL_U3 : -1, c.tag(l + 1, 6)};
            dec_lnb_rows(c, src, L.u3, L.mean3, L.rstd3, L.g3, c.drop(L.seed_d3), sm.ln32, (bf16_t*)L.du3b, L.part3, smb.pstage);
        }
        __syncthreads();
        if (!c.core) {
            // ================= B2 (workers): dhdn = gate(du3b W2) / (1 - p)
            if (c.wk < c.f_tiles) {
#pragma unroll
                for (int i = 0; i < DEC_NT; ++i) {
                    const int tile = c.wk + i * c.NW;
                    if (tile < c.f_tiles) {
                        dec_tile<2>(c, wA[i], c.ldE, tile * 16, [&](int m, int n, f32x4 v) {
                            dec_epi_bf16(c, LL_HDN, c.tag(l, 0), m * F + n, v, nullptr, DecAct{false, L.hdn, p.gate_scale}, nodrop, 0, L.dhdn);
                        });
                    }
                }
            }
            // ================= B6 (workers): attention backward of (b, h) = worker id, + number of workers, ...
            if (c.wk < c.n_bh) {
                const rt_drop d_ad2 = c.drop(L.seed_ad2);
                Q1KV kv;
                for (int bh = c.wk; bh < c.n_bh; bh += c.NW) {
                    dec_kv_prefetch(p, L, bh, kv);
                    dec_attn_bwd(c, p, L, l, bh, kv, d_ad2);
                    __syncthreads();
                }
            }
            continue;
        }
        // ================= B3 (core): dt2 = du3 + dhdn W1
        ll_rows_to_lds<16>(c, LL_HDN, c.tag(l, 0), F);
        __syncthreads();
        dec_tile<16>(c, wf, c.ldF, c.n0, [&](int m, int n, f32x4 v) { dec_epi_res(c, LL_U, c.tag(l, 1), m, n, v, nullptr, nodrop, nullptr); });
        // ================= B4: LayerNorm2 backward; B5: do2 = du2b Wo2
        dec_product<2>(c, L.WTo2, nullptr, [&] {
            const DecLnbSrc src{nullptr, nullptr, LL_U, c.tag(l, 1)};
            dec_lnb_rows(c, src, L.u2, L.mean2, L.rstd2, L.g2, c.drop(L.seed_d2), smb.res2, (bf16_t*)L.du2b, L.part2, smb.pstage);
        }, [&](int m, int n, f32x4 v, const f32x4*) {
            dec_epi_bf16(c, LL_O2, c.tag(l, 2), m * DEC_E + n, v, nullptr, DecAct{}, nodrop, 0, nullptr);
        });
        // ================= B8: dt1q = dq2 Wq, accumulated into d query_pos
        dec_product<2>(c, L.WTq, nullptr, [&] { ll_rows_to_lds<4>(c, LL_Q2, c.tag(l, 3), DEC_E); }, [&](int m, int n, f32x4 v, const f32x4*) {
            ll_put_f32x4(c.ll, LL_U2, c.tag(l, 4), m * DEC_E + n, v);
            f32x4* acc = reinterpret_cast<f32x4*>(p.dqpos + m * DEC_E + n);
            *acc += v;
        });
        // ================= B9: LayerNorm1 backward of (du2 + dt1q); B10: dv = head-mask(dub Wo)
        const rt_drop d_ad = c.drop(L.seed_ad);
        dec_product<2>(c, L.WTo, nullptr, [&] {
            const DecLnbSrc src{nullptr, &smb.res2[0][0], LL_U2, c.tag(l, 4)};
            dec_lnb_rows(c, src, L.u, L.mean1, L.rstd1, L.g1, c.drop(L.seed_d1), sm.ln32, (bf16_t*)L.dub, L.part1, smb.pstage);
        }, [&](int m, int n, f32x4 v, const f32x4*) {
            dec_epi_bf16(c, LL_O, c.tag(l, 5), m * DEC_E + n, v, nullptr, DecAct{}, d_ad, 5, L.dv);
        });
        // ================= B11: dta = du + dv Wv: to B1 of the layer below, from the first layer to memory
        dec_product<2>(c, L.WTv, nullptr, [&] { ll_rows_to_lds<4>(c, LL_O, c.tag(l, 5), DEC_E); }, [&](int m, int n, f32x4 v, const f32x4*) {
            dec_epi_res(c, l > 0 ? LL_U3 : -1, c.tag(l, 6), m, n, v, nullptr, nodrop, l > 0 ? nullptr : p.dta);
        });
    }
    // ---- the launch epoch moves on once nothing of this launch can still be read: workgroup 0 finished the first layer's B11 after
    // every hand-off it consumed; the other workgroups' last reads are of tags it has seen complete ...
    if (c.writer) {
        __syncthreads();
        if (c.t == 0) p.handoff[0] = c.epoch + 1;
    }
}

int g_spin_override = 0;              // rt_decoder_set_spin (tests force a hand-off timeout with 1)
int dec_spin() {
    static const int v = getenv("REFTR_DEC_SPIN") ? atoi(getenv("REFTR_DEC_SPIN")) : (1 << 20);
    return g_spin_override > 0 ? g_spin_override : v;
}
unsigned* dec_trace_buf() {           // REFTR_DEC_TRACE=1: 1024 words, read back by rt_decoder_trace
    static unsigned* buf = nullptr;
    static const int on = getenv("REFTR_DEC_TRACE") ? atoi(getenv("REFTR_DEC_TRACE")) : 0;
    static bool tried = false;
    if (on && !tried) {
        tried = true;
        if (hipMalloc(&buf, 4096) != hipSuccess) { buf = nullptr; (void)hipGetLastError(); } else (void)hipMemset(buf, 0, 4096);
    }
    return buf;
}
int dec_groups() {
    static const int g = getenv("REFTR_DEC_G") ? atoi(getenv("REFTR_DEC_G")) : 80;
    return g;
}
// what both kernels can run: the 256-wide model with 8 heads, M <= 16 rows, S <= 768 keys, F = 2048 spread over the workers
int dec_geometry(int M, int H, int S, int F, int ldkv) {
    const int G = dec_groups();
    if (G <= DEC_CORE || G > 144) return RT_ERR_UNSUPPORTED;
    if (M < 1 || M > 16 || H * 32 != DEC_E || S < 1 || S > 256 * Q1_MAXK) return RT_ERR_UNSUPPORTED;
    if (F != 2048 || (F >> 4) > DEC_NT * (G - DEC_CORE) || (ldkv & 7)) return RT_ERR_UNSUPPORTED;
    return RT_OK;
}
// dynamic LDS of the two kernels: their structure + the [16][F + 8] bf16 operand rows
size_t dec_lds_fwd(int F) { return sizeof(DecSmem) + (size_t)16 * (F + 8) * 2; }
size_t dec_lds_bwd(int F) { return sizeof(DecSmemB) + (size_t)16 * (F + 8) * 2; }
// Co-residency of the G spin-waiting workgroups is a REQUIREMENT of both kernels (a consumer polls a producer that must be running).
// They are launched with plain launches (a cooperative launch costs +17-20 us per replay and applies no check under graph replay
// anyway, MI355X_MICROARCH.md "Residency and cooperative launch"), so the check is made here, once per device: the occupancy query
// must admit at least one workgroup of each kernel per compute unit at its dynamic LDS size, and the device must have at least 2 G
// compute units (a margin of 2x against the query being one block per CU high and against other streams' resident workgroups:
// the BERT branch runs beside the decoder).  Anything else answers RT_ERR_UNSUPPORTED and the caller keeps the launched chain.
// This is also where both kernels are opted into the full 160 KiB of dynamic LDS: every launch comes behind it.
int dec_residency_ok(int F) {
    static int cached_dev = -1, cached_F = 0, cached = RT_ERR_UNSUPPORTED;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return RT_ERR_UNSUPPORTED;
    if (dev == cached_dev && F == cached_F) return cached;
    const int G = dec_groups();
    hipDeviceProp_t prop;
    int rc = RT_OK;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) rc = RT_ERR_UNSUPPORTED;
    else {
        int nf = 0, nb = 0;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(decoder_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(decoder_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nf, decoder_fwd_kernel, 256, dec_lds_fwd(F)) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, decoder_bwd_kernel, 256, dec_lds_bwd(F)) != hipSuccess) { (void)hipGetLastError(); rc = RT_ERR_UNSUPPORTED; }
        else if (nf < 1 || nb < 1 || prop.multiProcessorCount < 2 * G) rc = RT_ERR_UNSUPPORTED;
    }
    cached_dev = dev; cached_F = F; cached = rc;
    return rc;
}
// the checks both entry points make behind their pointer checks, in this order: the layer count, the geometry, the device
template <class Desc>
int dec_launchable(const Desc* d) {
    if (d->n_layers < 1 || d->n_layers > RT_DEC_MAX_LAYERS) return RT_ERR_UNSUPPORTED;
    return dec_geometry(d->M, d->H, d->S, d->F, d->ldkv);
}

}  // namespace

extern "C" int rt_decoder_fwd(const rt_decoder_fwd_desc* d, rt_stream_t stream) {
    if (!d || !d->t32 || !d->t16 || !d->qpos || !d->handoff) return RT_ERR_BADARG;
    if (dec_launchable(d) != RT_OK) return RT_ERR_UNSUPPORTED;
    for (int l = 0; l < d->n_layers; ++l) {
        const rt_decoder_layer_fwd& L = d->layer[l];
        if (!L.Wv || !L.Wo || !L.Wq || !L.Wo2 || !L.W1 || !L.W2 || !L.k2 || !L.v2 || !L.o || !L.u || !L.q2 || !L.o2 || !L.u2 ||
            !L.hdn || !L.u3 || !L.lse2 || !L.t1q16 || !L.t2_16 || !L.t3_16) return RT_ERR_BADARG;
    }
    if (dec_residency_ok(d->F) != RT_OK) return RT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(decoder_fwd_kernel, dim3(dec_groups()), dim3(256), dec_lds_fwd(d->F), (hipStream_t)stream, *d, dec_groups(), dec_spin(),
                       dec_trace_buf());
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_decoder_bwd(const rt_decoder_bwd_desc* d, rt_stream_t stream) {
    if (!d || !d->dta || !d->dqpos || !d->handoff) return RT_ERR_BADARG;
    if (dec_launchable(d) != RT_OK) return RT_ERR_UNSUPPORTED;
    for (int l = 0; l < d->n_layers; ++l) {
        const rt_decoder_layer_bwd& L = d->layer[l];
        if (!L.WT2 || !L.WT1 || !L.WTo2 || !L.WTq || !L.WTo || !L.WTv || !L.g1 || !L.g2 || !L.g3 || !L.u || !L.u2 || !L.u3 || !L.mean1 ||
            !L.rstd1 || !L.mean2 || !L.rstd2 || !L.mean3 || !L.rstd3 || !L.hdn || !L.q2 || !L.k2 || !L.v2 || !L.o2 || !L.lse2 || !L.dnorm ||
            !L.du3b || !L.dhdn || !L.du2b || !L.dq2 || !L.dub || !L.dv || !L.dk2 || !L.dv2 || (!L.dk2p != !L.dv2p) ||
            (L.dk2p && (d->ldkvp < DEC_E || (d->ldkvp & 7)))) return RT_ERR_BADARG;
    }
    if (dec_residency_ok(d->F) != RT_OK) return RT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(decoder_bwd_kernel, dim3(dec_groups()), dim3(256), dec_lds_bwd(d->F), (hipStream_t)stream, *d, dec_groups(), dec_spin());
    RT_CHECK_LAUNCH();
    return RT_OK;
}

/* RT_OK when the cooperative decoder launches may be used on the current device (see dec_residency_ok), else RT_ERR_UNSUPPORTED. */
extern "C" int rt_decoder_supported(int F) {
    if (dec_geometry(1, DEC_E / 32, 1, F, 0) != RT_OK) return RT_ERR_UNSUPPORTED;
    return dec_residency_ok(F);
}

/* Overrides the number of polls a consumer makes before it gives up and raises the failure word (<= 0: back to REFTR_DEC_SPIN /
   the default 2^20).  Tests use 1 to force a timeout. */
extern "C" int rt_decoder_set_spin(int spin) { g_spin_override = spin; return RT_OK; }

/* debugging aid (REFTR_DEC_TRACE=1): copies the 1024 stage time stamps of the last launch (100 MHz ticks; words 0.. = workgroup 0,
   words 512.. = the last workgroup) to `out`; returns RT_ERR_UNSUPPORTED when tracing is off. */
extern "C" int rt_decoder_trace(uint32_t* out) {
    unsigned* b = dec_trace_buf();
    if (!b) return RT_ERR_UNSUPPORTED;
    if (!out) return RT_OK;                  // allocation only (call once before any stream capture)
    if (hipDeviceSynchronize() != hipSuccess) return RT_ERR_BADARG;
    return (int)hipMemcpy(out, b, 4096, hipMemcpyDeviceToHost);
}
