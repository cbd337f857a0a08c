// Optimizer side of the step (engine_vg.py:62-67, main_vg.py:234-268) over ONE flat fp32 parameter buffer:
//   rt_sqnorm      global L2 norm^2 of the flat gradient (clip_grad_norm_'s total norm)
//   rt_adamw_flat  gradient scale (1/world) + clip coefficient + decoupled-weight-decay AdamW, 28 B/param of
//                  HBM traffic in a single streaming pass, per-range learning rates (param groups)
//   rt_grad_accum  the gradients of k micro-batches averaged in a second flat buffer before the one clip + update of the window
#include "rt_common.h"
#include <stdlib.h>

namespace {

// s + |v|^2, summed in the order each element type's norm has always used (the order is part of the result's bits)
__device__ __forceinline__ float sq_add(float s, f32x4 v) { return s + (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]); }
__device__ __forceinline__ float sq_add(float s, bf16x8 v) {
#pragma unroll
    for (int c = 0; c < 8; ++c) { const float f = (float)v[c]; s += f * f; }
    return s;
}
// T = float (V = f32x4) or bf16_t (V = bf16x8): 16-byte loads, the ragged tail one element at a time, one atomic per workgroup
template <class T, class V>
__global__ __launch_bounds__(256) void sqnorm_kernel(const T* __restrict__ g, size_t n, float* __restrict__ out) {
    constexpr int W = sizeof(V) / sizeof(T);
    __shared__ float sm[16];
    float s = 0.f;
    const size_t nv = n / W;
    const V* gv = reinterpret_cast<const V*>(g);
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) s = sq_add(s, gv[i]);
    for (size_t i = nv * W + blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const float f = (float)g[i]; s += f * f; }
    s = rt_block_sum(s, sm);
    if (threadIdx.x == 0) atomicAdd(out, s);
}

// ---- what every update kernel shares: the launch's coefficients, the range lookup, the gradient load, one rule per optimizer
// and the four-element step.  The flat, the chunk and the matrix kernels all call adam_elem: one definition of the arithmetic,
// inlined into three loops, each of which keeps the rounding it had (profiles/optim_unify_bits.txt).
struct AdamCoef { float gs, bc1, inv_sqrt_bc2; };
// grad_scale x clip coefficient (clip_grad_norm_: skipped when max_norm <= 0); the launch's first thread stores the total norm
__device__ __forceinline__ float clip_scale(const rt_adamw_desc& p) {
    const float total = sqrtf(p.gnorm_sq ? p.gnorm_sq[0] : 0.f) * p.grad_scale;
    float coef = 1.f;
    if (p.max_norm > 0.f) coef = fminf(1.f, p.max_norm / (total + 1e-6f));
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.gnorm_out) p.gnorm_out[0] = total;
    return p.grad_scale * coef;
}
__device__ __forceinline__ AdamCoef adam_coef(const rt_adamw_desc& p) {
    AdamCoef c;
    c.gs = clip_scale(p);
    const int step = p.step_dev ? p.step_dev[0] : p.step;
    c.bc1 = 1.f - powf(p.beta1, (float)step);
    c.inv_sqrt_bc2 = rsqrtf(1.f - powf(p.beta2, (float)step));
    return c;
}
__device__ __forceinline__ void adam_range(const rt_adamw_desc& p, size_t e, float& lr, float& wd) {
    lr = 0.f; wd = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r)
        if (r < p.n_ranges && e >= (size_t)p.range_begin[r] && e < (size_t)p.range_end[r]) {
            lr = p.lr_dev ? p.lr_dev[r] : p.range_lr[r]; wd = p.range_wd[r];
        }
}
// NT: streamed once per step -- do not displace the activations / operands in L2 and the MALL
template <bool NT>
__device__ __forceinline__ f32x4 ld4(const float* q) {
    const f32x4* q4 = reinterpret_cast<const f32x4*>(q);
    return NT ? __builtin_nontemporal_load(q4) : *q4;
}
template <bool NT>
__device__ __forceinline__ void st4(float* q, f32x4 v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(q)); else *reinterpret_cast<f32x4*>(q) = v;
}
// the four gradients at element e (a multiple of 4): from g (policy NT), or from its bf16 twin g16 (policy NT16) when the descriptor has one
template <bool NT, bool NT16>
__device__ __forceinline__ f32x4 grad4(const float* g, const bf16_t* g16, size_t e) {
    if (g16) {
        const bf16x4* q = reinterpret_cast<const bf16x4*>(g16 + e);
        const bf16x4 h = NT16 ? __builtin_nontemporal_load(q) : *q;
        return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    } else return ld4<NT>(g + e);
}
// AdamW with decoupled weight decay: the update of one element, the ONLY statement of this arithmetic.  What the plain text does not
// fix is which products the compiler fuses into the adds (fp-contract): that depends on the loop it is inlined into, and the
// kernels have always differed in it by an ulp -- the chunk kernel rounds m = fma(b1, m, (1 - b1) g), adamw_mat_kernel
// m = fma(1 - b1, g, b1 m), its element-wise path adds the two rounded products of v.  Those two keep the plain text and, with it, their
// bits.  FLAT is the flat pass: sharing the chunk kernel's step it would take over the chunk kernel's rounding, so the rounding its
// own loop had -- m = fma(1 - b1, g, b1 m), v = fma(g, (1 - b2) g, b2 v) -- is written out (profiles/optim_unify_bits.txt).
template <bool FLAT = false>
__device__ __forceinline__ void adam_elem(const rt_adamw_desc& p, const AdamCoef& c, float lr, float wd, float graw, float& pv, float& mv, float& vv) {
    const float g = graw * c.gs;
    if (FLAT) {
#pragma clang fp contract(off)
        mv = __builtin_fmaf(1.f - p.beta1, g, p.beta1 * mv);
        vv = __builtin_fmaf(g, (1.f - p.beta2) * g, p.beta2 * vv);
        const float denom = __builtin_fmaf(sqrtf(vv), c.inv_sqrt_bc2, p.eps);
        pv = __builtin_fmaf(__builtin_fmaf(-lr, wd, 1.f), pv, -((lr / c.bc1) * (mv / denom)));
    } else {
        pv *= (1.f - lr * wd);
        mv = p.beta1 * mv + (1.f - p.beta1) * g;
        vv = p.beta2 * vv + (1.f - p.beta2) * g * g;
        const float denom = sqrtf(vv) * c.inv_sqrt_bc2 + p.eps;
        pv -= (lr / c.bc1) * (mv / denom);
    }
}
// torch.optim.SGD(momentum, weight_decay) as the reference builds it with --sgd (main_vg.py:263-265: momentum 0.9, dampening 0, no
// Nesterov): g' = clip * scale * g + wd * p;  buf = momentum * buf + g'  (a zero-initialised buffer makes step 1 "buf = g'");
// p -= lr * buf.  Same descriptor as AdamW: m = momentum buffer, beta1 = momentum, v / beta2 / eps unused.  20 B per parameter.
// One kernel only, so its fused multiply-adds are written out (wd * p is the product that is rounded on its own).
__device__ __forceinline__ void sgd_elem(const rt_adamw_desc& p, const AdamCoef& c, float lr, float wd, float graw, float& pv, float& mv) {
#pragma clang fp contract(off)
    mv = __builtin_fmaf(p.beta1, mv, __builtin_fmaf(graw, c.gs, wd * pv));
    pv = __builtin_fmaf(-lr, mv, pv);
}
// the rule of a four-element step: AdamW as the chunk kernel applies it, AdamW as the flat pass rounds it, SGD
enum { RULE_ADAMW, RULE_ADAMW_FLAT, RULE_SGD };
template <int RULE>
__device__ __forceinline__ AdamCoef opt_coef(const rt_adamw_desc& p) { return RULE == RULE_SGD ? AdamCoef{clip_scale(p), 1.f, 1.f} : adam_coef(p); }
// the four elements at e: load p / m / v / g, apply the rule, store (NT: m, v and g both ways and the load of p; p is stored plain;
// the flat AdamW pass reads the bf16 twin non-temporally under either policy, as it always has)
template <int RULE, bool NT>
__device__ __forceinline__ void opt_step4(const rt_adamw_desc& p, const AdamCoef& cf, size_t e) {
    constexpr bool SGD = RULE == RULE_SGD;
    float lr, wd;
    adam_range(p, e, lr, wd);
    f32x4 pv = ld4<NT>(p.p + e), mv = ld4<NT>(p.m + e), vv = {0.f, 0.f, 0.f, 0.f};
    if (!SGD) vv = ld4<NT>(p.v + e);
    const f32x4 gv = grad4<NT, NT || RULE == RULE_ADAMW_FLAT>(p.g, reinterpret_cast<const bf16_t*>(p.g16), e);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float a = pv[c], b = mv[c], d = vv[c];
        if (SGD) sgd_elem(p, cf, lr, wd, gv[c], a, b); else adam_elem<RULE == RULE_ADAMW_FLAT>(p, cf, lr, wd, gv[c], a, b, d);
        pv[c] = a; mv[c] = b; vv[c] = d;
    }
    st4<false>(p.p + e, pv); st4<NT>(p.m + e, mv);
    if (!SGD) st4<NT>(p.v + e, vv);
}

// rt_adamw_flat (RULE_ADAMW_FLAT) and rt_sgd_flat (RULE_SGD): the rule over the span [span_begin, span_end), grid-strided.  Both rules
// keep this name, because the trace tools find the update by it: in a trace, adamw_kernel<2, false> is SGD.
template <int RULE, bool NT>
__global__ __launch_bounds__(256) void adamw_kernel(const rt_adamw_desc p) {
    if (p.active && p.active[0] == 0) return;
    const AdamCoef cf = opt_coef<RULE>(p);
    const size_t i0 = (size_t)p.span_begin >> 2, n4 = (size_t)p.span_end >> 2;
    for (size_t i = i0 + blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) opt_step4<RULE, NT>(p, cf, i << 2);
}

// ------------------------------------------------------------------------------------------------
// Matrix-aware AdamW (round 4): the same update, walked per WEIGHT MATRIX in 64(n) x 64(c) tiles per tap, so that the kernel that
// produces the new fp32 master also emits the bf16 GEMM operands the next forward / backward read -- W [N][T][C] (x FrozenBN scale)
// and its transpose [C][T][N] -- while the new values are still in registers.  The separate operand refresh (rt_weight_prep_batched:
// re-reads 4 B per parameter, one more dependent launch at the head of the step) disappears; the arithmetic is adam_elem, the
// rounding points of the operands those of weight_prep_batched_kernel.  Everything that is not a matrix job (biases, norm
// parameters, embeddings) is updated by adamw_chunks_kernel over a static chunk table (the complement of the jobs).
// table: int64 [njobs][8] = {element offset of the matrix in p/g/m/v, scale ptr | 0, dst ptr | 0, dst_t ptr | 0, N, T, C, first tile}
// A matrix [N][T][C] is walked as the 2-D array [N][K'] (K' = T * C: a row is contiguous) in tiles of 32 rows x 256 columns: a wave
// reads / writes ONE KB-contiguous row piece per instruction in each of p, g, m, v (the first version used 64 x 64 tiles -- 256-byte
// pieces from four arrays -- and ran at 3.2-4.1 TB/s against the flat pass's 6: a DRAM page was opened for a quarter of its bytes).
// The bf16 copy W goes out in the same pass (512 contiguous bytes per wave); the transposed copy [C][T][N] is staged through LDS and
// written by one thread per column as the 64 contiguous bytes of its 32 rows.
constexpr int AM_TN = 32, AM_TK = 256, AM_LD = AM_TK + 4;
__global__ __launch_bounds__(256) void adamw_mat_kernel(const rt_adamw_desc p, const int64_t* __restrict__ table, int njobs) {
    if (p.active && p.active[0] == 0) return;
    __shared__ __attribute__((aligned(16))) bf16_t tile[AM_TN][AM_LD];
    const AdamCoef cf = adam_coef(p);
    const int64_t* j = table + rt_job_of(table, njobs, blockIdx.x) * 8;
    const size_t base = (size_t)j[0];
    bf16_t* dst = reinterpret_cast<bf16_t*>(j[2]);
    bf16_t* dst_t = reinterpret_cast<bf16_t*>(j[3]);
    // Sparse-state jobs (round 4): a matrix WITHOUT bf16 operands (the embedding tables: 24 M of BERT's parameters, of which a step
    // touches <= B * L rows) may carry, in the otherwise unused scale slot, one byte per KB row piece: 0 = "m and v of this piece
    // are all zero".  A piece whose gradient is all zero too is then left alone WITHOUT reading p / m / v -- bit-exact, because with
    // g = m = v = 0 the update is p *= (1 - lr * wd) and nothing else, and the skip is only taken when that factor rounds to 1.0f
    // (lr_bert * wd = 1e-9 in every reference config: models the reference's own fp32 no-op).  4 B instead of 32 B per element.
    uint8_t* flags = (!dst && !dst_t && j[1]) ? reinterpret_cast<uint8_t*>(j[1]) : nullptr;
    const float* scale = flags ? nullptr : reinterpret_cast<const float*>(j[1]);
    const int N = (int)j[4], T = (int)j[5], C = (int)j[6];
    const int K = T * C;
    const int local = blockIdx.x - (int)j[7];
    const int kt = (K + AM_TK - 1) / AM_TK;
    const int tk = local % kt, tn = local / kt;        // column tiles fastest: neighbouring workgroups stream neighbouring KBs of the same rows
    const int n0 = tn * AM_TN, k0 = tk * AM_TK;
    float lr, wd;
    adam_range(p, base, lr, wd);                      // a matrix lies inside one learning-rate range
    float* P = p.p + base; float* Mo = p.m + base; float* Vo = p.v + base;
    const float* G = p.g ? p.g + base : nullptr;
    const bf16_t* G16 = p.g16 ? reinterpret_cast<const bf16_t*>(p.g16) + base : nullptr;
    const int t = threadIdx.x;
    const bool vec = (K & 3) == 0 && (base & 3) == 0 && (!dst || ((uintptr_t)dst & 7) == 0);
    if (vec) {
        const int r = t >> 6, q = (t & 63) * 4, k = k0 + q;
        const bool may_skip = flags && (1.f - lr * wd) == 1.f;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 pv[4], gv[4], mv[4], vv[4];
            bool ok[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int n = n0 + (half * 4 + jj) * 4 + r;
                ok[jj] = n < N && k < K;
                if (ok[jj]) {                       // (not grad4: inlined here it costs the kernel 60 VGPRs and an occupancy step)
                    const size_t o = (size_t)n * K + k;
                    if (G16) {
                        const bf16x4 h = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(G16 + o));
                        gv[jj] = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                    } else gv[jj] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(G + o));
                }
            }
            if (flags) {
                // a wave = one KB row piece (row n, column tile tk): the decisions below are wave-uniform
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int n = n0 + (half * 4 + jj) * 4 + r;
                    const bool nz = ok[jj] && (gv[jj][0] != 0.f || gv[jj][1] != 0.f || gv[jj][2] != 0.f || gv[jj][3] != 0.f);
                    const bool g_zero = __ballot(nz) == 0;
                    if (n < N && may_skip && g_zero && flags[(size_t)n * kt + tk] == 0) ok[jj] = false;      // nothing to do for this piece
                }
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int n = n0 + (half * 4 + jj) * 4 + r;
                if (ok[jj]) {
                    const size_t o = (size_t)n * K + k;
                    pv[jj] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + o));
                    mv[jj] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Mo + o));
                    vv[jj] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Vo + o));
                }
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int nl = (half * 4 + jj) * 4 + r, n = n0 + nl;
                bf16x4 ov = bf16x4{(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
                if (ok[jj]) {
                    const size_t o = (size_t)n * K + k;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { float a = pv[jj][e], b = mv[jj][e], d = vv[jj][e]; adam_elem(p, cf, lr, wd, gv[jj][e], a, b, d); pv[jj][e] = a; mv[jj][e] = b; vv[jj][e] = d; }
                    *reinterpret_cast<f32x4*>(P + o) = pv[jj];
                    __builtin_nontemporal_store(mv[jj], reinterpret_cast<f32x4*>(Mo + o));
                    __builtin_nontemporal_store(vv[jj], reinterpret_cast<f32x4*>(Vo + o));
                    if (flags) {                       // the state of this piece after the update (wave-uniform: ok[jj] is, within a row piece, except past K)
                        bool live = false;
#pragma unroll
                        for (int e = 0; e < 4; ++e) live = live || mv[jj][e] != 0.f || vv[jj][e] != 0.f;
                        const bool any_live = __ballot(live) != 0;
                        if ((t & 63) == 0) flags[(size_t)n * kt + tk] = any_live ? 1 : 0;
                    }
                    const float sc = scale ? scale[n] : 1.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) ov[e] = (bf16_t)(scale ? pv[jj][e] * sc : pv[jj][e]);
                    if (dst) *reinterpret_cast<bf16x4*>(dst + o) = ov;
                }
                if (dst_t) *reinterpret_cast<bf16x4*>(&tile[nl][q]) = ov;
            }
        }
    } else {                                          // ragged / misaligned matrices: element-wise over the same tile
        for (int idx = t; idx < AM_TN * AM_TK; idx += 256) {
            const int nl = idx / AM_TK, kk = idx - nl * AM_TK, n = n0 + nl, k = k0 + kk;
            float w = 0.f;
            if (n < N && k < K) {
                const size_t o = (size_t)n * K + k;
                float pv = P[o], mv = Mo[o], vv = Vo[o];
                const float gv = G16 ? (float)G16[o] : G[o];
                adam_elem(p, cf, lr, wd, gv, pv, mv, vv);
                P[o] = pv; Mo[o] = mv; Vo[o] = vv;
                w = scale ? pv * scale[n] : pv;
                if (dst) dst[o] = (bf16_t)w;
            }
            if (dst_t) tile[nl][kk] = (bf16_t)w;
        }
    }
    if (!dst_t) return;
    __syncthreads();
    const int k = k0 + t;                              // one column of the tile per thread: 32 rows = 64 contiguous bytes of dst_t
    if (k >= K) return;
    const int c = k % C, tap = k / C;
    bf16_t* out = dst_t + ((size_t)c * T + tap) * N + n0;
    const bool vec_n = (N & 7) == 0 && ((uintptr_t)dst_t & 15) == 0;
#pragma unroll
    for (int g8 = 0; g8 < AM_TN / 8; ++g8) {
        if (n0 + g8 * 8 >= N) break;
        if (vec_n) {                                   // N % 8 == 0: the 8 rows exist
            bf16x8 ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = tile[g8 * 8 + e][t];
            *reinterpret_cast<bf16x8*>(out + g8 * 8) = ov;
        } else {
            for (int e = 0; e < 8 && n0 + g8 * 8 + e < N; ++e) out[g8 * 8 + e] = tile[g8 * 8 + e][t];
        }
    }
}

// everything that is not a matrix job: table = nchunks x {int64 element offset (multiple of 4), int64 count (multiple of 4, <= 16384)}
__global__ __launch_bounds__(256) void adamw_chunks_kernel(const rt_adamw_desc p, const int64_t* __restrict__ table) {
    if (p.active && p.active[0] == 0) return;
    const AdamCoef cf = adam_coef(p);
    rt_chunk_walk<true>(table, [&](size_t e) { opt_step4<RULE_ADAMW, false>(p, cf, e); }, [](size_t) {});
}

// ---- gradient-norm accumulator (rt_common.h): passes over whole buffers / chunk tables, and the final sum of the slots
// A pass over up to 32 whole buffers (rt_sq_pass, rt_round_pass; L = SqList or RoundList): first[b] = the first workgroup of buffer
// b, 4096 elements per workgroup.  list_buffer finds the workgroup's buffer b; list_walk calls vec4(i) for every four elements
// i .. i + 3 of the workgroup's piece that the buffer still holds, one(k) for the elements of a ragged tail.
struct SqList { const float* buf[32]; long long cnt[32]; float sign[32]; int first[33]; int n; };
struct RoundList { const float* buf[32]; bf16_t* twin[32]; long long cnt[32]; int first[33]; int n; };
template <class L>
__device__ __forceinline__ int list_buffer(const L& l) { return rt_job_of(l.first, l.n, (int)blockIdx.x); }
template <class L, class V, class S>
__device__ __forceinline__ void list_walk(const L& l, int b, V vec4, S one) {
    const size_t n = (size_t)l.cnt[b];
    const size_t b0 = (size_t)((int)blockIdx.x - l.first[b]) * 4096;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t i = b0 + (size_t)j * 1024 + threadIdx.x * 4;
        if (i + 4 <= n) vec4(i);
        else for (size_t k = i; k < n; ++k) one(k);
    }
}
__global__ __launch_bounds__(256) void sq_list_kernel(const SqList l, float* __restrict__ slots) {
    __shared__ float sm[16];
    const int b = list_buffer(l);
    const float* g = l.buf[b];
    float s = 0.f;
    list_walk(l, b, [&](size_t i) { s = sq_add(s, *reinterpret_cast<const f32x4*>(g + i)); }, [&](size_t k) { s += g[k] * g[k]; });
    s = rt_block_sum(s, sm);
    if (threadIdx.x == 0) rt_sq_add(slots, blockIdx.x, l.sign[b] * s);
}
__global__ __launch_bounds__(256) void round_list_kernel(const RoundList l) {
    const int b = list_buffer(l);
    const float* g = l.buf[b]; bf16_t* tw = l.twin[b];
    list_walk(l, b, [&](size_t i) { rt_store_bf16(tw + i, *reinterpret_cast<const f32x4*>(g + i)); }, [&](size_t k) { tw[k] = (bf16_t)g[k]; });
}
// the tensors that are accumulated with atomics (the complement of the weight matrices): table = n x {element offset, count <= 16384}
__global__ __launch_bounds__(256) void sq_chunks_kernel(const float* __restrict__ base, const int64_t* __restrict__ table, float* __restrict__ slots) {
    __shared__ float sm[16];
    float s = 0.f;
    rt_chunk_walk<false>(table, [&](size_t e) { s = sq_add(s, *reinterpret_cast<const f32x4*>(base + e)); },
                         [&](size_t e) { s += base[e] * base[e]; });
    s = rt_block_sum(s, sm);
    if (threadIdx.x == 0) rt_sq_add(slots, blockIdx.x, s);
}
__global__ __launch_bounds__(256) void sq_sum_kernel(const float* __restrict__ slots, float* __restrict__ out, const float* __restrict__ extra) {
    __shared__ float sm[16];
    float s = slots[(size_t)threadIdx.x * RT_SQ_STRIDE];
    s = rt_block_sum(s, sm);
    if (threadIdx.x == 0) out[0] = fmaxf(s, 0.f) + (extra ? extra[0] : 0.f);      // (new^2 - old^2 terms may leave -1 ulp when everything is zero)
}
__global__ __launch_bounds__(256) void round_chunks_kernel(const float* __restrict__ base, bf16_t* __restrict__ twin, const int64_t* __restrict__ table) {
    rt_chunk_walk<false>(table, [&](size_t e) { rt_store_bf16(twin + e, *reinterpret_cast<const f32x4*>(base + e)); },
                         [&](size_t e) { twin[e] = (bf16_t)base[e]; });
}

// (the unconditional counter keeps its own kernel: as the conditional one with a null condition it measured slower than its bar)
__global__ void counter_add_kernel(int32_t* c, int32_t inc) { c[0] += inc; }
__global__ void counter_add_if_zero_kernel(int32_t* c, int32_t inc, const uint32_t* cond, int reset_else) {
    if (cond[0] == 0u) c[0] += inc; else if (reset_else) c[0] = 0;
}
__global__ void stamp_kernel(uint64_t* buf, int idx) { buf[idx] = wall_clock64(); }
// the end of an iteration in deferred mode, decided on the device: the update is armed (and the step counter advanced) only when no
// cooperative launch failed AND the iteration's total loss is finite; then the loop's numbers (rt_finish_stats; rt_finish_step has none)
__global__ void finish_stats_kernel(const rt_finish_desc d) {
    const uint32_t cw = d.cond ? d.cond[0] : 0u;
    const bool bad = cw != 0u || (d.loss && !isfinite(d.loss[0]));
    if (!bad) { d.step[0] += 1; d.active[0] += 1; } else d.active[0] = 0;
    float gn = d.grad_norm ? d.grad_norm[0] : 0.f;
    if (d.sq) { gn = sqrtf(d.sq[0]) * d.norm_scale; if (d.grad_norm) d.grad_norm[0] = gn; }
    if (d.stats) {
        int o = 0;
        for (int i = 0; i < d.n_src; ++i) d.stats[o++] = d.src[i][0];
        if (d.cond_in_stats) d.stats[o++] = (float)cw;
        d.stats[o] = gn;
    }
}

// ---- gradient accumulation over micro-batches (rt_grad_accum): acc = g | acc += g | g = (acc + g) * s with sum g^2 of what was written.
// A pure streaming pass: 16-byte accesses over the part of the buffers where g and acc are both 16-byte aligned, the (at most 3 + 3)
// elements in front of / behind it one by one; buffers whose two misalignments differ go one element at a time altogether (head == n),
// grid-strided over as many workgroups as the vector path would use per element -- coalesced 4-byte accesses, not one workgroup's walk.
// FINISH adds and scales in double: the value written is then ONE fp32 rounding away from (acc + g) * s, whatever s is.  Its squared
// norm leaves no atomics behind: every workgroup stores its partial sum into its own slot and grad_accum_sum_kernel adds the slots in
// a fixed order, so the clip norm of a window is the same from run to run.
constexpr int GA_FIRST = 0, GA_ADD = 1, GA_FINISH = 2;
template <int MODE>
__device__ __forceinline__ float grad_accum_elem(float gv, float av, float s) {
    if (MODE == GA_FIRST) return gv;
    if (MODE == GA_ADD) return av + gv;
    return (float)(((double)av + (double)gv) * (double)s);
}
template <int MODE>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ g, float* __restrict__ acc, size_t n, size_t head,
                                                         float scale, const float* __restrict__ scale_dev, float* __restrict__ partials) {
    __shared__ float sm[16];
    const float s = (MODE == GA_FINISH && scale_dev) ? scale_dev[0] : scale;
    const size_t n4 = (n - head) >> 2;
    f32x4* G4 = reinterpret_cast<f32x4*>(g + head);
    f32x4* A4 = reinterpret_cast<f32x4*>(acc + head);
    float sq = 0.f;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 gv = __builtin_nontemporal_load(G4 + i);
        f32x4 av = f32x4{0.f, 0.f, 0.f, 0.f};
        if (MODE != GA_FIRST) av = __builtin_nontemporal_load(A4 + i);
        f32x4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = grad_accum_elem<MODE>(gv[c], av[c], s);
        if (MODE == GA_FINISH) { G4[i] = r; sq += (r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]); }
        else __builtin_nontemporal_store(r, A4 + i);
    }
    {                                                   // the unaligned head and the tail: fewer than 8 elements unless head == n
        const size_t tail0 = head + (n4 << 2), rest = head + (n - tail0);
        for (size_t j = blockIdx.x * (size_t)256 + threadIdx.x; j < rest; j += (size_t)gridDim.x * 256) {
            const size_t i = j < head ? j : tail0 + (j - head);
            const float r = grad_accum_elem<MODE>(g[i], MODE != GA_FIRST ? acc[i] : 0.f, s);
            if (MODE == GA_FINISH) { g[i] = r; sq += r * r; } else acc[i] = r;
        }
    }
    if (MODE == GA_FINISH) {
        sq = rt_block_sum(sq, sm);
        if (threadIdx.x == 0) partials[blockIdx.x] = sq;
    }
}
__global__ __launch_bounds__(256) void grad_accum_sum_kernel(const float* __restrict__ partials, int n, float* __restrict__ out) {
    __shared__ double sd[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partials[i];
    sd[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sd[threadIdx.x] += sd[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)sd[0];
}

}  // namespace

extern "C" int rt_counter_add(int32_t* ctr, int32_t inc, rt_stream_t stream) {
    if (!ctr) return RT_ERR_BADARG;
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ctr, inc);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
extern "C" int rt_counter_add_if_zero(int32_t* ctr, int32_t inc, const uint32_t* cond, int reset_else, rt_stream_t stream) {
    if (!ctr || !cond) return RT_ERR_BADARG;
    hipLaunchKernelGGL(counter_add_if_zero_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ctr, inc, cond, reset_else);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_finish_stats(const rt_finish_desc* d, rt_stream_t stream) {
    if (!d || !d->step || !d->active || d->n_src < 0 || d->n_src > RT_STATS_MAX) return RT_ERR_BADARG;
    for (int i = 0; i < d->n_src; ++i) if (!d->src[i]) return RT_ERR_BADARG;
    hipLaunchKernelGGL(finish_stats_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, *d);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
extern "C" int rt_finish_step(int32_t* step, int32_t* active, const uint32_t* cond, const float* loss, rt_stream_t stream) {
    rt_finish_desc d = {};
    d.step = step; d.active = active; d.cond = cond; d.loss = loss;
    return rt_finish_stats(&d, stream);
}

extern "C" int rt_stamp(uint64_t* buf, int idx, rt_stream_t stream) {
    if (!buf || idx < 0) return RT_ERR_BADARG;
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, buf, idx);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

// the descriptor check of all four update entries (SGD has no v and no step)
static int opt_desc_ok(const rt_adamw_desc* d, bool sgd) {
    if (!d || !d->p || (!d->g && !d->g16) || !d->m || d->n <= 0 || (d->n & 3) || d->n_ranges < 1 || d->n_ranges > 8) return RT_ERR_BADARG;
    if (!sgd && (!d->v || (d->step < 1 && !d->step_dev))) return RT_ERR_BADARG;
    for (int r = 0; r < d->n_ranges; ++r) if ((d->range_begin[r] & 3) || (d->range_end[r] & 3)) return RT_ERR_BADARG;
    return RT_OK;
}

extern "C" int rt_adamw_mat(const rt_adamw_desc* d, const int64_t* table, int njobs, int total_tiles, rt_stream_t stream) {
    const int rc = opt_desc_ok(d, false);
    if (rc != RT_OK) return rc;
    if (!table || njobs <= 0 || total_tiles <= 0) return RT_ERR_BADARG;
    hipLaunchKernelGGL(adamw_mat_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, *d, table, njobs);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_adamw_chunks(const rt_adamw_desc* d, const int64_t* table, int nchunks, rt_stream_t stream) {
    const int rc = opt_desc_ok(d, false);
    if (rc != RT_OK) return rc;
    if (!table || nchunks <= 0) return RT_ERR_BADARG;
    hipLaunchKernelGGL(adamw_chunks_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, *d, table);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

// the host side of rt_sq_pass / rt_round_pass: the n <= 32 buffers that take(l, i) accepts and stores (null / empty ones are
// skipped) with their counts and first workgroups, in one launch
template <class L, class Take, class Launch>
static int list_pass(const long long* counts, int n, Take take, Launch launch) {
    if (n > 32) return RT_ERR_BADARG;
    L l; l.n = 0; int blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (counts[i] <= 0 || !take(l, i)) continue;
        l.cnt[l.n] = counts[i]; l.first[l.n] = blocks; ++l.n;
        blocks += (int)((counts[i] + 4095) / 4096);
    }
    if (!l.n) return RT_OK;
    l.first[l.n] = blocks;
    launch(l, blocks);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
int rt_sq_pass(float* const* bufs, const long long* counts, const float* signs, int n, float* slots, hipStream_t s) {
    return list_pass<SqList>(counts, n, [&](SqList& l, int i) { l.buf[l.n] = bufs[i]; l.sign[l.n] = signs[i]; return bufs[i] != nullptr; },
                             [&](const SqList& l, int blocks) { hipLaunchKernelGGL(sq_list_kernel, dim3((unsigned)blocks), dim3(256), 0, s, l, slots); });
}
int rt_round_pass(float* const* bufs, void* const* twins, const long long* counts, int n, hipStream_t s) {
    return list_pass<RoundList>(counts, n, [&](RoundList& l, int i) { l.buf[l.n] = bufs[i]; l.twin[l.n] = (bf16_t*)twins[i]; return bufs[i] && twins[i]; },
                                [&](const RoundList& l, int blocks) { hipLaunchKernelGGL(round_list_kernel, dim3((unsigned)blocks), dim3(256), 0, s, l); });
}

extern "C" int rt_round_chunks(const float* base, void* twin, const int64_t* table, int n, rt_stream_t stream) {
    if (!base || !twin || !table || n <= 0) return RT_ERR_BADARG;
    hipLaunchKernelGGL(round_chunks_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, base, (bf16_t*)twin, table);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_sqnorm_finish(const float* base, const int64_t* table, int nchunks, float* slots, const float* extra, float* out,
                                rt_stream_t stream) {
    if (!slots || !out || (nchunks > 0 && (!base || !table))) return RT_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (nchunks > 0) {
        hipLaunchKernelGGL(sq_chunks_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, base, table, slots);
        RT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sq_sum_kernel, dim3(1), dim3(256), 0, s, slots, out, extra);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

template <class T, class V>
static int sqnorm(const void* g, int64_t n, float* out, rt_stream_t stream) {
    if (!g || !out || n <= 0) return RT_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = rt_zero_f32(out, 1, s);
    if (e != hipSuccess) return (int)e;
    int blocks = (int)(((size_t)n / (sizeof(V) / sizeof(T)) + 255) / 256); if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((sqnorm_kernel<T, V>), dim3(blocks), dim3(256), 0, s, (const T*)g, (size_t)n, out);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
extern "C" int rt_sqnorm(const float* g, int64_t n, float* out, rt_stream_t stream) { return sqnorm<float, f32x4>(g, n, out, stream); }
extern "C" int rt_sqnorm_bf16(const void* g16, int64_t n, float* out, rt_stream_t stream) { return sqnorm<bf16_t, bf16x8>(g16, n, out, stream); }

// rt_adamw_flat / rt_sgd_flat: the descriptor check, the span (0, 0 = the whole buffer) and the launch
static int flat_update(const rt_adamw_desc* d, bool sgd, rt_stream_t stream) {
    const int rc = opt_desc_ok(d, sgd);
    if (rc != RT_OK) return rc;
    rt_adamw_desc a = *d;
    if (a.span_begin == 0 && a.span_end == 0) a.span_end = a.n;
    if (a.span_begin < 0 || a.span_end > a.n || a.span_begin >= a.span_end || (a.span_begin & 3) || (a.span_end & 3)) return RT_ERR_BADARG;
    int blocks = (int)(((size_t)(a.span_end - a.span_begin) / 4 + 255) / 256); if (blocks > 4096) blocks = 4096;
    static const int nt_env = RT_TUNE("REFTR_ADAMW_NT", 1);
    auto kernel = sgd ? adamw_kernel<RULE_SGD, false> : nt_env ? adamw_kernel<RULE_ADAMW_FLAT, true> : adamw_kernel<RULE_ADAMW_FLAT, false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
extern "C" int rt_adamw_flat(const rt_adamw_desc* d, rt_stream_t stream) { return flat_update(d, false, stream); }
extern "C" int rt_sgd_flat(const rt_adamw_desc* d, rt_stream_t stream) { return flat_update(d, true, stream); }

extern "C" int rt_grad_accum(int mode, float* g, float* acc, int64_t n, float scale, const float* scale_dev, float* partials,
                             float* out_sq, rt_stream_t stream) {
    if (!g || !acc || n <= 0) return RT_ERR_BADARG;
    if (mode != GA_FIRST && mode != GA_ADD && mode != GA_FINISH) return RT_ERR_UNSUPPORTED;
    if (mode == GA_FINISH && (!partials || !out_sq)) return RT_ERR_BADARG;
    if (((uintptr_t)g & 3) || ((uintptr_t)acc & 3)) return RT_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    // elements in front of the first 16-byte boundary; the vector part needs g and acc to reach it together
    size_t head = ((16 - ((uintptr_t)g & 15)) & 15) >> 2;
    if (((uintptr_t)g & 15) != ((uintptr_t)acc & 15) || head > (size_t)n) head = (size_t)n;
    const size_t n4 = ((size_t)n - head) >> 2;
    const size_t work = n4 ? n4 : (size_t)n;            // 16-byte accesses, or (n4 == 0) single elements over the whole grid
    int blocks = (int)((work + 255) / 256); if (blocks > RT_GRAD_ACCUM_SLOTS) blocks = RT_GRAD_ACCUM_SLOTS;
    if (mode == GA_FIRST) hipLaunchKernelGGL(grad_accum_kernel<GA_FIRST>, dim3(blocks), dim3(256), 0, s, g, acc, (size_t)n, head, scale, scale_dev, partials);
    else if (mode == GA_ADD) hipLaunchKernelGGL(grad_accum_kernel<GA_ADD>, dim3(blocks), dim3(256), 0, s, g, acc, (size_t)n, head, scale, scale_dev, partials);
    else hipLaunchKernelGGL(grad_accum_kernel<GA_FINISH>, dim3(blocks), dim3(256), 0, s, g, acc, (size_t)n, head, scale, scale_dev, partials);
    RT_CHECK_LAUNCH();
    if (mode == GA_FINISH) {
        hipLaunchKernelGGL(grad_accum_sum_kernel, dim3(1), dim3(256), 0, s, partials, blocks, out_sq);
        RT_CHECK_LAUNCH();
    }
    return RT_OK;
}
