// Shared pieces of the implicit-GEMM translation units (rt_gemm.hip, rt_gemm_ksplit.hip): the launch-side argument block and
// the fused epilogues.  Internal to the library (nothing here is part of the C ABI).
#pragma once
#include "rt_common.h"

struct GemmArgs {
    const bf16_t* src; const bf16_t* wgt;
    bf16_t* out_bf16; float* out_f32; bf16_t* out_preact; float* acc2_f32;
    const float* bias; const float* res_f32; const bf16_t* res_bf16; const bf16_t* gate; const bf16_t* preact; const bf16_t* dtanh;
    int B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad, transposed, act, res_first;
    float gate_scale, drop_p; uint32_t drop_seed; int drop_shift;
    int M, K, sshift, xcd, early, epi_lds, abl, prefetch, mfast, dil;
    unsigned src_bytes, wgt_bytes;
    const uint32_t* seed_dev;
};

// dense rows: a 1x1 / stride 1 / pad 0 product whose output pixels are its input pixels (every Linear, most bottleneck convs)
static inline bool gemm_dense(const GemmArgs& a) {
    return a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 && a.SH == a.DH && a.SW == a.DW;
}

// The fused epilogue on W consecutive output features of row m:
// +bias -> store preact -> [+res] -> act -> dropout -> [+res] -> *gate -> *gelu'(preact) -> *(1 - dtanh^2) -> stores
// W = 4: one lane's piece of the MFMA C/D layout.  W = 8: the LDS-staged, row-coalesced path, where every global access is a full
// 16-B (bf16) piece of one output row and an fp32 operand is two 16-B accesses.
template <int W> using epi_f32 = __attribute__((ext_vector_type(W))) float;
template <int W> using epi_bf16 = __attribute__((ext_vector_type(W))) __bf16;
typedef epi_f32<8> f32x8;
// The operands the epilogue reads, fetched ahead of the reduction: they depend on nothing the kernel computes.  (Skinny kernel: the
// M <= 16 launches are pure latency chains -- launch -> operand loads -> MFMA -> LDS reduce -> EPILOGUE LOADS -> stores -- so they are
// requested first and cost no round trip of their own; tile kernels: their HBM latency runs under the K loop.)
// The 8-wide form holds PIECES of them per thread for a whole K loop, so it holds the bf16 residual and gate only.
template <int W> struct EpiPre { epi_bf16<W> resb, gate; };
template <> struct EpiPre<4> { f32x4 bias, res; epi_bf16<4> resb, gate, preact, dtanh; };
template <int W> static __device__ __forceinline__ epi_bf16<W> epi_ld(const bf16_t* q) { return *reinterpret_cast<const epi_bf16<W>*>(q); }
template <int W> static __device__ __forceinline__ epi_f32<W> epi_ld(const float* q) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(q);
    if constexpr (W == 4) return lo;
    else {
        const f32x4 hi = *reinterpret_cast<const f32x4*>(q + 4);
        return f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
}
// o: element offset of the piece in the output (0 for a piece that will not be stored), n: its first feature
template <int W> static __device__ __forceinline__ EpiPre<W> epi_prefetch(const GemmArgs& p, size_t o, int n) {
    EpiPre<W> e;
    if constexpr (W == 4) {
        e.bias = p.bias ? epi_ld<W>(p.bias + n) : epi_f32<W>{};
        e.res = p.res_f32 ? epi_ld<W>(p.res_f32 + o) : epi_f32<W>{};
    }
    e.resb = p.res_bf16 ? epi_ld<W>(p.res_bf16 + o) : epi_bf16<W>{};
    e.gate = p.gate ? epi_ld<W>(p.gate + o) : epi_bf16<W>{};
    if constexpr (W == 4) {
        e.preact = p.preact ? epi_ld<W>(p.preact + o) : epi_bf16<W>{};
        e.dtanh = p.dtanh ? epi_ld<W>(p.dtanh + o) : epi_bf16<W>{};
    }
    return e;
}

// PRE (compile-time): the operands EpiPre<W> can hold come from *e, fetched at the start of the workgroup.
template <int W, bool PRE = false>
static __device__ __forceinline__ void epilogue(const GemmArgs& p, int m, int n, epi_f32<W> v, const EpiPre<W>* e = nullptr) {
    // an operand only EpiPre<4> holds: prefetched there, loaded here otherwise
    auto pre4_or_ld = [&](auto field, auto* q) __attribute__((always_inline)) {
        if constexpr (PRE && W == 4) return field(*e);
        else return epi_ld<W>(q);
    };
    auto to_bf16 = [&]() __attribute__((always_inline)) {
        epi_bf16<W> b;
#pragma unroll
        for (int r = 0; r < W; ++r) b[r] = (bf16_t)v[r];
        return b;
    };
    if (p.bias) {
        const epi_f32<W> bb = pre4_or_ld([](auto& x) { return x.bias; }, p.bias + n);
#pragma unroll
        for (int r = 0; r < W; ++r) v[r] += bb[r];
    }
    const size_t o = (size_t)m * p.N + n;
    if (p.out_preact) *reinterpret_cast<epi_bf16<W>*>(p.out_preact + o) = to_bf16();
    auto add_res = [&]() __attribute__((always_inline)) {
        if (p.res_f32) v += pre4_or_ld([](auto& x) { return x.res; }, p.res_f32 + o);
        if (p.res_bf16) {
            const epi_bf16<W> rr = PRE ? e->resb : epi_ld<W>(p.res_bf16 + o);
#pragma unroll
            for (int r = 0; r < W; ++r) v[r] += (float)rr[r];
        }
    };
    if (p.res_first) add_res();
    if (p.act == RT_ACT_RELU) {
#pragma unroll
        for (int r = 0; r < W; ++r) v[r] = fmaxf(v[r], 0.f);
    } else if (p.act == RT_ACT_GELU) {
#pragma unroll
        for (int r = 0; r < W; ++r) v[r] = rt_gelu(v[r]);
    } else if (p.act == RT_ACT_TANH) {
#pragma unroll
        for (int r = 0; r < W; ++r) v[r] = tanhf(v[r]);
    }
    if (p.drop_p > 0.f) {
        const uint32_t thresh = rt_drop_thresh(p.drop_p);
        const float keep_scale = 1.0f / (1.0f - p.drop_p);
        const uint32_t seed = rt_site_seed(p.seed_dev, p.drop_seed);
#pragma unroll
        for (int r = 0; r < W; ++r)
            v[r] = (rt_hash32(seed, (uint32_t)((o + r) >> p.drop_shift)) >= thresh) ? v[r] * keep_scale : 0.f;
    }
    if (!p.res_first) add_res();
    if (p.gate) {
        const epi_bf16<W> gg = PRE ? e->gate : epi_ld<W>(p.gate + o);
#pragma unroll
        for (int r = 0; r < W; ++r) v[r] = ((float)gg[r] > 0.f) ? v[r] * p.gate_scale : 0.f;
    }
    if (p.preact) {
        const epi_bf16<W> uu = pre4_or_ld([](auto& x) { return x.preact; }, p.preact + o);
#pragma unroll
        for (int r = 0; r < W; ++r) v[r] *= rt_gelu_grad((float)uu[r]);
    }
    if (p.dtanh) {
        const epi_bf16<W> tt = pre4_or_ld([](auto& x) { return x.dtanh; }, p.dtanh + o);
#pragma unroll
        for (int r = 0; r < W; ++r) v[r] *= (1.f - (float)tt[r] * (float)tt[r]);
    }
    auto quad = [&](int h) __attribute__((always_inline)) { return f32x4{v[h], v[h + 1], v[h + 2], v[h + 3]}; };
    if (p.out_f32) {
#pragma unroll
        for (int h = 0; h < W; h += 4) *reinterpret_cast<f32x4*>(p.out_f32 + o + h) = quad(h);
    }
    if (p.acc2_f32) {                                // a second, accumulating destination (one owner per element)
#pragma unroll
        for (int h = 0; h < W; h += 4) *reinterpret_cast<f32x4*>(p.acc2_f32 + o + h) += quad(h);
    }
    if (p.out_bf16) *reinterpret_cast<epi_bf16<W>*>(p.out_bf16 + o) = to_bf16();
}


// rt_gemm_pipe.hip: software-pipelined LDS-DMA variants (hints 2xx)
int rt_launch_gemm_pipe(const GemmArgs& a, int hint, hipStream_t s);
// rt_gemm_astat.hip: activation-stationary form of the short-K / wide-N dense products (hint 501)
bool rt_gemm_astat_ok(const GemmArgs& a);
int rt_launch_gemm_astat(const GemmArgs& a, hipStream_t s);
// rt_gemm_pp.hip: K-parity ping-pong LDS-DMA variants (hints 3xx)
int rt_launch_gemm_pp(const GemmArgs& a, int hint, hipStream_t s);
