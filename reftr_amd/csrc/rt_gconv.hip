// Grouped 3x3 convolution (ResNeXt conv2, torchvision Bottleneck with groups > 1; models/modeling/backbone.py:112-125 builds
// any torchvision ResNet by name): forward, backward-data and weight gradient on NHWC bf16 activations.
//
// Weight layout: [Cout][3][3][Cg] bf16 (torchvision's [Cout][Cg][3][3], channels-last like every conv weight here); the
// groups are square (Cout = Cin = G * Cg), Cg in {4, 8, 16, 32, 64}.
//
// Forward / backward-data (gconv_kernel): one wave owns 16 output channels x a run of 16-pixel tiles; the MFMA is
// v_mfma_f32_16x16x32_bf16 with A = the block-diagonal weights of its 16 channels (rows) over a channel block of
// Kb = max(Cg, 32) input channels, held in registers for all 9 taps, and B = 16 gathered pixels x Kb channels, one
// 16-byte global load per lane per 32 channels.  Zero blocks cost 8x / 4x / 2x MFMA work at Cg = 4 / 8 / 16: the kernel
// is bound by the activation stream, not by the MFMA rate.  The transposed form gathers dy with the transposed rule and
// reads the forward weight layout directly (no [C][T][N] copy).
//
// Weight gradient (gwgrad_kernel): one wave owns 16 output channels x one M split; D[n][c] over K = 32 pixels per MFMA,
// accumulators for all 9 taps x max(Cg, 16) columns in registers; the split partials go to the caller's workspace and
// one reduction pass applies scale, overwrite / accumulate, the clip-norm contribution and the bf16 twin.
#include "rt_common.h"

namespace {

struct GconvArgs {
    const bf16_t* src; const bf16_t* wgt; bf16_t* out_bf16; float* out_f32; const float* bias; const bf16_t* gate;
    float gate_scale; int act;
    int B, SH, SW, SC, DH, DW, N, stride, pad, dil, Cg, transposed, nslab, tiles_per_wave;
    long long M;
};

constexpr int GC_TILES = 8;          // 16-pixel tiles per wave (128 pixels): the register-resident weights are reused 8 times

// src pixel index of output pixel (b, oy, ox) for tap (kh, kw), -1 when the tap falls outside (zero padding / not divisible)
__device__ __forceinline__ long long gc_src_pixel(const GconvArgs& a, int b, int oy, int ox, int kh, int kw) {
    int iy, ix;
    if (!a.transposed) {
        iy = oy * a.stride - a.pad + kh * a.dil;
        ix = ox * a.stride - a.pad + kw * a.dil;
    } else {
        const int ty = oy + a.pad - kh * a.dil, tx = ox + a.pad - kw * a.dil;
        if (ty < 0 || tx < 0) return -1;
        if (a.stride == 2 && ((ty | tx) & 1)) return -1;
        iy = a.stride == 2 ? ty >> 1 : ty;
        ix = a.stride == 2 ? tx >> 1 : tx;
    }
    if (iy < 0 || iy >= a.SH || ix < 0 || ix >= a.SW) return -1;
    return ((long long)b * a.SH + iy) * a.SW + ix;
}

template <int KS>
__global__ __launch_bounds__(256) void gconv_kernel(const GconvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int slab = blockIdx.x % a.nslab;
    const long long mt0 = (long long)(blockIdx.x / a.nslab) * GC_TILES * 16;
    const int nb = slab * 4 + wave;
    if (nb * 16 >= a.N) return;
    constexpr int KB = KS * 32;
    const int kbase = (nb * 16 / KB) * KB;
    const int Cg = a.Cg;
    // A fragments: row = output channel o = nb*16 + li, k = input channel kbase + ks*32 + lg*8 + e (block diagonal)
    bf16x8 wf[9][KS];
    {
        const int o = nb * 16 + li, og = o / Cg;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 v;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = kbase + ks * 32 + lg * 8 + e;
                    float w = 0.f;
                    if (k / Cg == og) {
                        // forward: w[o][t][k % Cg]; transposed (o = dx channel, k = dy channel): w[k][t][o % Cg]
                        const size_t idx = a.transposed ? ((size_t)k * 9 + t) * Cg + (o % Cg) : ((size_t)o * 9 + t) * Cg + (k % Cg);
                        w = (float)a.wgt[idx];
                    }
                    v[e] = (bf16_t)w;
                }
                wf[t][ks] = v;
            }
    }
    const int n0 = nb * 16 + lg * 4;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.bias) bv = *reinterpret_cast<const f32x4*>(a.bias + n0);
    const int HWo = a.DH * a.DW;
    for (int tile = 0; tile < GC_TILES; ++tile) {
        const long long m = mt0 + tile * 16 + li;
        if (mt0 + tile * 16 >= a.M) break;
        const bool live = m < a.M;
        const int b = live ? (int)(m / HWo) : 0;
        const int r = live ? (int)(m % HWo) : 0;
        const int oy = r / a.DW, ox = r % a.DW;
        bf16x8 xf[9][KS];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const long long sp = live ? gc_src_pixel(a, b, oy, ox, t / 3, t % 3) : -1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (sp >= 0) xf[t][ks] = *reinterpret_cast<const bf16x8*>(a.src + sp * a.SC + kbase + ks * 32 + lg * 8);
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) xf[t][ks][e] = (bf16_t)0.f;
                }
            }
        }
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][ks], xf[t][ks], acc, 0, 0, 0);
        if (!live) continue;
        // lane holds output channels n0 .. n0 + 3 of pixel m
        f32x4 v = acc + bv;
        if (a.act == RT_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (a.gate) {
            const bf16x4 g = *reinterpret_cast<const bf16x4*>(a.gate + m * a.N + n0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= ((float)g[e] > 0.f ? a.gate_scale : 0.f);
        }
        if (a.out_f32) *reinterpret_cast<f32x4*>(a.out_f32 + m * a.N + n0) = v;
        if (a.out_bf16) {
            bf16x4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = (bf16_t)v[e];
            *reinterpret_cast<bf16x4*>(a.out_bf16 + m * a.N + n0) = ov;
        }
    }
}

struct GwgradArgs {
    const bf16_t* dy; const bf16_t* x; float* part;
    int B, SH, SW, SC, DH, DW, N, stride, pad, dil, Cg, nslab, nsplit;
    long long M, chunk;       // rows per split (multiple of 32)
};

// part[split][n][t][c] (E = N * 9 * Cg floats per split) = sum over the split's rows of dy[m][n] * x[gather(m, t)][g(n) * Cg + c]
template <int CB>
__global__ __launch_bounds__(256) void gwgrad_kernel(const GwgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int slab = blockIdx.x % a.nslab, split = blockIdx.x / a.nslab;
    const int nb = slab * 4 + wave;
    if (nb * 16 >= a.N) return;
    constexpr int KC = CB * 16;                       // columns: max(Cg, 16) input channels
    const int cbase = (nb * 16 / KC) * KC;
    const int Cg = a.Cg;
    f32x4 acc[9][CB];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[t][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long m_lo = (long long)split * a.chunk;
    long long m_hi = m_lo + a.chunk;
    if (m_hi > a.M) m_hi = a.M;
    const int HWo = a.DH * a.DW;
    const int n = nb * 16 + li;
    for (long long m0 = m_lo; m0 < m_hi; m0 += 32) {
        // A: row = n, k = pixel m0 + lg*8 + e;  B: col = input channel cbase + cb*16 + li, k = the same pixels
        bf16x8 af;
        int pb[8], py[8], px[8];                      // image, top-left source row / column of the 8 pixels (pb < 0: past the split)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long long m = m0 + lg * 8 + e;
            const bool live = m < m_hi;
            af[e] = live ? a.dy[m * a.N + n] : (bf16_t)0.f;
            const int r = live ? (int)(m % HWo) : 0;
            pb[e] = live ? (int)(m / HWo) : -1;
            py[e] = (r / a.DW) * a.stride - a.pad;
            px[e] = (r % a.DW) * a.stride - a.pad;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            long long sp[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int iy = py[e] + (t / 3) * a.dil, ix = px[e] + (t % 3) * a.dil;
                sp[e] = (pb[e] >= 0 && iy >= 0 && iy < a.SH && ix >= 0 && ix < a.SW) ? ((long long)pb[e] * a.SH + iy) * a.SW + ix : -1;
            }
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                bf16x8 xf;
                const int c = cbase + cb * 16 + li;
#pragma unroll
                for (int e = 0; e < 8; ++e) xf[e] = sp[e] >= 0 ? a.x[sp[e] * a.SC + c] : (bf16_t)0.f;
                acc[t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf, acc[t][cb], 0, 0, 0);
            }
        }
    }
    // lane holds D[n = nb*16 + lg*4 + r][c = cbase + cb*16 + li]: keep the block-diagonal entries
    const size_t E = (size_t)a.N * 9 * Cg;
    float* part = a.part + (size_t)split * E;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nn = nb * 16 + lg * 4 + r;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            const int c = cbase + cb * 16 + li;
            if (c / Cg != nn / Cg) continue;
#pragma unroll
            for (int t = 0; t < 9; ++t) part[((size_t)nn * 9 + t) * Cg + (c % Cg)] = acc[t][cb][r];
        }
    }
}

struct GwgradFinish {
    const float* part; float* dw; const float* scale; float* sqacc; bf16_t* g16;
    int nsplit, overwrite, per_n;      // per_n = 9 * Cg
    long long E;
};

__global__ __launch_bounds__(256) void gwgrad_finish_kernel(const GwgradFinish f) {
    __shared__ float sm[16];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float ss = 0.f;
    if (i < f.E) {
        float s = 0.f;
        for (int k = 0; k < f.nsplit; ++k) s += f.part[(size_t)k * f.E + i];
        if (f.scale) s *= f.scale[i / f.per_n];
        ss = rt_wg_commit(s, f.dw + i, f.g16 ? f.g16 + i : nullptr, !f.overwrite);
    }
    if (f.sqacc) {
        ss = rt_block_sum(ss, sm);
        if (threadIdx.x == 0) rt_sq_add(f.sqacc, blockIdx.x, ss);
    }
}

bool gc_cg_ok(int cg) { return cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64; }

}  // namespace

extern "C" int rt_gconv(const rt_conv_gemm_desc* d, int groups, rt_stream_t stream) {
    if (!d || !d->src || !d->wgt || (!d->out_bf16 && !d->out_f32) || groups <= 0) return RT_ERR_BADARG;
    if (d->res_f32 || d->res_bf16 || d->preact || d->dtanh || d->out_preact || d->acc2_f32 || d->drop_p != 0.f || d->tile_hint != 0 ||
        (d->act != RT_ACT_NONE && d->act != RT_ACT_RELU))
        return RT_ERR_UNSUPPORTED;
    if (d->SC % groups) return RT_ERR_UNSUPPORTED;
    const int Cg = d->SC / groups;
    const int dil = d->dil > 1 ? d->dil : 1;
    if (!gc_cg_ok(Cg) || d->N != d->SC || d->KH != 3 || d->KW != 3 || (d->stride != 1 && d->stride != 2) || (dil > 1 && d->stride != 1))
        return RT_ERR_UNSUPPORTED;
    const int KB = Cg > 32 ? Cg : 32;
    if (d->SC % KB || d->N % 16) return RT_ERR_UNSUPPORTED;
    if (d->B <= 0 || d->SH <= 0 || d->SW <= 0 || d->DH <= 0 || d->DW <= 0 || d->pad < 0) return RT_ERR_BADARG;
    if (((uintptr_t)d->src & 15) || ((uintptr_t)d->out_f32 & 15) || ((uintptr_t)d->out_bf16 & 7) || ((uintptr_t)d->gate & 7) ||
        ((uintptr_t)d->bias & 15))
        return RT_ERR_BADARG;
    GconvArgs a;
    a.src = (const bf16_t*)d->src; a.wgt = (const bf16_t*)d->wgt; a.out_bf16 = (bf16_t*)d->out_bf16; a.out_f32 = d->out_f32;
    a.bias = d->bias; a.gate = (const bf16_t*)d->gate; a.gate_scale = d->gate_scale; a.act = d->act;
    a.B = d->B; a.SH = d->SH; a.SW = d->SW; a.SC = d->SC; a.DH = d->DH; a.DW = d->DW; a.N = d->N;
    a.stride = d->stride; a.pad = d->pad; a.dil = dil; a.Cg = Cg; a.transposed = d->transposed ? 1 : 0;
    a.nslab = (d->N + 63) / 64;
    a.tiles_per_wave = GC_TILES;
    a.M = (long long)d->B * d->DH * d->DW;
    const long long mblocks = (a.M + GC_TILES * 16 - 1) / (GC_TILES * 16);
    const long long grid = mblocks * a.nslab;
    if (grid > 0x7fffffffLL) return RT_ERR_UNSUPPORTED;
    if (KB == 32) hipLaunchKernelGGL(gconv_kernel<1>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gconv_kernel<2>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_gconv_wgrad(const rt_conv_wgrad_desc* d, int groups, rt_stream_t stream) {
    if (!d || !d->dy || !d->x || !d->dw || groups <= 0) return RT_ERR_BADARG;
    if (d->dbias || d->variant != 0) return RT_ERR_UNSUPPORTED;
    if (d->SC % groups) return RT_ERR_UNSUPPORTED;
    const int Cg = d->SC / groups;
    const int dil = d->dil > 1 ? d->dil : 1;
    if (!gc_cg_ok(Cg) || d->N != d->SC || d->KH != 3 || d->KW != 3 || (d->stride != 1 && d->stride != 2) || (dil > 1 && d->stride != 1))
        return RT_ERR_UNSUPPORTED;
    const int KC = Cg > 16 ? Cg : 16;
    if (d->SC % KC || d->N % 16) return RT_ERR_UNSUPPORTED;
    if (d->B <= 0 || d->SH <= 0 || d->SW <= 0 || d->DH <= 0 || d->DW <= 0 || d->pad < 0) return RT_ERR_BADARG;
    const long long M = (long long)d->B * d->DH * d->DW;
    const long long E = (long long)d->N * 9 * Cg;
    if (!d->workspace || d->workspace_bytes < E * 4) return RT_ERR_BADARG;       // the split partials need scratch
    const int nslab = (d->N + 63) / 64;
    const long long chunks = (M + 31) / 32;
    long long ns = d->msplit;
    if (ns <= 0) {
        ns = (1024 + nslab - 1) / nslab;              // ~1024 workgroups over the chip ...
        const long long maxs = chunks / 8 > 0 ? chunks / 8 : 1;         // ... of >= 256 rows each
        if (ns > maxs) ns = maxs;
    }
    if (ns > chunks) ns = chunks;
    const long long cap = d->workspace_bytes / (E * 4);
    if (ns > cap) ns = cap;
    if (ns < 1) ns = 1;
    const long long per = (chunks + ns - 1) / ns;
    ns = (chunks + per - 1) / per;                    // no empty split
    GwgradArgs a;
    a.dy = (const bf16_t*)d->dy; a.x = (const bf16_t*)d->x; a.part = d->workspace;
    a.B = d->B; a.SH = d->SH; a.SW = d->SW; a.SC = d->SC; a.DH = d->DH; a.DW = d->DW; a.N = d->N;
    a.stride = d->stride; a.pad = d->pad; a.dil = dil; a.Cg = Cg; a.nslab = nslab; a.nsplit = (int)ns;
    a.M = M; a.chunk = per * 32;
    const unsigned grid = (unsigned)(nslab * ns);
    if (KC == 16) hipLaunchKernelGGL(gwgrad_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else if (KC == 32) hipLaunchKernelGGL(gwgrad_kernel<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gwgrad_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    RT_CHECK_LAUNCH();
    GwgradFinish f;
    f.part = d->workspace; f.dw = d->dw; f.scale = d->scale; f.sqacc = d->sqacc; f.g16 = (bf16_t*)d->g16;
    f.nsplit = (int)ns; f.overwrite = d->overwrite ? 1 : 0; f.per_n = 9 * Cg; f.E = E;
    hipLaunchKernelGGL(gwgrad_finish_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
