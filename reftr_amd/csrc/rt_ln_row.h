// LayerNorm of one row of 256 * V features by one 64-lane wave: lane l holds the f32x4 groups i * 64 + l (i < V), i.e. features
// 4 * (i * 64 + l) .. + 3.  Shared by rt_layernorm_fwd / rt_layernorm_bwd's vectorised kernels (rt_norm.hip), the fused query-region
// launches (rt_qregion.hip) and the cooperative decoder (rt_decoder.hip) so that all of them evaluate the same expression tree on a
// row: the fused launches are accepted because they are bit-identical to the chain of launches they replace.
// Loads, stores, tagged reads, row maps and the dropout masks (forward: on y; backward: on dy before rt_ln_bwd_group, on dx after
// rt_ln_bwd_dx) stay with the callers.
#pragma once
#include "rt_common.h"

// ---- forward (contraction at the compiler's default) ----
template <int V>
__device__ __forceinline__ void rt_ln_stats(const f32x4* v, const float eps, float& mean, float& rstd) {
    constexpr int D = 256 * V;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    mean = rt_wave_sum(s) * (1.f / D);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; ss += d * d; }
    rstd = rsqrtf(rt_wave_sum(ss) * (1.f / D) + eps);
}
__device__ __forceinline__ f32x4 rt_ln_affine(const f32x4 v, const float mean, const float rstd, const f32x4 gam, const f32x4 bet,
                                              const bool relu) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        y[e] = (v[e] - mean) * rstd * gam[e] + bet[e];
        if (relu) y[e] = fmaxf(y[e], 0.f);
    }
    return y;
}

// ---- backward: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma; no fused multiply-adds anywhere ----
// One group of the row: d = its dy (already through the forward's dropout mask), xv = its x.  Leaves xh and g for rt_ln_bwd_dx, adds
// the group's share to the row sums s1 / s2 and to the lane's d gamma / d beta.  relu: dy counts only where the forward's y was > 0.
__device__ __forceinline__ void rt_ln_bwd_group(const f32x4 d, const f32x4 xv, const float mean, const float rstd, const f32x4 gam,
                                                const f32x4 bet, const bool relu, f32x4& xh_out, f32x4& g_out, float& s1, float& s2,
                                                f32x4& dg, f32x4& db) {
#pragma clang fp contract(off)
    f32x4 xh, g, a = dg, b = db;        // worked on as values: element writes through the references keep the accumulators in memory
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xh[e] = (xv[e] - mean) * rstd;
        float de = d[e];
        if (relu) { if (xh[e] * gam[e] + bet[e] <= 0.f) de = 0.f; }
        a[e] += de * xh[e]; b[e] += de;
        g[e] = de * gam[e];
        s1 += g[e]; s2 += g[e] * xh[e];
    }
    xh_out = xh; g_out = g; dg = a; db = b;
}
// the lanes' s1 / s2 -> the row's mean(g), mean(g * xhat)
template <int V>
__device__ __forceinline__ void rt_ln_bwd_means(float& s1, float& s2) {
#pragma clang fp contract(off)
    constexpr int D = 256 * V;
    s1 = rt_wave_sum(s1) * (1.f / D); s2 = rt_wave_sum(s2) * (1.f / D);
}
__device__ __forceinline__ f32x4 rt_ln_bwd_dx(const f32x4 g, const f32x4 xh, const float rstd, const float s1, const float s2) {
#pragma clang fp contract(off)
    f32x4 dx;
#pragma unroll
    for (int e = 0; e < 4; ++e) dx[e] = rstd * (g[e] - s1 - xh[e] * s2);
    return dx;
}
