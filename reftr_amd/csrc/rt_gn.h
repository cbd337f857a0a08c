// GroupNorm arithmetic shared by the token-major kernels of rt_norm.hip (input_proj) and the NHWC kernels of rt_seg.hip (mask head, + ReLU):
// a group's statistics from {sum, sumsq}, xhat, the ReLU gate and the backward element; forward and backward agree on them bit for bit.
#pragma once

struct GnStat { float mean, rstd; };

// 1 / (elements of one group of one image)
__device__ __forceinline__ float rt_gn_inv_n(int cpg, int HW) { return 1.f / (float)(cpg * HW); }
// st = one group's {sum, sumsq}, in global memory or in LDS
__device__ __forceinline__ GnStat rt_gn_stat(const float* st, float inv_n, float eps) {
    const float mean = st[0] * inv_n;
    const float var = fmaxf(st[1] * inv_n - mean * mean, 0.f);
    return {mean, rsqrtf(var + eps)};
}
__device__ __forceinline__ float rt_gn_xhat(float x, const GnStat& s) { return (x - s.mean) * s.rstd; }
// dy behind the optional ReLU: it passes no gradient where y = xhat * gamma + beta <= 0
__device__ __forceinline__ float rt_gn_gate(float d, float xh, float gamma, float beta, bool relu) { return relu && xh * gamma + beta <= 0.f ? 0.f : d; }
// a * b rounded on its own, never fused into what follows (the build's contraction mode is the default fast-honor-pragmas, which obeys this)
__device__ __forceinline__ float rt_gn_mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
// dx of one element: dg = dy * gamma (dy already gated), bst = the group's {sum dg, sum dg * xhat}.  The caller forms the product: the
// token-major kernel writes d * gamma (fused into the first subtraction), the NHWC kernel has always rounded it first: rt_gn_mul_rounded.
__device__ __forceinline__ float rt_gn_dx(float dg, float xh, float rstd, const float* bst, float inv_n) {
    const float m1 = bst[0] * inv_n, m2 = bst[1] * inv_n;
    return rstd * (dg - m1 - xh * m2);
}
