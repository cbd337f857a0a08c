// rt_hsv_jitter: the reference's RandomIntensitySaturation on a batch of raw uint8 images, one launch, in front of rt_raw_stage
// (include/reftr_hip.h).  It writes the bytes of reftr_amd/data/jitter.py `apply` -- the 8-bit RGB -> HSV -> gains -> RGB round trip in
// integers and fp32 -- so every expression that rounds is written as it is there, and nothing in this file may be contracted into a
// fused multiply-add (the three products of hsv_to_rgb round differently when they are):
#pragma clang fp contract(off)
#include "rt_common.h"

namespace {

constexpr int HSV_SHIFT = 12, HSV_HALF = 1 << (HSV_SHIFT - 1);
constexpr int PIXELS = 16, UNIT_BYTES = 3 * PIXELS;       // a thread's unit: 16 consecutive pixels of the flat image, three 16-byte words
static_assert(sizeof(rt_hsv_jitter_args) <= 4096, "the argument block of a launch (the kernel takes nothing else)");

constexpr int WORDS = UNIT_BYTES / 4;

// c ? a : b without a branch (a thread walks 16 pixels, each with its own sector)
__device__ __forceinline__ int sel(bool c, int a, int b) {
    const int m = -(int)c;
    return (a & m) | (b & ~m);
}
__device__ __forceinline__ float sel(bool c, float a, float b) { return __int_as_float(sel(c, __float_as_int(a), __float_as_int(b))); }

// jitter.py _gain: fp32 product, clipped only when the gain exceeds one, truncated
__device__ __forceinline__ int gain8(int x, float gain) {
    float y = (float)x * gain;
    if (gain > 1.f) y = fminf(fmaxf(y, 0.f), 255.f);      // (the same for the whole image)
    return (int)(uint8_t)(int)y;
}

// which of tab[0 .. 3] a channel takes in each of the six sectors, two bits per sector
constexpr unsigned sectors(unsigned s0, unsigned s1, unsigned s2, unsigned s3, unsigned s4, unsigned s5) {
    return s0 | s1 << 2 | s2 << 4 | s3 << 6 | s4 << 8 | s5 << 10;
}
// (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], column by column
constexpr unsigned TAB_B = sectors(1, 1, 3, 0, 0, 2), TAB_G = sectors(3, 0, 0, 2, 1, 1), TAB_R = sectors(0, 2, 1, 1, 3, 0);

__device__ __forceinline__ float pick(unsigned code, int sector, float t0, float t1, float t2, float t3) {
    const unsigned k = code >> (2 * sector);
    return sel((k & 2u) != 0, sel((k & 1u) != 0, t3, t2), sel((k & 1u) != 0, t1, t0));
}

__device__ __forceinline__ unsigned out8(float c) {
    const float r = rintf(c * 255.f);                     // round half to even
    return (unsigned)(int)fminf(fmaxf(r, 0.f), 255.f);
}

// one pixel: r, g, b in [0, 255] -> r | g << 8 | b << 16
__device__ __forceinline__ unsigned jitter_pixel(int r, int g, int b, const int* sdiv, const int* hdiv, float s_gain, float v_gain) {
    const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), d = v - vmin;
    const int s = (d * sdiv[v] + HSV_HALF) >> HSV_SHIFT;
    const int h0 = sel(v == r, g - b, sel(v == g, b - r + 2 * d, r - g + 4 * d));
    int h = (h0 * hdiv[d] + HSV_HALF) >> HSV_SHIFT;       // arithmetic shift of a negative product
    h += sel(h < 0, 180, 0);
    const int s2 = gain8(s, s_gain), v2 = gain8(v, v_gain);
    const float hf = (float)h * (6.f / 180.f), sf = (float)s2 * (1.f / 255.f), vf = (float)v2 * (1.f / 255.f);
    // straight-line: the products of a grey pixel (s' == 0) are computed and dropped
    const float fl = floorf(hf);
    const bool outside = fl < 0.f || fl > 5.f;
    const int sector = sel(outside, 0, (int)fl);
    const float f = sel(outside, 0.f, hf - fl);
    const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * f), t3 = vf * (1.f - sf * (1.f - f));
    const bool grey = s2 == 0;
    const float fb = sel(grey, vf, pick(TAB_B, sector, t0, t1, t2, t3));
    const float fg = sel(grey, vf, pick(TAB_G, sector, t0, t1, t2, t3));
    const float fr = sel(grey, vf, pick(TAB_R, sector, t0, t1, t2, t3));
    return out8(fr) | out8(fg) << 8 | out8(fb) << 16;
}

// one unit of n <= 16 pixels from src to dst, held as twelve 32-bit words.  VEC (n = 16, both addresses 16-byte aligned): three
// 16-byte loads, three 16-byte stores; else byte accesses to the 3 n bytes alone.  Every byte of the unit is read before the first is
// written: dst == src is allowed.
template <bool VEC>
__device__ __forceinline__ void jitter_unit(const uint8_t* src, uint8_t* dst, int n, const int* sdiv, const int* hdiv, float s_gain,
                                            float v_gain) {
    unsigned in[WORDS], out[WORDS];
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint4 q = reinterpret_cast<const uint4*>(src)[j];
            in[4 * j] = q.x; in[4 * j + 1] = q.y; in[4 * j + 2] = q.z; in[4 * j + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < WORDS; ++j) in[j] = 0;
#pragma unroll
        for (int j = 0; j < UNIT_BYTES; ++j) if (j < 3 * n) in[j / 4] |= (unsigned)src[j] << (8 * (j % 4));
    }
#pragma unroll
    for (int j = 0; j < WORDS; ++j) out[j] = 0;
#pragma unroll
    for (int i = 0; i < PIXELS; ++i) {
        int c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (int)(in[(3 * i + k) / 4] >> (8 * ((3 * i + k) % 4)) & 255u);
        const unsigned px = jitter_pixel(c[0], c[1], c[2], sdiv, hdiv, s_gain, v_gain);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[(3 * i + k) / 4] |= (px >> (8 * k) & 255u) << (8 * ((3 * i + k) % 4));
    }
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 3; ++j) reinterpret_cast<uint4*>(dst)[j] = make_uint4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < UNIT_BYTES; ++j) if (j < 3 * n) dst[j] = (uint8_t)(out[j / 4] >> (8 * (j % 4)));
    }
}

// workgroup (x, b): units [256 x, 256 x + 256) of image b; the grid's x extent is that of the largest image
__global__ __launch_bounds__(256) void hsv_jitter_kernel(const rt_hsv_jitter_args a) {
    __shared__ int sdiv[256], hdiv[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int npix = a.h[b] * a.w[b];                     // (3 * h * w < 2^31: the entry point)
    if ((size_t)blockIdx.x * 256 * PIXELS >= (size_t)npix) return;          // (the same for the whole workgroup)
    // OpenCV's division tables: a double division, rounded half to even
    sdiv[tid] = tid ? (int)rint((double)(255 << HSV_SHIFT) / (1.0 * tid)) : 0;
    hdiv[tid] = tid ? (int)rint((double)(180 << HSV_SHIFT) / (6.0 * tid)) : 0;
    __syncthreads();
    const size_t p0 = ((size_t)blockIdx.x * 256 + tid) * PIXELS;
    if (p0 >= (size_t)npix) return;
    const int n = (size_t)npix - p0 < (size_t)PIXELS ? (int)((size_t)npix - p0) : PIXELS;
    const uint8_t* src = a.src[b] + p0 * 3;
    uint8_t* dst = a.dst[b] + p0 * 3;
    // 48 p0 is a multiple of 16: a whole unit is aligned where the two bases are
    const bool vec = n == PIXELS && ((reinterpret_cast<uintptr_t>(a.src[b]) | reinterpret_cast<uintptr_t>(a.dst[b])) & 15) == 0;
    const float s_gain = a.s_gain[b], v_gain = a.v_gain[b];
    if (vec) jitter_unit<true>(src, dst, PIXELS, sdiv, hdiv, s_gain, v_gain);
    else jitter_unit<false>(src, dst, n, sdiv, hdiv, s_gain, v_gain);
}

}  // namespace

extern "C" int rt_hsv_jitter(const rt_hsv_jitter_args* a, rt_stream_t stream) {
    if (!a || a->B <= 0) return RT_ERR_BADARG;
    const int B = a->B;
    if (B > RT_BATCH_STAGE_MAX_B) return RT_ERR_UNSUPPORTED;
    bool too_large = false;
    int64_t most = 0;
    for (int b = 0; b < B; ++b) {
        const float sg = a->s_gain[b], vg = a->v_gain[b];
        if (!a->src[b] || !a->dst[b] || a->h[b] <= 0 || a->w[b] <= 0) return RT_ERR_BADARG;
        if (!(sg >= 0.f && sg <= 3.402823466e+38f) || !(vg >= 0.f && vg <= 3.402823466e+38f)) return RT_ERR_BADARG;   // negative, NaN, infinite
        const int64_t npix = (int64_t)a->h[b] * a->w[b];
        too_large = too_large || 3 * npix >= ((int64_t)1 << 31);
        most = npix > most ? npix : most;
    }
    if (too_large) return RT_ERR_UNSUPPORTED;
    const int64_t units = (most + PIXELS - 1) / PIXELS;
    hipLaunchKernelGGL(hsv_jitter_kernel, dim3((unsigned)((units + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, *a);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
