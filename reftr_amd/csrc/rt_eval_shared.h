// What rt_post.hip (post-processing) and rt_eval.hip (metrics) both need, each defined ONCE: the mask decision, the ordered box
// selection, the scored rectangle and the workgroup's {I, U} store.
//
// Contraction.  The fp32 operations below are spelled with HIP's __fmul_rn / __fadd_rn / __fsub_rn, which are plain operators in a
// header: what they compile to follows the INCLUDING file's contraction setting.  rt_post.hip compiles under the compiler's default
// (a product feeding a sum may become one fused operation), rt_eval.hip under `#pragma clang fp contract(off)`.
//   * mask_decision / bilinear_axis are contraction-sensitive (a borderline pixel flips with one fused multiply-add), so EVERY kernel
//     that takes a mask decision is compiled in rt_post.hip: rt_mask_postprocess's, rt_eval_canvas's, rt_predict_canvas's and
//     rt_eval_orig's mask kernels sit side by side there and rt_eval.hip reaches its two through rt_eval_canvas_launch_mask and
//     rt_eval_orig_launch_mask below.  rt_eval.hip must not call mask_decision.
//   * select_scale_box is not: its only product that feeds a sum is 0.5f * w, which is exact, so the fused and the un-fused forms
//     round the same value once.  It is used from both files.
#pragma once
#include "rt_common.h"

namespace rt_eval_shared {

// torch's index / weight rule for mode='bilinear', align_corners=False (ATen UpSample.h: area_pixel_compute_source_index,
// guard_index_and_lambda): src = max(scale * (dst + 0.5) - 0.5, 0), i0 = min(int(src), in - 1), lambda1 = clamp(src - i0, 0, 1)
__device__ __forceinline__ void bilinear_axis(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    if (src < 0.f) src = 0.f;
    i0 = min((int)floorf(src), in - 1);
    l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l0 = __fsub_rn(1.f, l1);
}

// decision of frame pixel (y, x): sigmoid(bilinear(logits)) > threshold
__device__ __forceinline__ bool mask_decision(const float* __restrict__ lg, int h, int w, int y, int x, float sh, float sw, float thr) {
    int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
    bilinear_axis(y, sh, h, y0, y1, ly0, ly1);
    bilinear_axis(x, sw, w, x0, x1, lx0, lx1);
    const float a = lg[y0 * w + x0], b = lg[y0 * w + x1], c = lg[y1 * w + x0], d = lg[y1 * w + x1];
    // ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d), the reference kernel's association
    const float top = __fadd_rn(__fmul_rn(lx0, a), __fmul_rn(lx1, b));
    const float bot = __fadd_rn(__fmul_rn(lx0, c), __fmul_rn(lx1, d));
    const float v = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
    const float s = 1.f / (1.f + expf(-v));
    return s > thr;
}

// PostProcessVGMultiPhrase's box of one selected phrase (post_process.py:62-83): cxcywh -> xyxy, x - 0.5 * w first, then -- when
// `scale` -- times {img_w, img_h, img_w, img_h}; four stores to o
__device__ __forceinline__ void select_scale_box(const float* __restrict__ s, bool scale, float ih, float iw, float* __restrict__ o) {
    const float cx = s[0], cy = s[1], w = s[2], h = s[3];
    float x0 = __fsub_rn(cx, __fmul_rn(0.5f, w)), y0 = __fsub_rn(cy, __fmul_rn(0.5f, h));
    float x1 = __fadd_rn(cx, __fmul_rn(0.5f, w)), y1 = __fadd_rn(cy, __fmul_rn(0.5f, h));
    if (scale) { x0 = __fmul_rn(x0, iw); y0 = __fmul_rn(y0, ih); x1 = __fmul_rn(x1, iw); y1 = __fmul_rn(y1, ih); }
    o[0] = x0; o[1] = y0; o[2] = x1; o[3] = y1;
}

// One image's result rows by one whole wave (rt_box_postprocess's rows, scaled to the original size): the r-th VALID phrase of
// pred_b [P, K, 4] / valid_b [P, K] (rt_phrase_rank: masked_select order) -> rows[r] = xyxy * {ow, oh, ow, oh}, the rows behind them
// 0.  Returns the image's count of valid phrases.  What rt_eval_canvas writes to its ring and rt_predict_canvas to out_boxes.
__device__ __forceinline__ int write_scaled_rows(const float* __restrict__ pred_b, const uint8_t* __restrict__ valid_b, int P, int K,
                                                 float oh, float ow, float* __restrict__ rows, int lane) {
    int base = 0, rank;
    for (int j0 = 0; j0 < P; j0 += 64) {
        const int ph = j0 + lane;
        if (rt_phrase_rank(valid_b, P, K, ph, lane, base, rank))
            select_scale_box(pred_b + ((size_t)ph * K) * 4, true, oh, ow, rows + (size_t)rank * 4);
    }
    for (int i = base * 4 + lane; i < P * 4; i += 64) rows[i] = 0.f;
    return base;
}

// the image's scored rectangle: its size, never past the target's own extent or the frame (equal to the size for consistent input)
__device__ __forceinline__ void scored_rect(int size_h, int size_w, int th, int tw, int max_h, int max_w, int& ih, int& iw) {
    ih = min(min(size_h, th), max_h);
    iw = min(min(size_w, tw), max_w);
}

// rt_eval_orig: the pixels of image b's raw frame that are scored -- orig_h * orig_w of its facts row f, or 0 where the image cannot be
// scored (a zero table entry, a non-positive size, more pixels than the grid was sized for).  Both launches decide by this one function:
// the finish adds exactly the partials the mask kernel wrote.
__device__ __forceinline__ long long orig_pixels(const int32_t* __restrict__ f, int64_t entry, int64_t max_pixels) {
    if (entry == 0 || f[0] <= 0 || f[1] <= 0 || f[2] <= 0 || f[3] <= 0) return 0;
    const long long n = (long long)f[2] * f[3];
    return n <= max_pixels ? n : 0;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a 256-thread workgroup's integer {I, U} to its own slot (plain stores); sm = 8 ints of shared memory
__device__ __forceinline__ void store_block_iu(int I, int U, int* sm, int32_t* __restrict__ o) {
    I = wave_sum_int(I); U = wave_sum_int(U);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm[wid * 2] = I; sm[wid * 2 + 1] = U; }
    __syncthreads();
    if (threadIdx.x == 0) {
        o[0] = (sm[0] + sm[2]) + (sm[4] + sm[6]);
        o[1] = (sm[1] + sm[3]) + (sm[5] + sm[7]);
    }
}

}  // namespace rt_eval_shared

// launch (a) of rt_eval_canvas, defined in rt_post.hip beside rt_mask_postprocess's kernel (see "Contraction" above); the caller has
// checked the arguments.  Returns RT_OK or the launch's hipError.
__attribute__((visibility("hidden"))) int rt_eval_canvas_launch_mask(const rt_eval_canvas_args& a, int nchunks, hipStream_t stream);

// launch (b) of rt_predict_canvas (rt_predict.hip), defined in rt_post.hip for the same reason: `units` = capacity / 16, the 16-byte
// units the grid covers.  The caller has checked the arguments.  Returns RT_OK or the launch's hipError.
#define RT_PREDICT_UNITS_PER_WG 256
__attribute__((visibility("hidden"))) int rt_predict_canvas_launch_mask(const rt_predict_canvas_args& a, int units, hipStream_t stream);

// launch (a) of rt_eval_orig (the rest: rt_eval.hip), defined in rt_post.hip for the same reason; the caller has checked the arguments.
// Returns RT_OK or the launch's hipError.
__attribute__((visibility("hidden"))) int rt_eval_orig_launch_mask(const rt_eval_orig_args& a, int nchunks, hipStream_t stream);
