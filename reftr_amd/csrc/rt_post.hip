// Evaluation-side post-processing of RefTR as two kernels:
//   rt_mask_postprocess  PostProcessSegm.forward (models/reftr_segmentation.py:282-302): bilinear resize of the mask logits
//                        to the padded frame (align_corners=False) -> sigmoid > threshold -> crop to the image's own size
//                        -> nearest resize to the original size.  Both outputs are produced from the logits in ONE pass
//                        (a masks_origin pixel recomputes the decision of the cropped-mask pixel it samples), so neither
//                        the fp32 up-sampled frame (B x max_h x max_w x 4 B) nor the float copy of the boolean mask that
//                        the reference materialises ever exists in HBM: traffic = logits once (L2-resident, 16x smaller
//                        than the frame) + 1 B per output pixel.
//   rt_box_postprocess   PostProcessVGMultiPhrase.forward (models/post_process.py:45-83): ordered selection of every
//                        image's valid phrases (exact integer logic, = torch.masked_select order), cxcywh -> xyxy, optional
//                        scaling to the image size.  fp32 operations are issued un-fused in the reference's order
//                        (x - 0.5*w, then * scale) so the boxes are bit-identical to its CPU result.
// HBM-bound byte kernels: one thread per output pixel / box, coalesced 1-B stores along the row.
// Also here: launch (a) of rt_eval_canvas (the mask partials of a canvas evaluation batch, taken from the logits), because it calls
// mask_decision and must be compiled under this file's contraction setting -- see rt_eval_shared.h -- and, for the same reason,
// launch (b) of rt_predict_canvas (masks_origin of a canvas batch, packed in 16-byte units) and launch (a) of rt_eval_orig (the same
// decisions counted against the raw target mask).
#include "rt_eval_shared.h"

namespace {

using rt_eval_shared::mask_decision;        // with bilinear_axis in rt_eval_shared.h: compiled HERE, under this file's contraction

// torch 'nearest' (legacy) source index: out == in -> dst; out == 2 in -> dst >> 1; else min(int(floorf(dst * (float)in/out)), in - 1)
__device__ __forceinline__ int nearest_src(int dst, int in, int out) {
    if (out == in) return dst;
    if (out == 2 * in) return dst >> 1;
    const float scale = (float)in / (float)out;
    return min((int)floorf(__fmul_rn((float)dst, scale)), in - 1);
}

__global__ __launch_bounds__(256) void mask_postprocess_kernel(const rt_mask_post_desc p) {
    const int img = blockIdx.y / p.Q, q = blockIdx.y - img * p.Q;
    const float* lg = p.pred + (size_t)blockIdx.y * p.h * p.w;
    const float sh = (float)p.h / (float)p.max_h, sw = (float)p.w / (float)p.max_w;
    const int ih = p.sizes[img * 2], iw = p.sizes[img * 2 + 1];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.max_h * p.max_w) {                    // frame pixel: the cropped mask, zero outside the image's own size
        const int y = i / p.max_w, x = i - y * p.max_w;
        const bool in = y < ih && x < iw;
        p.masks[((size_t)blockIdx.y * p.max_h + y) * p.max_w + x] = (in && mask_decision(lg, p.h, p.w, y, x, sh, sw, p.threshold)) ? 1 : 0;
    }
    if (p.masks_origin) {
        const int oh = p.orig[img * 2], ow = p.orig[img * 2 + 1];
        if (i < oh * ow) {
            const int y = i / ow, x = i - y * ow;
            const int sy = nearest_src(y, ih, oh), sx = nearest_src(x, iw, ow);
            p.masks_origin[p.origin_off[img] + (size_t)q * oh * ow + i] = mask_decision(lg, p.h, p.w, sy, sx, sh, sw, p.threshold) ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(64) void box_postprocess_kernel(const rt_box_post_desc p) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    // phrase_mask is [B, P, K]; any P: the wave walks the phrases 64 at a time, rt_phrase_rank (rt_common.h) gives each selected
    // phrase its place in the reference's masked_select order
    int base = 0, rank;
    for (int j0 = 0; j0 < p.P; j0 += 64) {
        const int ph = j0 + lane;
        if (!rt_phrase_rank(p.valid + (size_t)b * p.P * p.K, p.P, p.K, ph, lane, base, rank)) continue;
        const bool scale = p.sizes != nullptr;          // scale_to_original_shape: boxes * [img_w, img_h, img_w, img_h]
        rt_eval_shared::select_scale_box(p.boxes + ((size_t)(b * p.P + ph) * p.K) * 4, scale, scale ? p.sizes[b * 2] : 1.f,
                                         scale ? p.sizes[b * 2 + 1] : 1.f, p.out + ((size_t)b * p.P + rank) * 4);
    }
    if (lane == 0) p.counts[b] = base;
}

// launch (a) of rt_eval_canvas (the rest: rt_eval.hip): integer {I, U} of query 0's decisions against the staged target mask over one
// run of RT_EVAL_CHUNK pixels of the image's scored rectangle.  The decision is mask_postprocess_kernel's, frame = canvas, taken from
// the logits (L2-resident, 16x smaller than the frame); it lives in THIS file so that both are compiled under one contraction setting.
__global__ __launch_bounds__(256) void eval_canvas_mask_kernel(const rt_eval_canvas_args a, int nchunks) {
    __shared__ int sm[8];
    const int b = blockIdx.y, c = blockIdx.x;
    const int32_t* f = a.facts + (size_t)b * 6;
    int ih, iw;
    rt_eval_shared::scored_rect(f[0], f[1], f[4], f[5], a.Hc, a.Wc, ih, iw);
    int I = 0, U = 0;
    if (ih > 0 && iw > 0) {
        const float* lg = a.pred_masks + (size_t)b * a.Q * a.h * a.w;                  // query 0
        const uint8_t* tg = a.tgt_masks + (size_t)b * a.Hc * a.Wc;
        const float sh = (float)a.h / (float)a.Hc, sw = (float)a.w / (float)a.Wc;
        const long long n = (long long)ih * iw, end = min(n, ((long long)c + 1) * RT_EVAL_CHUNK);
        for (long long i = (long long)c * RT_EVAL_CHUNK + threadIdx.x; i < end; i += 256) {
            const int y = (int)(i / iw), x = (int)(i - (long long)y * iw);
            const int p = mask_decision(lg, a.h, a.w, y, x, sh, sw, a.threshold) ? 1 : 0, t = tg[(size_t)y * a.Wc + x] != 0;
            I += p & t; U += p | t;
        }
    }
    rt_eval_shared::store_block_iu(I, U, sm, a.partials + ((size_t)b * nchunks + c) * 2);
}

// launch (b) of rt_predict_canvas (the rest: rt_predict.hip): masks_origin of mask_postprocess_kernel with the canvas as the frame,
// packed at rt_predict_facts' 16-byte block offsets.  One thread per 16-byte unit of the buffer: it finds its image among the blocks'
// end offsets (LDS), divides ONCE to get (q, y, x) of its first byte, walks its sixteen pixels row by row (the row's source row is
// looked up again only where the row changes) and issues ONE 16-byte store; bytes behind the image's Q * oh * ow are 0.  The written
// range is [0, min(facts' total, units)): nothing at or behind the total, nothing past the capacity, whatever the facts hold -- and
// every logit index is clamped by bilinear_axis, so that foreign facts cannot direct a read outside image b's Q planes either.
__global__ __launch_bounds__(RT_PREDICT_UNITS_PER_WG) void predict_canvas_mask_kernel(const rt_predict_canvas_args a, int units) {
    __shared__ int s_end[RT_BATCH_STAGE_MAX_B];
    const int total = min(a.facts[6], units);
    if ((int)(blockIdx.x * RT_PREDICT_UNITS_PER_WG) >= total) return;          // (the whole workgroup: the grid covers the capacity)
    if ((int)threadIdx.x < a.B) s_end[threadIdx.x] = a.facts[threadIdx.x * RT_PREDICT_FACTS_WORDS + 5];
    __syncthreads();
    const int u = blockIdx.x * RT_PREDICT_UNITS_PER_WG + threadIdx.x;
    if (u >= total) return;
    int b = 0;
    while (b < a.B - 1 && u >= s_end[b]) ++b;
    const int32_t* f = a.facts + (size_t)b * RT_PREDICT_FACTS_WORDS;
    const int ih = f[0], iw = f[1], oh = f[2], ow = f[3];
    const long long first = ((long long)u - f[4]) * 16;                        // the unit's first byte within the image's block
    long long n = oh > 0 && ow > 0 && first >= 0 ? (long long)a.Q * oh * ow : 0;
    if (n > 0x7fffffffLL) n = 0;                                               // (not rt_predict_facts' table)
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (first < n) {
        const unsigned plane = (unsigned)oh * (unsigned)ow, i0 = (unsigned)first;
        const unsigned q = i0 / plane, r = i0 - q * plane;
        int y = (int)(r / (unsigned)ow), x = (int)(r - (unsigned)y * (unsigned)ow);
        const float* lg = a.pred_masks + ((size_t)b * a.Q + q) * a.h * a.w;
        const float sh = (float)a.h / (float)a.Hc, sw = (float)a.w / (float)a.Wc;
        const int left = (int)min(n - first, 16ll);
        int sy = nearest_src(y, ih, oh);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < left) {
                const int sx = nearest_src(x, iw, ow);
                word[k >> 2] |= (mask_decision(lg, a.h, a.w, sy, sx, sh, sw, a.threshold) ? 1u : 0u) << ((k & 3) * 8);
                if (++x == ow) {
                    x = 0;
                    if (++y == oh) { y = 0; lg += (size_t)a.h * a.w; }         // the next query's plane (never read behind the last)
                    sy = nearest_src(y, ih, oh);
                }
            }
        }
    }
    *reinterpret_cast<uint4*>(a.out_masks + (size_t)u * 16) = make_uint4(word[0], word[1], word[2], word[3]);
}

// launch (a) of rt_eval_orig (the rest: rt_eval.hip): integer {I, U} of query 0's masks_origin decisions -- predict_canvas_mask_kernel's,
// frame = canvas -- against the image's RAW target mask, read where it lies, over one run of RT_EVAL_CHUNK pixels of the raw frame.
// The grid covers max_pixels: a workgroup whose chunk starts at or behind the image's pixels leaves at once and writes nothing.
// A thread takes 16-byte units of the flat raw mask (unit = thread, thread + 256, ...: the workgroup's loads stay contiguous): it
// divides ONCE per unit to get (y, x) of its first byte, walks its sixteen pixels row by row (the row's source row is looked up again
// only where the row changes) and reads the sixteen target bytes with ONE 16-byte load where the unit lies wholly inside the image and
// its address is 16-byte aligned, with byte loads otherwise (the image's last, partial unit; a mask base that is not aligned).  No
// byte at or behind orig_h * orig_w is read, and every logit index is clamped by bilinear_axis, whatever the facts hold.
__global__ __launch_bounds__(256) void eval_orig_mask_kernel(const rt_eval_orig_args a, int nchunks) {
    __shared__ int sm[8];
    const int b = blockIdx.y, c = blockIdx.x;
    const int32_t* f = a.facts + (size_t)b * 6;
    const int64_t entry = a.mask_table[b];
    const long long n = rt_eval_shared::orig_pixels(f, entry, a.max_pixels), start = (long long)c * RT_EVAL_CHUNK;
    if (start >= n) return;                                                    // (the whole workgroup)
    const int ih = f[0], iw = f[1], oh = f[2], ow = f[3];
    const uint8_t* tg = reinterpret_cast<const uint8_t*>(entry);
    const float* lg = a.pred_masks + (size_t)b * a.Q * a.h * a.w;              // query 0
    const float sh = (float)a.h / (float)a.Hc, sw = (float)a.w / (float)a.Wc;
    const long long end = min(n, start + RT_EVAL_CHUNK);
    int I = 0, U = 0;
    for (long long first = start + (long long)threadIdx.x * 16; first < end; first += 256 * 16) {
        const int left = (int)min(end - first, 16ll);
        const uint8_t* p = tg + first;
        uint32_t word[4] = {0u, 0u, 0u, 0u};
        if (left == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            word[0] = v.x; word[1] = v.y; word[2] = v.z; word[3] = v.w;
        } else {
            for (int k = 0; k < left; ++k) word[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
        }
        const unsigned i0 = (unsigned)first;                                   // (n <= max_pixels < 2^31)
        int y = (int)(i0 / (unsigned)ow), x = (int)(i0 - (unsigned)y * (unsigned)ow);
        int sy = nearest_src(y, ih, oh);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < left) {
                const int sx = nearest_src(x, iw, ow);
                const int pr = mask_decision(lg, a.h, a.w, sy, sx, sh, sw, a.threshold) ? 1 : 0;
                const int t = ((word[k >> 2] >> ((k & 3) * 8)) & 0xffu) != 0u;
                I += pr & t; U += pr | t;
                if (++x == ow) { x = 0; ++y; sy = nearest_src(y, ih, oh); }
            }
        }
    }
    rt_eval_shared::store_block_iu(I, U, sm, a.partials + ((size_t)b * nchunks + c) * 2);
}

}  // namespace

int rt_eval_orig_launch_mask(const rt_eval_orig_args& a, int nchunks, hipStream_t stream) {
    hipLaunchKernelGGL(eval_orig_mask_kernel, dim3((unsigned)nchunks, (unsigned)a.B), dim3(256), 0, stream, a, nchunks);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

int rt_predict_canvas_launch_mask(const rt_predict_canvas_args& a, int units, hipStream_t stream) {
    if (units <= 0) return RT_OK;
    hipLaunchKernelGGL(predict_canvas_mask_kernel, dim3((unsigned)((units + RT_PREDICT_UNITS_PER_WG - 1) / RT_PREDICT_UNITS_PER_WG)),
                       dim3(RT_PREDICT_UNITS_PER_WG), 0, stream, a, units);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

int rt_eval_canvas_launch_mask(const rt_eval_canvas_args& a, int nchunks, hipStream_t stream) {
    hipLaunchKernelGGL(eval_canvas_mask_kernel, dim3((unsigned)nchunks, (unsigned)a.B), dim3(256), 0, stream, a, nchunks);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_mask_postprocess(const rt_mask_post_desc* d, rt_stream_t stream) {
    if (!d || !d->pred || !d->sizes || !d->masks) return RT_ERR_BADARG;
    if (d->B <= 0 || d->Q <= 0 || d->h <= 0 || d->w <= 0 || d->max_h <= 0 || d->max_w <= 0) return RT_ERR_BADARG;
    if (d->masks_origin && (!d->orig || !d->origin_off || d->max_origin <= 0)) return RT_ERR_BADARG;
    if ((long long)d->max_h * d->max_w >= 0x7fffffffLL || (long long)d->max_origin >= 0x7fffffffLL) return RT_ERR_UNSUPPORTED;
    const long long n = d->masks_origin && d->max_origin > (long long)d->max_h * d->max_w ? d->max_origin : (long long)d->max_h * d->max_w;
    hipLaunchKernelGGL(mask_postprocess_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(d->B * d->Q)), dim3(256), 0,
                       (hipStream_t)stream, *d);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_box_postprocess(const rt_box_post_desc* d, rt_stream_t stream) {
    if (!d || !d->boxes || !d->valid || !d->out || !d->counts) return RT_ERR_BADARG;
    if (d->B <= 0 || d->P <= 0 || d->K <= 0) return RT_ERR_BADARG;
    hipLaunchKernelGGL(box_postprocess_kernel, dim3((unsigned)d->B), dim3(64), 0, (hipStream_t)stream, *d);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
