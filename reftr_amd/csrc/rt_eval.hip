// The metric stage of engine_vg.evaluate (engine_vg.py:127-152) as two launches per batch, running totals on the device:
//   eval_mask_kernel    grid (chunk, image): integer intersection / union counts of query 0's post-processed mask against the
//                       image's target mask over one run of RT_EVAL_CHUNK pixels, stored (plain stores) to the workgroup's own slot
//   eval_finish_kernel  ONE wave, image ascending then row ascending: box IoU of every valid phrase against its target box
//                       (util/box_ops.py's arithmetic, un-fused, in its order -> the bits of diag(box_iou)), the mask partials added
//                       up per image, and the 16 running accumulators (counts int64, the two IoU sums double) updated in that order
// rt_eval_canvas / rt_eval_facts (below): the same finish with every per-batch fact in device memory, for a captured evaluation step
// on a batch canvas; its mask launch lives in rt_post.hip (rt_eval_shared.h says why).
// rt_eval_raw_facts / rt_eval_orig (below): the facts of a RAW batch from host values in the argument block, and the mask scored once
// more on the raw frame against the raw annotation -- the mask launch in rt_post.hip again, the finish here with finish_mask.
// No floating-point atomics and nothing to clear beforehand: the same bits from run to run.  Latency-bound (0.4 MB per 640 x 640
// image, a few hundred box rows): byte loads, one thread per pixel, and a serial walk over the rows for the ordered double sums.
#include "rt_eval_shared.h"

// The box arithmetic must keep torch's roundings: one per operation.  HIP's __fmul_rn / __fadd_rn / __fsub_rn are plain operators
// defined in a header, under the compiler's default contraction: inlined here, a product feeding a sum still becomes one fused
// operation ((a1 + a2) - inter with a2 and inter products lost two roundings that way).  So contraction is switched off for this
// file and the operations are spelled with the operators of this file (nothing in it gains from contraction).
#pragma clang fp contract(off)

namespace {

using rt_eval_shared::wave_sum_int;
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float f_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float f_mul(float a, float b) { return a * b; }

// torch.max / torch.min / clamp(min=0) hand a NaN operand on; the hardware max / min would drop it
__device__ __forceinline__ float t_max(float a, float b) { return a != a ? a : b != b ? b : fmaxf(a, b); }
__device__ __forceinline__ float t_min(float a, float b) { return a != a ? a : b != b ? b : fminf(a, b); }

struct xyxy { float x0, y0, x1, y1; };
// box_cxcywh_to_xyxy (util/box_ops.py:6-8), as rt_box_postprocess issues it
__device__ __forceinline__ xyxy to_xyxy(const float* __restrict__ s) {
    const float cx = s[0], cy = s[1], w = s[2], h = s[3];
    return xyxy{f_sub(cx, f_mul(0.5f, w)), f_sub(cy, f_mul(0.5f, h)),
                f_add(cx, f_mul(0.5f, w)), f_add(cy, f_mul(0.5f, h))};
}
// one diagonal entry of box_iou(a, b) (util/box_ops.py:16-27)
__device__ __forceinline__ float box_iou_pair(const xyxy a, const xyxy b) {
    const float a1 = f_mul(f_sub(a.x1, a.x0), f_sub(a.y1, a.y0));
    const float a2 = f_mul(f_sub(b.x1, b.x0), f_sub(b.y1, b.y0));
    const float w = t_max(f_sub(t_min(a.x1, b.x1), t_max(a.x0, b.x0)), 0.f);
    const float h = t_max(f_sub(t_min(a.y1, b.y1), t_max(a.y0, b.y0)), 0.f);
    const float inter = f_mul(w, h);
    const float uni = f_sub(f_add(a1, a2), inter);
    return __fdiv_rn(inter, uni);
}

__global__ __launch_bounds__(256) void eval_mask_kernel(const rt_eval_metrics_args a, int nchunks) {
    __shared__ int sm[8];
    const int b = blockIdx.y, c = blockIdx.x;
    const int64_t* row = a.table + (size_t)b * 5;
    const uint8_t* tg = reinterpret_cast<const uint8_t*>(row[2]);
    int I = 0, U = 0;
    if (tg) {
        const int tw = (int)row[4];
        int ih, iw;
        rt_eval_shared::scored_rect(a.sizes[b * 2], a.sizes[b * 2 + 1], (int)row[3], tw, a.max_h, a.max_w, ih, iw);
        if (ih > 0 && iw > 0) {
            const uint8_t* pm = a.masks + (size_t)b * a.Q * a.max_h * a.max_w;          // query 0
            const long long n = (long long)ih * iw, end = min(n, ((long long)c + 1) * RT_EVAL_CHUNK);
            for (long long i = (long long)c * RT_EVAL_CHUNK + threadIdx.x; i < end; i += 256) {
                const int y = (int)(i / iw), x = (int)(i - (long long)y * iw);
                const int p = pm[(size_t)y * a.max_w + x] != 0, t = tg[(size_t)y * tw + x] != 0;
                I += p & t; U += p | t;
            }
        }
    }
    rt_eval_shared::store_block_iu(I, U, sm, a.partials + ((size_t)b * nchunks + c) * 2);
}

__device__ __forceinline__ void count_sample(float v, long long& n, long long* hit, double& sum) {
    const float thr[5] = {0.5f, 0.6f, 0.7f, 0.8f, 0.9f};
    n += 1;
#pragma unroll
    for (int t = 0; t < 5; ++t) hit[t] += v > thr[t] ? 1 : 0;
    sum += (double)v;
}

// the 16 running accumulators while a finish kernel runs: lane 0 owns them
struct totals {
    long long det_n = 0, det_hit[5] = {0, 0, 0, 0, 0}, seg_n = 0, seg_hit[5] = {0, 0, 0, 0, 0}, seg_i = 0, seg_u = 0;
    double det_sum = 0.0, seg_sum = 0.0;
    __device__ __forceinline__ void load(const void* acc) {
        const long long* acc_i = reinterpret_cast<const long long*>(acc);
        const double* acc_d = reinterpret_cast<const double*>(acc);
        det_n = acc_i[RT_EVAL_DET_N]; seg_n = acc_i[RT_EVAL_SEG_N];
        for (int t = 0; t < 5; ++t) { det_hit[t] = acc_i[RT_EVAL_DET_HIT + t]; seg_hit[t] = acc_i[RT_EVAL_SEG_HIT + t]; }
        seg_i = acc_i[RT_EVAL_SEG_I]; seg_u = acc_i[RT_EVAL_SEG_U];
        det_sum = acc_d[RT_EVAL_DET_SUM]; seg_sum = acc_d[RT_EVAL_SEG_SUM];
    }
    __device__ __forceinline__ void store(void* acc) const {
        long long* acc_i = reinterpret_cast<long long*>(acc);
        double* acc_d = reinterpret_cast<double*>(acc);
        acc_i[RT_EVAL_DET_N] = det_n; acc_i[RT_EVAL_SEG_N] = seg_n;
        for (int t = 0; t < 5; ++t) { acc_i[RT_EVAL_DET_HIT + t] = det_hit[t]; acc_i[RT_EVAL_SEG_HIT + t] = seg_hit[t]; }
        acc_i[RT_EVAL_SEG_I] = seg_i; acc_i[RT_EVAL_SEG_U] = seg_u;
        acc_d[RT_EVAL_DET_SUM] = det_sum; acc_d[RT_EVAL_SEG_SUM] = seg_sum;
    }
};

// One image's box rows, by the whole wave: the r-th valid phrase of pred_b [P, K, 4] / valid_b [P, K] against target row r of tb
// (nb rows, already clamped to [0, P]) -> out[0 .. P) (unused rows 0), counted by lane 0 in row order.  s_iou: 64 floats of shared memory.
__device__ __forceinline__ void finish_boxes(const float* tb, int nb, const float* pred_b, const uint8_t* valid_b, int P, int K,
                                             float* out, float* s_iou, int lane, totals& t) {
    int base = 0, rank;
    for (int j0 = 0; j0 < P && base < nb; j0 += 64) {
        const int ph = j0 + lane, before = base;
        const bool mine = rt_phrase_rank(valid_b, P, K, ph, lane, base, rank);
        if (mine && rank < nb) {
            const float v = box_iou_pair(to_xyxy(tb + (size_t)rank * 4), to_xyxy(pred_b + ((size_t)ph * K) * 4));
            out[rank] = v;
            s_iou[rank - before] = v;
        }
        __syncthreads();
        if (lane == 0) {
            const int m = min(base, nb) - before;
            for (int i = 0; i < m; ++i) count_sample(s_iou[i], t.det_n, t.det_hit, t.det_sum);
        }
        __syncthreads();
    }
    for (int r = min(base, nb) + lane; r < P; r += 64) out[r] = 0.f;
}

// One image's mask partials pp [nchunks][2] added up by the wave -> iou_seg_b, iu_b[2], and lane 0's totals when the image is scored
__device__ __forceinline__ void finish_mask(const int32_t* pp, int nchunks, bool scored, int lane, float* iou_seg_b, int64_t* iu_b,
                                            totals& t) {
    long long I = 0, U = 0;
    if (scored) {
        for (int c = lane; c < nchunks; c += 64) { I += pp[c * 2]; U += pp[c * 2 + 1]; }
        I = wave_sum_i64(I); U = wave_sum_i64(U);              // integers: exact in any order
    }
    if (lane == 0) {
        const float v = scored ? __fdiv_rn((float)I, (float)U) : 0.f;
        *iou_seg_b = v; iu_b[0] = I; iu_b[1] = U;
        if (scored) { count_sample(v, t.seg_n, t.seg_hit, t.seg_sum); t.seg_i += I; t.seg_u += U; }
    }
}

__global__ __launch_bounds__(64) void eval_finish_kernel(const rt_eval_metrics_args a, int nchunks) {
    __shared__ float s_iou[64];
    const int lane = threadIdx.x;
    totals t;
    if (lane == 0 && !a.reset) t.load(a.acc);
    for (int b = 0; b < a.B; ++b) {
        const int64_t* row = a.table + (size_t)b * 5;
        const float* tb = reinterpret_cast<const float*>(row[0]);
        const int nb = tb ? (int)min((long long)a.P, max(0ll, (long long)row[1])) : 0;
        finish_boxes(tb, nb, a.pred_boxes + (size_t)b * a.P * a.K * 4, a.valid + (size_t)b * a.P * a.K, a.P, a.K,
                     a.iou_det + (size_t)b * a.P, s_iou, lane, t);
        if (!a.masks) continue;
        finish_mask(a.partials + (size_t)b * nchunks * 2, nchunks, row[2] != 0, lane, a.iou_seg + b, a.iu + b * 2, t);
    }
    if (lane == 0) t.store(a.acc);
}

// launch (b) of rt_eval_canvas: eval_finish_kernel's walk with every per-batch fact read from device memory -- the target boxes from
// rt_batch_stage's packed buffer, the original sizes and image ids from rt_eval_facts' tables -- plus the batch's slot of the results
// ring (rt_box_postprocess's rows, scaled to the original size) and the cursor, which this kernel advances itself.
__global__ __launch_bounds__(64) void eval_canvas_finish_kernel(const rt_eval_canvas_args a, int nchunks) {
    __shared__ float s_iou[64];
    const int lane = threadIdx.x;
    totals t;
    if (lane == 0) t.load(a.acc);
    const bool keep = !a.veto || a.veto[0] == 0;                             // a vetoed batch leaves totals, ring and cursor alone
    const int slot = a.cursor[0];
    const bool room = keep && slot >= 0 && slot < a.slots;
    for (int b = 0; b < a.B; ++b) {
        const float* pred_b = a.pred_boxes + (size_t)b * a.P * a.K * 4;
        const uint8_t* valid_b = a.valid + (size_t)b * a.P * a.K;
        const int off = a.tgt_off[b];
        int nb = min(a.P, max(0, a.tgt_off[b + 1] - off));
        if (off < 0 || off > a.tgt_rows - nb) nb = 0;                        // offsets that leave the staged buffer: no rows read
        finish_boxes(a.tgt_boxes + (size_t)max(off, 0) * 4, nb, pred_b, valid_b, a.P, a.K, a.iou_det + (size_t)b * a.P, s_iou, lane, t);
        if (a.pred_masks) finish_mask(a.partials + (size_t)b * nchunks * 2, nchunks, true, lane, a.iou_seg + b, a.iu + b * 2, t);
        if (!room) continue;
        const int32_t* f = a.facts + (size_t)b * 6;
        const float oh = (float)f[2], ow = (float)f[3];
        float* rows = a.ring_boxes + ((size_t)slot * a.B + b) * a.P * 4;
        const int base = rt_eval_shared::write_scaled_rows(pred_b, valid_b, a.P, a.K, oh, ow, rows, lane);
        if (lane == 0) {
            a.ring_counts[(size_t)slot * a.B + b] = base;
            a.ring_ids[(size_t)slot * a.B + b] = a.image_ids[b];
        }
    }
    if (lane == 0 && keep) {
        t.store(a.acc);
        if (room) a.cursor[0] = slot + 1; else a.cursor[1] = 1;
    }
}

// rt_eval_facts: thread b gathers image b's int64 facts; the pointers ride in the argument block (2.1 KB of the 4 KB a launch carries)
struct EvalFactsArgs {
    const int64_t* size_ptr[RT_BATCH_STAGE_MAX_B]; const int64_t* orig_ptr[RT_BATCH_STAGE_MAX_B]; const int64_t* id_ptr[RT_BATCH_STAGE_MAX_B];
    int32_t tm_hw[2 * RT_BATCH_STAGE_MAX_B];
    int32_t* facts; int64_t* image_ids; int B;
};
static_assert(sizeof(EvalFactsArgs) <= 4096, "the argument block of a launch");

__global__ __launch_bounds__(RT_BATCH_STAGE_MAX_B) void eval_facts_kernel(const EvalFactsArgs a) {
    const int b = threadIdx.x;
    if (b >= a.B) return;
    const int64_t* sz = a.size_ptr[b];
    const int64_t* og = a.orig_ptr[b] ? a.orig_ptr[b] : sz;
    int32_t* f = a.facts + (size_t)b * 6;
    f[0] = (int32_t)sz[0]; f[1] = (int32_t)sz[1]; f[2] = (int32_t)og[0]; f[3] = (int32_t)og[1];
    f[4] = a.tm_hw[2 * b]; f[5] = a.tm_hw[2 * b + 1];
    a.image_ids[b] = a.id_ptr[b] ? a.id_ptr[b][0] : -1;
}

// rt_eval_raw_facts: thread b writes image b's rows from the values in the argument block (2.1 KB of the 4 KB a launch carries)
static_assert(sizeof(rt_eval_raw_facts_args) <= 4096, "the argument block of a launch");

__global__ __launch_bounds__(RT_BATCH_STAGE_MAX_B) void eval_raw_facts_kernel(const rt_eval_raw_facts_args a) {
    const int b = threadIdx.x;
    if (b >= a.B) return;
    int32_t* f = a.facts + (size_t)b * 6;
    f[0] = a.img_h[b]; f[1] = a.img_w[b]; f[2] = a.orig_h[b]; f[3] = a.orig_w[b];
    f[4] = a.img_h[b]; f[5] = a.img_w[b];                                    // the extent of what rt_raw_stage staged
    a.image_ids[b] = a.has_ids ? a.image_id[b] : -1;
    if (a.mask_table) a.mask_table[b] = (int64_t)reinterpret_cast<uintptr_t>(a.tm_ptr[b]);
}

// launch (b) of rt_eval_orig: finish_mask over the images in ascending order, each with the partials ITS pixels filled (what the mask
// launch in rt_post.hip wrote: both ask rt_eval_shared::orig_pixels), counted into the RT_EVAL_ORIG_* slots.
__global__ __launch_bounds__(64) void eval_orig_finish_kernel(const rt_eval_orig_args a, int nchunks) {
    const int lane = threadIdx.x;
    const bool keep = !a.veto || a.veto[0] == 0;                             // a vetoed batch leaves the totals alone
    long long* acc_i = reinterpret_cast<long long*>(a.acc);
    double* acc_d = reinterpret_cast<double*>(a.acc);
    totals t;                                                                // (its seg_* fields hold the original-frame totals here)
    if (lane == 0) {
        t.seg_n = acc_i[RT_EVAL_ORIG_N]; t.seg_i = acc_i[RT_EVAL_ORIG_I]; t.seg_u = acc_i[RT_EVAL_ORIG_U];
        for (int k = 0; k < 5; ++k) t.seg_hit[k] = acc_i[RT_EVAL_ORIG_HIT + k];
        t.seg_sum = acc_d[RT_EVAL_ORIG_SUM];
    }
    for (int b = 0; b < a.B; ++b) {
        const long long n = rt_eval_shared::orig_pixels(a.facts + (size_t)b * 6, a.mask_table[b], a.max_pixels);
        const int mine = (int)((n + RT_EVAL_CHUNK - 1) / RT_EVAL_CHUNK);
        finish_mask(a.partials + (size_t)b * nchunks * 2, mine, n > 0, lane, a.iou_seg + b, a.iu + b * 2, t);
    }
    if (lane == 0 && keep) {
        acc_i[RT_EVAL_ORIG_N] = t.seg_n; acc_i[RT_EVAL_ORIG_I] = t.seg_i; acc_i[RT_EVAL_ORIG_U] = t.seg_u;
        for (int k = 0; k < 5; ++k) acc_i[RT_EVAL_ORIG_HIT + k] = t.seg_hit[k];
        acc_d[RT_EVAL_ORIG_SUM] = t.seg_sum;
    }
}

}  // namespace

extern "C" int rt_eval_raw_facts(const rt_eval_raw_facts_args* a, rt_stream_t stream) {
    if (!a || !a->facts || !a->image_ids || a->B <= 0 || a->Hc <= 0 || a->Wc <= 0) return RT_ERR_BADARG;
    if (a->B > RT_BATCH_STAGE_MAX_B || a->max_pixels >= 0x80000000LL) return RT_ERR_UNSUPPORTED;
    for (int b = 0; b < a->B; ++b) {
        if (a->img_h[b] <= 0 || a->img_w[b] <= 0 || a->orig_h[b] <= 0 || a->orig_w[b] <= 0) return RT_ERR_BADARG;
        if (a->img_h[b] > a->Hc || a->img_w[b] > a->Wc) return RT_ERR_BADARG;
        if ((long long)a->orig_h[b] * a->orig_w[b] > a->max_pixels) return RT_ERR_BADARG;
        if (a->mask_table && !a->tm_ptr[b]) return RT_ERR_BADARG;
    }
    hipLaunchKernelGGL(eval_raw_facts_kernel, dim3(1), dim3(RT_BATCH_STAGE_MAX_B), 0, (hipStream_t)stream, *a);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_eval_orig(const rt_eval_orig_args* a, rt_stream_t stream) {
    if (!a || !a->pred_masks || !a->facts || !a->mask_table || !a->partials || !a->iou_seg || !a->iu || !a->acc) return RT_ERR_BADARG;
    if (a->B <= 0 || a->Q <= 0 || a->h <= 0 || a->w <= 0 || a->Hc <= 0 || a->Wc <= 0 || a->max_pixels <= 0) return RT_ERR_BADARG;
    if (a->B > RT_BATCH_STAGE_MAX_B || a->max_pixels >= 0x80000000LL) return RT_ERR_UNSUPPORTED;
    if ((long long)a->h * a->w >= 0x80000000LL || (long long)a->Hc * a->Wc >= 0x80000000LL) return RT_ERR_UNSUPPORTED;
    const int nchunks = (int)((a->max_pixels + RT_EVAL_CHUNK - 1) / RT_EVAL_CHUNK);
    const int rc = rt_eval_orig_launch_mask(*a, nchunks, (hipStream_t)stream);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(eval_orig_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a, nchunks);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_eval_metrics(const rt_eval_metrics_args* a, rt_stream_t stream) {
    if (!a || !a->pred_boxes || !a->valid || !a->table || !a->iou_det || !a->acc) return RT_ERR_BADARG;
    if (a->B <= 0 || a->P <= 0 || a->K <= 0) return RT_ERR_BADARG;
    int nchunks = 0;
    if (a->masks) {
        if (!a->sizes || !a->partials || !a->iou_seg || !a->iu) return RT_ERR_BADARG;
        if (a->Q <= 0 || a->max_h <= 0 || a->max_w <= 0 || a->B > 65535) return RT_ERR_BADARG;
        const long long px = (long long)a->max_h * a->max_w;
        if (px >= 0x7fffffffLL) return RT_ERR_UNSUPPORTED;
        nchunks = (int)((px + RT_EVAL_CHUNK - 1) / RT_EVAL_CHUNK);
        hipLaunchKernelGGL(eval_mask_kernel, dim3((unsigned)nchunks, (unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a, nchunks);
        RT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a, nchunks);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_eval_facts(const int64_t* const* size_ptrs, const int64_t* const* orig_ptrs, const int64_t* const* id_ptrs,
                             const int32_t* tm_hw, int B, int32_t* facts, int64_t* image_ids, rt_stream_t stream) {
    if (!size_ptrs || !facts || !image_ids || B <= 0) return RT_ERR_BADARG;
    if (B > RT_BATCH_STAGE_MAX_B) return RT_ERR_UNSUPPORTED;
    EvalFactsArgs a{};
    for (int b = 0; b < B; ++b) {
        if (!size_ptrs[b] || (orig_ptrs && !orig_ptrs[b]) || (id_ptrs && !id_ptrs[b])) return RT_ERR_BADARG;
        a.size_ptr[b] = size_ptrs[b];
        a.orig_ptr[b] = orig_ptrs ? orig_ptrs[b] : nullptr;
        a.id_ptr[b] = id_ptrs ? id_ptrs[b] : nullptr;
        a.tm_hw[2 * b] = tm_hw ? tm_hw[2 * b] : 0; a.tm_hw[2 * b + 1] = tm_hw ? tm_hw[2 * b + 1] : 0;
    }
    a.facts = facts; a.image_ids = image_ids; a.B = B;
    hipLaunchKernelGGL(eval_facts_kernel, dim3(1), dim3(RT_BATCH_STAGE_MAX_B), 0, (hipStream_t)stream, a);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_eval_canvas(const rt_eval_canvas_args* a, rt_stream_t stream) {
    if (!a || !a->pred_boxes || !a->valid || !a->tgt_boxes || !a->tgt_off || !a->facts || !a->image_ids || !a->iou_det || !a->acc)
        return RT_ERR_BADARG;
    if (!a->ring_boxes || !a->ring_counts || !a->ring_ids || !a->cursor) return RT_ERR_BADARG;
    if (a->B <= 0 || a->P <= 0 || a->K <= 0 || a->tgt_rows < 0 || a->slots <= 0) return RT_ERR_BADARG;
    if (a->B > RT_BATCH_STAGE_MAX_B) return RT_ERR_UNSUPPORTED;
    int nchunks = 0;
    if (a->pred_masks) {
        if (!a->tgt_masks || !a->partials || !a->iou_seg || !a->iu) return RT_ERR_BADARG;
        if (a->Q <= 0 || a->h <= 0 || a->w <= 0 || a->Hc <= 0 || a->Wc <= 0) return RT_ERR_BADARG;
        const long long px = (long long)a->Hc * a->Wc;
        if (px >= 0x7fffffffLL || (long long)a->h * a->w >= 0x7fffffffLL) return RT_ERR_UNSUPPORTED;
        nchunks = (int)((px + RT_EVAL_CHUNK - 1) / RT_EVAL_CHUNK);
        const int rc = rt_eval_canvas_launch_mask(*a, nchunks, (hipStream_t)stream);
        if (rc != RT_OK) return rc;
    }
    hipLaunchKernelGGL(eval_canvas_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a, nchunks);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
