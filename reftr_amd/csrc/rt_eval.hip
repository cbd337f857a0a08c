// The metric stage of engine_vg.evaluate (engine_vg.py:127-152) as two launches per batch, running totals on the device:
//   eval_mask_kernel    grid (chunk, image): integer intersection / union counts of query 0's post-processed mask against the
//                       image's target mask over one run of RT_EVAL_CHUNK pixels, stored (plain stores) to the workgroup's own slot
//   eval_finish_kernel  ONE wave, image ascending then row ascending: box IoU of every valid phrase against its target box
//                       (util/box_ops.py's arithmetic, un-fused, in its order -> the bits of diag(box_iou)), the mask partials added
//                       up per image, and the 16 running accumulators (counts int64, the two IoU sums double) updated in that order
// No floating-point atomics and nothing to clear beforehand: the same bits from run to run.  Latency-bound (0.4 MB per 640 x 640
// image, a few hundred box rows): byte loads, one thread per pixel, and a serial walk over the rows for the ordered double sums.
#include "rt_common.h"

// The box arithmetic must keep torch's roundings: one per operation.  HIP's __fmul_rn / __fadd_rn / __fsub_rn are plain operators
// defined in a header, under the compiler's default contraction: inlined here, a product feeding a sum still becomes one fused
// operation ((a1 + a2) - inter with a2 and inter products lost two roundings that way).  So contraction is switched off for this
// file and the operations are spelled with the operators of this file (nothing in it gains from contraction).
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
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

// the image's scored rectangle: sizes[b], never past the target's own extent or the frame (equal to sizes[b] for consistent input)
__device__ __forceinline__ void scored_rect(const rt_eval_metrics_args& a, int b, int th, int tw, int& ih, int& iw) {
    ih = min(min(a.sizes[b * 2], th), a.max_h);
    iw = min(min(a.sizes[b * 2 + 1], tw), a.max_w);
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
        scored_rect(a, b, (int)row[3], tw, ih, iw);
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
    I = wave_sum_int(I); U = wave_sum_int(U);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm[wid * 2] = I; sm[wid * 2 + 1] = U; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t* o = a.partials + ((size_t)b * nchunks + c) * 2;
        o[0] = (sm[0] + sm[2]) + (sm[4] + sm[6]);
        o[1] = (sm[1] + sm[3]) + (sm[5] + sm[7]);
    }
}

__device__ __forceinline__ void count_sample(float v, long long& n, long long* hit, double& sum) {
    const float thr[5] = {0.5f, 0.6f, 0.7f, 0.8f, 0.9f};
    n += 1;
#pragma unroll
    for (int t = 0; t < 5; ++t) hit[t] += v > thr[t] ? 1 : 0;
    sum += (double)v;
}

__global__ __launch_bounds__(64) void eval_finish_kernel(const rt_eval_metrics_args a, int nchunks) {
    __shared__ float s_iou[64];
    const int lane = threadIdx.x;
    long long* acc_i = reinterpret_cast<long long*>(a.acc);
    double* acc_d = reinterpret_cast<double*>(a.acc);
    // lane 0 owns the running totals
    long long det_n = 0, det_hit[5] = {0, 0, 0, 0, 0}, seg_n = 0, seg_hit[5] = {0, 0, 0, 0, 0}, seg_i = 0, seg_u = 0;
    double det_sum = 0.0, seg_sum = 0.0;
    if (lane == 0 && !a.reset) {
        det_n = acc_i[RT_EVAL_DET_N]; seg_n = acc_i[RT_EVAL_SEG_N];
        for (int t = 0; t < 5; ++t) { det_hit[t] = acc_i[RT_EVAL_DET_HIT + t]; seg_hit[t] = acc_i[RT_EVAL_SEG_HIT + t]; }
        seg_i = acc_i[RT_EVAL_SEG_I]; seg_u = acc_i[RT_EVAL_SEG_U];
        det_sum = acc_d[RT_EVAL_DET_SUM]; seg_sum = acc_d[RT_EVAL_SEG_SUM];
    }
    for (int b = 0; b < a.B; ++b) {
        const int64_t* row = a.table + (size_t)b * 5;
        const float* tb = reinterpret_cast<const float*>(row[0]);
        const int nb = tb ? (int)min((long long)a.P, max(0ll, (long long)row[1])) : 0;
        float* out = a.iou_det + (size_t)b * a.P;
        int base = 0, rank;
        for (int j0 = 0; j0 < a.P && base < nb; j0 += 64) {
            const int ph = j0 + lane, before = base;
            const bool mine = rt_phrase_rank(a.valid + (size_t)b * a.P * a.K, a.P, a.K, ph, lane, base, rank);
            if (mine && rank < nb) {
                const float v = box_iou_pair(to_xyxy(tb + (size_t)rank * 4), to_xyxy(a.pred_boxes + ((size_t)(b * a.P + ph) * a.K) * 4));
                out[rank] = v;
                s_iou[rank - before] = v;
            }
            __syncthreads();
            if (lane == 0) {
                const int m = min(base, nb) - before;
                for (int i = 0; i < m; ++i) count_sample(s_iou[i], det_n, det_hit, det_sum);
            }
            __syncthreads();
        }
        for (int r = min(base, nb) + lane; r < a.P; r += 64) out[r] = 0.f;
        if (!a.masks) continue;
        long long I = 0, U = 0;
        const bool scored = row[2] != 0;
        if (scored) {
            const int32_t* pp = a.partials + (size_t)b * nchunks * 2;
            for (int c = lane; c < nchunks; c += 64) { I += pp[c * 2]; U += pp[c * 2 + 1]; }
            I = wave_sum_i64(I); U = wave_sum_i64(U);              // integers: exact in any order
        }
        if (lane == 0) {
            const float v = scored ? __fdiv_rn((float)I, (float)U) : 0.f;
            a.iou_seg[b] = v; a.iu[b * 2] = I; a.iu[b * 2 + 1] = U;
            if (scored) { count_sample(v, seg_n, seg_hit, seg_sum); seg_i += I; seg_u += U; }
        }
    }
    if (lane == 0) {
        acc_i[RT_EVAL_DET_N] = det_n; acc_i[RT_EVAL_SEG_N] = seg_n;
        for (int t = 0; t < 5; ++t) { acc_i[RT_EVAL_DET_HIT + t] = det_hit[t]; acc_i[RT_EVAL_SEG_HIT + t] = seg_hit[t]; }
        acc_i[RT_EVAL_SEG_I] = seg_i; acc_i[RT_EVAL_SEG_U] = seg_u;
        acc_d[RT_EVAL_DET_SUM] = det_sum; acc_d[RT_EVAL_SEG_SUM] = seg_sum;
    }
}

}  // namespace

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
