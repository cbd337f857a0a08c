// The result tail of a prediction on the batch canvas (reftr_amd/predict.py): what rt_box_postprocess + rt_mask_postprocess's
// masks_origin give, with every per-batch fact in device memory, so that it sits inside the captured graph behind the forward.
//   rt_predict_facts   one launch per batch, OUTSIDE the graph: the images' sizes (host values, by value in the argument block) and
//                      the 16-byte block offsets of their masks -> the device `facts` table
//   rt_predict_canvas  (a) predict_boxes_kernel, one wave per image: rt_eval_canvas's ring rows (rt_eval_shared::write_scaled_rows)
//                      (b) the mask kernel, which takes mask decisions and therefore lives in rt_post.hip (rt_eval_shared.h says why)
// Latency-bound: a few hundred box rows, and one byte per original pixel from L2-resident logits.  No atomics.
#include "rt_eval_shared.h"

namespace {

// 16-byte units of a block of Q * oh * ow bytes
__host__ __device__ __forceinline__ long long block_units(int Q, int oh, int ow) { return ((long long)Q * oh * ow + 15) / 16; }

// thread b: image b's row.  Every thread adds up the B block sizes itself (B <= 64 additions): no LDS, no second pass.
__global__ __launch_bounds__(RT_BATCH_STAGE_MAX_B) void predict_facts_kernel(const rt_predict_facts_args a) {
    const int b = threadIdx.x;
    if (b >= a.B) return;
    long long off = 0, total = 0;
    for (int i = 0; i < a.B; ++i) {
        if (i == b) off = total;
        total += block_units(a.Q, a.orig_h[i], a.orig_w[i]);
    }
    int32_t* f = a.facts + (size_t)b * RT_PREDICT_FACTS_WORDS;
    f[0] = a.img_h[b]; f[1] = a.img_w[b]; f[2] = a.orig_h[b]; f[3] = a.orig_w[b];
    f[4] = (int32_t)off; f[5] = (int32_t)(off + block_units(a.Q, a.orig_h[b], a.orig_w[b])); f[6] = (int32_t)total; f[7] = 0;
}

__global__ __launch_bounds__(64) void predict_boxes_kernel(const rt_predict_canvas_args a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t* f = a.facts + (size_t)b * RT_PREDICT_FACTS_WORDS;
    const int n = rt_eval_shared::write_scaled_rows(a.pred_boxes + (size_t)b * a.P * a.K * 4, a.valid + (size_t)b * a.P * a.K, a.P, a.K,
                                                    (float)f[2], (float)f[3], a.out_boxes + (size_t)b * a.P * 4, lane);
    if (lane == 0) a.out_counts[b] = n;
}

}  // namespace

extern "C" int rt_predict_facts(const rt_predict_facts_args* a, rt_stream_t stream) {
    if (!a || !a->facts || a->B <= 0 || a->Q < 0 || a->capacity < 0 || a->Hc <= 0 || a->Wc <= 0) return RT_ERR_BADARG;
    if (a->B > RT_BATCH_STAGE_MAX_B) return RT_ERR_UNSUPPORTED;
    long long total = 0;
    for (int b = 0; b < a->B; ++b) {
        if (a->img_h[b] <= 0 || a->img_w[b] <= 0 || a->orig_h[b] <= 0 || a->orig_w[b] <= 0) return RT_ERR_BADARG;
        if (a->img_h[b] > a->Hc || a->img_w[b] > a->Wc) return RT_ERR_BADARG;
        total += block_units(a->Q, a->orig_h[b], a->orig_w[b]);
        if (16 * total >= 0x80000000LL) return RT_ERR_UNSUPPORTED;
    }
    if (16 * total > a->capacity) return RT_ERR_BADARG;
    hipLaunchKernelGGL(predict_facts_kernel, dim3(1), dim3(RT_BATCH_STAGE_MAX_B), 0, (hipStream_t)stream, *a);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_predict_canvas(const rt_predict_canvas_args* a, rt_stream_t stream) {
    if (!a || !a->pred_boxes || !a->valid || !a->facts || !a->out_boxes || !a->out_counts) return RT_ERR_BADARG;
    if (a->B <= 0 || a->P <= 0 || a->K <= 0) return RT_ERR_BADARG;
    if (a->B > RT_BATCH_STAGE_MAX_B) return RT_ERR_UNSUPPORTED;
    if (a->pred_masks) {
        if (!a->out_masks || a->capacity < 0 || (reinterpret_cast<uintptr_t>(a->out_masks) & 15) != 0) return RT_ERR_BADARG;
        if (a->Q <= 0 || a->h <= 0 || a->w <= 0 || a->Hc <= 0 || a->Wc <= 0) return RT_ERR_BADARG;
        if (a->capacity >= 0x80000000LL || (long long)a->h * a->w >= 0x7fffffffLL || (long long)a->Hc * a->Wc >= 0x7fffffffLL)
            return RT_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(predict_boxes_kernel, dim3((unsigned)a->B), dim3(64), 0, (hipStream_t)stream, *a);
    RT_CHECK_LAUNCH();
    if (a->pred_masks) return rt_predict_canvas_launch_mask(*a, (int)(a->capacity / 16), (hipStream_t)stream);
    return RT_OK;
}
