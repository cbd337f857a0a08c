// Host input pipeline on the device: Pillow-compatible antialiased bilinear resampling of uint8 images
// (datasets/transforms.py:81-116 -> torchvision F.resize on PIL images -> Pillow ImagingResample, 8-bit path) and
// ToTensor + Normalize + batch padding (transforms.py:233-263, util/collate_fn.py:24-41) in one pass.
// Integer / byte work, HBM-bound: bit-exact by construction -- the 22-bit fixed-point filter taps are computed on the host
// in double precision exactly as Pillow does (reftr_amd/data/resample.py) and the kernels only multiply-accumulate int32.
#include "rt_stage.h"

namespace {

// One resampling pass along `axis` (0 = rows / vertical, 1 = columns / horizontal) of src[n0][n1][C] (uint8):
// out[i][j][c] = clip8(2^21 + sum_t src[..][lo + t][..] * k[t]); bounds[o] = {lo, n taps}, coeffs[o][ksize].
__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const int* __restrict__ bounds, const int* __restrict__ coeffs,
                                                          int n0, int n1, int C, int out_len, int ksize, int axis) {
    const int o0 = axis == 0 ? out_len : n0, o1 = axis == 1 ? out_len : n1;
    const size_t total = (size_t)o0 * o1 * C;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C); const size_t t = i / C;
        const int x = (int)(t % o1), y = (int)(t / o1);
        const int o = axis == 0 ? y : x;
        const int lo = bounds[2 * o], n = bounds[2 * o + 1];
        const int* k = coeffs + (size_t)o * ksize;
        int acc = RT_RESAMPLE_HALF;
        if (axis == 1) {
            const uint8_t* s = src + ((size_t)y * n1 + lo) * C + c;
            for (int j = 0; j < n; ++j) acc += (int)s[(size_t)j * C] * k[j];
        } else {
            const uint8_t* s = src + ((size_t)lo * n1 + x) * C + c;
            for (int j = 0; j < n; ++j) acc += (int)s[(size_t)j * n1 * C] * k[j];
        }
        dst[i] = rt_clip8(acc);
    }
}

// tab[b] = {device pointer of image b (uint8 [h][w][3]), h, w}; out[b][c][y][x] = (u8/255 - mean[c]) / std[c] inside the
// image, 0 in the padding; mask[b][y][x] = 1 in the padding (NestedTensor convention: True = padded).
__global__ __launch_bounds__(256) void collate_norm_kernel(const long long* __restrict__ tab, float* __restrict__ out,
                                                           uint8_t* __restrict__ mask, int B, int H, int W,
                                                           float m0, float m1, float m2, float s0, float s1, float s2) {
    const size_t total = (size_t)B * H * W;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % W); const size_t t = i / W; const int y = (int)(t % H); const int b = (int)(t / H);
        const uint8_t* img = reinterpret_cast<const uint8_t*>(tab[3 * b]);
        const int h = (int)tab[3 * b + 1], w = (int)tab[3 * b + 2];
        const bool in = y < h && x < w;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (in) {
            const uint8_t* px = img + ((size_t)y * w + x) * 3;
            v0 = rt_norm_u8(px[0], m0, s0); v1 = rt_norm_u8(px[1], m1, s1); v2 = rt_norm_u8(px[2], m2, s2);
        }
        const size_t plane = (size_t)H * W, o = (size_t)b * 3 * plane + (size_t)y * W + x;
        out[o] = v0; out[o + plane] = v1; out[o + 2 * plane] = v2;
        mask[i] = in ? 0 : 1;
    }
}

// ---- rt_batch_stage: one batch of any size into the fixed canvas buffers a captured step reads.
// Every per-batch fact rides in the kernel argument block (1.9 KB of the 4 KB a launch carries): no device table, so no host -> device
// copy and no host synchronisation between two replays.  The index space is [image units | mask units | target-mask units | box words];
// a unit is one 16-byte store where the destination rows allow it (W_c % 4 == 0 for fp32, W_c % 16 == 0 for bytes, 16-byte aligned base),
// else one element.  Sources are read with one 16-byte load when the four / sixteen elements lie inside the row at an aligned address,
// element by element otherwise (source row starts are aligned only by accident).  Plain loads and stores: the same bits every run.
struct BatchStageArgs {
    const float* src_img; const uint8_t* src_mask; float* img; uint8_t* mask;
    float* boxes; int32_t* tgt_off; float* num_boxes; uint8_t* tgt_masks;
    int B, hs, ws, Hc, Wc, box_rows;
    int img_vec, mask_vec, tm_vec;                 // elements per unit: 4 | 1 (fp32), 16 | 1 (bytes)
    unsigned n_img, n_mask, n_tm, n_box;           // units per segment
    const float* box_ptr[RT_BATCH_STAGE_MAX_B]; const uint8_t* tm_ptr[RT_BATCH_STAGE_MAX_B];
    int32_t box_n[RT_BATCH_STAGE_MAX_B], tm_h[RT_BATCH_STAGE_MAX_B], tm_w[RT_BATCH_STAGE_MAX_B];
};
static_assert(sizeof(BatchStageArgs) <= 4096, "the argument block of a launch");

// unit u of a [planes][Hc][Wc] destination with `vec` elements per unit: plane p, row y, first column x
__device__ __forceinline__ void unit_at(unsigned u, int vec, int Hc, int Wc, int& p, int& y, int& x) {
    const unsigned ru = (unsigned)(Wc / vec), t = u / ru;
    x = (int)(u % ru) * vec; y = (int)(t % (unsigned)Hc); p = (int)(t / (unsigned)Hc);
}

// the unit at (p, y, x) of a [planes][Hc][Wc] destination <- src[h][w] (plane p's source), `fill` outside: one element (vec == 1), or the
// 16-byte unit of rt_stage.h, read with one 16-byte load when it lies inside the source row at an aligned address
__device__ __forceinline__ void stage_unit(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int h, int w, int Hc, int Wc, int vec,
                                           int p, int y, int x, uint8_t fill) {
    uint8_t* d = dst + ((size_t)p * Hc + y) * Wc + x;
    const uint8_t* s = src + (size_t)y * w + x;
    if (vec == 1) { *d = (y < h && x < w) ? *s : fill; return; }
    rt_bytes16 v;
    if (y < h && x + 15 < w && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        v.q = *reinterpret_cast<const uint4*>(s);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) v.e[j] = (y < h && x + j < w) ? s[j] : fill;
    }
    rt_store_unit(d, v, true, x, Wc);
}
__device__ __forceinline__ void stage_unit(float* __restrict__ dst, const float* __restrict__ src, int h, int w, int Hc, int Wc, int vec,
                                           int p, int y, int x, float fill) {
    float* d = dst + ((size_t)p * Hc + y) * Wc + x;
    const float* s = src + (size_t)y * w + x;
    if (vec == 1) { *d = (y < h && x < w) ? *s : fill; return; }
    float v[4] = {fill, fill, fill, fill};
    if (y < h && x + 3 < w && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(s);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if (y < h) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (x + j < w) v[j] = s[j];
    }
    *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
}

__global__ __launch_bounds__(256) void batch_stage_kernel(const BatchStageArgs a) {
    const size_t total = (size_t)a.n_img + a.n_mask + a.n_tm + a.n_box;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        int p, y, x;
        size_t j = i;
        if (j < a.n_img) {                                // p = b * 3 + c
            unit_at((unsigned)j, a.img_vec, a.Hc, a.Wc, p, y, x);
            stage_unit(a.img, a.src_img + (size_t)p * a.hs * a.ws, a.hs, a.ws, a.Hc, a.Wc, a.img_vec, p, y, x, 0.f);
            continue;
        }
        j -= a.n_img;
        if (j < a.n_mask) {
            unit_at((unsigned)j, a.mask_vec, a.Hc, a.Wc, p, y, x);
            stage_unit(a.mask, a.src_mask + (size_t)p * a.hs * a.ws, a.hs, a.ws, a.Hc, a.Wc, a.mask_vec, p, y, x, (uint8_t)1);
            continue;
        }
        j -= a.n_mask;
        if (j < a.n_tm) {
            unit_at((unsigned)j, a.tm_vec, a.Hc, a.Wc, p, y, x);
            stage_unit(a.tgt_masks, a.tm_ptr[p], a.tm_h[p], a.tm_w[p], a.Hc, a.Wc, a.tm_vec, p, y, x, (uint8_t)0);
            continue;
        }
        j -= a.n_tm;
        const int k = (int)j, nbox = a.box_rows * 4;
        if (k < nbox) {                                   // boxes[box_rows][4]: packed in image order, zero behind the last box
            const int r = k >> 2, c = k & 3;
            float v = 0.f;
            int off = 0;
            for (int b = 0; b < a.B; ++b) {
                const int n = a.box_n[b];
                if (r >= off && r < off + n) v = a.box_ptr[b][(size_t)(r - off) * 4 + c];
                off += n;
            }
            a.boxes[k] = v;
        } else {                                          // tgt_off[0 .. B] (exclusive prefix sums), then num_boxes
            const int b = k - nbox;
            int off = 0;
            for (int q = 0; q < (b < a.B ? b : a.B); ++q) off += a.box_n[q];
            if (b <= a.B) a.tgt_off[b] = off;
            else a.num_boxes[0] = (float)off;
        }
    }
}

}  // namespace

extern "C" int rt_batch_stage(const float* src_img, const uint8_t* src_mask, int B, int hs, int ws, float* img, uint8_t* mask,
                              int Hc, int Wc, const float* const* box_ptrs, const int32_t* box_counts, int boxes_per_image,
                              float* boxes, int32_t* tgt_off, float* num_boxes, const uint8_t* const* tm_ptrs, const int32_t* tm_hw,
                              uint8_t* tgt_masks, rt_stream_t stream) {
    if (!src_img || !src_mask || !img || !mask || !box_ptrs || !box_counts || !boxes || !tgt_off || !num_boxes) return RT_ERR_BADARG;
    if (B <= 0 || hs <= 0 || ws <= 0 || Hc <= 0 || Wc <= 0 || boxes_per_image <= 0) return RT_ERR_BADARG;
    if ((tm_ptrs || tm_hw || tgt_masks) && !(tm_ptrs && tm_hw && tgt_masks)) return RT_ERR_BADARG;
    if (B > RT_BATCH_STAGE_MAX_B) return RT_ERR_UNSUPPORTED;
    if (hs > Hc || ws > Wc) return RT_ERR_BADARG;
    BatchStageArgs a{};
    for (int b = 0; b < B; ++b) {
        const int n = box_counts[b];
        if (!rt_stage_boxes_ok(n, box_ptrs[b], boxes_per_image)) return RT_ERR_BADARG;
        a.box_ptr[b] = box_ptrs[b]; a.box_n[b] = n;
        if (tm_ptrs) {
            const int h = tm_hw[2 * b], w = tm_hw[2 * b + 1];
            if (!tm_ptrs[b] || h <= 0 || w <= 0 || h > Hc || w > Wc) return RT_ERR_BADARG;
            a.tm_ptr[b] = tm_ptrs[b]; a.tm_h[b] = h; a.tm_w[b] = w;
        }
    }
    const size_t plane = (size_t)Hc * Wc;
    if ((size_t)B * 3 * plane >= ((size_t)1 << 32) || rt_box_tail_words(B, boxes_per_image) >= ((size_t)1 << 31)) return RT_ERR_UNSUPPORTED;
    a.src_img = src_img; a.src_mask = src_mask; a.img = img; a.mask = mask;
    a.boxes = boxes; a.tgt_off = tgt_off; a.num_boxes = num_boxes; a.tgt_masks = tgt_masks;
    a.B = B; a.hs = hs; a.ws = ws; a.Hc = Hc; a.Wc = Wc; a.box_rows = B * boxes_per_image;
    a.img_vec = rt_stage_vec(Wc, img, 4); a.mask_vec = rt_stage_vec(Wc, mask, 16); a.tm_vec = rt_stage_vec(Wc, tgt_masks, 16);   // each on its own
    a.n_img = (unsigned)((size_t)B * 3 * plane / a.img_vec);
    a.n_mask = (unsigned)((size_t)B * plane / a.mask_vec);
    a.n_tm = tgt_masks ? (unsigned)((size_t)B * plane / a.tm_vec) : 0u;
    a.n_box = (unsigned)rt_box_tail_words(B, boxes_per_image);
    const size_t total = (size_t)a.n_img + a.n_mask + a.n_tm + a.n_box;
    size_t blocks = (total + 255) / 256; if (blocks > 2048) blocks = 2048;       // 256 CUs x 8 workgroups, grid-stride beyond
    hipLaunchKernelGGL(batch_stage_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_resample_u8(const void* src, void* dst, const int32_t* bounds, const int32_t* coeffs, int n0, int n1, int C,
                              int out_len, int ksize, int axis, rt_stream_t stream) {
    if (!src || !dst || !bounds || !coeffs) return RT_ERR_BADARG;
    if (n0 <= 0 || n1 <= 0 || C <= 0 || out_len <= 0 || ksize <= 0 || (axis != 0 && axis != 1)) return RT_ERR_BADARG;
    const size_t total = (size_t)(axis == 0 ? out_len : n0) * (axis == 1 ? out_len : n1) * C;
    size_t blocks = (total + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,
                       (uint8_t*)dst, bounds, coeffs, n0, n1, C, out_len, ksize, axis);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_img_collate_norm(const int64_t* table, float* out, uint8_t* mask, int B, int H, int W, const float* mean3,
                                   const float* std3, rt_stream_t stream) {
    if (!table || !out || !mask || !mean3 || !std3 || B <= 0 || H <= 0 || W <= 0) return RT_ERR_BADARG;
    size_t blocks = ((size_t)B * H * W + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(collate_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const long long*)table, out,
                       mask, B, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
