// rt_raw_stage: a batch of raw uint8 images, pixel boxes and raw-sized target masks into the canvas buffers of a captured step, one
// launch (include/reftr_hip.h).  It writes the bytes of the chain rt_resample_u8 (horizontal) -> rt_resample_u8 (vertical) ->
// rt_img_collate_norm(pad_to) -> DeviceInputPipeline._target -> rt_batch_stage (rt_input.hip, reftr_amd/data/device_input.py), so every
// expression that rounds is written as it is there, and nothing in this file may be contracted into a fused multiply-add:
#pragma clang fp contract(off)
#include "rt_stage.h"

namespace {

constexpr int TH = RT_RAW_STAGE_TILE_H, TW = RT_RAW_STAGE_TILE_W;
constexpr int KMAX = 2 * RT_RAW_STAGE_MAX_SCALE + 1;                 // taps per output index at the largest down-scale
// Source rows under one tile: the first and last output rows' centres lie (TH - 1) * scale apart, each reaches `support` = scale to
// either side, and the two int() truncations add one: (TH - 1) * S + 2 * S + 1 at S = RT_RAW_STAGE_MAX_SCALE.
constexpr int ROWS_MAX = (TH + 1) * RT_RAW_STAGE_MAX_SCALE + 1;
constexpr int ROW_BYTES = TW * 3;
// The LDS budget of a tile: 4.1 KB of taps + 3 KB of normalised values per byte and channel (static) + the intermediate rows (dynamic:
// what the steepest image of the batch needs, at most ROWS_MAX * ROW_BYTES = 24.9 KB).  An up-scaling batch asks for 14 KB in all and
// runs seven workgroups per compute unit (the kernel's 68 registers allow no more); the steepest admitted one 32.1 KB, four.
static_assert(ROWS_MAX * ROW_BYTES + (TW + TH) * (KMAX + 2) * 4 + 3 * 256 * 4 <= 40 * 1024, "the LDS budget of a tile: four workgroups per compute unit");
static_assert(((TW + TH) * (KMAX + 2) * 4 + 3 * 256 * 4) % 16 == 0, "the dynamic LDS base stays 16-byte aligned");
static_assert(sizeof(rt_raw_stage_args) + 5 * 4 <= 4096, "the argument block of a launch");
static_assert(TW % 16 == 0 && TH * (TW / 16) <= 256, "one 16-byte unit of a byte plane per thread");

// reftr_amd/data/resample.py taps(), output index xx: IEEE doubles, int() = truncation toward zero, the weights summed in order.
// k[0 .. cap) receives the 22-bit coefficients, zero behind the count; the count is clamped to cap (only reachable beyond the scale the
// entry points admit).
__device__ void resample_taps(int in_size, int out_size, int xx, int cap, int* lo, int* cnt, int* k) {
    const double scale = (double)in_size / (double)out_size;
    const double fscale = scale > 1.0 ? scale : 1.0;
    const double support = 1.0 * fscale;
    const double ss = 1.0 / fscale;
    const double one = (double)(1 << RT_PRECISION_BITS);
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    int n = xmax - xmin;
    if (n > cap) n = cap;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        const double a = fabs(((double)(x + xmin) - center + 0.5) * ss);
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int x = 0; x < cap; ++x) {
        int c = 0;
        if (x < n) {
            const double a = fabs(((double)(x + xmin) - center + 0.5) * ss);
            double v = a < 1.0 ? 1.0 - a : 0.0;
            if (ww != 0.0) v = v / ww;
            c = v < 0.0 ? (int)(-0.5 + v * one) : (int)(0.5 + v * one);
        }
        k[x] = c;
    }
    *lo = xmin; *cnt = n;
}

__global__ __launch_bounds__(256) void resample_taps_kernel(int in_size, int out_size, int* __restrict__ bounds, int* __restrict__ coeffs,
                                                            int ksize) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= out_size) return;
    int lo, n;
    resample_taps(in_size, out_size, o, ksize, &lo, &n, coeffs + (size_t)o * ksize);
    bounds[2 * o] = lo; bounds[2 * o + 1] = n;
}

// 2^21 + sum_j s[j * stride] * k[j] over the `last + 1` taps of one output index, as NT independent loads: k[] is zero behind the count
// (resample_taps), so the taps behind it re-read the last one and add nothing.  A loop over the count would wait for every load in turn.
template <int NT>
__device__ __forceinline__ int dot_taps(const uint8_t* s, int stride, const int* k, int last) {
    int acc = RT_RESAMPLE_HALF;
#pragma unroll
    for (int j = 0; j < NT; ++j) acc += (int)s[(j < last ? j : last) * stride] * k[j];
    return acc;
}

// Horizontal pass into LDS: thread xc < ROW_BYTES owns byte column xc (pixel xc / 3, channel xc % 3) of the tile's intermediate rows --
// its first index and coefficients stay in registers -- and walks the source rows; three of the four waves, none of them partial.
template <int NT>
__device__ __forceinline__ void horizontal_pass(uint8_t* rows, const uint8_t* src, int w, int row_lo, int nrows, int nx, const int* h_lo,
                                                const int* h_n, const int* h_k, int xc) {
    if (xc >= nx * 3) return;
    const int xl = xc / 3, last = h_n[xl] > 0 ? h_n[xl] - 1 : 0;
    int k[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) k[j] = h_k[xl * KMAX + j];
    const uint8_t* s = src + ((size_t)row_lo * w + h_lo[xl]) * 3 + xc % 3;
    for (int r = 0; r < nrows; ++r, s += (size_t)w * 3) rows[r * ROW_BYTES + xc] = rt_clip8(dot_taps<NT>(s, 3, k, last));
}

// torch's `nearest` source index (upsample_nearest2d: fp32 scale, fp32 product)
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
    const int s = (int)floorf((float)dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

// workgroups [0, B * tiles): one tile of one image; workgroup B * tiles: the boxes, their offsets and their count
__global__ __launch_bounds__(256) void raw_stage_kernel(const rt_raw_stage_args a, int tiles_x, int tiles_y, int img_vec, int byte_vec,
                                                        int rows_cap) {
    __shared__ int h_lo[TW], h_n[TW], h_k[TW * KMAX], v_lo[TH], v_n[TH], v_k[TH * KMAX];
    __shared__ float norm[3 * 256];                       // ToTensor + Normalize of every byte value, per channel
    extern __shared__ __align__(16) uint8_t rows[];       // [rows_cap][ROW_BYTES]
    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    if (b >= a.B) {
        // batch_stage_kernel's box tail (rt_input.hip) with the xyxy-pixels -> cxcywh-normalised value of a live word; why the two are
        // not one function: DESIGN.md, rt_raw_stage
        const int nbox = a.B * a.boxes_per_image * 4;
        for (int k = tid; k < nbox + a.B + 2; k += 256) {
            if (k < nbox) {                               // boxes[B * boxes_per_image][4]: packed in image order, zero behind the last box
                const int r = k >> 2, c = k & 3;
                float v = 0.f;
                int off = 0;
                for (int q = 0; q < a.B; ++q) {
                    const int n = a.box_n[q];
                    if (r >= off && r < off + n) {
                        const float* p = a.box_ptr[q] + (size_t)(r - off) * 4;
                        const float lo = p[c & 1] * ((c & 1) ? a.rh[q] : a.rw[q]), hi = p[2 + (c & 1)] * ((c & 1) ? a.rh[q] : a.rw[q]);
                        const float e = c < 2 ? (lo + hi) / 2 : hi - lo;
                        v = e / (float)((c & 1) ? a.oh[q] : a.ow[q]);
                    }
                    off += n;
                }
                a.boxes[k] = v;
            } else {                                      // tgt_off[0 .. B] (exclusive prefix sums), then num_boxes
                const int q = k - nbox;
                int off = 0;
                for (int i = 0; i < (q < a.B ? q : a.B); ++i) off += a.box_n[i];
                if (q <= a.B) a.tgt_off[q] = off;
                else a.num_boxes[0] = (float)off;
            }
        }
        return;
    }
    const int t = (int)(blockIdx.x % (unsigned)tiles);
    const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
    const int Hc = a.Hc, Wc = a.Wc;
    const int h = a.h[b], w = a.w[b], oh = a.oh[b], ow = a.ow[b];
    const bool live = y0 < oh && x0 < ow;                 // (the same for the whole workgroup)
    const int nx = live ? (ow - x0 < TW ? ow - x0 : TW) : 0, ny = live ? (oh - y0 < TH ? oh - y0 : TH) : 0;
    // the two byte planes first, one 16-byte unit per thread: threads [0, 128) the padding mask, [128, 256) the target mask, whose loads
    // are then under way while the first two waves compute the taps
    constexpr int UNITS = TH * (TW / 16);
    const int plane = tid / UNITS, u = tid % UNITS;
    if (plane == 0 || (plane == 1 && a.tgt_masks)) {
        const int yl = u / (TW / 16), xl = (u % (TW / 16)) * 16;
        const int y = y0 + yl, x = x0 + xl;
        if (y < Hc && x < Wc) {
            rt_bytes16 v;
            if (plane == 0) {
#pragma unroll
                for (int j = 0; j < 16; ++j) v.e[j] = (y < oh && x + j < ow) ? 0 : 1;
            } else {
                const uint8_t* s = a.tm_ptr[b];
                const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
                const size_t row = y < oh ? (size_t)nearest_src(y, sy, h) * w : 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) v.e[j] = (y < oh && x + j < ow) ? (s[row + nearest_src(x + j, sx, w)] != 0 ? 1 : 0) : 0;
            }
            rt_store_unit((plane == 0 ? a.mask : a.tgt_masks) + ((size_t)b * Hc + y) * Wc + x, v, byte_vec == 16, x, Wc);
        }
    }
    int row_lo = 0;
    const bool up = h <= oh && w <= ow;                   // no axis shrinks: support 1, at most three taps per output index
    if (live) {
        const int cap = up ? 3 : KMAX;                    // the coefficients the passes read
        if (tid < nx) resample_taps(w, ow, x0 + tid, cap, &h_lo[tid], &h_n[tid], &h_k[tid * KMAX]);
        else if (tid >= TW && tid - TW < ny) resample_taps(h, oh, y0 + tid - TW, cap, &v_lo[tid - TW], &v_n[tid - TW], &v_k[(tid - TW) * KMAX]);
        for (int i = tid; i < 3 * 256; i += 256) norm[i] = rt_norm_u8((uint8_t)(i & 255), a.mean[i >> 8], a.std[i >> 8]);
        __syncthreads();
        // horizontal pass of the source rows [row_lo, row_lo + nrows) the tile's vertical taps read (first indices and ends both
        // grow with the output index), columns x0 .. x0 + nx, into LDS as bytes
        row_lo = v_lo[0];
        int nrows = v_lo[ny - 1] + v_n[ny - 1] - row_lo;
        if (nrows > rows_cap) nrows = rows_cap;
        if (up) horizontal_pass<3>(rows, a.src[b], w, row_lo, nrows, nx, h_lo, h_n, h_k, tid);
        else horizontal_pass<KMAX>(rows, a.src[b], w, row_lo, nrows, nx, h_lo, h_n, h_k, tid);
        __syncthreads();
    }
    // vertical pass from LDS, ToTensor + Normalize: thread (tid / 16, tid % 16) owns four columns of rows tid / 16 and tid / 16 + 16, whose
    // taps serve the three channels; zeros outside oh x ow (ny = nx = 0 on a tile that lies in the padding altogether)
    static_assert(TW == 64 && TH == 32, "256 threads: 16 column groups x 16 rows, two rows each");
    const int xl = (tid % 16) * 4, x = x0 + xl;
    for (int yl = tid / 16; yl < TH; yl += 16) {
        const int y = y0 + yl;
        if (y >= Hc || x >= Wc) continue;
        const bool inside = yl < ny && xl < nx;
        const uint8_t* s = rows + (inside ? (v_lo[yl] - row_lo) * ROW_BYTES + xl * 3 : 0);
        const int* k = &v_k[(inside ? yl : 0) * KMAX];
        const int last = inside && v_n[yl] > 0 ? v_n[yl] - 1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (inside) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (xl + e < nx) {
                        const int acc = up ? dot_taps<3>(s + e * 3 + c, ROW_BYTES, k, last) : dot_taps<KMAX>(s + e * 3 + c, ROW_BYTES, k, last);
                        v[e] = norm[c * 256 + rt_clip8(acc)];
                    }
                }
            }
            float* d = a.img + (((size_t)b * 3 + c) * Hc + y) * Wc + x;       // (written out like the box tail: DESIGN.md)
            if (img_vec == 4) {
                *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (x + e < Wc) d[e] = v[e];
            }
        }
    }
}

int taps_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    return (int)ceil(scale > 1.0 ? scale : 1.0) * 2 + 1;
}

}  // namespace

extern "C" int rt_resample_taps(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize, rt_stream_t stream) {
    if (!bounds || !coeffs || in_size <= 0 || out_size <= 0 || ksize < taps_ksize(in_size, out_size)) return RT_ERR_BADARG;
    hipLaunchKernelGGL(resample_taps_kernel, dim3((unsigned)((out_size + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in_size, out_size,
                       bounds, coeffs, ksize);
    RT_CHECK_LAUNCH();
    return RT_OK;
}

extern "C" int rt_raw_stage(const rt_raw_stage_args* a, rt_stream_t stream) {
    if (!a || !a->img || !a->mask || !a->boxes || !a->tgt_off || !a->num_boxes) return RT_ERR_BADARG;
    const int B = a->B, Hc = a->Hc, Wc = a->Wc;
    if (B <= 0 || Hc <= 0 || Wc <= 0 || a->boxes_per_image <= 0) return RT_ERR_BADARG;
    if (B > RT_BATCH_STAGE_MAX_B) return RT_ERR_UNSUPPORTED;
    bool too_steep = false;
    for (int b = 0; b < B; ++b) {
        const int n = a->box_n[b];
        if (!a->src[b] || a->h[b] <= 0 || a->w[b] <= 0 || a->oh[b] <= 0 || a->ow[b] <= 0 || a->oh[b] > Hc || a->ow[b] > Wc) return RT_ERR_BADARG;
        if (!rt_stage_boxes_ok(n, a->box_ptr[b], a->boxes_per_image) || (a->tgt_masks && !a->tm_ptr[b])) return RT_ERR_BADARG;
        too_steep = too_steep || (int64_t)a->h[b] > (int64_t)RT_RAW_STAGE_MAX_SCALE * a->oh[b]
                    || (int64_t)a->w[b] > (int64_t)RT_RAW_STAGE_MAX_SCALE * a->ow[b];
    }
    const int tiles_x = (Wc + TW - 1) / TW, tiles_y = (Hc + TH - 1) / TH;
    const size_t blocks = (size_t)B * tiles_x * tiles_y + 1;
    if (too_steep || (size_t)Hc * Wc >= ((size_t)1 << 31) || blocks >= ((size_t)1 << 31)
        || rt_box_tail_words(B, a->boxes_per_image) >= ((size_t)1 << 31)) return RT_ERR_UNSUPPORTED;
    const int img_vec = rt_stage_vec(Wc, a->img, 4);
    // one width for the two byte planes (a thread's unit goes to either): 16 where both allow it
    const int byte_vec = rt_stage_vec(Wc, a->mask, 16) == 16 ? rt_stage_vec(Wc, a->tgt_masks, 16) : 1;
    // rows under a tile (ROWS_MAX's bound at this image's scale, rounded up), for the steepest image of the batch
    int rows_cap = 1;
    for (int b = 0; b < B; ++b) {
        const int64_t h = a->h[b], oh = a->oh[b], reach = h > oh ? (h + oh - 1) / oh : 1;
        const int need = (int)((TH - 1) * h / oh + 2 * reach + 3);
        rows_cap = need > rows_cap ? need : rows_cap;
    }
    if (rows_cap > ROWS_MAX) rows_cap = ROWS_MAX;
    hipLaunchKernelGGL(raw_stage_kernel, dim3((unsigned)blocks), dim3(256), (size_t)rows_cap * ROW_BYTES, (hipStream_t)stream, *a, tiles_x, tiles_y,
                       img_vec, byte_vec, rows_cap);
    RT_CHECK_LAUNCH();
    return RT_OK;
}
