// What the launched input chain (rt_input.hip: rt_resample_u8 x 2 -> rt_img_collate_norm -> rt_batch_stage) and the one launch that must write
// the same bytes (rt_raw_stage.hip) share: the resampling constants, ToTensor + Normalize, the unit store of a byte plane, and the host's choice
// of a unit's width and check of the box arguments.
// rt_raw_stage.hip is compiled with `#pragma clang fp contract(off)`, rt_input.hip with the default, and nothing here may depend on the
// includer: a function that does floating-point arithmetic turns contraction off at the top of its own body (a file-scope pragma here
// would leak into the includer).
#pragma once
#include "rt_common.h"

// Pillow's 8-bit resampling (ImagingResample): 22-bit fixed-point coefficients, the accumulator starts at one half
constexpr int RT_PRECISION_BITS = 32 - 8 - 2;
constexpr int RT_RESAMPLE_HALF = 1 << (RT_PRECISION_BITS - 1);

__device__ __forceinline__ uint8_t rt_clip8(int v) {
    v >>= RT_PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ToTensor + Normalize of one byte
__device__ __forceinline__ float rt_norm_u8(uint8_t byte, float mean, float std) {
#pragma clang fp contract(off)
    return ((float)byte / 255.0f - mean) / std;
}

// A unit of a byte plane, 16 computed bytes for columns [x, x + 16), to d: one 16-byte store where the host allowed it (rt_stage_vec),
// else the elements that lie inside the row.
union rt_bytes16 { uint4 q; uint8_t e[16]; };

__device__ __forceinline__ void rt_store_unit(uint8_t* d, const rt_bytes16& v, bool vec, int x, int Wc) {
    if (vec) {
        *reinterpret_cast<uint4*>(d) = v.q;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) if (x + j < Wc) d[j] = v.e[j];
    }
}

// words of [boxes[B * boxes_per_image][4] | tgt_off[0 .. B] | num_boxes], the box tail both kernels write (each its own: see DESIGN.md)
constexpr size_t rt_box_tail_words(int B, int boxes_per_image) { return (size_t)B * boxes_per_image * 4 + B + 2; }

// Elements per unit of a destination with rows of Wc elements at `base`: `per_unit` (16 bytes' worth) where every row starts 16-byte
// aligned, else 1.  (A NULL base counts as aligned.)
inline int rt_stage_vec(int Wc, const void* base, int per_unit) {
    return (Wc % per_unit == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0) ? per_unit : 1;
}

// the box arguments of one image of a stage call
inline bool rt_stage_boxes_ok(int n, const float* ptr, int boxes_per_image) { return n >= 0 && n <= boxes_per_image && (n == 0 || ptr); }
