// What the weight-gradient kernels share (rt_wgrad.hip: register-staged and first-generation DMA; rt_wgrad2.hip: second generation):
// the problem geometry and its checks, which output tile and which row chunks a workgroup owns, the LDS-DMA request of contiguous
// operand rows and the fused bias gradient; the gather walker is shared by the two kernels of rt_wgrad.hip (the second generation
// writes its own out: through this one it measured slower).  The main loops, the MFMA shapes, the fragment addressing and the
// epilogues are what the kernels differ in and stay with them.  Internal to the library.
#pragma once
#include "rt_common.h"
#include "rt_lds.h"

// What every weight-gradient kernel is told about its problem (the head of WgradArgs and of W2Prob)
struct WgGeom {
    const bf16_t* dy; const bf16_t* x; float* dw; const float* scale; float* dbias;
    int SH, SW, SC, DH, DW, N, KH, KW, stride, pad, dil, M;
    unsigned dy_bytes, x_bytes;
};
// Fills it from a descriptor; RT_OK, or why the kernels cannot take the problem.  sc_mask / n_mask: the channel granularity of the
// kernel family (SC & sc_mask and N & n_mask must be 0).  Both operands are addressed with 32-bit byte offsets.
static inline int wg_fill_geom(const rt_conv_wgrad_desc& d, WgGeom& g, int sc_mask, int n_mask) {
    if (!d.dy || !d.x || !d.dw) return RT_ERR_BADARG;
    if (d.SC <= 0 || (d.SC & sc_mask) || (d.N & n_mask) || d.N <= 0) return RT_ERR_UNSUPPORTED;
    if (d.KH <= 0 || d.KW <= 0 || d.B <= 0 || d.DH <= 0 || d.DW <= 0 || d.stride <= 0) return RT_ERR_BADARG;
    const long long M = (long long)d.B * d.DH * d.DW, xe = (long long)d.B * d.SH * d.SW * d.SC;
    if (M > 0x7fffffffLL / 4) return RT_ERR_UNSUPPORTED;
    if (M * d.N >= 0x3fffffffLL || xe >= 0x3fffffffLL) return RT_ERR_UNSUPPORTED;
    g.dy = (const bf16_t*)d.dy; g.x = (const bf16_t*)d.x; g.dw = d.dw; g.scale = d.scale; g.dbias = d.dbias;
    g.SH = d.SH; g.SW = d.SW; g.SC = d.SC; g.DH = d.DH; g.DW = d.DW; g.N = d.N;
    g.KH = d.KH; g.KW = d.KW; g.stride = d.stride; g.pad = d.pad; g.dil = d.dil > 1 ? d.dil : 1;
    g.M = (int)M; g.dy_bytes = (unsigned)(M * d.N * 2); g.x_bytes = (unsigned)(xe * 2);
    return RT_OK;
}

constexpr int WG_OOB = 0x7fffffff;      // an offset behind every descriptor: the load gives zeros

// Linear tile id -> output tile: n tiles fastest, then c tiles, then the filter tap.
struct WgTile { int tile_c, tap, kh, kw, n0, c0; };
template <int BN, int BC>
__device__ __forceinline__ WgTile wg_tile(int tile, int n_tiles, int c_tiles, int KW) {
    WgTile t;
    const int tile_n = tile % n_tiles;
    const int rest = tile / n_tiles;
    t.tile_c = rest % c_tiles;
    t.tap = rest / c_tiles;
    t.kh = t.tap / KW; t.kw = t.tap - t.kh * KW;
    t.n0 = tile_n * BN; t.c0 = t.tile_c * BC;
    return t;
}

// The CR-row chunks [begin, end) of row split `split` (end <= begin: the split is empty)
struct WgChunks { int begin, end; };
template <int CR>
__device__ __forceinline__ WgChunks wg_chunks(int M, int split, int chunks_per_split) {
    const int total_chunks = (M + CR - 1) / CR;
    WgChunks c;
    c.begin = split * chunks_per_split;
    c.end = c.begin + chunks_per_split;
    if (c.end > total_chunks) c.end = total_chunks;
    return c;
}

// Running (image, y, x) of one staged output pixel m of a gathered problem (anything but 1x1 / stride 1 / pad 0).  P: the kernel's
// problem struct (SH, SW, DH, DW, stride, pad, dil).
struct WgGather {
    int b, y, x;
    __device__ __forceinline__ void init(int m, int DH, int DW) {
        x = m % DW; const int tmp = m / DW; y = tmp % DH; b = tmp / DH;
    }
    // source pixel of filter tap (kh, kw); false: it lies in the padding (pix is then meaningless)
    template <class P>
    __device__ __forceinline__ bool src(const P& p, int kh, int kw, int& pix) const {
        const int sy = y * p.stride - p.pad + kh * p.dil, sx = x * p.stride - p.pad + kw * p.dil;
        pix = (b * p.SH + sy) * p.SW + sx;
        return (unsigned)sy < (unsigned)p.SH && (unsigned)sx < (unsigned)p.SW;
    }
    // the pixel ROWS rows further on (ROWS may span several image rows: DW < ROWS)
    template <int ROWS>
    __device__ __forceinline__ void advance(int DH, int DW) {
        x += ROWS;
        while (x >= DW) { x -= DW; if (++y >= DH) { y = 0; ++b; } }
    }
};

// LDS-DMA request of contiguous rows (dy always; x of a 1x1 / stride-1 / pad-0 problem): the descriptor is re-based per chunk with scalar arithmetic
// (base += chunk bytes, num_records -= chunk bytes), so the per-lane offsets are loop-invariant and the rows past the last one fall
// off the end of the descriptor, i.e. read as zeros.
template <int CR, int NJ>
__device__ __forceinline__ void wg_issue_rows(const bf16_t* base, unsigned bytes, int row_elems, int chunk, unsigned lds, const int (&voff)[NJ]) {
    const unsigned off = (unsigned)chunk * (unsigned)(CR * 2) * (unsigned)row_elems;
    const i32x4 rs = rt_make_rsrc(reinterpret_cast<const unsigned char*>(base) + off, bytes - off);
#pragma unroll
    for (int j = 0; j < NJ; ++j) rt_dma16(rs, lds + j * 4096, voff[j]);
}

// ---- fused bias gradient: the workgroup of the first c tile and tap of an n tile adds up the columns of every dy tile it stages
__device__ __forceinline__ bool wg_do_bias(const float* dbias, const WgTile& t) { return dbias && t.tile_c == 0 && t.tap == 0; }

struct WgNoSwz { static __device__ __forceinline__ int of(int) { return 0; } };

// bsum += column (t % BN) of this thread's rows of a staged [ROWS][STRIDE bytes] dy tile (THREADS / BN threads share a column)
template <int BN, int ROWS, int THREADS, int STRIDE, class SWZ>
__device__ __forceinline__ void wg_bias_cols(const unsigned char* bA, int t, float& bsum) {
    constexpr int TPC = THREADS / BN, RPT = ROWS / TPC;
    const int col = t % BN, r0 = (t / BN) * RPT;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int row = r0 + r;
        bsum += (float)*reinterpret_cast<const bf16_t*>(bA + row * STRIDE + ((((col >> 3) ^ SWZ::of(row)) << 4) | ((col & 7) * 2)));
    }
}
template <int BN>
__device__ __forceinline__ void wg_bias_commit(float* dbias, int n0, int N, int t, float bsum) {
    const int n = n0 + t % BN;
    if (n < N) atomicAdd(dbias + n, bsum);
}
