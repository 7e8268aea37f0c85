// The load plan of the bf16 3x3 implicit GEMM (csrc/conv3x3_bf16.hip): which 16-byte chunk of which pixel of x thread t of the
// workgroup at row block m0 loads for K-step k0, or that it loads nothing -- as __host__ __device__ functions, so that the kernel and
// a stand-alone CPU program (tests/host/conv3x3_bf16_plan_main.cpp) run the SAME decision: the program makes every access of a launch
// against an x whose allocation ends with its last byte and checks that every (row, valid tap, chunk) is fetched once, no tap
// outside the image ever, none outside the tensor, and that what is staged is the im2col tile.
//
// x [B, h, w, c_in] bf16, dense channels-last, 16-byte aligned, c_in % 64 == 0, fewer than 2^31 elements.  The product's row
// m = (b * ho + oy) * wo + ox is an output pixel, its K = 9 * c_in columns are k = tap * c_in + ci with tap = 3 * ky + kx:
//     A[m][k] = x[b, s * oy - d + d * ky, s * ox - d + d * kx, ci]        (zero where that pixel lies outside the image)
// stride s 1 or 2, dilation d = padding 1, 2 or 4, ho = (h - 1) / s + 1.  A K-step of 64 columns lies inside ONE tap (c_in % 64 == 0).
//
// Per K-step a thread stages one 16-byte chunk (8 channels) of four rows: chunk column s_col = (t % 8) * 8, rows
// m0 + p * 32 + t / 8, p = 0..3 -- csrc/bf16_tile_shape.hpp's staging map.  What depends on the row alone is computed ONCE per
// workgroup (conv3x3_bf16_plan_rows): the element offset of the window's CENTRE pixel (s * oy, s * ox), which always lies inside the
// image, and a 9-bit mask of the taps that do.  Per K-step (conv3x3_bf16_plan_a) the tap's offset from the centre is added -- for a
// tap whose bit is set; a tap whose bit is clear, and every tap of a row >= M, is not loaded at all: its registers keep their zeros,
// so the padding contributes exactly zero whatever memory holds (no multiplication by zero: 0 x NaN), and no address outside x is
// ever formed for a load.
#pragma once
#include <cstdint>

#include "bf16_tile_shape.hpp"

namespace opa {

// the shared tile's constants under the names that the CPU program of this plan (tests/host/conv3x3_bf16_plan_main.cpp) uses
constexpr int kConv3Bf16BM = kBf16BM, kConv3Bf16BK = kBf16BK, kConv3Bf16Threads = kBf16Threads, kConv3Bf16Passes = kBf16Passes;

// output rows / columns of h / w input ones
OPA_TILE_HD int conv3x3_bf16_out(int h, int stride) { return (h - 1) / stride + 1; }

// the geometry of one launch (every member positive; the products below 2^31 are the caller's to check)
struct Conv3Bf16Geometry {
    int batch, h, w, c_in, stride, dilation;
};

// one staged row: the element offset of its window's centre pixel (channel 0) and the taps inside the image (bit 3 * ky + kx)
struct Conv3Bf16Row {
    int centre;
    unsigned taps;
};

// Thread t's four rows of the workgroup whose first row is m0.  A row >= M = batch * ho * wo has no taps.
OPA_TILE_HD void conv3x3_bf16_plan_rows(const Conv3Bf16Geometry& g, int m0, int t, Conv3Bf16Row (&rows)[kBf16Passes]) {
    const int ho = conv3x3_bf16_out(g.h, g.stride), wo = conv3x3_bf16_out(g.w, g.stride);
    const long long M = (long long)g.batch * ho * wo;
    const int s_row = bf16_tile_stage(t).row;
    OPA_TILE_UNROLL
    for (int p = 0; p < kBf16Passes; p++) {
        const long long row = (long long)m0 + p * 32 + s_row;          // (64-bit: m0 + 127 may pass 2^31)
        rows[p].centre = 0;
        rows[p].taps = 0u;
        if (row >= M) continue;
        const int m = (int)row;
        const int b = m / (ho * wo), rest = m - b * (ho * wo);
        const int oy = rest / wo, ox = rest - oy * wo;
        const int cy = g.stride * oy, cx = g.stride * ox;              // the centre: 0 <= cy < h, 0 <= cx < w
        rows[p].centre = (int)((((long long)b * g.h + cy) * g.w + cx) * g.c_in);
        unsigned taps = 0u;
        OPA_TILE_UNROLL
        for (int ky = 0; ky < 3; ky++) {
            OPA_TILE_UNROLL
            for (int kx = 0; kx < 3; kx++) {
                const int iy = cy + (ky - 1) * g.dilation, ix = cx + (kx - 1) * g.dilation;
                if (iy >= 0 && iy < g.h && ix >= 0 && ix < g.w) taps |= 1u << (3 * ky + kx);
            }
        }
        rows[p].taps = taps;
    }
}

// Thread t's accesses of x for K-step k0 (a multiple of 64, below 9 * c_in).
// emit(p, elem_offset): load 16 bytes from element offset `elem_offset` (from x's first element) into the chunk of pass p.
template <typename Emit>
OPA_TILE_HD void conv3x3_bf16_plan_a(const Conv3Bf16Geometry& g, const Conv3Bf16Row (&rows)[kBf16Passes], int t, int k0,
                                           Emit&& emit) {
    const int tap = k0 / g.c_in, ci0 = k0 - tap * g.c_in;              // (uniform for the workgroup)
    const int ky = tap / 3, kx = tap - 3 * ky;
    const long long delta = ((long long)(ky - 1) * g.w + (kx - 1)) * g.dilation * g.c_in + ci0 + bf16_tile_stage(t).col;
    OPA_TILE_UNROLL
    for (int p = 0; p < kBf16Passes; p++)
        if ((rows[p].taps >> tap) & 1u) emit(p, (long long)rows[p].centre + delta);
}

}  // namespace opa
