// The load plan of the bf16 7x7 stem implicit GEMM (csrc/stem7x7_bf16.hip): which 2-byte elements of the image thread t of the
// workgroup at row block m0 loads for K-step k0, and into which slot of its 16-byte chunks -- as __host__ __device__ functions, so that
// the kernel and a stand-alone CPU program (tests/host/stem7x7_bf16_plan_main.cpp) run the SAME decision: the program makes every
// access of a launch against an x whose allocation begins at the first addressed element and ends at the last, and checks that every
// (row, valid tap, channel) is fetched once, no tap outside the image ever, none outside the tensor, and that what is staged is the
// im2col tile.
//
// x [B, 3, h, w] bf16, read where it lies through four positive element strides (batch, channel, row, pixel): channels-last, NCHW, a
// cropped view of either; first to last addressed element fewer than 2^31 apart.  The product's row m = (b * ho + oy) * wo + ox is an
// output pixel, stride s 1 or 2, padding 3, ho = (h - 1) / s + 1.  Its K = 192 columns are
//     k = ky * 24 + kx * 3 + ci        ky, kx = 0 .. 6, ci = 0 .. 2
//     A[m][k] = x[b, ci, s * oy - 3 + ky, s * ox - 3 + kx]                  (zero where that pixel lies outside the image)
// and zero in the 3 columns that pad a window row's 21 to 24 and in the 24 of the eighth "row" ky = 7 (the weight holds zeros there
// too, csrc/stem7x7_bf16.hip).  A 16-byte chunk of 8 columns lies inside ONE ky (24 = 3 x 8); in a channels-last image a window row
// is 21 contiguous elements.
//
// Per K-step a thread stages one chunk of four rows: chunk column (t % 8) * 8, rows m0 + p * 32 + t / 8, p = 0..3 --
// csrc/bf16_tile_shape.hpp's staging map.  What depends on the row alone is computed ONCE per workgroup (stem7x7_bf16_plan_rows): the
// element offset of the window's CENTRE pixel (s * oy, s * ox) in channel 0, which always lies inside the image, and -- the window is
// separable -- a 7-bit mask of the window rows ky and one of the window columns kx that do.  Per K-step (stem7x7_bf16_plan_a) the
// tap's offset from the centre is added, element by element -- for a tap whose two bits are set; any other, every zero column of K
// and every element of a row >= M is not loaded at all: its bits keep their zeros, so the padding contributes exactly zero whatever
// memory holds (no multiplication by zero: 0 x NaN), and no address outside x is ever formed for a load.
//
// Offsets are formed modulo 2^32 (unsigned): the offset of a tap INSIDE the image is a sum of (index) * (stride) terms with every
// index below its dimension, each term and the sum below 2^31 -- exact.  The stride of a dimension of one element may be anything
// (torch reports what it likes there); it only ever meets the index 0, or a tap that its mask drops.
#pragma once
#include <cstdint>

#include "bf16_tile_shape.hpp"

namespace opa {

constexpr int kStem7Bf16K = 192;               // 7 window rows of 24 columns (7 pixels x 3 channels + 3 zeros) + one row of zeros

// output rows / columns of h / w input ones
OPA_TILE_HD int stem7x7_bf16_out(int h, int stride) { return (h - 1) / stride + 1; }

// the geometry of one launch: sizes and stride positive, the four element strides of x positive
struct Stem7Bf16Geometry {
    int batch, h, w, stride;
    long long x_batch, x_channel, x_row, x_pixel;
};

// one staged row: the element offset of its window's centre pixel (channel 0), the window rows (bit ky) and columns (bit kx) inside
// the image
struct Stem7Bf16Row {
    unsigned centre, rows, cols;
};

// Thread t's four rows of the workgroup whose first row is m0.  A row >= M = batch * ho * wo has no taps.
OPA_TILE_HD void stem7x7_bf16_plan_rows(const Stem7Bf16Geometry& g, int m0, int t, Stem7Bf16Row (&rows)[kBf16Passes]) {
    const int ho = stem7x7_bf16_out(g.h, g.stride), wo = stem7x7_bf16_out(g.w, g.stride);
    const long long M = (long long)g.batch * ho * wo;
    const int s_row = bf16_tile_stage(t).row;
    OPA_TILE_UNROLL
    for (int p = 0; p < kBf16Passes; p++) {
        const long long row = (long long)m0 + p * 32 + s_row;          // (64-bit: m0 + 127 may pass 2^31)
        rows[p].centre = 0u;
        rows[p].rows = 0u;
        rows[p].cols = 0u;
        if (row >= M) continue;
        const int m = (int)row;
        const int b = m / (ho * wo), rest = m - b * (ho * wo);
        const int oy = rest / wo, ox = rest - oy * wo;
        const int cy = g.stride * oy, cx = g.stride * ox;              // the centre: 0 <= cy < h, 0 <= cx < w
        rows[p].centre = (unsigned)b * (unsigned)g.x_batch + (unsigned)cy * (unsigned)g.x_row + (unsigned)cx * (unsigned)g.x_pixel;
        unsigned in_rows = 0u, in_cols = 0u;
        OPA_TILE_UNROLL
        for (int k = 0; k < 7; k++) {
            if (cy + k - 3 >= 0 && cy + k - 3 < g.h) in_rows |= 1u << k;
            if (cx + k - 3 >= 0 && cx + k - 3 < g.w) in_cols |= 1u << k;
        }
        rows[p].rows = in_rows;
        rows[p].cols = in_cols;
    }
}

// Thread t's accesses of x for K-step k0 (0, 64 or 128).
// emit(p, slot, elem_offset): load the 2-byte element at offset `elem_offset` (from x's first element) into element `slot` (0 .. 7) of
// the chunk of pass p.
template <typename Emit>
OPA_TILE_HD void stem7x7_bf16_plan_a(const Stem7Bf16Geometry& g, const Stem7Bf16Row (&rows)[kBf16Passes], int t, int k0, Emit&& emit) {
    const int chunk = (k0 + bf16_tile_stage(t).col) / 8;               // 0 .. 23, three to a window row
    const int ky = chunk / 3, r0 = (chunk - 3 * ky) * 8;               // the chunk's first column within its window row: 0, 8, 16
    if (ky >= 7) return;                                               // K's eighth row: zeros
    const unsigned xr = (unsigned)g.x_row, xp = (unsigned)g.x_pixel, xc = (unsigned)g.x_channel;
    const unsigned dy = (unsigned)(ky - 3) * xr;
    OPA_TILE_UNROLL
    for (int slot = 0; slot < 8; slot++) {
        const int r = r0 + slot, kx = r / 3, ci = r - 3 * kx;          // kx 0 .. 7; 7: the window row's three zero columns
        if (kx >= 7) continue;
        const unsigned delta = dy + (unsigned)(kx - 3) * xp + (unsigned)ci * xc;
        OPA_TILE_UNROLL
        for (int p = 0; p < kBf16Passes; p++)
            if (((rows[p].rows >> ky) & (rows[p].cols >> kx)) & 1u) emit(p, slot, (long long)(unsigned)(rows[p].centre + delta));
    }
}

}  // namespace opa
