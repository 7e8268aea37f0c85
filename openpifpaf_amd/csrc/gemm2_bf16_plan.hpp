// The load plan of the bf16 two-source GEMM (csrc/gemm2_bf16.hip): which 16-byte chunk of which row of A1 or which pixel of x thread t
// of the workgroup at row block m0 loads for K-step k0, or that it loads nothing -- as __host__ __device__ functions, so that the
// kernel and a stand-alone CPU program (tests/host/gemm2_bf16_plan_main.cpp) run the SAME decision: the program makes every access of
// a launch against A1 and x allocations that end with their last byte and checks that every (row < M, K chunk) is fetched once from
// the right source and offset, nothing for a row >= M, and that what is staged is the concatenated matrix.
//
// A1 [M, k1] bf16, dense (k1 % 64 == 0, k1 == 0: there is none); x [B, h, w, k2] bf16, dense channels-last (k2 % 64 == 0, k2 > 0);
// both 16-byte aligned, x, M * k1 fewer than 2^31 elements.  The product's row m = (b * ho + oy) * wo + ox is an output pixel, its
// K = k1 + k2 columns are
//     A[m][k] = k < k1 ? A1[m][k] : x[b, s * oy, s * ox, k - k1]
// stride s 1 or 2, ho = (h - 1) / s + 1.  A K-step of 64 columns lies inside ONE source (k1 % 64 == 0).
//
// Per K-step a thread stages one 16-byte chunk (8 channels) of four rows: chunk column s_col = (t % 8) * 8, rows
// m0 + p * 32 + t / 8, p = 0..3 -- csrc/bf16_tile_shape.hpp's staging map.  What depends on the row alone is computed ONCE per thread
// before the loop (gemm2_bf16_plan_rows): the element offset m * k1 of its row of A1, the element offset of its pixel (s * oy, s * ox)
// of x, which always lies inside the image, and whether m < M.  Per K-step (gemm2_bf16_plan_a) k0 < k1 selects the source -- the same
// for the whole workgroup -- and the column is added.  A row >= M is not loaded at all: its registers keep their zeros, and no
// address outside A1 or x is ever formed for a load.
#pragma once
#include <cstdint>

#include "bf16_tile_shape.hpp"

namespace opa {

// output rows / columns of h / w input ones
OPA_TILE_HD int gemm2_bf16_out(int h, int stride) { return (h - 1) / stride + 1; }

// the geometry of one launch (batch, h, w, k2 positive, k1 not negative; the products below 2^31 are the caller's to check)
struct Gemm2Bf16Geometry {
    int batch, h, w, k1, k2, stride;
};

// the two sources of A
constexpr int kGemm2Bf16A1 = 0, kGemm2Bf16X = 1;

// one staged row: the element offsets of its row of A1 and of its pixel of x (channel 0), and whether it is a row of the product
struct Gemm2Bf16Row {
    int a1, x;
    bool live;
};

// Thread t's four rows of the workgroup whose first row is m0.  A row >= M = batch * ho * wo is not live.
OPA_TILE_HD void gemm2_bf16_plan_rows(const Gemm2Bf16Geometry& g, int m0, int t, Gemm2Bf16Row (&rows)[kBf16Passes]) {
    const int ho = gemm2_bf16_out(g.h, g.stride), wo = gemm2_bf16_out(g.w, g.stride);
    const long long M = (long long)g.batch * ho * wo;
    const int s_row = bf16_tile_stage(t).row;
    OPA_TILE_UNROLL
    for (int p = 0; p < kBf16Passes; p++) {
        const long long row = (long long)m0 + p * 32 + s_row;          // (64-bit: m0 + 127 may pass 2^31)
        rows[p].a1 = 0;
        rows[p].x = 0;
        rows[p].live = row < M;
        if (!rows[p].live) continue;
        const int m = (int)row;
        const int b = m / (ho * wo), rest = m - b * (ho * wo);
        const int oy = rest / wo, ox = rest - oy * wo;
        rows[p].a1 = (int)((long long)m * g.k1);
        rows[p].x = (int)((((long long)b * g.h + g.stride * oy) * g.w + g.stride * ox) * g.k2);      // 0 <= s * oy < h, 0 <= s * ox < w
    }
}

// Thread t's accesses for K-step k0 (a multiple of 64, below k1 + k2).
// emit(p, source, elem_offset): load 16 bytes from element offset `elem_offset` of `source` (kGemm2Bf16A1: from A1's first element,
// kGemm2Bf16X: from x's) into the chunk of pass p.
template <typename Emit>
OPA_TILE_HD void gemm2_bf16_plan_a(const Gemm2Bf16Geometry& g, const Gemm2Bf16Row (&rows)[kBf16Passes], int t, int k0, Emit&& emit) {
    const int col = bf16_tile_stage(t).col;
    if (k0 < g.k1) {                                                   // (uniform for the workgroup)
        OPA_TILE_UNROLL
        for (int p = 0; p < kBf16Passes; p++)
            if (rows[p].live) emit(p, kGemm2Bf16A1, (long long)rows[p].a1 + k0 + col);
    } else {
        OPA_TILE_UNROLL
        for (int p = 0; p < kBf16Passes; p++)
            if (rows[p].live) emit(p, kGemm2Bf16X, (long long)rows[p].x + (k0 - g.k1) + col);
    }
}

}  // namespace opa
