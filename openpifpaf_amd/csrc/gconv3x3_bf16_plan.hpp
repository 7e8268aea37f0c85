// The load plan of the bf16 GROUPED 3x3 implicit GEMM (csrc/gconv3x3_bf16.hip): which 16-byte chunk of which pixel of x thread t of
// the workgroup at row block m0 and N-tile n0 loads for K-step k0, or that it loads nothing -- as a __host__ __device__ function, so
// that the kernel and a stand-alone CPU program (tests/host/gconv3x3_bf16_plan_main.cpp) run the SAME decision.
//
// x [B, h, w, C] bf16, dense channels-last, 16-byte aligned, C % 64 == 0, fewer than 2^31 elements; as many output as input channels
// and a group width that divides 64, so the 64 output channels n0 .. n0 + 63 of an N-tile depend on the input channels n0 .. n0 + 63
// alone.  Per N-tile the product has K = 9 * 64 columns, k = tap * 64 + j with tap = 3 * ky + kx:
//     A[m][k] = x[b, s * oy - d + d * ky, s * ox - d + d * kx, n0 + j]        (zero where that pixel lies outside the image)
// A K-step of 64 columns is ONE tap of the tile's own 64 channels; the pixel pitch is C.  Rows, centres and tap masks are the dense
// plan's (csrc/conv3x3_bf16_plan.hpp: Conv3Bf16Geometry with c_in = C, conv3x3_bf16_plan_rows), unchanged: a tap whose bit is clear,
// and every tap of a row >= M, is not loaded at all -- its registers keep their zeros -- and no address outside x is ever formed.
#pragma once
#include "conv3x3_bf16_plan.hpp"

namespace opa {

constexpr int kGconv3Bf16BN = 64;       // the N-tile: 64 output channels and the 64 input channels they depend on
constexpr int kGconv3Bf16K = 9 * 64;    // columns of the product per N-tile

// Thread t's accesses of x for K-step k0 (a multiple of 64, below 576) of the N-tile whose first channel is n0 (a multiple of 64,
// below g.c_in).  emit(p, elem_offset): load 16 bytes from element offset `elem_offset` (from x's first element) into the chunk of pass p.
template <typename Emit>
OPA_TILE_HD void gconv3x3_bf16_plan_a(const Conv3Bf16Geometry& g, const Conv3Bf16Row (&rows)[kBf16Passes], int t, int n0, int k0,
                                      Emit&& emit) {
    const int tap = k0 / kGconv3Bf16BN;                                // (uniform for the workgroup)
    const int ky = tap / 3, kx = tap - 3 * ky;
    const long long delta = ((long long)(ky - 1) * g.w + (kx - 1)) * g.dilation * g.c_in + n0 + bf16_tile_stage(t).col;
    OPA_TILE_UNROLL
    for (int p = 0; p < kBf16Passes; p++)
        if ((rows[p].taps >> tap) & 1u) emit(p, (long long)rows[p].centre + delta);
}

}  // namespace opa
