// The GROUPED 3x3 convolution of a ResNeXt cast to bfloat16 (reference network/basenetworks.py:71-150: torchvision's Bottleneck with
// groups = 32 through torch.nn.Conv2d) as an implicit GEMM per 64-channel chunk on v_mfma_f32_32x32x16_bf16, float32 accumulation,
// ONE rounding at the store.  As many output as input channels C, C % 64 == 0, group width CG = C / groups in {4, 8, 16, 32, 64}: the
// 64 output channels n0 .. n0 + 63 depend on the 64 input channels n0 .. n0 + 63 alone, so per N-tile the grouped convolution is a
// dense 64 -> 64 3x3 convolution whose weight is block diagonal:
//     out[b, oy, ox, co] = bf16_rne(act(sum_{ky,kx} sum_{j<64} x[b, s*oy - d + d*ky, s*ox - d + d*kx, 64*(co/64) + j] * w[co][3*ky + kx][j]
//                                       + bias[co]))
// x [B, h, w, C] dense channels-last bf16; w [C][9][64] bf16 (K-major, K = 576): column j of row co is the weight of input channel
// 64*(co/64) + j, ZERO wherever j / CG != (co % 64) / CG; bias float32 [C] or null; out dense bf16 [B, ho, wo, C]; stride s 1 or 2,
// dilation d = padding 1, 2 or 4 (above 1 at stride 1 only).  No residual operand: no grouped block has one.
//
// Tile (Bf16Tile<64>: 128 rows x 64 columns, a wave owns 32 columns), tile order, patch, fence and the epilogue's 16-byte rows are
// csrc/bf16_tile.hpp's.  A is the dense kernel's tap gather with the channel base at n0 (csrc/gconv3x3_bf16_plan.hpp, which a CPU
// program enumerates: tests/test_gconv3x3_bf16_plan.py); this kernel forms no address of x itself.  The main loop is written out
// here, as csrc/gemm_unit_bf16.hip's is, because of what is this kernel's own:
//   HALF (CG <= 32): wave wn's 32 columns depend on the input channels 32 * wn .. 32 * wn + 31 of the chunk alone, so of the four
//   16-wide k-substeps of a K-step it runs kk = 32 * wn and 32 * wn + 16 -- two MFMAs and two fragment reads per row block instead
//   of four; the other two would multiply exact zeros.  CG = 64 runs all four.
//
// NON-FINITE VALUES.  The off-group weights are zeros that the MFMA does multiply (0 x NaN = NaN, 0 x Inf = NaN).  A NaN or Inf in
// an input channel therefore reaches every output channel of the same 32-ALIGNED CHANNEL BLOCK (CG = 4, 8, 16) at the pixels whose
// window holds it, not only its own group's; for CG = 32 and 64 it reaches only its own group.  Padding is never multiplied (a tap
// outside the image is not loaded: exact zeros whatever memory holds).  The ReLU is a select: NaN stays NaN.
//
// No im2col buffer, no workspace, no atomics (equal inputs give equal bits), no scratch.
//
// The same kernel serves a ResNeXt cast to float16 on v_mfma_f32_32x32x16_f16: DT, the C ABI's dtype code (2 bfloat16, 1 float16), is the
// element type of x, w and out (csrc/bf16_tile.hpp's TileElem<DT>: the fragment type, the MFMA, the rounding at the store); the bias
// stays float32, everything else moves raw 16-bit words.  The NON-FINITE contract above holds for BOTH types: the f16 MFMA multiplies
// the off-group zeros as the bf16 one does, and float16's store keeps NaN and sends what lies beyond 65504 to +-inf.
#include "bf16_tile.hpp"
#include "gconv3x3_bf16_plan.hpp"

namespace opa {

namespace {

// M = batch * ho * wo output pixels, N = C, K = 576 per N-tile
template <int DT, bool HALF, bool RELU>
__global__ __launch_bounds__(256, 3) void gconv3x3_bf16_kernel(
        const unsigned short* __restrict__ x, const unsigned short* __restrict__ W, const float* __restrict__ bias,
        unsigned short* __restrict__ out, Conv3Bf16Geometry g, int M) {
    constexpr int BN = kGconv3Bf16BN, K = kGconv3Bf16K;
    using T = Bf16Tile<BN>;
    typedef typename TileElem<DT>::frag_t frag_t;
    static_assert(T::NT == 1 && T::WN == 32, "a wave owns one 32-column block");
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    const int tid = threadIdx.x, lane = bf16_tile_wave().lane, wm = bf16_tile_wave().wm, wn = bf16_tile_wave().wn;
    const int N = g.c_in;
    const Bf16TileOrigin org = bf16_tile_origin<BN>(N);
    const int m0 = org.m0, n0 = org.n0;

    Conv3Bf16Row rows[kBf16Passes];            // this thread's four output pixels: centre and tap mask, once per workgroup
    conv3x3_bf16_plan_rows(g, m0, tid, rows);

    f32x16_t acc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.0f;

    unsigned short* sA = reinterpret_cast<unsigned short*>(smem);
    unsigned short* sB = sA + T::LDS_A;
    const int s_row = bf16_tile_stage(tid).row, s_col = bf16_tile_stage(tid).col;
    u32x4_t ra[kBf16Passes], rb[BN / 32];
    auto fetch = [&](int k0) {                 // global -> registers for K-step k0 (= tap k0 / 64); a tap outside the image keeps its zeros
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++) ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
        gconv3x3_bf16_plan_a(g, rows, tid, n0, k0, [&](int p, long long at) { ra[p] = *reinterpret_cast<const u32x4_t*>(x + at); });
#pragma unroll
        for (int p = 0; p < BN / 32; p++)
            rb[p] = *reinterpret_cast<const u32x4_t*>(W + (size_t)(n0 + p * 32 + s_row) * K + k0 + s_col);
    };
    const int kk0 = HALF ? 32 * wn : 0;        // this wave's first k-substep of a K-step
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kBf16BK) {
        __syncthreads();                       // previous step's fragment reads are done
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++)
            *reinterpret_cast<u32x4_t*>(sA + (p * 32 + s_row) * kBf16Pitch + s_col) = ra[p];
#pragma unroll
        for (int p = 0; p < BN / 32; p++)
            *reinterpret_cast<u32x4_t*>(sB + (p * 32 + s_row) * kBf16Pitch + s_col) = rb[p];
        __syncthreads();
        if (k0 + kBf16BK < K) fetch(k0 + kBf16BK);   // the next tap's operands travel while this one multiplies
#pragma unroll
        for (int q = 0; q < (HALF ? 2 : 4); q++) {
            const int kof = kk0 + q * 16 + (lane >> 5) * 8;
            frag_t fa[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                fa[i] = *reinterpret_cast<const frag_t*>(sA + (wm * 64 + i * 32 + (lane & 31)) * kBf16Pitch + kof);
            const frag_t fb = *reinterpret_cast<const frag_t*>(sB + (wn * T::WN + (lane & 31)) * kBf16Pitch + kof);
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i] = TileElem<DT>::mfma(fa[i], fb, acc[i]);
        }
    }
    __syncthreads();                           // staging LDS is free: reuse it for the epilogue

    // epilogue, one 32-row block of the wave tile at a time
    float* patch = bf16_tile_patch<BN>(smem);
    u32x4_t none[T::VPL];                      // (no residual: never read)
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int col = lane & 31;
        const float b = bias ? bias[n0 + wn * T::WN + col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) patch[bf16_tile_acc_row(r) * T::WN + col] = acc[i][r] + b;
        bf16_tile_patch_sync();
        bf16_tile_store_rows<BN, false, RELU, DT>(patch, none, out, M, N, m0, n0, i,
                                                  [](float v) { return v < 0.0f ? 0.0f : v; });   // (a select: NaN stays NaN)
        bf16_tile_patch_sync();
    }
}

}  // namespace

long long gconv3x3_bf16_workgroups(int B, int H, int W, int C, int S) {
    const long long M = (long long)B * conv3x3_bf16_out(H, S) * conv3x3_bf16_out(W, S);
    return (M + kBf16BM - 1) / kBf16BM * (C / kGconv3Bf16BN);
}

hipError_t launch_gconv3x3_bf16(const void* x, const void* w, const float* bias, void* out, int B, int H, int W, int C, int CG, int S,
                                int D, int relu, hipStream_t st, int dtype) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 64 != 0 || (CG != 4 && CG != 8 && CG != 16 && CG != 32 && CG != 64) || C == CG ||
        (S != 1 && S != 2) || (D != 1 && D != 2 && D != 4) || (D > 1 && S != 1))
        return hipErrorInvalidValue;
    const long long M = (long long)B * conv3x3_bf16_out(H, S) * conv3x3_bf16_out(W, S);
    const long long blocks = gconv3x3_bf16_workgroups(B, H, W, C, S);
    if ((long long)B * H * W * C > 0x7fffffffll || M * C > 0x7fffffffll || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const Conv3Bf16Geometry g = {B, H, W, C, S, D};
    return with_value<1, 2>(dtype, [&](auto DT) {
    return with_flag(CG <= 32, [&](auto HALF) {
    return with_flag(relu != 0, [&](auto RELU) {
        gconv3x3_bf16_kernel<DT, HALF, RELU><<<(unsigned)blocks, kBf16Threads, 0, st>>>(
            (const unsigned short*)x, (const unsigned short*)w, bias, (unsigned short*)out, g, (int)M);
        return hipGetLastError();
    }); }); });
}

}  // namespace opa
