// 1x1 convolution of the field-producing network as an MFMA GEMM with the whole epilogue fused:
//     out[M,N] = act( A[M,K] * W[N,K]^T + bias[N] (+ residual[M,N]) )        (bf16 or f16 in/out, f32 math)
// A is an NHWC activation viewed as [M = B*H*W, K = C_in] (row-major, K contiguous), W the conv
// weight [C_out, C_in] -- both operands are "K-major", exactly the fragment order of
// v_mfma_f32_32x32x16_bf16 (lane l holds 8 consecutive k of row l&31, k-offset 8*(l>>5)) and of
// v_mfma_f32_32x32x16_f16.  DT, the C ABI's dtype code, is the element type of every operand: 2 bfloat16, 1 float16.
//
// Why: at 641 px / batch 32 the 1x1 convs of ResNet blocks 2-3 are bandwidth bound (CK's kernels
// already run them at ~5 TB/s) and the separate bias/residual/ReLU pass over the 1.7 GB outputs
// costs more than the convolution.  Fusing it removes one read and one write of the output.
//
// Tile, main loop and the epilogue's 16-B rows are csrc/bf16_tile.hpp's.  What is this kernel's own is A: a row of
// a matrix, optionally with the preceding convolution's bias + ReLU applied on the way into LDS (PRO).
#include "bf16_tile.hpp"

namespace opa {

// PRO: the A operand is the RAW output of the preceding convolution; its bias + ReLU epilogue
// (a_bias[k], per input channel) is applied while the tile is staged into LDS -- same f32 add, max and
// round-to-nearest-even as the separate bias_act pass, which is thereby saved (one read and one write
// of the 3x3 convolution's output per bottleneck).
// The ReLU: bfloat16 keeps fmaxf, which takes a NaN to 0, as it always has; float16 is a select, so NaN stays NaN as in torch.relu.
template <int DT, int BN, bool RES, bool RELU, bool PRO>
__global__ __launch_bounds__(256, 3) void gemm_bias_act_kernel(
        const unsigned short* __restrict__ A, const unsigned short* __restrict__ W,
        const unsigned short* __restrict__ bias, const unsigned short* __restrict__ res,
        unsigned short* __restrict__ out, int M, int N, int K, const unsigned short* __restrict__ a_bias) {
    using T = Bf16Tile<BN>;
    using E = TileElem<DT>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    const int lane = bf16_tile_wave().lane, wn = bf16_tile_wave().wn;
    const Bf16TileOrigin org = bf16_tile_origin<BN>(N);
    const int m0 = org.m0, n0 = org.n0;

    u32x4_t rpre[2][T::VPL];
    if (RES) bf16_tile_fetch_residual<BN>(rpre[0], res, M, N, m0, n0, 0);   // the second half is fetched when the operand registers are free

    const int s_row = bf16_tile_stage(threadIdx.x).row, s_col = bf16_tile_stage(threadIdx.x).col;
    f32x16_t acc[2][T::NT];
    bf16_tile_mainloop<BN, DT>(smem, W, K, n0, acc, [&](int k0, u32x4_t (&ra)[kBf16Passes]) {   // (with the operand prologue)
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++) {
            const int m = m0 + p * 32 + s_row;
            ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
            if (m < M) ra[p] = *reinterpret_cast<const u32x4_t*>(A + (size_t)m * K + k0 + s_col);
        }
        if (PRO) {
            const u32x4_t ab = *reinterpret_cast<const u32x4_t*>(a_bias + k0 + s_col);
#pragma unroll
            for (int p = 0; p < kBf16Passes; p++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float lo = fmaxf(E::lo(ra[p][q]) + E::lo(ab[q]), 0.0f);
                    const float hi = fmaxf(E::hi(ra[p][q]) + E::hi(ab[q]), 0.0f);
                    ra[p][q] = E::rne(lo) | (E::rne(hi) << 16);
                }
        }
    });
    if (RES) bf16_tile_fetch_residual<BN>(rpre[1], res, M, N, m0, n0, 1);

    // epilogue, one 32-row block of the wave tile at a time
    float* patch = bf16_tile_patch<BN>(smem);
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < T::NT; j++) {
            const int col = j * 32 + (lane & 31);
            const float b = E::lo((unsigned)bias[n0 + wn * T::WN + col]);
#pragma unroll
            for (int r = 0; r < 16; r++) patch[bf16_tile_acc_row(r) * T::WN + col] = acc[i][j][r] + b;
        }
        bf16_tile_patch_sync();
        bf16_tile_store_rows<BN, RES, RELU, DT>(patch, rpre[i], out, M, N, m0, n0, i,
                                                [](float v) { return DT == 2 ? fmaxf(v, 0.0f) : v < 0.0f ? 0.0f : v; });
        bf16_tile_patch_sync();
    }
}

hipError_t launch_gemm_bias_act(const void* A, const void* W, const void* bias, const void* res, void* out,
                                int M, int N, int K, int relu, hipStream_t st, const void* a_bias, int dtype) {
    const unsigned short *a = (const unsigned short*)A, *w = (const unsigned short*)W, *b = (const unsigned short*)bias,
                         *r = (const unsigned short*)res, *ab = (const unsigned short*)a_bias;
    unsigned short* o = (unsigned short*)out;
    const int bn = N % 128 == 0 ? 128 : 64;
    const long long blocks = (long long)((M + kBf16BM - 1) / kBf16BM) * (N / bn);
    return with_value<1, 2>(dtype, [&](auto DT) {
    return with_value<64, 128>(bn, [&](auto BN) {
    return with_flag(res != nullptr, [&](auto RES) {
    return with_flag(relu != 0, [&](auto RELU) {
    return with_flag(a_bias != nullptr, [&](auto PRO) {
        gemm_bias_act_kernel<DT, BN, RES, RELU, PRO><<<(unsigned)blocks, 256, 0, st>>>(a, w, b, r, o, M, N, K, ab);
        return hipGetLastError();
    }); }); }); }); });
}

}  // namespace opa
