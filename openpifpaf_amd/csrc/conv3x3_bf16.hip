// The 3x3 convolutions of a ResNet cast to bfloat16 (reference network/basenetworks.py:71-150: torchvision's BasicBlock and Bottleneck
// through torch.nn.Conv2d) as an implicit GEMM on v_mfma_f32_32x32x16_bf16, float32 accumulation, ONE rounding at the store:
//     out[b, oy, ox, co] = bf16_rne(act(sum_{ky,kx,ci} x[b, s*oy - d + d*ky, s*ox - d + d*kx, ci] * w[co][3*ky + kx][ci]
//                                       + bias[co] (+ residual[b, oy, ox, co])))
// x [B, h, w, c_in] dense channels-last bf16, w [c_out][9][c_in] bf16 (K-major, K = 9 c_in), bias float32 [c_out] or null, residual
// and out dense bf16 [B, ho, wo, c_out]; c_in % 64 == 0, c_out % 64 == 0, stride s 1 or 2, dilation d = padding 1, 2 or 4.
//
// Tile, main loop and the epilogue's 16-byte rows are csrc/bf16_tile.hpp's (BN = 128 where c_out allows, else 64).  What is this
// kernel's own is A: a tap gather instead of a row of a matrix.  Which 16 bytes of which pixel a thread loads for a K-step -- or that
// it loads nothing, for a tap outside the image -- is decided in csrc/conv3x3_bf16_plan.hpp, which a CPU program enumerates
// (tests/test_conv3x3_bf16_plan.py); each staged row's centre pixel and 9-bit tap mask are computed once per workgroup.  No im2col
// buffer, no atomics (equal inputs give equal bits), no scratch.
//
// The same kernel serves a ResNet cast to float16 on v_mfma_f32_32x32x16_f16: DT, the C ABI's dtype code (2 bfloat16, 1 float16), is
// the element type of x, w, residual and out (csrc/bf16_tile.hpp's TileElem<DT>); the bias stays float32, the gather moves raw words.
#include "bf16_tile.hpp"
#include "conv3x3_bf16_plan.hpp"

namespace opa {

namespace {

// M = batch * ho * wo output pixels, N = c_out, K = 9 * c_in
template <int DT, int BN, bool RES, bool RELU>
__global__ __launch_bounds__(256, 3) void conv3x3_bf16_kernel(
        const unsigned short* __restrict__ x, const unsigned short* __restrict__ W, const float* __restrict__ bias,
        const unsigned short* __restrict__ res, unsigned short* __restrict__ out, Conv3Bf16Geometry g, int M, int N) {
    using T = Bf16Tile<BN>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    const int tid = threadIdx.x, lane = bf16_tile_wave().lane, wn = bf16_tile_wave().wn;
    const Bf16TileOrigin org = bf16_tile_origin<BN>(N);
    const int m0 = org.m0, n0 = org.n0;

    u32x4_t rpre[2][T::VPL];
    if (RES) bf16_tile_fetch_residual<BN>(rpre[0], res, M, N, m0, n0, 0);   // the second half is fetched when the operand registers are free

    Conv3Bf16Row rows[kBf16Passes];            // this thread's four output pixels: centre and tap mask, once per workgroup
    conv3x3_bf16_plan_rows(g, m0, tid, rows);
    f32x16_t acc[2][T::NT];
    bf16_tile_mainloop<BN, DT>(smem, W, 9 * g.c_in, n0, acc, [&](int k0, u32x4_t (&ra)[kBf16Passes]) {   // a tap outside the image keeps its zeros
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++) ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
        conv3x3_bf16_plan_a(g, rows, tid, k0, [&](int p, long long at) { ra[p] = *reinterpret_cast<const u32x4_t*>(x + at); });
    });
    if (RES) bf16_tile_fetch_residual<BN>(rpre[1], res, M, N, m0, n0, 1);

    // epilogue, one 32-row block of the wave tile at a time
    float* patch = bf16_tile_patch<BN>(smem);
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < T::NT; j++) {
            const int col = j * 32 + (lane & 31);
            const float b = bias ? bias[n0 + wn * T::WN + col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) patch[bf16_tile_acc_row(r) * T::WN + col] = acc[i][j][r] + b;
        }
        bf16_tile_patch_sync();
        bf16_tile_store_rows<BN, RES, RELU, DT>(patch, rpre[i], out, M, N, m0, n0, i,
                                                [](float v) { return v < 0.0f ? 0.0f : v; });   // (a select: NaN stays NaN)
        bf16_tile_patch_sync();
    }
}

}  // namespace

long long conv3x3_bf16_workgroups(int B, int H, int W, int c_out, int S) {
    const long long M = (long long)B * conv3x3_bf16_out(H, S) * conv3x3_bf16_out(W, S);
    return (M + kBf16BM - 1) / kBf16BM * (c_out / (c_out % 128 == 0 ? 128 : 64));
}

hipError_t launch_conv3x3_bf16(const void* x, const void* w, const float* bias, const void* residual, void* out, int B, int H, int W,
                               int c_in, int c_out, int S, int D, int relu, hipStream_t st, int dtype) {
    if (B <= 0 || H <= 0 || W <= 0 || c_in <= 0 || c_out <= 0 || c_in % 64 != 0 || c_out % 64 != 0 || (S != 1 && S != 2) ||
        (D != 1 && D != 2 && D != 4) || (D > 1 && S != 1))
        return hipErrorInvalidValue;
    const long long M = (long long)B * conv3x3_bf16_out(H, S) * conv3x3_bf16_out(W, S);
    const long long blocks = conv3x3_bf16_workgroups(B, H, W, c_out, S);
    if ((long long)B * H * W * c_in > 0x7fffffffll || M * c_out > 0x7fffffffll || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const Conv3Bf16Geometry g = {B, H, W, c_in, S, D};
    return with_value<1, 2>(dtype, [&](auto DT) {
    return with_value<64, 128>(c_out % 128 == 0 ? 128 : 64, [&](auto BN) {
    return with_flag(residual != nullptr, [&](auto RES) {
    return with_flag(relu != 0, [&](auto RELU) {
        conv3x3_bf16_kernel<DT, BN, RES, RELU><<<(unsigned)blocks, kBf16Threads, 0, st>>>(
            (const unsigned short*)x, (const unsigned short*)w, bias, (const unsigned short*)residual, (unsigned short*)out, g, (int)M, c_out);
        return hipGetLastError();
    }); }); }); });
}

}  // namespace opa
