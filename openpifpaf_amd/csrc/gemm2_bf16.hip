// The tail of the first block of a ResNet stage cast to bfloat16 (reference network/basenetworks.py:71-150: torchvision's Bottleneck
// and BasicBlock through torch.nn.Conv2d): the block's last 1x1 convolution and its downsampling 1x1 convolution as ONE product on
// v_mfma_f32_32x32x16_bf16, float32 accumulation, ONE rounding at the store:
//     out[b, oy, ox, :] = bf16_rne(act([A1[m, 0:k1] | x[b, s*oy, s*ox, 0:k2]] * Wcat[n, 0:k1+k2]^T + bias[n])),  m = (b*ho + oy)*wo + ox
// A1 [M, k1] dense bf16 (the block's inner activation), x [B, h, w, k2] dense channels-last bf16 (the block's input), Wcat [n][k1 + k2]
// bf16 (K-major: both weights side by side), bias float32 [n] or null, out dense bf16 [B, ho, wo, n]; k1 % 64 == 0 (k1 == 0 with a
// null A1: the strided 1x1 convolution alone), k2 % 64 == 0, n % 64 == 0, stride s 1 or 2.  The identity tensor is never written.
//
// Tile, main loop and the epilogue's 16-byte rows are csrc/bf16_tile.hpp's (BN = 128 where n allows, else 64).  What is this
// kernel's own is A: per K-step a row of A1 or a pixel of x.  Which 16 bytes a thread loads for a K-step -- or that it loads nothing,
// for a row >= M -- is decided in csrc/gemm2_bf16_plan.hpp, which a CPU program enumerates (tests/test_gemm2_bf16_plan.py); each
// staged row's two offsets are computed once per thread.  No workspace, no atomics (equal inputs give equal bits), no scratch.
//
// The same kernel serves a ResNet cast to float16 on v_mfma_f32_32x32x16_f16: DT, the C ABI's dtype code (2 bfloat16, 1 float16), is
// the element type of A1, x, Wcat, a_bias and out (csrc/bf16_tile.hpp's TileElem<DT>); the bias stays float32.
#include "bf16_tile.hpp"
#include "gemm2_bf16_plan.hpp"

namespace opa {

namespace {

// PRO: A1 is the RAW output of the preceding convolution; its bias + ReLU (a_bias[k], per channel of A1) are applied while a K-step
// of A1 is staged -- csrc/gemm_epilogue.hip's arithmetic: f32 add, max, round to nearest even.  K-steps of x are staged as they are.
// M = batch * ho * wo output pixels, N = n, K = k1 + k2
template <int DT, int BN, bool RELU, bool PRO>
__global__ __launch_bounds__(256, 3) void gemm2_bf16_kernel(
        const unsigned short* __restrict__ A1, const unsigned short* __restrict__ x, const unsigned short* __restrict__ W,
        const float* __restrict__ bias, unsigned short* __restrict__ out, Gemm2Bf16Geometry g, int M, int N,
        const unsigned short* __restrict__ a_bias) {
    using T = Bf16Tile<BN>;
    using E = TileElem<DT>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    const int tid = threadIdx.x, lane = bf16_tile_wave().lane, wn = bf16_tile_wave().wn;
    const Bf16TileOrigin org = bf16_tile_origin<BN>(N);
    const int m0 = org.m0, n0 = org.n0;

    Gemm2Bf16Row rows[kBf16Passes];            // this thread's four rows: offsets into both sources, once per thread
    gemm2_bf16_plan_rows(g, m0, tid, rows);
    f32x16_t acc[2][T::NT];
    bf16_tile_mainloop<BN, DT>(smem, W, g.k1 + g.k2, n0, acc, [&](int k0, u32x4_t (&ra)[kBf16Passes]) {   // a row >= M keeps its zeros
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++) ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
        gemm2_bf16_plan_a(g, rows, tid, k0, [&](int p, int source, long long at) {
            ra[p] = *reinterpret_cast<const u32x4_t*>((source == kGemm2Bf16A1 ? A1 : x) + at);
        });
        if (PRO && k0 < g.k1) {
            const u32x4_t ab = *reinterpret_cast<const u32x4_t*>(a_bias + k0 + bf16_tile_stage(tid).col);
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

    // epilogue, one 32-row block of the wave tile at a time
    const u32x4_t none[T::VPL] = {};
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
        bf16_tile_store_rows<BN, false, RELU, DT>(patch, none, out, M, N, m0, n0, i,
                                                  [](float v) { return v < 0.0f ? 0.0f : v; });   // (a select: NaN stays NaN)
        bf16_tile_patch_sync();
    }
}

}  // namespace

long long gemm2_bf16_workgroups(int B, int H, int W, int n, int S) {
    const long long M = (long long)B * gemm2_bf16_out(H, S) * gemm2_bf16_out(W, S);
    return (M + kBf16BM - 1) / kBf16BM * (n / (n % 128 == 0 ? 128 : 64));
}

hipError_t launch_gemm2_bf16(const void* a1, int k1, const void* x, int k2, int B, int H, int W, int S, const void* a_bias,
                             const void* wcat, const float* bias, void* out, int n, int relu, hipStream_t st, int dtype) {
    if (B <= 0 || H <= 0 || W <= 0 || k1 < 0 || k2 <= 0 || n <= 0 || k1 % 64 != 0 || k2 % 64 != 0 || n % 64 != 0 || (S != 1 && S != 2) ||
        (a1 == nullptr) != (k1 == 0) || (a_bias != nullptr && k1 == 0) || !x || !wcat || !out)
        return hipErrorInvalidValue;
    const long long M = (long long)B * gemm2_bf16_out(H, S) * gemm2_bf16_out(W, S);
    const long long blocks = gemm2_bf16_workgroups(B, H, W, n, S);
    if ((long long)B * H * W * k2 > 0x7fffffffll || M * k1 > 0x7fffffffll || M * n > 0x7fffffffll || blocks > 0x7fffffffll)
        return hipErrorInvalidValue;
    const Gemm2Bf16Geometry g = {B, H, W, k1, k2, S};
    return with_value<1, 2>(dtype, [&](auto DT) {
    return with_value<64, 128>(n % 128 == 0 ? 128 : 64, [&](auto BN) {
    return with_flag(relu != 0, [&](auto RELU) {
    return with_flag(a_bias != nullptr, [&](auto PRO) {
        gemm2_bf16_kernel<DT, BN, RELU, PRO><<<(unsigned)blocks, kBf16Threads, 0, st>>>(
            (const unsigned short*)a1, (const unsigned short*)x, (const unsigned short*)wcat, bias, (unsigned short*)out, g, (int)M, n,
            (const unsigned short*)a_bias);
        return hipGetLastError();
    }); }); }); });
}

}  // namespace opa
