// The 7x7 RGB stem of a ResNet cast to bfloat16 (reference network/basenetworks.py:71-150: torchvision's conv1 through torch.nn.Conv2d)
// as an implicit GEMM on v_mfma_f32_32x32x16_bf16, float32 accumulation, ONE rounding at the store:
//     out[b, oy, ox, co] = bf16_rne(act(sum_{ky,kx,ci} x[b, ci, s*oy - 3 + ky, s*ox - 3 + kx] * w[co][ky * 24 + kx * 3 + ci] + bias[co]))
// x [B, 3, h, w] bf16 read WHERE IT LIES through its four element strides (channels-last, NCHW, a cropped view: no padded copy, no
// 4-channel copy), w [c_out][192] bf16 (K-major; zeros in the columns kx = 7 and ky = 7 that pad 147 to 192), bias float32 [c_out] or
// null, out dense channels-last bf16 [B, ho, wo, c_out]; c_out % 64 == 0, stride s 1 or 2, padding 3.
//
// Tile, main loop and the epilogue's 16-byte rows are csrc/bf16_tile.hpp's (BN = 128 where c_out allows, else 64): this is its fourth
// operand fetcher.  A is a gather of single 2-byte elements -- nearly all of them L1 / L2 hits, the image is far smaller than what is
// written --, assembled into the thread's four 16-byte chunks.  Which element goes where, or that nothing is loaded (a tap outside
// the image, a zero column of K, a row >= M), is decided in csrc/stem7x7_bf16_plan.hpp, which a CPU program enumerates
// (tests/test_stem7x7_bf16_plan.py); each staged row's centre pixel and its two 7-bit masks are computed once per workgroup.  No
// im2col buffer, no atomics (equal inputs give equal bits), no scratch.
//
// The same kernel serves a ResNet cast to float16 on v_mfma_f32_32x32x16_f16: DT, the C ABI's dtype code (2 bfloat16, 1 float16), is the
// element type of x, w and out (csrc/bf16_tile.hpp's TileElem<DT>); the bias stays float32, and the gather ORs raw 16-bit words into the
// chunks whatever they encode.
#include "bf16_tile.hpp"
#include "stem7x7_bf16_plan.hpp"

namespace opa {

namespace {

// M = batch * ho * wo output pixels, N = c_out, K = 192
template <int DT, int BN, bool RELU>
__global__ __launch_bounds__(256, 3) void stem7x7_bf16_kernel(
        const unsigned short* __restrict__ x, const unsigned short* __restrict__ W, const float* __restrict__ bias,
        unsigned short* __restrict__ out, Stem7Bf16Geometry g, int M, int N) {
    using T = Bf16Tile<BN>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    const int tid = threadIdx.x, lane = bf16_tile_wave().lane, wn = bf16_tile_wave().wn;
    const Bf16TileOrigin org = bf16_tile_origin<BN>(N);
    const int m0 = org.m0, n0 = org.n0;

    Stem7Bf16Row rows[kBf16Passes];            // this thread's four output pixels: centre and masks, once per workgroup
    stem7x7_bf16_plan_rows(g, m0, tid, rows);
    f32x16_t acc[2][T::NT];
    bf16_tile_mainloop<BN, DT>(smem, W, kStem7Bf16K, n0, acc, [&](int k0, u32x4_t (&ra)[kBf16Passes]) {   // what is not loaded keeps its zeros
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++) ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
        stem7x7_bf16_plan_a(g, rows, tid, k0, [&](int p, int slot, long long at) { ra[p][slot >> 1] |= (unsigned)*(x + at) << (16 * (slot & 1)); });
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

long long stem7x7_bf16_workgroups(int B, int H, int W, int c_out, int S) {
    const long long M = (long long)B * stem7x7_bf16_out(H, S) * stem7x7_bf16_out(W, S);
    return (M + kBf16BM - 1) / kBf16BM * (c_out / (c_out % 128 == 0 ? 128 : 64));
}

hipError_t launch_stem7x7_bf16(const void* x, long long xb, long long xc, long long xr, long long xp, const void* w, const float* bias,
                               void* out, int B, int H, int W, int c_out, int S, int relu, hipStream_t st, int dtype) {
    if (B <= 0 || H <= 0 || W <= 0 || c_out <= 0 || c_out % 64 != 0 || (S != 1 && S != 2) || xb <= 0 || xc <= 0 || xr <= 0 || xp <= 0)
        return hipErrorInvalidValue;
    const long long M = (long long)B * stem7x7_bf16_out(H, S) * stem7x7_bf16_out(W, S);
    const long long blocks = stem7x7_bf16_workgroups(B, H, W, c_out, S);
    // the last element of x addressed (in double: the stride of a dimension of one element may be anything, and addresses nothing)
    const double last = (B - 1.0) * (double)xb + 2.0 * (double)xc + (H - 1.0) * (double)xr + (W - 1.0) * (double)xp;
    if (last >= 2147483648.0 || M * c_out > 0x7fffffffll || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const Stem7Bf16Geometry g = {B, H, W, S, xb, xc, xr, xp};
    return with_value<1, 2>(dtype, [&](auto DT) {
    return with_value<64, 128>(c_out % 128 == 0 ? 128 : 64, [&](auto BN) {
    return with_flag(relu != 0, [&](auto RELU) {
        stem7x7_bf16_kernel<DT, BN, RELU><<<(unsigned)blocks, kBf16Threads, 0, st>>>(
            (const unsigned short*)x, (const unsigned short*)w, bias, (unsigned short*)out, g, (int)M, c_out);
        return hipGetLastError();
    }); }); });
}

}  // namespace opa
