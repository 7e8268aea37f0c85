// A 16-bit head in ONE kernel: the 1x1 convolution on the 16-bit MFMA and everything CompositeField4 does behind it
// (reference network/heads.py:330-378),
//     fields[B, F, C, H, W] (float32) = field( shuffle_crop( x[M, K] * Wp[Np, K]^T + bias[Np] ) )
// x the trunk's output, dense channels-last, viewed as [M = B * hc * wc][K] (bf16: DT 2, f16: DT 1; K % 64 == 0), Wp the weight padded
// with zero rows from N = F * C * us^2 to Np, a multiple of the 64-wide N-tile, bias float32 [Np].  The float32 accumulators never
// become 16-bit: + bias they go through the wave's LDS patch and csrc/head_field.hpp's field function to their shuffled, cropped
// places.  What torch's 16-bit convolution + csrc/head.hip write and read back between the two -- [M][N] rounded to 8 or 11
// significand bits -- does not exist here.
//
// Tile and main loop are csrc/bf16_tile.hpp's at BN = 64, A a plain row fetch (csrc/gemm_epilogue.hip's: a row >= M is not loaded).
// This kernel's own is the epilogue, and every output address of it comes from csrc/head16_plan.hpp (lane map, patch pitch and
// the bank arithmetic: there).  Columns >= N are multiplied and never stored.  Plain vector stores, each element by exactly one
// thread: no atomics, no workspace, equal bits from equal inputs.
#include "bf16_tile.hpp"
#include "head16_plan.hpp"
#include "head_field.hpp"

namespace opa {

static_assert(4 * 32 * (kHead16WN + 2) * 4 <= Bf16Tile<kHead16BN>::LDS_BYTES, "the four patches at their widest pitch fit the staging LDS");

template <int DT, int US>
__global__ __launch_bounds__(256, 4) void head16_kernel(
        const unsigned short* __restrict__ X, const unsigned short* __restrict__ W, const float* __restrict__ bias,
        float* __restrict__ out, Head16Geometry g, int M, int Np, int K, int n_conf, int n_vec, unsigned offset_mask, int n_scales) {
    constexpr int BN = kHead16BN;
    using T = Bf16Tile<BN>;
    static_assert(T::NT == 1 && T::WN == kHead16WN, "one 32 x 32 accumulator block per 32-row block of the wave tile");
    constexpr int PITCH = kHead16WN + US;                  // words of a patch row: conflict-free column reads (csrc/head16_plan.hpp)
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    const int lane = bf16_tile_wave().lane, wave = bf16_tile_wave().wave, wn = bf16_tile_wave().wn;
    const Bf16TileOrigin org = bf16_tile_origin<BN>(Np);
    const int m0 = org.m0, n0 = org.n0;
    g.us = US;                                             // (the launcher's dispatch: the plan's branches on it fold)

    const int s_row = bf16_tile_stage(threadIdx.x).row, s_col = bf16_tile_stage(threadIdx.x).col;
    f32x16_t acc[2][T::NT];
    bf16_tile_mainloop<BN, DT>(smem, W, K, n0, acc, [&](int k0, u32x4_t (&ra)[kBf16Passes]) {
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++) {
            const int m = m0 + p * 32 + s_row;
            ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
            if (m < M) ra[p] = *reinterpret_cast<const u32x4_t*>(X + (size_t)m * K + k0 + s_col);
        }
    });

    Head16Row rows[2];
    head16_plan_rows(g, m0, threadIdx.x, rows);
    // epilogue, one 32-row block of the wave tile at a time
    float* patch = reinterpret_cast<float*>(smem) + wave * (32 * PITCH);
    const int col = lane & 31;
    const float b = bias[n0 + wn * T::WN + col];
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int r = 0; r < 16; r++) patch[bf16_tile_acc_row(r) * PITCH + col] = acc[i][0][r] + b;
        bf16_tile_patch_sync();
        head16_plan_block(g, rows[i], n0, threadIdx.x, [&](int prow, int pcol, int at, int plane, int y, int x) {
            out[at] = head_field(patch[prow * PITCH + pcol], plane % g.n_comp, x, y, n_conf, n_vec, offset_mask, n_scales);
        });
        bf16_tile_patch_sync();
    }
}

long long head16_workgroups(int B, int hc, int wc, int n_fields, int n_comp, int us) {
    const Head16Geometry g{B, hc, wc, n_fields, n_comp, us};
    const long long M = (long long)B * hc * wc;
    return (M + kBf16BM - 1) / kBf16BM * (head16_n_padded(g) / kHead16BN);
}

hipError_t launch_head16(const void* x, const void* w, const float* bias, float* out, int B, int hc, int wc, int K, int n_fields,
                         int n_comp, int us, int n_conf, int n_vec, unsigned offset_mask, int n_scales, hipStream_t st, int dtype) {
    const Head16Geometry g{B, hc, wc, n_fields, n_comp, us};
    const int M = B * hc * wc, Np = head16_n_padded(g);
    const unsigned blocks = (unsigned)head16_workgroups(B, hc, wc, n_fields, n_comp, us);
    return with_value<1, 2>(dtype, [&](auto DT) {
    return with_value<1, 2>(us, [&](auto US) {
        head16_kernel<DT, US><<<blocks, 256, 0, st>>>((const unsigned short*)x, (const unsigned short*)w, bias, out, g, M, Np, K, n_conf,
                                                      n_vec, offset_mask, n_scales);
        return hipGetLastError();
    }); });
}

}  // namespace opa
