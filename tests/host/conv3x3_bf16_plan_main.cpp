// Stand-alone check of csrc/conv3x3_bf16_plan.hpp, the load plan of the bf16 3x3 implicit GEMM: every access the kernel's threads
// would make is made here, on the CPU, against an x whose allocation ends with its last byte (so that an over-read is a heap
// overflow for the address sanitizer this program is built with), and counted per (row, tap, 16-byte chunk).  For every
// (B, h, w) x c_in x (stride, dilation) of the lists in main:
//   * no access reaches outside [x, x + B * h * w * c_in), and each is 16 bytes on a 16-byte boundary,
//   * every (row < M, tap inside the image, chunk) is fetched exactly once per N-tile pass,
//   * no tap outside the image, and no row >= M, is fetched at all,
//   * the staged 128 x 64 tile of every (m0, k0) equals a plainly computed im2col: zeros in the padding and in rows >= M.
// Prints one line and returns 0, or prints the first failures and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "conv3x3_bf16_plan.hpp"

namespace {

int failures = 0;
long long fetches = 0, skipped = 0;

void fail(const char* what, const opa::Conv3Bf16Geometry& g, long long row, int tap, long long at) {
    if (failures++ < 20)
        std::printf("FAIL %s: B %d h %d w %d c_in %d stride %d dilation %d row %lld tap %d at %lld\n", what, g.batch, g.h, g.w, g.c_in,
                    g.stride, g.dilation, row, tap, at);
}

// the plain definition: element (row m, column k) of the im2col matrix -> its offset in x, or -1 in the padding and for m >= M
long long im2col_at(const opa::Conv3Bf16Geometry& g, long long m, int k) {
    const int ho = (g.h - 1) / g.stride + 1, wo = (g.w - 1) / g.stride + 1;
    if (m >= (long long)g.batch * ho * wo) return -1;
    const int b = (int)(m / (ho * wo)), oy = (int)(m / wo % ho), ox = (int)(m % wo);
    const int tap = k / g.c_in, ci = k % g.c_in, ky = tap / 3, kx = tap % 3;
    const int iy = g.stride * oy - g.dilation + g.dilation * ky, ix = g.stride * ox - g.dilation + g.dilation * kx;
    if (iy < 0 || iy >= g.h || ix < 0 || ix >= g.w) return -1;
    return (((long long)b * g.h + iy) * g.w + ix) * g.c_in + ci;
}

void check(const opa::Conv3Bf16Geometry& g) {
    const long long elems = (long long)g.batch * g.h * g.w * g.c_in;
    void* block = nullptr;
    if (posix_memalign(&block, 16, (size_t)(elems * 2)) != 0) std::abort();       // (ends with x's last byte)
    unsigned short* x = static_cast<unsigned short*>(block);
    for (long long i = 0; i < elems; i++) x[i] = (unsigned short)(1 + (i * 2654435761u >> 7) % 65535);   // (never 0)
    const int ho = opa::conv3x3_bf16_out(g.h, g.stride), wo = opa::conv3x3_bf16_out(g.w, g.stride);
    const long long M = (long long)g.batch * ho * wo;
    const int K = 9 * g.c_in, chunks = g.c_in / 8;
    std::vector<unsigned char> count((size_t)(M * 9 * chunks), 0);                  // fetches per (row, tap, chunk)
    for (int m0 = 0; m0 < M; m0 += opa::kConv3Bf16BM) {
        for (int t = 0; t < opa::kConv3Bf16Threads; t++) {
            opa::Conv3Bf16Row rows[opa::kConv3Bf16Passes];
            opa::conv3x3_bf16_plan_rows(g, m0, t, rows);                           // once per workgroup, as the kernel does
            for (int k0 = 0; k0 < K; k0 += opa::kConv3Bf16BK) {
                unsigned short chunk[opa::kConv3Bf16Passes][8] = {};
                const int tap = k0 / g.c_in, col = k0 % g.c_in + (t & 7) * 8;
                opa::conv3x3_bf16_plan_a(g, rows, t, k0, [&](int p, long long at) {
                    const long long row = (long long)m0 + p * 32 + (t >> 3);
                    fetches++;
                    if (at < 0 || at + 8 > elems || at % 8 != 0) { fail("outside x or misaligned", g, row, tap, at); return; }
                    if (row >= M) { fail("a row >= M fetched", g, row, tap, at); return; }
                    std::memcpy(chunk[p], x + at, 16);
                    count[(size_t)((row * 9 + tap) * chunks + col / 8)]++;
                });
                for (int p = 0; p < opa::kConv3Bf16Passes; p++)
                    for (int e = 0; e < 8; e++) {
                        const long long row = (long long)m0 + p * 32 + (t >> 3);
                        const long long at = im2col_at(g, row, k0 + (t & 7) * 8 + e);
                        if (chunk[p][e] != (at < 0 ? 0 : x[at])) fail("the staged tile is not the im2col tile", g, row, tap, at);
                    }
            }
        }
    }
    for (long long row = 0; row < M; row++)
        for (int tap = 0; tap < 9; tap++) {
            const int want = im2col_at(g, row, tap * g.c_in) >= 0 ? 1 : 0;
            skipped += (1 - want) * chunks;
            for (int c = 0; c < chunks; c++)
                if (count[(size_t)((row * 9 + tap) * chunks + c)] != want)
                    fail(want ? "a chunk of a valid tap not fetched exactly once" : "a tap outside the image fetched", g, row, tap, c);
        }
    std::free(block);
}

}  // namespace

int main() {
    const int shapes[][3] = {{1, 1, 1}, {1, 3, 3}, {2, 7, 5}, {3, 23, 19}}, channels[] = {64, 128};
    const int modes[][2] = {{1, 1}, {2, 1}, {1, 2}, {1, 4}};                       // (stride, dilation)
    int launches = 0;
    for (const auto& s : shapes)
        for (int c_in : channels)
            for (const auto& m : modes) {
                check(opa::Conv3Bf16Geometry{s[0], s[1], s[2], c_in, m[0], m[1]});
                launches++;
            }
    std::printf("conv3x3_bf16_plan: %d launches, %lld fetches, %lld chunks of padding left alone, %d failures\n", launches, fetches, skipped,
                failures);
    return failures ? 1 : 0;
}
