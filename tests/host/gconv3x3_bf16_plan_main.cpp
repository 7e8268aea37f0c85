// Stand-alone check of csrc/gconv3x3_bf16_plan.hpp, the load plan of the bf16 GROUPED 3x3 implicit GEMM: every access the kernel's
// threads would make is made here, on the CPU, against an x whose allocation ends with its last byte (so that an over-read is a heap
// overflow for the address sanitizer this program is built with), and counted per (row, tap, 16-byte chunk of ALL C channels) and
// N-tile.  For every (B, h, w) x C x (stride, dilation) of the lists in main, and every N-tile n0 of the launch:
//   * no access reaches outside [x, x + B * h * w * C), and each is 16 bytes on a 16-byte boundary,
//   * every (row < M, tap inside the image, chunk of the channels n0 .. n0 + 63) is fetched exactly once,
//   * no chunk of another tile's channels, no tap outside the image, and no row >= M, is fetched at all,
//   * the staged 128 x 64 tile of every (m0, k0) equals a plainly computed im2col of the channel slice n0 .. n0 + 63: zeros in the
//     padding and in rows >= M.
// Prints one line and returns 0, or prints the first failures and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gconv3x3_bf16_plan.hpp"

namespace {

int failures = 0;
long long fetches = 0, skipped = 0;

void fail(const char* what, const opa::Conv3Bf16Geometry& g, int n0, long long row, int tap, long long at) {
    if (failures++ < 20)
        std::printf("FAIL %s: B %d h %d w %d C %d stride %d dilation %d n0 %d row %lld tap %d at %lld\n", what, g.batch, g.h, g.w, g.c_in,
                    g.stride, g.dilation, n0, row, tap, at);
}

// the plain definition: element (row m, column k = tap * 64 + j) of the im2col matrix of the channel slice n0 .. n0 + 63 -> its offset
// in x, or -1 in the padding and for m >= M
long long im2col_at(const opa::Conv3Bf16Geometry& g, int n0, long long m, int k) {
    const int ho = (g.h - 1) / g.stride + 1, wo = (g.w - 1) / g.stride + 1;
    if (m >= (long long)g.batch * ho * wo) return -1;
    const int b = (int)(m / (ho * wo)), oy = (int)(m / wo % ho), ox = (int)(m % wo);
    const int tap = k / 64, j = k % 64, ky = tap / 3, kx = tap % 3;
    const int iy = g.stride * oy - g.dilation + g.dilation * ky, ix = g.stride * ox - g.dilation + g.dilation * kx;
    if (iy < 0 || iy >= g.h || ix < 0 || ix >= g.w) return -1;
    return (((long long)b * g.h + iy) * g.w + ix) * g.c_in + n0 + j;
}

void check(const opa::Conv3Bf16Geometry& g) {
    const long long elems = (long long)g.batch * g.h * g.w * g.c_in;
    void* block = nullptr;
    if (posix_memalign(&block, 16, (size_t)(elems * 2)) != 0) std::abort();       // (ends with x's last byte)
    unsigned short* x = static_cast<unsigned short*>(block);
    for (long long i = 0; i < elems; i++) x[i] = (unsigned short)(1 + (i * 2654435761u >> 7) % 65535);   // (never 0)
    const int ho = opa::conv3x3_bf16_out(g.h, g.stride), wo = opa::conv3x3_bf16_out(g.w, g.stride);
    const long long M = (long long)g.batch * ho * wo;
    const int chunks = g.c_in / 8;                                                  // of ALL channels
    for (int n0 = 0; n0 < g.c_in; n0 += opa::kGconv3Bf16BN) {
        std::vector<unsigned char> count((size_t)(M * 9 * chunks), 0);              // fetches per (row, tap, chunk) of this N-tile
        for (int m0 = 0; m0 < M; m0 += opa::kBf16BM) {
            for (int t = 0; t < opa::kBf16Threads; t++) {
                opa::Conv3Bf16Row rows[opa::kBf16Passes];
                opa::conv3x3_bf16_plan_rows(g, m0, t, rows);                       // once per workgroup, as the kernel does
                for (int k0 = 0; k0 < opa::kGconv3Bf16K; k0 += opa::kBf16BK) {
                    unsigned short chunk[opa::kBf16Passes][8] = {};
                    const int tap = k0 / 64;
                    opa::gconv3x3_bf16_plan_a(g, rows, t, n0, k0, [&](int p, long long at) {
                        const long long row = (long long)m0 + p * 32 + (t >> 3);
                        fetches++;
                        if (at < 0 || at + 8 > elems || at % 8 != 0) { fail("outside x or misaligned", g, n0, row, tap, at); return; }
                        if (row >= M) { fail("a row >= M fetched", g, n0, row, tap, at); return; }
                        std::memcpy(chunk[p], x + at, 16);
                        const long long pixel = at / g.c_in, want = im2col_at(g, n0, row, k0);
                        if (want < 0 || pixel != want / g.c_in) { fail("a chunk of the wrong pixel", g, n0, row, tap, at); return; }
                        count[(size_t)((row * 9 + tap) * chunks + at % g.c_in / 8)]++;
                    });
                    for (int p = 0; p < opa::kBf16Passes; p++)
                        for (int e = 0; e < 8; e++) {
                            const long long row = (long long)m0 + p * 32 + (t >> 3);
                            const long long at = im2col_at(g, n0, row, k0 + (t & 7) * 8 + e);
                            if (chunk[p][e] != (at < 0 ? 0 : x[at])) fail("the staged tile is not the im2col tile", g, n0, row, tap, at);
                        }
                }
            }
        }
        for (long long row = 0; row < M; row++)
            for (int tap = 0; tap < 9; tap++) {
                const int valid = im2col_at(g, n0, row, tap * 64) >= 0 ? 1 : 0;
                skipped += (1 - valid) * 8;
                for (int c = 0; c < chunks; c++) {
                    const bool own = c >= n0 / 8 && c < n0 / 8 + 8;
                    const int got = count[(size_t)((row * 9 + tap) * chunks + c)];
                    if (!own && got != 0) fail("a chunk of another tile's channels fetched", g, n0, row, tap, c);
                    if (own && got != valid)
                        fail(valid ? "a chunk of a valid tap not fetched exactly once" : "a tap outside the image fetched", g, n0, row, tap, c);
                }
            }
    }
    std::free(block);
}

}  // namespace

int main() {
    const int shapes[][3] = {{1, 1, 1}, {1, 3, 3}, {2, 7, 5}, {3, 23, 19}}, channels[] = {64, 192};
    const int modes[][2] = {{1, 1}, {2, 1}, {1, 2}, {1, 4}};                       // (stride, dilation)
    int launches = 0;
    for (const auto& s : shapes)
        for (int c : channels)
            for (const auto& m : modes) {
                check(opa::Conv3Bf16Geometry{s[0], s[1], s[2], c, m[0], m[1]});
                launches++;
            }
    std::printf("gconv3x3_bf16_plan: %d launches, %lld fetches, %lld chunks of padding left alone, %d failures\n", launches, fetches,
                skipped, failures);
    return failures ? 1 : 0;
}
