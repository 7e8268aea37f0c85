// Stand-alone check of csrc/stem7x7_bf16_plan.hpp, the load plan of the bf16 7x7 stem implicit GEMM: every access the kernel's threads
// would make is made here, on the CPU, against an x whose allocation begins at the first addressed element and ends at the last (so
// that a read before or behind is a heap overflow for the address sanitizer this program is built with), and counted per
// (row, tap, channel).  For every (B, h, w) x stride x layout (NCHW, channels-last, a view cropped out of a larger channels-last image)
// of the lists in main:
//   * no access reaches outside [x, x + last addressed element],
//   * every (row < M, tap inside the image, channel) is fetched exactly once per N-tile pass,
//   * no tap outside the image, no zero column of K and no row >= M is fetched at all,
//   * the staged 128 x 64 tile of every (m0, k0) equals a plainly computed im2col in the plan's K order: zeros in the padding, in K's
//     zero columns and in rows >= M.
// Prints one line and returns 0, or prints the first failures and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stem7x7_bf16_plan.hpp"

namespace {

int failures = 0;
long long fetches = 0, skipped = 0, zero_columns = 0;

void fail(const char* what, const opa::Stem7Bf16Geometry& g, long long row, int k, long long at) {
    if (failures++ < 20)
        std::printf("FAIL %s: B %d h %d w %d stride %d strides %lld %lld %lld %lld row %lld k %d at %lld\n", what, g.batch, g.h, g.w, g.stride,
                    g.x_batch, g.x_channel, g.x_row, g.x_pixel, row, k, at);
}

// the plain definition: element (row m, column k) of the im2col matrix -> its offset in x, -1 in the padding and for m >= M, -2 in a
// zero column of K
long long im2col_at(const opa::Stem7Bf16Geometry& g, long long m, int k) {
    const int ho = (g.h - 1) / g.stride + 1, wo = (g.w - 1) / g.stride + 1;
    const int ky = k / 24, kx = k % 24 / 3, ci = k % 3;
    if (ky >= 7 || kx >= 7) return -2;
    if (m >= (long long)g.batch * ho * wo) return -1;
    const int b = (int)(m / (ho * wo)), oy = (int)(m / wo % ho), ox = (int)(m % wo);
    const int iy = g.stride * oy - 3 + ky, ix = g.stride * ox - 3 + kx;
    if (iy < 0 || iy >= g.h || ix < 0 || ix >= g.w) return -1;
    return b * g.x_batch + ci * g.x_channel + iy * g.x_row + ix * g.x_pixel;
}

void check(const opa::Stem7Bf16Geometry& g) {
    // first element addressed: offset 0; last: every index at its maximum
    const long long elems = (g.batch - 1) * g.x_batch + 2 * g.x_channel + (g.h - 1) * g.x_row + (g.w - 1) * g.x_pixel + 1;
    unsigned short* x = static_cast<unsigned short*>(std::malloc((size_t)(elems * 2)));      // (begins and ends with x's extent)
    if (!x) std::abort();
    for (long long i = 0; i < elems; i++) x[i] = (unsigned short)(1 + (i * 2654435761u >> 7) % 65535);   // (never 0)
    const int ho = opa::stem7x7_bf16_out(g.h, g.stride), wo = opa::stem7x7_bf16_out(g.w, g.stride);
    const long long M = (long long)g.batch * ho * wo;
    const int K = opa::kStem7Bf16K;
    std::vector<unsigned char> count((size_t)(M * K), 0);                          // fetches per (row, k)
    for (int m0 = 0; m0 < M; m0 += opa::kBf16BM) {
        for (int t = 0; t < opa::kBf16Threads; t++) {
            opa::Stem7Bf16Row rows[opa::kBf16Passes];
            opa::stem7x7_bf16_plan_rows(g, m0, t, rows);                           // once per workgroup, as the kernel does
            for (int k0 = 0; k0 < K; k0 += opa::kBf16BK) {
                unsigned short chunk[opa::kBf16Passes][8] = {};
                const int col = k0 + (t & 7) * 8;
                opa::stem7x7_bf16_plan_a(g, rows, t, k0, [&](int p, int slot, long long at) {
                    const long long row = (long long)m0 + p * 32 + (t >> 3);
                    fetches++;
                    if (p < 0 || p >= opa::kBf16Passes || slot < 0 || slot > 7) { fail("a pass or slot out of range", g, row, col, at); return; }
                    if (at < 0 || at >= elems) { fail("outside x", g, row, col + slot, at); return; }
                    if (row >= M) { fail("a row >= M fetched", g, row, col + slot, at); return; }
                    chunk[p][slot] = x[at];
                    count[(size_t)(row * K + col + slot)]++;
                });
                for (int p = 0; p < opa::kBf16Passes; p++)
                    for (int e = 0; e < 8; e++) {
                        const long long row = (long long)m0 + p * 32 + (t >> 3);
                        const long long at = im2col_at(g, row, col + e);
                        if (chunk[p][e] != (at < 0 ? 0 : x[at])) fail("the staged tile is not the im2col tile", g, row, col + e, at);
                    }
            }
        }
    }
    for (long long row = 0; row < M; row++)
        for (int k = 0; k < K; k++) {
            const long long at = im2col_at(g, row, k);
            const int want = at >= 0 ? 1 : 0;
            if (at == -1) skipped++;
            if (at == -2) zero_columns++;
            if (count[(size_t)(row * K + k)] != want)
                fail(want ? "an element of a valid tap not fetched exactly once" : at == -1 ? "a tap outside the image fetched" : "a zero column of K fetched",
                     g, row, k, at);
        }
    std::free(x);
}

}  // namespace

int main() {
    const int shapes[][3] = {{1, 1, 1}, {1, 3, 3}, {2, 7, 5}, {3, 23, 19}};
    int launches = 0;
    for (const auto& s : shapes)
        for (int stride = 1; stride <= 2; stride++) {
            const long long h = s[1], w = s[2], H = h + 5, W = w + 4;              // (H, W: the larger image of the cropped view)
            check(opa::Stem7Bf16Geometry{s[0], s[1], s[2], stride, 3 * h * w, h * w, w, 1});            // NCHW
            check(opa::Stem7Bf16Geometry{s[0], s[1], s[2], stride, h * w * 3, 1, w * 3, 3});            // channels-last
            check(opa::Stem7Bf16Geometry{s[0], s[1], s[2], stride, H * W * 3, 1, W * 3, 3});            // a crop of [B, 3, H, W] channels-last
            launches += 3;
        }
    std::printf("stem7x7_bf16_plan: %d launches, %lld fetches, %lld elements of padding left alone, %lld zero columns left alone, %d failures\n",
                launches, fetches, skipped, zero_columns, failures);
    return failures ? 1 : 0;
}
