// Stand-alone check of csrc/gemm2_bf16_plan.hpp, the load plan of the bf16 two-source GEMM: every access the kernel's threads would
// make is made here, on the CPU, against an A1 and an x whose allocations end with their last byte (so that an over-read is a heap
// overflow for the address sanitizer this program is built with), and counted per (row, 16-byte chunk of K).  For every
// (B, h, w, stride, k1, k2) of the list in main:
//   * no access reaches outside [A1, A1 + M * k1) or [x, x + B * h * w * k2), and each is 16 bytes on a 16-byte boundary,
//   * every (row < M, chunk) is fetched exactly once, from the source and the offset that the definition gives,
//   * no row >= M is fetched at all,
//   * the staged 128 x 64 tile of every (m0, k0) equals the plainly computed concatenated matrix: zeros in rows >= M.
// Prints one line and returns 0, or prints the first failures and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm2_bf16_plan.hpp"

namespace {

int failures = 0;
long long fetches = 0, dead_rows = 0;

void fail(const char* what, const opa::Gemm2Bf16Geometry& g, long long row, int k, long long at) {
    if (failures++ < 20)
        std::printf("FAIL %s: B %d h %d w %d k1 %d k2 %d stride %d row %lld k %d at %lld\n", what, g.batch, g.h, g.w, g.k1, g.k2, g.stride,
                    row, k, at);
}

// the plain definition: element (row m, column k) of [A1 | x at stride] -> its source and its offset there; source -1 for m >= M
struct Where {
    int source;
    long long at;
};
Where concat_at(const opa::Gemm2Bf16Geometry& g, long long m, int k) {
    const int ho = (g.h - 1) / g.stride + 1, wo = (g.w - 1) / g.stride + 1;
    if (m >= (long long)g.batch * ho * wo) return {-1, -1};
    if (k < g.k1) return {opa::kGemm2Bf16A1, m * g.k1 + k};
    const int b = (int)(m / (ho * wo)), oy = (int)(m / wo % ho), ox = (int)(m % wo);
    return {opa::kGemm2Bf16X, (((long long)b * g.h + g.stride * oy) * g.w + g.stride * ox) * g.k2 + (k - g.k1)};
}

unsigned short* filled(long long elems, unsigned salt) {               // (ends with the tensor's last byte; never 0)
    if (elems == 0) return nullptr;
    void* block = nullptr;
    if (posix_memalign(&block, 16, (size_t)(elems * 2)) != 0) std::abort();
    unsigned short* p = static_cast<unsigned short*>(block);
    for (long long i = 0; i < elems; i++) p[i] = (unsigned short)(1 + ((i + salt) * 2654435761u >> 7) % 65535);
    return p;
}

void check(const opa::Gemm2Bf16Geometry& g) {
    const int ho = opa::gemm2_bf16_out(g.h, g.stride), wo = opa::gemm2_bf16_out(g.w, g.stride);
    const long long M = (long long)g.batch * ho * wo;
    const long long elems[2] = {M * g.k1, (long long)g.batch * g.h * g.w * g.k2};
    unsigned short* const src[2] = {filled(elems[0], 0u), filled(elems[1], 12345u)};
    const int K = g.k1 + g.k2, chunks = K / 8;
    std::vector<unsigned char> count((size_t)(M * chunks), 0);                      // fetches per (row, chunk)
    for (long long m0 = 0; m0 < M; m0 += opa::kBf16BM) {
        for (int t = 0; t < opa::kBf16Threads; t++) {
            opa::Gemm2Bf16Row rows[opa::kBf16Passes];
            opa::gemm2_bf16_plan_rows(g, (int)m0, t, rows);                         // once per thread, as the kernel does
            for (int k0 = 0; k0 < K; k0 += opa::kBf16BK) {
                unsigned short chunk[opa::kBf16Passes][8] = {};
                const int col = k0 + (t & 7) * 8;
                opa::gemm2_bf16_plan_a(g, rows, t, k0, [&](int p, int source, long long at) {
                    const long long row = m0 + p * 32 + (t >> 3);
                    fetches++;
                    if (source != opa::kGemm2Bf16A1 && source != opa::kGemm2Bf16X) { fail("no such source", g, row, col, at); return; }
                    if (at < 0 || at + 8 > elems[source] || at % 8 != 0) { fail("outside the tensor or misaligned", g, row, col, at); return; }
                    if (row >= M) { fail("a row >= M fetched", g, row, col, at); return; }
                    const Where want = concat_at(g, row, col);
                    if (want.source != source || want.at != at) { fail("wrong source or offset", g, row, col, at); return; }
                    std::memcpy(chunk[p], src[source] + at, 16);
                    count[(size_t)(row * chunks + col / 8)]++;
                });
                for (int p = 0; p < opa::kBf16Passes; p++)
                    for (int e = 0; e < 8; e++) {
                        const long long row = m0 + p * 32 + (t >> 3);
                        const Where w = concat_at(g, row, col + e);
                        if (chunk[p][e] != (w.source < 0 ? 0 : src[w.source][w.at]))
                            fail("the staged tile is not the concatenated matrix", g, row, col + e, w.at);
                    }
            }
        }
    }
    for (long long row = 0; row < M; row++)
        for (int c = 0; c < chunks; c++)
            if (count[(size_t)(row * chunks + c)] != 1) fail("a chunk not fetched exactly once", g, row, c * 8, count[(size_t)(row * chunks + c)]);
    dead_rows += (M + opa::kBf16BM - 1) / opa::kBf16BM * opa::kBf16BM - M;
    std::free(src[0]);
    std::free(src[1]);
}

}  // namespace

int main() {
    const opa::Gemm2Bf16Geometry launches[] = {      // {batch, h, w, k1, k2, stride}
        {3, 23, 19, 64, 64, 1}, {3, 23, 19, 128, 192, 2}, {2, 7, 5, 0, 128, 2}, {1, 1, 1, 64, 64, 2}};
    int n = 0;
    for (const auto& g : launches) {
        check(g);
        n++;
    }
    std::printf("gemm2_bf16_plan: %d launches, %lld fetches, %lld rows behind M left alone, %d failures\n", n, fetches, dead_rows, failures);
    return failures ? 1 : 0;
}
