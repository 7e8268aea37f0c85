// Stand-alone check of csrc/head16_plan.hpp, the store plan of the 16-bit head kernel: every store the kernel's threads would make is
// made here, on the CPU, against an output whose allocation ends with its last byte (so that a store behind it is a heap overflow for
// the address sanitizer this program is built with), and counted per element.  What is stored is the (m, n) of the product that the
// plan names as the store's source.  For every (B, hc, wc, F, C, us) of the list in main:
//   * no offset lies outside [0, B * F * C * H * W),
//   * every output element is stored exactly once,
//   * from the (m, n) that the definition gives for it, and with the plane and the output row and column the field function is told,
//   * nothing is stored for m >= M, n >= N or a cropped position (such a store could only be a second one or a wrong source: counted too).
// Prints one line and returns 0, or prints the first failures and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "head16_plan.hpp"

namespace {

int failures = 0;
long long stores = 0, dead_rows = 0, dead_cols = 0, cropped = 0;

void fail(const char* what, const opa::Head16Geometry& g, long long m, long long n, long long at) {
    if (failures++ < 20)
        std::printf("FAIL %s: B %d hc %d wc %d F %d C %d us %d m %lld n %lld at %lld\n", what, g.batch, g.hc, g.wc, g.n_fields, g.n_comp, g.us, m,
                    n, at);
}

void check(const opa::Head16Geometry& g) {
    const int us = g.us, H = opa::head16_out(g.hc, us), W = opa::head16_out(g.wc, us), low = opa::head16_low_cut(us);
    const int planes = g.n_fields * g.n_comp, N = opa::head16_n(g), Np = opa::head16_n_padded(g);
    const long long M = (long long)g.batch * g.hc * g.wc, elems = (long long)g.batch * planes * H * W;
    if (N != planes * us * us || Np % opa::kHead16BN != 0 || Np < N || Np - N >= opa::kHead16BN) fail("N or its padding", g, 0, N, Np);
    // the fields: what each element was stored from, m * Np + n + 1 (0: not stored); ends with the tensor's last byte
    std::int64_t* out = static_cast<std::int64_t*>(std::malloc((size_t)elems * sizeof(std::int64_t)));
    if (!out) std::abort();
    for (long long e = 0; e < elems; e++) out[e] = 0;
    std::vector<unsigned char> count((size_t)elems, 0);
    for (long long m0 = 0; m0 < M; m0 += opa::kBf16BM)
        for (int n0 = 0; n0 < Np; n0 += opa::kHead16BN)
            for (int t = 0; t < opa::kBf16Threads; t++) {
                opa::Head16Row rows[2];
                opa::head16_plan_rows(g, (int)m0, t, rows);                             // once per thread, as the kernel does
                const int wm = (t >> 6) >> 1, wn = (t >> 6) & 1;
                for (int i = 0; i < 2; i++) {
                    int emitted = 0;
                    opa::head16_plan_block(g, rows[i], n0, t, [&](int prow, int pcol, int at, int plane, int y, int x) {
                        const long long m = m0 + wm * 64 + i * 32 + prow, n = (long long)n0 + wn * opa::kHead16WN + pcol;
                        stores++;
                        emitted++;
                        if (prow < 0 || prow >= 32 || pcol < 0 || pcol >= opa::kHead16WN) { fail("outside the patch", g, m, n, at); return; }
                        if (at < 0 || at >= elems) { fail("outside the fields", g, m, n, at); return; }
                        if (m >= M) { fail("a row >= M stored", g, m, n, at); return; }
                        if (n >= N) { fail("a column >= N stored", g, m, n, at); return; }
                        if (plane != n / (us * us) || y < 0 || y >= H || x < 0 || x >= W) fail("wrong plane, row or column", g, m, n, at);
                        if ((((long long)(m / (g.hc * g.wc)) * planes + plane) * H + y) * W + x != at) fail("offset is not (b, plane, y, x)", g, m, n, at);
                        out[at] = m * Np + n + 1;                                      // (the store: the sanitizer watches it)
                        if (count[(size_t)at] < 255) count[(size_t)at]++;
                    });
                    if (emitted > opa::kHead16Steps) fail("more stores than steps", g, m0, n0, emitted);
                }
            }
    // the definition, element by element: (b, f, c, Y, X) comes from pixel (Y + low) / us, (X + low) / us and sub-pixel ((Y + low) % us, (X + low) % us)
    for (int b = 0; b < g.batch; b++)
        for (int p = 0; p < planes; p++)
            for (int Y = 0; Y < H; Y++)
                for (int X = 0; X < W; X++) {
                    const long long at = (((long long)b * planes + p) * H + Y) * W + X;
                    const int ys = Y + low, xs = X + low;
                    const long long m = ((long long)b * g.hc + ys / us) * g.wc + xs / us, n = (long long)p * us * us + (ys % us) * us + xs % us;
                    if (count[(size_t)at] != 1) fail("an element not stored exactly once", g, m, n, count[(size_t)at]);
                    else if (out[at] != m * Np + n + 1) fail("an element stored from the wrong (m, n)", g, m, n, out[at] - 1);
                }
    dead_rows += (M + opa::kBf16BM - 1) / opa::kBf16BM * opa::kBf16BM - M;
    dead_cols += Np - N;
    cropped += M * N - elems;
    std::free(out);
}

}  // namespace

int main() {
    const opa::Head16Geometry launches[] = {      // {batch, hc, wc, n_fields, n_comp, us}
        {2, 5, 7, 2, 5, 2}, {3, 9, 11, 3, 8, 2}, {1, 33, 4, 13, 6, 1}, {1, 1, 1, 1, 5, 2}, {1, 8, 16, 17, 5, 2}};
    int n = 0;
    for (const auto& g : launches) {
        check(g);
        n++;
    }
    std::printf("head16_plan: %d launches, %lld stores, %lld rows behind M, %lld columns behind N and %lld cropped positions left alone, %d failures\n",
                n, stores, dead_rows, dead_cols, cropped, failures);
    return failures ? 1 : 0;
}
