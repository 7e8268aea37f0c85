// Stand-alone check of csrc/unit_bf16_plan.hpp, the load plan of the bf16 unit-mode GEMM: every access the kernel's threads would make
// is made here, on the CPU, against an operand whose allocation ends with its last byte (so that an over-read is a heap overflow
// for the address sanitizer this program is built with), and counted per byte.  For A, and for the partner / residual:
//   * every byte of the columns below k (n) of every row is fetched exactly once per N-tile pass, no other byte at all,
//   * no access reaches outside [a, a + ((m - 1) * pitch + k) * 2),
//   * no access is wider than its address is aligned, and none wider than the launch's width,
//   * (A) what was staged is the operand where it exists and zero from column k on.
// Prints one line per operand kind and returns 0, or prints the first failures and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "unit_bf16_plan.hpp"

namespace {

int failures = 0;
void fail(const char* what, int m, int k, long long pitch, int residue, long long at) {
    if (failures++ < 20) std::printf("FAIL %s: m %d k %d pitch %lld base %% 16 = %d at %lld\n", what, m, k, pitch, residue, at);
}

// an operand [m, cols] with `pitch` elements between rows at an address = residue (mod 16), ending with its allocation
struct Operand {
    void* block = nullptr;
    unsigned short* a = nullptr;
    long long elems = 0;
    std::vector<unsigned char> count;          // fetches per byte
    Operand(int m, int cols, long long pitch, int residue) {
        elems = (long long)(m - 1) * pitch + cols;
        if (posix_memalign(&block, 16, (size_t)(residue + elems * 2)) != 0) std::abort();
        a = reinterpret_cast<unsigned short*>(static_cast<unsigned char*>(block) + residue);
        for (long long i = 0; i < elems; i++) a[i] = (unsigned short)(1 + (i * 2654435761u >> 7) % 65535);   // (never 0)
        count.assign((size_t)(elems * 2), 0);
    }
    ~Operand() { std::free(block); }
    // one access: `bytes` from element offset `at`; returns false where it must not be made
    bool fetch(long long at, int bytes, void* to) {
        if (at < 0 || at * 2 + bytes > elems * 2) return false;
        if (reinterpret_cast<uintptr_t>(a + at) % (uintptr_t)bytes != 0) return false;
        std::memcpy(to, a + at, (size_t)bytes);
        for (int b = 0; b < bytes; b++) count[(size_t)(at * 2 + b)]++;
        return true;
    }
    // every byte of columns < cols of every row exactly `times`, every other byte never
    long long miscounted(int m, int cols, long long pitch, int times) const {
        for (long long i = 0; i < elems; i++) {
            const int want = i % pitch < cols ? times : 0;
            if (count[(size_t)(2 * i)] != want || count[(size_t)(2 * i + 1)] != want) return i;
        }
        (void)m;
        return -1;
    }
};

template <int W>
void check_a(int m, int k, long long pitch, int residue) {
    Operand op(m, k, pitch, residue);
    const int kp = (k + 63) / 64 * 64;
    for (int m0 = 0; m0 < m; m0 += opa::kUnitBf16BM) {
        for (int k0 = 0; k0 < kp; k0 += opa::kUnitBf16BK) {
            for (int t = 0; t < opa::kUnitBf16Threads; t++) {
                unsigned short chunk[opa::kUnitBf16Passes][8] = {};
                auto emit = [&](int p, int e, long long at, int bytes) {
                    if (bytes != W && bytes != 4) fail("A: a width that is neither the launch's nor 4", m, k, pitch, residue, at);
                    if (bytes > W) fail("A: wider than the launch's width", m, k, pitch, residue, at);
                    if (!op.fetch(at, bytes, &chunk[p][e])) fail("A: outside the operand or misaligned", m, k, pitch, residue, at);
                };
                // (the kernel's two call sites: a whole K-step with k out of the way, the last one with it)
                if (k0 + opa::kUnitBf16BK <= k) opa::unit_bf16_plan_a<W>(m, 0x7fffffff, pitch, m0, t, k0, emit);
                else opa::unit_bf16_plan_a<W>(m, k, pitch, m0, t, k0, emit);
                for (int p = 0; p < opa::kUnitBf16Passes; p++)
                    for (int e = 0; e < 8; e++) {
                        const long long row = (long long)m0 + p * 32 + (t >> 3);
                        const int col = k0 + (t & 7) * 8 + e;
                        const unsigned short want = row < m && col < k ? op.a[row * pitch + col] : 0;
                        if (chunk[p][e] != want) fail("A: the staged tile is not the operand", m, k, pitch, residue, row * pitch + col);
                    }
            }
        }
    }
    const long long bad = op.miscounted(m, k, pitch, 1);
    if (bad >= 0) fail("A: a byte not fetched exactly once (or one behind column k fetched)", m, k, pitch, residue, bad);
}

template <int BN>
void check_third(int m, int n, long long pitch, int residue) {
    constexpr int WN = BN / 2;
    const int np = (n + 63) / 64 * 64;
    if (np % BN != 0) return;
    Operand op(m, n, pitch, residue);
    for (int m0 = 0; m0 < m; m0 += opa::kUnitBf16BM)
        for (int n0 = 0; n0 < np; n0 += BN)
            for (int wave = 0; wave < 4; wave++)
                for (int i = 0; i < 2; i++)
                    for (int lane = 0; lane < 64; lane++) {
                        const long long m0w = (long long)m0 + (wave >> 1) * 64 + i * 32;
                        const int n0w = n0 + (wave & 1) * WN;
                        opa::unit_bf16_plan_third<WN>(m, n, pitch, m0w, n0w, lane, [&](int, long long row, int col, long long at) {
                            unsigned pair;
                            if (at != row * pitch + col || row < m0w || row >= m0w + 32 || col < n0w || col + 1 >= n0w + WN)
                                fail("third: a pair outside its wave's block", m, n, pitch, residue, at);
                            if (!op.fetch(at, 4, &pair)) fail("third: outside the operand or misaligned", m, n, pitch, residue, at);
                        });
                    }
    const long long bad = op.miscounted(m, n, pitch, 1);
    if (bad >= 0) fail("third: a byte not fetched exactly once (or one behind column n fetched)", m, n, pitch, residue, bad);
}

}  // namespace

int main() {
    const int ms[] = {1, 127, 128, 129, 1311}, ks[] = {2, 24, 62, 64, 66, 174}, residues[] = {0, 4, 8, 12};
    int launches = 0, widths[17] = {};
    for (int m : ms)
        for (int k : ks)
            for (long long pitch : {(long long)k, (long long)k + 2, 2ll * k})
                for (int residue : residues) {
                    // the launcher's choice, from the address the operand really has
                    Operand probe(1, 2, 2, residue);
                    const int w = opa::unit_bf16_width(reinterpret_cast<uintptr_t>(probe.a), pitch);
                    if (w == 16) check_a<16>(m, k, pitch, residue);
                    else if (w == 8) check_a<8>(m, k, pitch, residue);
                    else if (w == 4) check_a<4>(m, k, pitch, residue);
                    else fail("unit_bf16_width", m, k, pitch, residue, w);
                    // a narrower width than the choice is always allowed too
                    if (w > 4) check_a<4>(m, k, pitch, residue);
                    if (w > 8) check_a<8>(m, k, pitch, residue);
                    check_third<64>(m, k, pitch, residue);
                    check_third<128>(m, k, pitch, residue);
                    widths[w]++;
                    launches++;
                }
    std::printf("unit_bf16_plan: %d operands (width 16: %d, 8: %d, 4: %d), %d failures\n", launches, widths[16], widths[8], widths[4], failures);
    return failures ? 1 : 0;
}
