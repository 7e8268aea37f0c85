// The load plan of the bf16 unit-mode GEMM (csrc/gemm_unit_bf16.hip): which bytes of A, and of the partner or residual, thread t of
// the workgroup at row block m0 loads, and how wide -- as __host__ __device__ functions, so that the kernel and a stand-alone CPU
// program (tests/host/unit_bf16_plan_main.cpp) run the SAME decision: the program enumerates every access of a launch and checks
// that each byte of the operand is fetched once, none outside it, and none wider than its address is aligned.
//
// The contract guarantees 4 bytes only: A [m, k] bf16 with `pitch` elements between rows, base and pitch on even element counts
// (k16's stage-2 slice starts 348 bytes into the pixel).  The width of a launch is chosen once, on the host, uniformly for the grid
// (unit_bf16_width): the widest of 16 / 8 / 4 bytes that divides both the base address and the row pitch in bytes.
//
// A: per K-step of 64 columns a thread stages one 16-byte chunk (8 columns) of four rows: chunk column s_col = (t % 8) * 8, rows
// m0 + p * 32 + t / 8, p = 0..3.  The chunk is 16 / W pieces of W bytes.  A piece that ends at or before column k is ONE access of
// W bytes; a piece that reaches across k (only where W > 4: k is even) is loaded in 4-byte accesses, those below k; a piece at or
// behind k, and every piece of a row >= m, is not loaded at all: its registers keep their zeros, so the columns from k on
// contribute exactly zero whatever the memory holds (no multiplication by a zero weight: 0 x NaN), and no byte behind column k of
// the last row is ever addressed.
// Partner / residual: [m, n] with `pitch` elements between rows; the epilogue works in column pairs, one 4-byte access per pair
// below n and row below m (a pair lies inside n or outside: n is even) -- the width every launch is guaranteed.
#pragma once
#include <cstdint>

#include "bf16_tile_shape.hpp"

namespace opa {

// the shared tile's constants under the names that the CPU program of this plan (tests/host/unit_bf16_plan_main.cpp) uses
constexpr int kUnitBf16BM = kBf16BM, kUnitBf16BK = kBf16BK, kUnitBf16Threads = kBf16Threads, kUnitBf16Passes = kBf16Passes;

// the widest access (bytes) that a base address and a row pitch (in bf16 elements) allow for every row: 16, 8 or 4
OPA_TILE_HD int unit_bf16_width(uintptr_t base, long long pitch_elems) {
    const uintptr_t bits = base | (uintptr_t)(pitch_elems * 2);
    return (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : 4;
}

// Thread t's accesses of A for K-step k0 (a multiple of 64) of the workgroup whose first row is m0.
// emit(p, e, elem_offset, bytes): load `bytes` (W or 4) from element offset `elem_offset` (from A's first element, 64-bit) into
// elements e ... e + bytes / 2 - 1 of the chunk of pass p.
template <int W, typename Emit>
OPA_TILE_HD void unit_bf16_plan_a(int m, int k, long long pitch, int m0, int t, int k0, Emit&& emit) {
    static_assert(W == 16 || W == 8 || W == 4, "access widths");
    constexpr int PE = W / 2;                       // elements of a piece
    const int s_row = bf16_tile_stage(t).row, s_col = bf16_tile_stage(t).col;
    OPA_TILE_UNROLL
    for (int p = 0; p < kBf16Passes; p++) {
        const long long row = (long long)m0 + p * 32 + s_row;      // (64-bit: m0 + 127 may pass 2^31)
        if (row >= m) continue;
        const long long at = row * pitch + k0 + s_col;
        OPA_TILE_UNROLL
        for (int e = 0; e < 8; e += PE) {
            const long long col = (long long)k0 + s_col + e;
            if (col + PE <= k) emit(p, e, at + e, W);
            else {
                OPA_TILE_UNROLL
                for (int d = 0; d < PE; d += 2)
                    if (col + d < k) emit(p, e + d, at + e + d, 4);
            }
        }
    }
}

// The epilogue's map of a wave's 32 x WN patch onto its lanes: pair v = i * 64 + lane (i = 0 .. 32 * (WN / 2) / 64 - 1) is row
// v / (WN / 2), columns 2 * (v % (WN / 2)) and the next.  emit(i, row, col, elem_offset): the 4-byte access of the partner or
// residual for that pair -- rows from m and columns from n on have none.
// (m0w, n0w: the first row and column of the wave's 32-row block in the whole product)
template <int WN, typename Emit>
OPA_TILE_HD void unit_bf16_plan_third(int m, int n, long long pitch, long long m0w, int n0w, int lane, Emit&& emit) {
    constexpr int PPR = WN / 2, PPL = 32 * PPR / 64;
    OPA_TILE_UNROLL
    for (int i = 0; i < PPL; i++) {
        const int v = i * 64 + lane;
        const long long row = m0w + v / PPR;
        const int col = n0w + (v % PPR) * 2;
        if (row < m && col < n) emit(i, row, col, row * pitch + col);
    }
}

}  // namespace opa
