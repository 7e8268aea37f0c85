// The store plan of the 16-bit head kernel (csrc/head16.hip): which float32 elements of the fields [B, F, C, H, W] thread t of the
// workgroup at tile origin (m0, n0) stores for each 32-row block of its wave tile, from which place of its wave's patch, or that it
// stores nothing -- as __host__ __device__ functions, so that the kernel and a stand-alone CPU program
// (tests/host/head16_plan_main.cpp) run the SAME decision: the program performs every store of a launch against an output allocation
// that ends with its last byte and checks that every element is stored exactly once, from the right (m, n), and nothing else.
//
// The product is [M = B * hc * wc][N = F * C * us^2] (us 1 or 2): row m = (b * hc + y) * wc + x is a pixel of the trunk's output,
// column n = (f * C + c) * us^2 + dy * us + dx one sub-pixel of plane (f, c).  It goes to
//     fields[b, f, c, y * us + dy - low_cut, x * us + dx - low_cut]        low_cut = (us - 1) / 2, H = hc * us - (us - 1), W likewise
// (the pixel shuffle and the crop of reference network/heads.py:330-343; launch_head_epilogue's values), and nowhere when that row or
// column lies outside [0, H) x [0, W), when m >= M or when n >= N (the weight's zero rows up to the N-tile).
//
// The tile is csrc/bf16_tile.hpp's with BN = 64: 4 waves as 2 (M) x 2 (N), a wave tile 64 x 32, worked off in two 32-row blocks
// through the wave's 32 x 32 float32 patch.  Per block a lane makes kHead16Steps = 16 stores: in step s it reads patch row `row`,
// patch column 2 * s + `sel`, where
//     us = 2:  row = lane >> 1, sel = lane & 1   (= dx: the two sub-columns of one pixel; the step's column pair is one dy of one plane)
//     us = 1:  row = lane & 31, sel = lane >> 5  (the two 32-lane halves take two neighbouring planes)
// so that ONE store instruction covers consecutive x of one plane and output row: 64 consecutive floats for us = 2 (two runs of 32
// for us = 1) while the 32 rows stay inside one image row.  The patch is read column-wise; with a row pitch of 32 + us words the 32
// lanes of a half (what a ds_read_b32 serves in one cycle) fall on 32 different banks:
//     us = 2, pitch 34:  (34 * row + sel) % 32 = 2 * row + sel,  row 0..15 or 16..31, sel 0..1
//     us = 1, pitch 33:  (33 * row) % 32 = row,                  row 0..31
// and the accumulators' writes (one patch row, 32 neighbouring columns per half) do so with any pitch.
//
// What depends on the row alone is computed once per thread and block (head16_plan_rows): the element offset of plane 0 at the pixel's
// first sub-pixel, its output row and column, and whether m < M.  Offsets are 32-bit: the caller refuses B * F * C * H * W >= 2^31.
#pragma once
#include <cstdint>

#include "bf16_tile_shape.hpp"

namespace opa {

constexpr int kHead16BN = 64;            // the N-tile: the weight and the bias are padded to it
constexpr int kHead16WN = kHead16BN / 2; // a wave tile's (and its patch's) columns
constexpr int kHead16Steps = 16;         // stores per lane and 32-row block: 32 x 32 patch elements / 64 lanes

// the geometry of one launch (every size positive, us 1 or 2; the products below 2^31 are the caller's to check)
struct Head16Geometry {
    int batch, hc, wc, n_fields, n_comp, us;
};

OPA_TILE_HD int head16_low_cut(int us) { return (us - 1) / 2; }
OPA_TILE_HD int head16_out(int hc, int us) { return hc * us - (us - 1); }          // H of hc, W of wc
OPA_TILE_HD int head16_n(const Head16Geometry& g) { return g.n_fields * g.n_comp * g.us * g.us; }
OPA_TILE_HD int head16_n_padded(const Head16Geometry& g) { return (head16_n(g) + kHead16BN - 1) / kHead16BN * kHead16BN; }

// thread t's place in its wave's patch: the row it reads in every step and which column of the step's pair
struct Head16Lane {
    int row, sel;
};
OPA_TILE_HD Head16Lane head16_lane(int us, int t) {
    const int lane = t & 63;
    return us == 2 ? Head16Lane{lane >> 1, lane & 1} : Head16Lane{lane & 31, lane >> 5};
}

// one patch row of a thread: the element offset of (b, plane 0, y0, x0) -- y0 = y * us - low_cut, the output row of dy = 0, x0 the
// output column of dx = 0 -- which may lie outside the plane by low_cut (then only dy, dx > 0 are stored); whether m < M
struct Head16Row {
    int base, y0, x0;
    bool live;
};

// Thread t's patch row in both 32-row blocks of its wave tile, for the workgroup whose first row is m0.
OPA_TILE_HD void head16_plan_rows(const Head16Geometry& g, int m0, int t, Head16Row (&rows)[2]) {
    const long long M = (long long)g.batch * g.hc * g.wc;
    const int H = head16_out(g.hc, g.us), W = head16_out(g.wc, g.us), low = head16_low_cut(g.us);
    const int wm = (t >> 6) >> 1, row = head16_lane(g.us, t).row;
    OPA_TILE_UNROLL
    for (int i = 0; i < 2; i++) {
        const long long mm = (long long)m0 + wm * 64 + i * 32 + row;     // (64-bit: m0 + 127 may pass 2^31)
        rows[i] = Head16Row{0, 0, 0, mm < M};
        if (!rows[i].live) continue;
        const int m = (int)mm;
        const int b = m / (g.hc * g.wc), rest = m - b * (g.hc * g.wc);
        const int y = rest / g.wc, x = rest - y * g.wc;
        rows[i].y0 = y * g.us - low;
        rows[i].x0 = x * g.us - low;
        rows[i].base = (int)((((long long)b * g.n_fields * g.n_comp) * H + rows[i].y0) * W + rows[i].x0);
    }
}

// Thread t's stores for one 32-row block (`row`: head16_plan_rows' entry of that block) of the tile whose first column is n0.
// emit(patch_row, patch_col, elem_offset, plane, y, x): store the patch element [patch_row][patch_col] of the thread's wave -- the
// product's row m0 + wm * 64 + i * 32 + patch_row, column n0 + wn * 32 + patch_col -- behind the field function of component
// plane % n_comp at output row y, column x, to float32 element `elem_offset` of the fields.
template <typename Emit>
OPA_TILE_HD void head16_plan_block(const Head16Geometry& g, const Head16Row& row, int n0, int t, Emit&& emit) {
    if (!row.live) return;
    const int H = head16_out(g.hc, g.us), W = head16_out(g.wc, g.us), N = head16_n(g);
    const int wn = (t >> 6) & 1;
    const Head16Lane lane = head16_lane(g.us, t);
    OPA_TILE_UNROLL
    for (int s = 0; s < kHead16Steps; s++) {
        const int col = 2 * s + lane.sel, n = n0 + wn * kHead16WN + col;
        if (n >= N) continue;
        int plane = n, dy = 0, dx = 0;
        if (g.us == 2) { plane = n >> 2; dy = (n >> 1) & 1; dx = n & 1; }
        const int y = row.y0 + dy, x = row.x0 + dx;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;                  // cropped
        emit(lane.row, col, row.base + (plane * H + dy) * W + dx, plane, y, x);
    }
}

}  // namespace opa
