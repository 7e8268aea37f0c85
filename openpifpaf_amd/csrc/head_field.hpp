// What a field value is: the ONE definition of what CompositeField4 applies to a head's pre-activation value behind the pixel shuffle and the
// crop (reference network/heads.py:360-378), shared by the two kernels that write the decoder's float32 fields -- csrc/head.hip (from
// a convolution's output) and csrc/head16.hip (from the 16-bit MFMA's float32 accumulators).  Equal float32 values in, equal bits out.
#pragma once
#include <hip/hip_runtime.h>

namespace opa {

// `v`: the pre-activation value of component `c` of its field (0: the pass-through, then n_conf confidences, n_vec (x, y) pairs,
// n_scales scales; what lies behind them passes through) at column `x`, row `y` of the cropped output plane.
__device__ __forceinline__ float head_field(float v, int c, int x, int y, int n_conf, int n_vec, unsigned offset_mask, int n_scales) {
    if (c >= 1 && c < 1 + n_conf) {
        v = 1.0f / (1.0f + expf(-v));                // sigmoid (heads.py:364)
    } else if (c >= 1 + n_conf && c < 1 + n_conf + 2 * n_vec) {
        const int vi = (c - 1 - n_conf) >> 1, is_y = (c - 1 - n_conf) & 1;
        if ((offset_mask >> vi) & 1u) v += is_y ? (float)y : (float)x;              // heads.py:366-370
    } else if (c >= 1 + n_conf + 2 * n_vec && c < 1 + n_conf + 2 * n_vec + n_scales) {
        v = v > 20.0f ? v : log1pf(expf(v));         // softplus, beta 1, threshold 20 (heads.py:374)
    }
    return v;
}

}  // namespace opa
