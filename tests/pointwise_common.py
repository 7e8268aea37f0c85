"""Shared by the regime tests of the four small producer-side kernels (test_pointwise_cases.py on the CPU,
test_gpu_pointwise_regimes.py on the GPU): ``bias_act_kernel`` (csrc/epilogue.hip), ``dwconv_kernel`` and
``channel_interleave_kernel`` (csrc/dwconv.hip), ``head_epilogue_kernel`` (csrc/head.hip).

Every case is a plain tuple, and a pure function restates the launcher's arithmetic for it: which template instantiation and
which loop regime the launch takes.  The CPU file asserts that the lists reach every regime; the GPU file runs them.  A buffer
from torch's caching allocator starts on a 256-byte boundary, so a slice's alignment is its byte offset into the buffer."""
import torch
from torch.nn import functional as F

DTYPES = {'float32': torch.float32, 'float16': torch.float16, 'bfloat16': torch.bfloat16}
ELEM_BYTES = {'float32': 4, 'float16': 2, 'bfloat16': 2}
SENTINEL = 12352.0                       # 193 * 64: exact in float32, float16 and bfloat16
PAD = 256                                # elements of sentinel in front of and behind a tensor: a multiple of 16 bytes
FLT_MIN = 2.0 ** -126


# ---- bias_act (epilogue.hip: launch_dt, bias_act_kernel) ---------------------------------------------------------------------
BIAS_UNROLL, BIAS_MAX_BLOCKS = 4, 4096


def bias_act_regime(rows, C, dtype):
    """-> (vec_per_row, blocks, col_step, outer_iterations, tail): ``tail`` is the number of vectors the last outer iteration of the
    grid still covers when that is not all ``4 * blocks * 256`` of them (0: the last iteration is full)."""
    per_vec = 16 // ELEM_BYTES[dtype]
    assert C % per_vec == 0
    vec_per_row = C // per_vec
    n_vec = rows * vec_per_row
    blocks = (n_vec + 255) // 256
    blocks = max(1, min((blocks + BIAS_UNROLL - 1) // BIAS_UNROLL, BIAS_MAX_BLOCKS))
    stride = blocks * 256
    per_iteration = BIAS_UNROLL * stride
    return vec_per_row, blocks, stride % vec_per_row, (n_vec + per_iteration - 1) // per_iteration, n_vec % per_iteration


# (rows, C, dtype); each runs with and without a residual, with and without ReLU
BIAS_CASES = [
    # fewer than 256 vectors, one row, one vector per row
    (7, 24, 'float32'), (1, 348, 'float32'), (1, 4, 'float32'), (1000, 4, 'float32'),
    (7, 24, 'bfloat16'), (1, 696, 'bfloat16'), (1, 8, 'bfloat16'), (1000, 8, 'bfloat16'),
    (7, 24, 'float16'), (1, 64, 'float16'), (1, 8, 'float16'), (1000, 8, 'float16'),
    # one pass of an uncapped grid: col_step 0 (C = 64) and not 0 (348 fills 16-byte vectors in float32 only)
    (4551, 64, 'float32'), (4551, 348, 'float32'), (2001, 696, 'float32'), (5003, 24, 'float32'),
    (4551, 64, 'bfloat16'), (4551, 1392, 'bfloat16'), (2001, 696, 'bfloat16'), (5003, 24, 'bfloat16'),
    (4551, 64, 'float16'), (2001, 696, 'float16'), (5003, 24, 'float16'),
]
# (rows, C, dtype, residual, relu): the capped grid, three outer iterations, the last one ragged (the ShuffleNet stem's regime)
BIAS_CAPPED_CASES = [
    (1_750_003, 24, 'float32', True, True), (1_750_003, 24, 'float32', False, False),
    (2_800_003, 24, 'bfloat16', True, False), (2_800_003, 24, 'float16', False, True),
]
BIAS_HUGE_CASE = (33_554_500, 64, 'bfloat16')          # more than 2^31 elements


def bias_act_reference(x, bias, res, relu):
    """The kernel's operations on the CPU: float32 ``(x + b) + r``, ``clamp_min(0)``, one rounding to the dtype."""
    want = x.float() + bias.float()
    if res is not None:
        want = want + res.float()
    if relu:
        want = want.clamp_min(0)
    return want.to(x.dtype)


def bits(t):
    """An integer view of a float tensor: equality of bits, NaN payloads and the sign of zero included."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- depthwise convolution (dwconv.hip: launch_dw_t, launch_dw_v, dwconv_kernel) ---------------------------------------------
DW_STRIP = 4


def _dw(dtype, k, s, B, H, W, C, xs=None, x_off=0, os=None, o_off=0, bias=True):
    """``xs`` / ``os``: elements between neighbouring pixels of the input / output; ``x_off`` / ``o_off``: elements from the
    256-byte aligned start of the pixel grid to the first channel (a channel slice of a wider tensor)."""
    return (dtype, k, s, B, H, W, C, C if xs is None else xs, x_off, C if os is None else os, o_off, bias)


def dw_out_size(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def dwconv_regime(case):
    """-> (V, Wo % 4, blocks along x).  The weight and the bias are allocations of their own (aligned)."""
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias = case

    def ok(v):
        return C % v == 0 and xs % v == 0 and os_ % v == 0 and x_off % v == 0 and o_off % v == 0
    V = 4 if ok(4) else 2 if ok(2) else 1
    Wo = dw_out_size(W, k, s)
    strips = (Wo + DW_STRIP - 1) // DW_STRIP
    return V, Wo % DW_STRIP, (C // V * strips + 255) // 256


DW_KS = [(5, 1), (5, 2), (3, 1), (3, 2)]
DW_CASES = (
    # all 24 instantiations through C % 4 in 0, 2, 1; B in 1, 3; even and odd extents under stride 2
    [_dw(d, k, s, (1, 3)[i % 2], H, W, C) for d in ('float32', 'bfloat16') for i, (k, s) in enumerate(DW_KS)
     for C, (H, W) in ((8, (9, 13)), (6, (6, 7)), (5, (5, 10)))] +
    [
        # strip tails, narrow and flat images (W < K, H = 1)
        _dw('float32', 3, 1, 1, 4, 8, 8), _dw('float32', 5, 1, 3, 3, 1, 8), _dw('float32', 5, 1, 1, 3, 2, 6),
        _dw('float32', 3, 1, 3, 2, 3, 5), _dw('float32', 5, 2, 1, 1, 9, 8), _dw('float32', 3, 2, 3, 1, 1, 5),
        _dw('bfloat16', 5, 1, 1, 3, 1, 8), _dw('bfloat16', 3, 2, 3, 4, 2, 6), _dw('bfloat16', 3, 1, 1, 1, 3, 5),
        _dw('bfloat16', 5, 2, 1, 7, 8, 8), _dw('float32', 5, 2, 1, 8, 8, 6), _dw('bfloat16', 3, 1, 3, 2, 8, 5),
        _dw('bfloat16', 5, 1, 3, 2, 2, 6),
        # more than one block along x
        _dw('float32', 5, 1, 1, 2, 13, 348), _dw('bfloat16', 3, 2, 1, 3, 29, 348),
        # V from the input's pixel stride while C % 4 == 0: odd, even, the second half of a wider tensor
        _dw('float32', 3, 2, 1, 5, 6, 8, xs=11), _dw('float32', 5, 1, 1, 5, 6, 8, xs=10), _dw('float32', 5, 2, 3, 5, 6, 8, xs=16, x_off=8),
        _dw('bfloat16', 3, 2, 1, 5, 6, 8, xs=11), _dw('bfloat16', 5, 1, 1, 5, 6, 8, xs=10), _dw('bfloat16', 3, 1, 3, 5, 6, 8, xs=16, x_off=8),
        _dw('float32', 3, 1, 1, 5, 6, 8, xs=16), _dw('bfloat16', 5, 2, 1, 5, 6, 8, xs=16),          # the first half
        # V from the input pointer: 8 bytes, then 4 bytes off a 16-byte boundary in float32 (4 and 2 bytes off 8 in bfloat16)
        _dw('float32', 3, 1, 1, 5, 6, 8, xs=16, x_off=2), _dw('float32', 3, 2, 1, 5, 6, 8, xs=16, x_off=1),
        _dw('bfloat16', 5, 2, 1, 5, 6, 8, xs=16, x_off=2), _dw('bfloat16', 5, 1, 1, 5, 6, 8, xs=16, x_off=1),
        # V from the output's pixel stride or pointer (the C entry point only); an output pixel stride above C
        _dw('float32', 5, 1, 1, 5, 6, 8, os=10), _dw('float32', 3, 2, 1, 5, 6, 8, os=11), _dw('float32', 5, 2, 1, 5, 6, 8, os=16, o_off=2),
        _dw('float32', 3, 1, 3, 5, 6, 8, os=16, o_off=1), _dw('float32', 3, 2, 3, 5, 7, 8, os=16), _dw('float32', 5, 1, 1, 4, 5, 8, os=24, o_off=8),
        _dw('bfloat16', 5, 1, 1, 5, 6, 8, os=10), _dw('bfloat16', 3, 2, 1, 5, 6, 8, os=11), _dw('bfloat16', 5, 2, 1, 5, 6, 8, os=16, o_off=2),
        _dw('bfloat16', 3, 1, 3, 5, 6, 8, os=16, o_off=1), _dw('bfloat16', 3, 2, 3, 5, 7, 8, os=16),
        # no bias
        _dw('float32', 3, 2, 1, 6, 5, 8, bias=False), _dw('float32', 5, 1, 3, 4, 4, 5, bias=False),
        _dw('bfloat16', 5, 2, 1, 6, 5, 6, bias=False), _dw('bfloat16', 3, 1, 3, 4, 4, 8, xs=16, x_off=8, bias=False),
    ])
# grid.y = B * Ho: the largest grid that can be launched, and one row more (refused on the host)
DW_GRID_OK = _dw('float32', 3, 1, 1, 65535, 1, 1)
DW_GRID_REFUSED = _dw('float32', 3, 1, 1, 65536, 1, 1)


def dw_channel_scales(C):
    """A power of two per channel from 2^-20 to 2^20: every channel is held to its own magnitude."""
    return torch.tensor([2.0 ** ((7 * c) % 41 - 20) for c in range(C)], dtype=torch.float64)


def dw_inputs(case, seed=0):
    """-> (x [B, C, H, W], w_taps [k*k, C], bias [C] or None) on the CPU, rounded to the case's dtype."""
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias = case
    g = torch.Generator().manual_seed(seed)
    scale = dw_channel_scales(C)
    x = (torch.randn((B, C, H, W), generator=g, dtype=torch.float64) * scale.view(1, C, 1, 1)).to(DTYPES[dtype])
    w = (torch.randn((k * k, C), generator=g, dtype=torch.float64) / k).to(DTYPES[dtype])
    b = (torch.randn((C,), generator=g, dtype=torch.float64) * scale).to(DTYPES[dtype]) if has_bias else None
    return x, w, b


def dw_reference(x, w_taps, bias, k, s, relu):
    """Float64 depthwise convolution of the operands as stored, and the derived bound on a float32 accumulation of it in any
    order: ``gamma_n (sum |x| |w| + |b|)`` with ``n = k*k + 1`` and ``u = 2^-24``; for a bfloat16 result one more rounding to
    nearest, half a unit in the last place of the result: ``2^-8 (|ref| + that)``.  -> (ref, bound), float64."""
    C = x.shape[1]
    w4 = w_taps.double().t().reshape(C, 1, k, k)
    b = None if bias is None else bias.double()
    ref = F.conv2d(x.double(), w4, b, stride=s, padding=k // 2, groups=C)
    mag = F.conv2d(x.double().abs(), w4.abs(), None if b is None else b.abs(), stride=s, padding=k // 2, groups=C)
    n, u = k * k + 1, 2.0 ** -24
    bound = n * u / (1 - n * u) * mag
    if relu:
        ref = ref.clamp_min(0)              # 1-Lipschitz: the bound carries over
    if x.dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    return ref, bound


# ---- channel interleave (dwconv.hip: launch_il_t, channel_interleave_kernel) -------------------------------------------------
def interleave_regime(case):
    """-> V.  The output is dense ([rows, 2 * half]) and needs twice the operands' alignment."""
    dtype, rows, half, pa, a_off, pb, b_off, o_off = case

    def ok(v):
        return half % v == 0 and pa % v == 0 and pb % v == 0 and a_off % v == 0 and b_off % v == 0 and o_off % (2 * v) == 0
    return 4 if ok(4) else 2 if ok(2) else 1


def interleave_items(case):
    """Threads with work: the launch has ``ceil(items / 256)`` blocks."""
    return case[1] * (case[2] // interleave_regime(case))


# (dtype, rows, half, pitch of a, offset of a, pitch of b, offset of b, offset of out), in elements
INTERLEAVE_CASES = (
    [c for d in ('float32', 'float16', 'bfloat16') for c in (
        (d, 13, 176, 176, 0, 176, 0, 0),         # V = 4, 572 items
        (d, 221, 174, 174, 0, 174, 0, 0),        # V = 2 through half % 4
        (d, 3, 87, 87, 0, 87, 0, 0),             # V = 1 through half % 2, 261 items: just above 256
        (d, 51, 5, 5, 0, 5, 0, 0),               # 255 items: just below
        (d, 300, 1, 1, 0, 1, 0, 0),              # half = 1
        (d, 64, 8, 16, 0, 8, 0, 0),              # a is the first half of a wider tensor, b dense: pa != pb, both multiples of 4
        (d, 37, 8, 12, 0, 16, 8, 0),             # b the second half
        (d, 37, 8, 10, 0, 8, 0, 0),              # pa even
        (d, 37, 8, 8, 0, 9, 0, 0),               # pb odd
        (d, 37, 8, 11, 0, 10, 0, 0),             # pa odd, pb even
        (d, 37, 8, 16, 2, 8, 0, 0),              # pointer of a: V = 2
        (d, 37, 8, 8, 0, 16, 1, 0),              # pointer of b: V = 1
        (d, 37, 8, 8, 0, 8, 0, 4),               # pointer of out: V = 2
        (d, 37, 8, 8, 0, 8, 0, 2),               # pointer of out: V = 1
    )])


# ---- head epilogue (head.hip: launch_head_epilogue, head_epilogue_kernel) ----------------------------------------------------
HEAD_PLANES = 16
HEAD_LDS_LIMIT = 64 * 1024
HEAD_WC_LIMIT = {1: 1023, 2: 255}


def head_meta(name, upsample_stride):
    from openpifpaf_amd import constants, headmeta
    if name in ('cif', 'caf', 'caf25'):
        meta = dict(zip(('cif', 'caf', 'caf25'), headmeta.cocokp_dense_metas(upsample_stride)))[name]
    elif name in ('wb_cif', 'wb_caf'):
        meta = dict(zip(('wb_cif', 'wb_caf'), headmeta.wholebody_metas(upsample_stride)))[name]
    elif name == 'cifdet':
        meta = headmeta.CifDet('cifdet', 'cocodet', categories=['category%d' % i for i in range(80)])
    elif name == 'tcaf':
        meta = headmeta.Tcaf('tcaf', 'posetrack2018', keypoints_single_frame=constants.COCO_KEYPOINTS,
                             sigmas_single_frame=constants.COCO_PERSON_SIGMAS, pose_single_frame=constants.COCO_UPRIGHT_POSE,
                             draw_skeleton_single_frame=constants.COCO_PERSON_SKELETON)
    else:
        raise KeyError(name)
    meta.upsample_stride = upsample_stride
    return meta


def head_components(meta):
    return 1 + meta.n_confidences + 2 * meta.n_vectors + meta.n_scales


def head_regime(case):
    """-> (LDS bytes, plane blocks, planes in the last block when it is not full else 0)."""
    name, us, dtype, B, Hc, Wc = case
    meta = head_meta(name, us)
    n_planes = meta.n_fields * head_components(meta)
    return 4 * HEAD_PLANES * us * us * (Wc + 1), (n_planes + HEAD_PLANES - 1) // HEAD_PLANES, n_planes % HEAD_PLANES


# (meta, upsample stride, dtype, B, Hc, Wc)
HEAD_CASES = (
    [(m, us, 'float32', 2, 9, 13) for m in ('cif', 'caf', 'caf25', 'cifdet', 'tcaf', 'wb_cif', 'wb_caf') for us in (1, 2)] +
    [(m, us, d, 2, 9, 13) for m in ('cif', 'cifdet') for us in (1, 2) for d in ('float16', 'bfloat16')] +
    [('caf', 2, 'bfloat16', 1, 9, 13), ('wb_cif', 2, 'float16', 1, 9, 13)] +
    [(m, us, 'float32', B, hc, wc) for m, B in (('cif', 3), ('caf', 1)) for us in (1, 2) for hc, wc in ((1, 1), (41, 41))] +
    # Wc at the limit of the 64 KiB LDS row buffer
    [('cif', 2, 'float32', 1, 2, 255), ('cif', 1, 'float32', 1, 2, 1023), ('cifdet', 2, 'bfloat16', 1, 1, 255),
     ('caf', 1, 'float16', 1, 1, 1023), ('wb_cif', 2, 'float32', 1, 1, 255)])
HEAD_OVER_LIMIT = [('cif', 2, 256), ('cif', 1, 1024)]          # (meta, upsample stride, Wc): the kernel cannot run

_F32 = torch.float32
HEAD_VALUE_GRID = torch.cat([
    torch.tensor([0.0, -0.0, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 110.0, -110.0, 88.0, -88.0, 1.0, -1.0], dtype=_F32),
    torch.nextafter(torch.tensor([20.0, 20.0, -20.0, -20.0], dtype=_F32), torch.tensor([float('inf'), float('-inf')] * 2, dtype=_F32)),
    torch.linspace(-110.0, 110.0, 89, dtype=_F32)])


def head_input(case, seed=0, special=False):
    """A convolution output [B, F * C * us^2, Hc, Wc], channels_last, on the CPU: half of the values from ``HEAD_VALUE_GRID``, half
    uniform in [-110, 110]; with ``special`` NaN and +-inf in one value of sixteen."""
    name, us, dtype, B, Hc, Wc = case
    meta = head_meta(name, us)
    ctot = meta.n_fields * head_components(meta) * us * us
    g = torch.Generator().manual_seed(seed)
    shape = (B, Hc, Wc, ctot)
    grid = HEAD_VALUE_GRID
    if special:
        grid = torch.cat([grid, torch.tensor([float('nan'), float('inf'), float('-inf')] * 5, dtype=_F32)])
    pick = grid[torch.randint(len(grid), shape, generator=g)]
    uniform = torch.rand(shape, generator=g) * 220.0 - 110.0
    x = torch.where(torch.rand(shape, generator=g) < 0.5, pick, uniform).to(DTYPES[dtype])
    return x.permute(0, 3, 1, 2)                                 # NHWC in memory = channels_last


def head_layout(x, meta):
    """The layout-only part of ``CompositeField4``: PixelShuffle, crop, [B, F, C, H, W] float32 (exact)."""
    us = meta.upsample_stride
    x = x.float()
    if us > 1:
        x = F.pixel_shuffle(x, us)
        low_cut = (us - 1) // 2
        high_cut = us - 1 - low_cut
        x = x[:, :, low_cut:x.shape[2] - high_cut, low_cut:x.shape[3] - high_cut]
    B, _, H, W = x.shape
    return x.reshape(B, meta.n_fields, head_components(meta), H, W).contiguous()


def head_reference(lay, meta):
    """The post-processing of ``CompositeField4`` on ``head_layout``'s result.  -> (exact, ref64, kind): ``exact`` float32 holds
    what must come out bit for bit (raw component, vectors with and without their index offset, scales above the softplus
    threshold), ``ref64`` the float64 sigmoid / softplus elsewhere; ``kind`` [C]: 0 exact, 1 sigmoid, 2 softplus."""
    nc, nv, ns = meta.n_confidences, meta.n_vectors, meta.n_scales
    H, W = lay.shape[-2:]
    exact, ref64 = lay.clone(), lay.double()
    kind = torch.zeros(lay.shape[2], dtype=torch.long)
    kind[1:1 + nc] = 1
    ref64[:, :, 1:1 + nc] = torch.sigmoid(ref64[:, :, 1:1 + nc])
    for i, on in enumerate(meta.vector_offsets):
        if on:
            exact[:, :, 1 + nc + 2 * i] += torch.arange(W, dtype=torch.float32)
            exact[:, :, 1 + nc + 2 * i + 1] += torch.arange(H, dtype=torch.float32).unsqueeze(1)
    first = 1 + nc + 2 * nv
    kind[first:first + ns] = 2
    ref64[:, :, first:first + ns] = F.softplus(ref64[:, :, first:first + ns])     # beta 1, threshold 20: the identity above it
    return exact, ref64, kind


def ulp32(ref64):
    """The spacing of float32 at ``|ref64|`` (2^-149 below the normal range)."""
    _, e = torch.frexp(ref64.abs())                              # |ref| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref64), (e - 24).clamp_min(-149))
