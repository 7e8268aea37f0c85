"""CPU side of the regime tests of the small producer-side kernels: the case lists of ``pointwise_common`` reach every launch
regime the GPU file (test_gpu_pointwise_regimes.py) is meant to run -- an edit that drops one fails here, without a GPU -- and the
float64 reference and error bound of the depthwise convolution hold for torch's own CPU convolution."""
import ctypes

import pytest

torch = pytest.importorskip('torch')

import pointwise_common as pc  # noqa: E402


def test_bias_act_regime_restates_the_launcher():
    # the ShuffleNet stem of the benchmark, 32 x 24 x 321 x 321 float32
    assert pc.bias_act_regime(32 * 321 * 321, 24, 'float32')[:4] == (6, 4096, 4, 5)
    vec_per_row, blocks, col_step, outer, tail = pc.bias_act_regime(1_750_003, 24, 'float32')
    assert (vec_per_row, blocks, col_step, outer) == (6, 4096, 4, 3) and 0 < tail < 4 * 4096 * 256
    # the one shape of test_gpu_epilogue.py: 72 blocks, one iteration, no column step
    assert pc.bias_act_regime(3 * 37 * 41, 64, 'float32')[1:4] == (72, 0, 1)


def test_bias_act_cases_cover_every_regime():
    for dtype in ('float32', 'float16', 'bfloat16'):
        regimes = [pc.bias_act_regime(r, c, d) + (r, c) for r, c, d in pc.BIAS_CASES if d == dtype]
        assert any(col_step == 0 and vpr > 1 and outer == 1 and blocks > 1 for vpr, blocks, col_step, outer, tail, r, c in regimes)
        assert any(col_step != 0 and blocks > 1 for vpr, blocks, col_step, outer, tail, r, c in regimes)
        assert any(vpr == 1 and r > 1 for vpr, blocks, col_step, outer, tail, r, c in regimes)
        assert any(r * vpr < 256 and r > 1 for vpr, blocks, col_step, outer, tail, r, c in regimes)              # fewer than 256 vectors
        assert any(r == 1 and vpr > 1 for vpr, blocks, col_step, outer, tail, r, c in regimes)
        assert any(r == 1 and vpr == 1 for vpr, blocks, col_step, outer, tail, r, c in regimes)
        assert any(1 < blocks < pc.BIAS_MAX_BLOCKS and outer == 1 and r * vpr > blocks * 256 for vpr, blocks, col_step, outer, tail, r, c in regimes)
        capped = [pc.bias_act_regime(r, c, d) for r, c, d, res, relu in pc.BIAS_CAPPED_CASES if d == dtype]
        assert any(blocks == pc.BIAS_MAX_BLOCKS and col_step != 0 and outer >= 3 and tail != 0 for vpr, blocks, col_step, outer, tail in capped)
    channels = {c for r, c, d in pc.BIAS_CASES}
    assert {24, 348, 696, 64, 4, 8} <= channels
    assert {(res, relu) for r, c, d, res, relu in pc.BIAS_CAPPED_CASES} == {(True, True), (False, False), (True, False), (False, True)}
    rows, C, dtype = pc.BIAS_HUGE_CASE
    assert rows * C > 2 ** 31 and dtype == 'bfloat16'


def test_dwconv_cases_cover_every_regime():
    cases = pc.DW_CASES
    inst = {(c[0], c[1], c[2], pc.dwconv_regime(c)[0]) for c in cases}
    assert inst == {(d, k, s, v) for d in ('float32', 'bfloat16') for k, s in pc.DW_KS for v in (4, 2, 1)}          # all 24
    for dtype in ('float32', 'bfloat16'):
        mine = [c for c in cases if c[0] == dtype]

        def has(pred):
            return any(pred(*c) for c in mine)
        dense = lambda xs, xo, os_, oo, C: xs == C and xo == 0 and os_ == C and oo == 0      # noqa: E731
        # every cause of V on its own
        for c_mod, v in ((0, 4), (2, 2), (1, 1)):
            assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == c_mod and dense(xs, xo, os_, oo, C))
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs % 2 == 1 and xo == 0 and os_ == C and oo == 0)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs % 4 == 2 and xo == 0 and os_ == C and oo == 0)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs % 4 == 0 and xs > C and xo % 4 == 0 and xo > 0)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs % 4 == 0 and xs >= 2 * C and xo == 0)      # either half of a wider tensor
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs % 4 == 0 and xo % 4 == 2 and os_ == C and oo == 0)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs % 4 == 0 and xo % 2 == 1 and os_ == C and oo == 0)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs == C and os_ % 4 == 2 and oo == 0)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs == C and os_ % 2 == 1 and oo == 0)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs == C and os_ % 4 == 0 and oo % 4 == 2)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: C % 4 == 0 and xs == C and os_ % 4 == 0 and oo % 2 == 1)
        assert has(lambda d, k, s, B, H, W, C, xs, xo, os_, oo, b: os_ > C and os_ % 4 == 0 and oo == 0)          # gaps between pixels, V = 4
        # geometry
        assert {pc.dwconv_regime(c)[1] for c in mine} == {0, 1, 2, 3}
        assert {1, 2, 3} <= {pc.dw_out_size(c[5], c[1], c[2]) for c in mine}
        assert {1, 2} <= {c[5] for c in mine} and 1 in {c[4] for c in mine}
        assert {(c[4] % 2, c[5] % 2) for c in mine if c[2] == 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert any(pc.dwconv_regime(c)[2] > 1 for c in mine)
        assert {1, 3} <= {c[3] for c in mine}
        assert {True, False} == {c[11] for c in mine}
    for c in cases + [pc.DW_GRID_OK]:
        assert c[3] * pc.dw_out_size(c[4], c[1], c[2]) <= 65535 and c[7] >= c[6] and c[9] >= c[6]
    ok, refused = pc.DW_GRID_OK, pc.DW_GRID_REFUSED
    assert ok[3] * pc.dw_out_size(ok[4], ok[1], ok[2]) == 65535 and refused[3] * pc.dw_out_size(refused[4], refused[1], refused[2]) == 65536


def test_interleave_cases_cover_every_regime():
    cases = pc.INTERLEAVE_CASES
    assert {(c[0], pc.interleave_regime(c)) for c in cases} == {(d, v) for d in ('float32', 'float16', 'bfloat16') for v in (4, 2, 1)}
    for dtype in ('float32', 'float16', 'bfloat16'):
        mine = [c for c in cases if c[0] == dtype]

        def has(pred):
            return any(pred(*c) for c in mine)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: half % 4 == 2 and pa == half == pb and ao == bo == oo == 0)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: half % 2 == 1 and half > 1 and pa == half == pb and ao == bo == oo == 0)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: half == 1)
        aligned = lambda half, ao, bo, oo: half % 4 == 0 and ao % 4 == 0 and bo % 4 == 0 and oo % 8 == 0      # noqa: E731
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: aligned(half, ao, bo, oo) and pa != pb and pa % 4 == 0 and pb % 4 == 0)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: aligned(half, ao, bo, oo) and pa % 4 == 2 and pb % 4 == 0)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: aligned(half, ao, bo, oo) and pa % 4 == 0 and pb % 2 == 1)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: aligned(half, ao, bo, oo) and pa % 2 == 1 and pb % 4 == 2)
        dense = lambda half, pa, pb: half % 4 == 0 and pa % 4 == 0 and pb % 4 == 0                              # noqa: E731
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: dense(half, pa, pb) and ao % 4 == 2 and bo == 0 and oo == 0)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: dense(half, pa, pb) and ao == 0 and bo % 2 == 1 and oo == 0)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: dense(half, pa, pb) and ao == 0 and bo == 0 and oo % 8 == 4)
        assert has(lambda d, rows, half, pa, ao, pb, bo, oo: dense(half, pa, pb) and ao == 0 and bo == 0 and oo % 4 == 2)
        items = [pc.interleave_items(c) % 256 for c in mine]
        assert any(0 < i <= 16 for i in items) and any(i >= 240 for i in items)          # just above and just below a multiple of 256
        assert any(pc.interleave_items(c) > 256 for c in mine) and any(pc.interleave_items(c) < 256 for c in mine)
        assert all(c[3] >= c[2] and c[5] >= c[2] for c in mine)


def test_head_cases_cover_every_regime():
    cases = pc.HEAD_CASES
    assert {c[0] for c in cases} == {'cif', 'caf', 'caf25', 'cifdet', 'tcaf', 'wb_cif', 'wb_caf'}
    assert {(c[0], c[1]) for c in cases if c[2] == 'float32'} >= {(m, us) for m in ('cif', 'caf', 'caf25', 'cifdet', 'tcaf', 'wb_cif', 'wb_caf')
                                                                   for us in (1, 2)}
    assert {(c[1], c[2]) for c in cases} == {(us, d) for us in (1, 2) for d in ('float32', 'float16', 'bfloat16')}
    for us in (1, 2):
        assert {(1, 1), (9, 13), (41, 41)} <= {(c[4], c[5]) for c in cases if c[1] == us}
        at_limit = [c for c in cases if c[1] == us and c[5] == pc.HEAD_WC_LIMIT[us]]
        assert at_limit and all(pc.head_regime(c)[0] == pc.HEAD_LDS_LIMIT for c in at_limit)
    assert all(pc.head_regime(c)[0] <= pc.HEAD_LDS_LIMIT for c in cases)
    for name, us, wc in pc.HEAD_OVER_LIMIT:
        assert wc == pc.HEAD_WC_LIMIT[us] + 1 and pc.head_regime((name, us, 'float32', 1, 1, wc))[0] > pc.HEAD_LDS_LIMIT
    assert {us for name, us, wc in pc.HEAD_OVER_LIMIT} == {1, 2}
    assert pc.head_regime(('wb_cif', 2, 'float32', 1, 1, 1))[1:] == (42, 9)                # 133 fields, 665 planes
    tails = {pc.head_regime(c)[2] for c in cases}
    assert 0 in tails and len(tails) > 2
    # CifDet: an offset on the first vector only, no scale; the grid holds the values the issue names
    det = pc.head_meta('cifdet', 2)
    assert list(det.vector_offsets) == [True, False] and det.n_scales == 0
    grid = pc.HEAD_VALUE_GRID
    for v in (0.0, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0):
        assert (grid == v).any()
    assert ((grid > 20.0) & (grid < 20.00001)).any() and ((grid < 20.0) & (grid > 19.99999)).any()
    assert (pc.bits(grid) == -2 ** 31).any()                                               # -0.0
    assert float(grid.min()) == -110.0 and float(grid.max()) == 110.0


def test_head_reference_helpers():
    assert float(pc.ulp32(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -23
    assert float(pc.ulp32(torch.tensor([0.75], dtype=torch.float64))) == 2.0 ** -24
    assert float(pc.ulp32(torch.tensor([1e-45], dtype=torch.float64))) == 2.0 ** -149
    case = ('cifdet', 2, 'float32', 1, 3, 4)
    meta = pc.head_meta('cifdet', 2)
    x = pc.head_input(case)
    assert x.is_contiguous(memory_format=torch.channels_last) and x.shape == (1, 80 * 6 * 4, 3, 4)
    lay = pc.head_layout(x, meta)
    assert lay.shape == (1, 80, 6, 5, 7)
    assert lay[0, 3, 2, 1, 2] == x[0, (3 * 6 + 2) * 4 + 1 * 2 + 0, 0, 1]                   # nothing is cut in front: row 1 = 2 * 0 + 1, column 2 = 2 * 1 + 0
    exact, ref64, kind = pc.head_reference(lay, meta)
    assert kind.tolist() == [0, 1, 0, 0, 0, 0]
    assert torch.equal(exact[:, :, 2], lay[:, :, 2] + torch.arange(7.0)) and torch.equal(exact[:, :, 4:], lay[:, :, 4:])


@pytest.mark.parametrize('case', pc.DW_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_depthwise_bound_holds_for_torch_on_the_cpu(case):
    """The float64 reference and the derived bound against torch's own CPU depthwise convolution in the case's dtype (float32
    accumulation, one rounding for bfloat16): error / bound <= 1 at every element, each channel on its own scale."""
    dtype, k, s, B, H, W, C = case[:7]
    x, w, b = pc.dw_inputs(case)
    ref, bound = pc.dw_reference(x, w, b, k, s, relu=False)
    w4 = w.t().reshape(C, 1, k, k).contiguous()
    theirs = torch.nn.functional.conv2d(x, w4, b, stride=s, padding=k // 2, groups=C)
    assert theirs.dtype == x.dtype and theirs.shape == ref.shape
    ratio = ((theirs.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    assert ratio <= 1.0, ratio
    # the bound is relative to each channel's own magnitude: it does not let a small channel hide behind a large one
    per_channel = (bound / ref.abs().clamp_min(1e-300)).permute(1, 0, 2, 3).reshape(C, -1).median(dim=1).values
    assert float(per_channel.max()) < (2.0 ** -6 if dtype == 'bfloat16' else 2.0 ** -16)


def test_bias_act_reference_known_answers():
    """One rounding to nearest even of the float32 sum."""
    bf = torch.bfloat16
    x = torch.tensor([1.0, 1.0078125], dtype=bf)
    b = torch.tensor([2.0 ** -8, 2.0 ** -8], dtype=bf)
    assert pc.bias_act_reference(x, b, None, False).tolist() == [1.0, 1.015625]
    h = torch.float16
    assert pc.bias_act_reference(torch.tensor([1.0, 1.0 + 2.0 ** -10, 65504.0], dtype=h), torch.tensor([2.0 ** -11, 2.0 ** -11, 16.0], dtype=h),
                                 None, True).tolist() == [1.0, 1.0 + 2.0 ** -9, float('inf')]


def test_c_entry_refuses_a_grid_it_cannot_launch_on_the_host():
    """``B * Ho = 65536`` exceeds grid.y: OPA_ERR_INVALID_ARGUMENT before anything is launched (the pointers are never read: no
    device is needed, and none is touched)."""
    from openpifpaf_amd import _lib
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias = pc.DW_GRID_REFUSED
    fake = ctypes.c_void_p(4096)
    rc = _lib.lib().opa_dwconv_bias_act(fake, xs, fake, None, fake, os_, B, H, W, C, k, s, 0, 0, None)
    assert rc == 1 and _lib.ERROR_NAMES[rc] == 'INVALID_ARGUMENT'
    assert b'65535' in _lib.lib().opa_last_error()
