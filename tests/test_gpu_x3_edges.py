"""The split-operand kernels (csrc/gemm_f32x3.hip: plain, pair, implicit 3x3, stem rows, unit / head; csrc/winograd.hip variant 4 on its 64-channel kernel
and variant 5, the 128-channel one, each named by the test and not picked by the launcher's rule) on the data the other suites never use, with six and with nine terms:
  (a) known answers, bit for bit -- selection weights, one-hot activations, integers inside the bit budget;
  (b) power-of-two scaling of the operands scales the result exactly;
  (c) a wide dynamic range against float64 in the COMPONENTWISE measure ``|got - ref| / (sum_k |a||w| + |bias| + |res|)``;
  (d) operands whose low pieces are subnormal bfloat16 numbers, and subnormal float32 operands;
  (e) NaN and +-Inf in every operand: what they turn into, and that nothing leaks to their neighbours in the tile.
tests/test_x3_cases.py proves on the CPU that these expectations follow from the arithmetic (``x3_common.model``), checks the bit
budgets and the scaling ranges that (a) and (b) rely on, and shows mutants of the arithmetic failing the measures used here."""
import contextlib

import pytest

torch = pytest.importorskip('torch')

import x3_common as xc  # noqa: E402

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TERMS = [6, 9]
NAN, INF = float('nan'), float('inf')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cl(t):
    return t.cuda().contiguous(memory_format=CL)


@contextlib.contextmanager
def _terms(terms):
    from openpifpaf_amd import fused
    old, fused.X3_TERMS = fused.X3_TERMS, terms
    try:
        yield
    finally:
        fused.X3_TERMS = old


def _module(w4d, stride=1, padding=0, bias=None):
    n, c, k, _ = w4d.shape
    conv = torch.nn.Conv2d(c, n, k, stride, padding, bias=bias is not None).cuda().requires_grad_(False)
    conv.weight.copy_(w4d)
    if bias is not None:
        conv.bias.copy_(bias)
    return conv


def _slice_of(t, half, fill=NAN):
    """``t`` [B, C, H, W] as the first (0) / second (1) half of the channels of a channels-last tensor whose other half is ``fill``
    (first half: ``fill`` lies right behind the operand's last column)."""
    b, c, h, w = t.shape
    big = torch.full((b, 2 * c, h, w), fill, device='cuda').contiguous(memory_format=CL)
    view = big[:, half * c:(half + 1) * c]
    view.copy_(t)
    return view


def _run(spec, nat, w, bias, res=None, a_bias=None, relu=False, terms=6, layout='dense', partner=None, head=False):
    """One launch of the case's entry point -> the result as rows ``[M, N]`` on the CPU (with a partner: ``[M, 2N]``)."""
    from openpifpaf_amd import fused
    mode = spec[0]
    K, N = xc.dims(spec)
    B, ho, wo = xc.out_shape(spec)
    bias_d = bias.cuda()
    ab = None if a_bias is None else a_bias.cuda()
    with torch.no_grad(), _terms(terms):
        if mode == 'plain':
            r = None if res is None else _cl(xc.image_of(res, B, ho, wo))
            out = fused.conv1x1_bias_act_x3(_cl(nat[0]), fused.split_weight(w.cuda()), bias_d, r, relu, ab, terms)
        elif mode == 'pair':
            k1 = spec[1]
            conv, dconv = _module(w[:, :k1].reshape(N, k1, 1, 1)), _module(w[:, k1:].reshape(N, K - k1, 1, 1), spec[4])
            h, x = _cl(nat[0]), _cl(nat[1])
            assert fused.pair_supported(conv, dconv, h, x, bias_d, ab)
            out = fused.conv1x1_pair_bias_act_x3(conv, dconv, h, x, bias_d, relu, ab)
        elif mode == 'conv3':
            conv, x = _module(xc.weight_4d(w, 64, 3), spec[1], 1), _cl(nat[0])
            assert fused.conv3x3_x3_supported(conv, x, bias_d)
            out = fused.conv3x3_bias_act_x3(conv, x, bias_d, relu)
        elif mode == 'stem':
            conv = _module(xc.weight_4d(w, 3, 7), 2, 3)
            x = _cl(nat[0]) if layout == 'channels_last' else nat[0].cuda()
            assert fused.stem_x3_supported(conv, x, bias_d)
            out = fused.stem7x7_bias_act_x3(conv, x, bias_d, relu)
        else:
            conv = _module(w.reshape(N, K, 1, 1), bias=bias)
            x = _cl(nat[0]) if layout == 'dense' else _slice_of(nat[0].cuda(), 0 if layout == 'first-half' else 1)
            if head:
                assert not relu and fused.head_conv_x3_supported(conv, x)
                out = fused.head_conv_x3(conv, x)
            else:
                p = None if partner is None else _slice_of(xc.image_of(partner, B, ho, wo).cuda(), 1)
                r = None if res is None else _slice_of(xc.image_of(res, B, ho, wo).cuda(), 0)
                assert fused.unit_conv_x3_supported(conv, x, p, r)
                out = fused.conv1x1_unit_x3(conv, x, relu, partner=p, residual=r)
        torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_contiguous(memory_format=CL)
    assert tuple(out.shape) == (B, N * (2 if partner is not None else 1), ho, wo)
    return xc.rows_of(out.cpu())


def _torch32(spec, nat, w, bias, res=None, a_bias=None, relu=False):
    """torch's own float32 convolution(s) of the case -> rows ``[M, N]``.  On the CPU: its algorithm is fixed, while the GPU library
    picks one per run and machine (direct, implicit GEMM, a Winograd of its own), which moved e0_c -- and the bar -- up to
    eightfold from one run to the next."""
    F = torch.nn.functional
    K, N = xc.dims(spec)
    B, ho, wo = xc.out_shape(spec)
    mode = spec[0]
    with torch.no_grad():
        x = nat[0]
        if a_bias is not None:
            x = (x + a_bias.view(1, -1, 1, 1)).clamp_min(0)
        if mode == 'pair':
            k1 = spec[1]
            out = F.conv2d(x, w[:, :k1].reshape(N, k1, 1, 1)) + F.conv2d(nat[1], w[:, k1:].reshape(N, K - k1, 1, 1), stride=spec[4])
        elif mode == 'conv3':
            out = F.conv2d(x, xc.weight_4d(w, 64, 3), stride=spec[1], padding=1)
        elif mode == 'stem':
            out = F.conv2d(x, xc.weight_4d(w, 3, 7), stride=2, padding=3)
        else:
            out = F.conv2d(x, w.reshape(N, K, 1, 1))
        out = out + bias.view(1, -1, 1, 1)
        if res is not None:
            out = out + xc.image_of(res, B, ho, wo)
        if relu:
            out = torch.relu(out)
    return xc.rows_of(out)


@pytest.fixture(autouse=True)
def _winograd_variant_4_on_its_64_channel_kernel(monkeypatch):
    """Variant 4 takes the 128-channel kernel where the launcher's rule says it pays; the Winograd tests here name the kernel they
    run (``_wino_variant``) instead of following the rule.  The launcher reads the variable on every launch."""
    monkeypatch.setenv('OPA_WINO_X3_BN', '64')


def _wino_variant(shape):
    """Variant 4 (64-channel workgroups, pinned above) on ``x3_common.WINO``, variant 5 (128-channel ones) on ``WINO_WIDE``."""
    assert (shape in xc.WINO) != (shape in xc.WINO_WIDE)
    return 5 if shape in xc.WINO_WIDE else 4


def _run_wino(x, f, bias, relu, order):
    from openpifpaf_amd import winograd
    variant = _wino_variant((x.shape[0], x.shape[1], f.shape[0], x.shape[2], x.shape[3]))
    with torch.no_grad():
        out = winograd.conv3x3_x3(_cl(x), winograd.split_filter(f.cuda()), f.shape[0], bias=None if bias is None else bias.cuda(),
                                  relu=relu, variant=variant, order=order)
        torch.cuda.synchronize()
    assert out.is_contiguous(memory_format=CL)
    return out.cpu().contiguous()


def _torch32_wino(x, f, bias, relu):
    """torch's float32 convolution on the CPU (see ``_torch32``)."""
    out = torch.nn.functional.conv2d(x, f, bias, padding=1)
    return (torch.relu(out) if relu else out).contiguous()


def _layouts(spec):
    """The operand layouts a case is run with (the unit mode: dense and as either half of a wider tensor whose other half is NaN;
    the stem: NCHW and channels-last)."""
    if spec[0] == 'unit':
        return ['dense', 'first-half', 'second-half']
    return ['nchw', 'channels_last'] if spec[0] == 'stem' else ['dense']


def _variants(spec):
    """(layout, head) pairs: every layout, and ``head_conv_x3`` where the head takes the shape (K a multiple of 64)."""
    out = [(layout, False) for layout in _layouts(spec)]
    if spec[0] == 'unit' and spec[1] % 64 == 0:
        out.append(('dense', True))
    return out


# ---- (a) known answers -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', xc.GEMM_SPECS, ids=xc.spec_id)
def test_selection_weight_returns_the_chosen_columns_bit_for_bit(spec, terms):
    """Row n of the weight is 1.0 at one column: ``out[:, n]`` IS that column of the operand -- 24-bit significands, exponents over
    2^+-60, every K column over the offsets (for the implicit modes every tap, every border and the seam between images: +0.0
    where the tap lies in the padding); with ReLU, ``clamp_min(0)`` of it.  Bias zero, residual none or zero."""
    g = xc.gen(21)
    K, N = xc.dims(spec)
    nat, a = xc.activations(spec, lambda shape: xc.full_significand(shape, g))
    zero_bias = torch.zeros(N)
    seen = torch.zeros(K, dtype=torch.bool)
    for i, off in enumerate(xc.selection_offsets(N, K)):
        cols = xc.selection_columns(N, K, off, g)
        seen[cols] = True
        w = xc.selection_weight(cols, K)
        want = a[:, cols]
        res = torch.zeros_like(want) if i % 2 == 1 and spec[0] == 'plain' else None
        for layout, head in _variants(spec):
            got = _run(spec, nat, w, zero_bias, res, None, False, terms, layout, head=head)
            assert torch.equal(_bits(got), _bits(want)), (off, layout, head)
            if not head:
                got = _run(spec, nat, w, zero_bias, res, None, True, terms, layout)
                assert torch.equal(got, want.clamp_min(0)), (off, layout, 'relu')
    assert bool(seen.all())


@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', xc.PLAIN + xc.UNIT, ids=xc.spec_id)
def test_one_hot_activation_returns_the_weight_bit_for_bit(spec, terms):
    """Row m of the operand is 1.0 at column ``m mod K``: ``out[m, :]`` IS that column of the weight -- every plane position of the
    weight operand and of ``_unit_weight_of``'s padding (M = 286 >= K: every column is read)."""
    g = xc.gen(22)
    K, N = xc.dims(spec)
    B, H, W = xc.BHW
    a = xc.one_hot(B * H * W, K)
    w = xc.full_significand((N, K), g)
    want = w[:, torch.arange(a.shape[0]) % K].t().contiguous()
    for layout, head in _variants(spec):
        got = _run(spec, [xc.image_of(a, B, H, W)], w, torch.zeros(N), None, None, False, terms, layout, head=head)
        assert torch.equal(_bits(got), _bits(want)), (layout, head)


@pytest.mark.parametrize('with_res,with_pro', [(False, False), (True, True)], ids=['bare', 'res-pro'])
@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', xc.GEMM_SPECS, ids=xc.spec_id)
def test_integer_operands_give_the_int64_result(spec, terms, with_res, with_pro):
    """A, W, bias, residual and a_bias integers sized so that every partial sum stays below 2^24 (asserted in test_x3_cases.py):
    the result is the int64 one whatever the order of summation -- bias, residual, prologue, ReLU and the partner interleave
    in the exact regime."""
    nat, a, w, bias, res, ab = xc.integer_problem(spec, 5, with_res, with_pro)
    ab_all = None if ab is None else xc.prologue_bias(spec, ab)
    for relu in (False, True):
        want = xc.ref64(a, w, bias, res, ab_all, relu)
        for layout, head in _variants(spec):
            if head and (relu or res is not None):
                continue
            got = _run(spec, nat, w, bias, res, ab, relu, terms, layout, head=head)
            assert torch.equal(got.double(), want), (relu, layout, head)
    if spec[0] == 'unit' and not with_res:                               # the partner's bits pass, the product sits between them
        p = xc.integers((a.shape[0], w.shape[0]), xc.gen(23), 20)
        p[0, 0], p[1, 1], p[-1, -1], p[130, 2] = NAN, -0.0, INF, -INF
        got = _run(spec, nat, w, bias, None, None, True, terms, 'second-half', partner=p)
        assert torch.equal(_bits(got[:, 0::2]), _bits(p))
        assert torch.equal(got[:, 1::2].double(), xc.ref64(a, w, bias, None, None, True))


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('shape', xc.WINO + xc.WINO_WIDE, ids=str)
def test_winograd_power_of_two_taps_on_16_bit_integers(shape, order):
    """One power-of-two tap per output channel on 16-bit integer inputs: ``out[b, o, y, x] = 2^p x[b, c(o), y + r - 1, x + s - 1]``,
    zero in the padding -- every intermediate of the transforms fits float32 (asserted in test_x3_cases.py)."""
    x, f, want = xc.winograd_integer_case(shape, 6)
    for relu in (False, True):
        got = _run_wino(x, f, None, relu, order)
        assert torch.equal(got.double(), want.clamp_min(0) if relu else want), relu


# ---- (b) power-of-two scaling ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', xc.GEMM_SPECS, ids=xc.spec_id)
def test_power_of_two_scaling_is_exact(spec, terms):
    """``f(2^s A, 2^t W, 2^(s+t) bias, 2^(s+t) res) == 2^(s+t) f(A, W, bias, res)`` bit for bit on N(0, 1) data (a_bias goes with
    A), without an activation and with ReLU; the ranges neither overflow nor underflow (test_x3_cases.py)."""
    for with_res, with_pro, relu in ((False, False, False), (True, True, True)):
        nat, a, w, bias, res, ab = xc.randn_problem(spec, 7, with_res, with_pro)
        runs = [(_layouts(spec)[-1], False)]
        if not relu and res is None:
            runs += [v for v in _variants(spec) if v[1]]                 # head_conv_x3 where it takes the shape
        for layout, head in runs:
            base = _run(spec, nat, w, bias, res, ab, relu, terms, layout, head=head)
            assert bool(base.isfinite().all()) and float(base.abs().max()) > 0
            for s, t in xc.SCALINGS:
                fa, fo = 2.0 ** s, 2.0 ** (s + t)
                got = _run(spec, [v * fa for v in nat], w * 2.0 ** t, bias * fo, None if res is None else res * fo,
                           None if ab is None else ab * fa, relu, terms, layout, head=head)
                assert torch.equal(got, base * fo), (s, t, relu, head)


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('shape', xc.WINO + xc.WINO_WIDE, ids=str)
def test_winograd_power_of_two_scaling_is_exact(shape, order):
    x, f, bias = xc.winograd_randn_case(shape, 8)
    for relu in (False, True):
        base = _run_wino(x, f, bias, relu, order)
        assert bool(base.isfinite().all()) and float(base.abs().max()) > 0
        for s, t in xc.SCALINGS:
            got = _run_wino(x * 2.0 ** s, f * 2.0 ** t, bias * 2.0 ** (s + t), relu, order)
            assert torch.equal(got, base * 2.0 ** (s + t)), (s, t, relu)


# ---- (c) wide dynamic range ----------------------------------------------------------------------------------------------------------------

def _median(values):
    return sorted(values)[len(values) // 2]


def _report(what, e0, err, extra, note=''):
    bar = 2 * e0 + extra
    print('X3EDGE %s | e0_c %.3e | err_c %.3e | err_c/e0_c %.2f | bar %.3e %s%s'
          % (what, e0, err, err / max(e0, 1e-30), bar, 'ok' if err <= bar else 'ABOVE', note))
    return err <= bar


@pytest.mark.parametrize('relu', [False, True], ids=['none', 'relu'])
@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', xc.PLAIN + xc.PAIR + xc.CONV3 + xc.UNIT, ids=xc.spec_id)
def test_wide_dynamic_range_componentwise(spec, terms, relu):
    """Rows of A scaled by 2^U(-40, 40), elements by 2^U(-12, 12), weights by 2^U(-6, 6): ``err_c <= 2 e0_c + extra`` with e0_c the
    same measure of torch's own float32 convolution on the same operands (on the CPU, median of nine calls), extra = 0 with nine terms and
    2^-23 with six (the three dropped products)."""
    nat, a, w, bias = xc.wide_problem(spec, 9)
    ref, S = xc.ref64(a, w, bias, relu=relu), xc.scale_of(a, w, bias)
    e0 = _median([xc.err_c(_torch32(spec, nat, w, bias, relu=relu), ref, S) for _ in range(9)])
    for layout in _layouts(spec)[:2]:
        got = _run(spec, nat, w, bias, None, None, relu, terms, layout)
        assert bool(got.isfinite().all())
        err = xc.err_c(got, ref, S)
        assert _report('wide %s %s terms=%d act=%s' % (xc.spec_id(spec), layout, terms, 'relu' if relu else 'none'), e0, err,
                       xc.EXTRA[terms]), (e0, err)


@pytest.mark.parametrize('relu', [False, True], ids=['none', 'relu'])
@pytest.mark.parametrize('shape', xc.WINO + xc.WINO_WIDE, ids=str)
def test_winograd_wide_dynamic_range(shape, relu):
    """Inputs inside a window span 2^+-4, only the scale per image keeps its 2^+-40, weights 2^+-6.  Winograd's transforms add
    across the taps and across the 4x4 tile and the output transform takes the sums apart again, so the error is measured
    against ``x3_common.winograd_scale`` -- the sum of the magnitudes of every term the algorithm forms, which is the
    convolution's ``sum |x||w|`` over the window and all channels plus what the transforms add to it (test_x3_cases.py: never
    below it; against the window's sum alone no float32 F(2x2, 3x3) meets the bar, at the 1x1 image by a factor of 40).
    ``err_c <= 2 e0_c + 2^-23`` (variant 4 has six terms), e0_c the same measure of torch's float32 convolution on the CPU."""
    x, f = xc.wino_wide_case(shape, 11)
    ref = torch.nn.functional.conv2d(x.double(), f.double(), padding=1)
    ref = ref.clamp_min(0) if relu else ref
    Sw = xc.winograd_scale(x, f)
    e0 = _median([xc.err_c(_torch32_wino(x, f, None, relu), ref, Sw) for _ in range(9)])
    for order in (0, 1):
        got = _run_wino(x, f, None, relu, order)
        assert bool(got.isfinite().all())
        err = xc.err_c(got, ref, Sw)
        assert _report('wide winograd %s order=%d act=%s' % (shape, order, 'relu' if relu else 'none'), e0, err, xc.EXTRA[6]), (e0, err)


# ---- (d) subnormal pieces ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('small', ['a', 'w'])
@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', xc.SUBNORMAL_SPECS, ids=xc.spec_id)
def test_subnormal_pieces(spec, terms, small):
    """small = 'a': every fourth row of A has ``|a|`` in [2^-126, 2^-104) and every sixteenth is subnormal float32, against weights
    of order 1; small = 'w': the same rows of W against activations of order 1 (the two never meet: their products underflow in
    any float32 result).  The low pieces of such numbers are subnormal bfloat16 numbers, and below 2^-133 bfloat16 has nothing.
    Required: ``|got - ref| <= (2 e0_c + extra) S + 2^-125 sum_k (|a_mk| + |w_nk|)`` -- the second term is what flushing every
    subnormal piece would cost; it also covers what bfloat16 cannot hold at all and, with six terms, the dropped products of a
    subnormal float32 operand (its second piece is empty, its third has 16 bits).  Printed: whether the bar holds without the
    second term, and whether the pieces were kept -- the error of the telling elements against ``x3_common.KEPT_BELOW``, which
    test_x3_cases.py shows to lie between a pipe that keeps subnormal inputs and one that flushes them."""
    K, N = xc.dims(spec)
    nat, a, w, tell = xc.subnormal_problem(spec, small)
    bias = torch.zeros(N)
    ref, S, cost = xc.ref64(a, w, bias), xc.scale_of(a, w, bias), xc.flush_cost(a, w)
    # e0_c and the printed err_c are taken where a float32 result CAN be exact to its last bit, S >= 2^-102: below, the result is
    # near or in the subnormal range itself, and "relative to S" measures the format, not the product
    full = S >= 2.0 ** -102
    assert bool(full.any())
    e0 = _median([xc.err_c(_torch32(spec, nat, w, bias)[full], ref[full], S[full]) for _ in range(9)])
    got = _run(spec, nat, w, bias, None, None, False, terms, _layouts(spec)[-1])
    assert bool(got.isfinite().all())
    d = (got.double() - ref).abs()
    bar = 2 * e0 + xc.EXTRA[terms]
    note = ' | bar met without the flush term: %s' % bool((d <= bar * S).all())
    if tell is not None:
        # the elements that tell: rows in [2^-110, 2^-104) have three bfloat16 pieces, part of the third ones subnormal.  Kept, they
        # are as exact as any other; flushed, they are off by 1e-06 and more (test_x3_cases.py derives KEPT_BELOW from both)
        e_tell = float((d / S)[tell].max())
        note += (' | err_c of the telling elements %.3e (threshold %.3e): pieces %s'
                 % (e_tell, xc.KEPT_BELOW, 'KEPT' if e_tell < xc.KEPT_BELOW else 'FLUSHED'))
    _report('subnormal-%s %s terms=%d' % (small, xc.spec_id(spec), terms), e0, xc.err_c(got[full], ref[full], S[full]), xc.EXTRA[terms], note)
    assert bool((d <= bar * S + cost).all()), float((d - bar * S - cost).max())


# ---- (e) non-finite values -----------------------------------------------------------------------------------------------------------------

def _pixel(shape, m):
    """Row m of ``rows_of`` of a [B, C, H, W] tensor -> (b, y, x)."""
    _, _, h, w = shape
    return m // (h * w), (m // w) % h, m % w


def _plant_rows(t, rows_cols_values):
    """A copy of the [B, C, H, W] tensor ``t`` with ``value`` at channel ``col`` of pixel ``row`` for every (row, col, value)."""
    t = t.clone()
    for row, col, value in rows_cols_values:
        b, y, x = _pixel(t.shape, row % (t.shape[0] * t.shape[2] * t.shape[3]))
        t[b, col % t.shape[1], y, x] = value
    return t


NONFINITE = [('plain', 192, 128), ('plain', 64, 64), ('plain', 64, 192), ('pair', 32, 96, 64, 2), ('pair', 64, 64, 128, 1),
             ('conv3', 1), ('conv3', 2), ('unit', 174, 128), ('unit', 72, 40), ('unit', 64, 34)]


def _check(what, got, clean, cls, relu, zeroed=None):
    bad = xc.nonfinite_violations(got, clean, cls, relu, zeroed)
    assert not any(bad.values()), (what, bad)


@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', NONFINITE, ids=xc.spec_id)
def test_non_finite_activations_stay_in_their_rows(spec, terms):
    """NaN, +Inf and -Inf in A -- one per kind in different 128-row tiles where the case has them, one in the last row, one at
    column K - 1, for the unit mode NaN right behind the operand's last column in a wider tensor.  With ``ref32`` the float32
    result: where it is finite the kernel's result is finite and bit for bit that of the run with the planted values replaced
    by finite ones; where it is NaN the result is NaN; where it is +-Inf the result is that Inf or NaN (an Inf operand leaves the
    split as (Inf, NaN, NaN)); with ReLU at those places NaN, 0 or +Inf.  Under the prologue ``fmaxf(a + a_bias, 0)`` turns a NaN
    operand into 0 (as -Inf): there the row may also be the clean run's, whose operand is 0 at that place."""
    g = xc.gen(41)
    K, N = xc.dims(spec)
    for with_pro in ([False, True] if xc.has_prologue(spec) else [False]):
        nat, a, w, bias, _, ab = xc.randn_problem(spec, 12, False, with_pro)
        first = nat[0]
        rows = first.shape[0] * first.shape[2] * first.shape[3]
        places = [(5 % rows, 3, NAN), (140 % rows, 0, INF), (270 % rows, 7, -INF), (rows - 1, 1, NAN), (200 % rows, first.shape[1] - 1, INF)]
        bad_nat = [_plant_rows(first, places)] + nat[1:]
        # the clean run: a finite value in every planted place -- one the prologue turns into 0, where there is a prologue
        clean_nat = [_plant_rows(first, [(r, c, -3e38 if with_pro else 0.0) for r, c, _ in places])] + nat[1:]
        if spec[0] == 'pair':                     # the second activation (never negative under a prologue), at pixels both strides read
            bad_nat[1] = _plant_rows(nat[1], [(0, nat[1].shape[1] - 1, INF), (93, 2, NAN)])
            clean_nat[1] = _plant_rows(nat[1], [(0, nat[1].shape[1] - 1, 0.0), (93, 2, 0.0)])
        ab_all = None if ab is None else xc.prologue_bias(spec, ab)
        a_bad = xc.operand_of(spec, bad_nat)
        cls = xc.nonfinite_class(xc.ref32(a_bad, w, bias, None, ab_all))
        assert bool((cls == xc.FINITE).any()) and bool((cls != xc.FINITE).any())
        zeroed = None
        if with_pro:                       # rows holding a planted NaN: the prologue runs over every column (the pair's second
            zeroed = a_bad.isnan().any(1, keepdim=True).expand(-1, N)         # activation meets a_bias = 0)
        for relu in (False, True):
            for layout, head in _variants(spec):
                if head and relu:
                    continue
                clean = _run(spec, clean_nat, w, bias, None, ab, relu, terms, layout, head=head)
                assert bool(clean.isfinite().all())
                got = _run(spec, bad_nat, w, bias, None, ab, relu, terms, layout, head=head)
                _check((with_pro, relu, layout, head), got, clean, cls, relu, zeroed)


@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', NONFINITE + xc.STEM, ids=xc.spec_id)
def test_non_finite_weights_bias_residual_and_partner_stay_in_their_places(spec, terms):
    """NaN, +Inf and -Inf in three weight rows (columns 0, K - 1 and 5), +Inf in the bias, NaN / -Inf in the residual; the unit
    mode's partner with NaN, +-Inf and -0.0 is copied bit for bit and touches nothing else.  (In the implicit modes a non-finite
    weight meets the padding's zeros: 0 x Inf is NaN in the kernel and in the im2col reference alike.)"""
    K, N = xc.dims(spec)
    nat, a, w, bias, res, _ = xc.randn_problem(spec, 13, True, False)
    w_bad = xc.plant(w, [((1, 0), NAN), ((N // 2, K - 1), INF), ((N - 1, 5), -INF)])
    bias_bad = xc.plant(bias, [((3,), INF)])
    res_bad = None if res is None else xc.plant(res, [((7, 9), NAN), ((a.shape[0] - 1, N - 2), -INF), ((129, 0), INF)])
    cls = xc.nonfinite_class(xc.ref32(a, w_bad, bias_bad, res_bad))
    assert bool((cls == xc.FINITE).any()) and bool((cls != xc.FINITE).any())
    for relu in (False, True):
        for layout in _layouts(spec):
            clean = _run(spec, nat, w, bias, res, None, relu, terms, layout)
            assert bool(clean.isfinite().all())
            got = _run(spec, nat, w_bad, bias_bad, res_bad, None, relu, terms, layout)
            _check((relu, layout), got, clean, cls, relu)
    if spec[0] == 'unit':
        p = torch.randn((a.shape[0], N), generator=xc.gen(14))
        p[0, 0], p[1, 1], p[-1, -1], p[130, 2], p[128, N - 1] = NAN, -0.0, INF, -INF, NAN
        cls = xc.nonfinite_class(xc.ref32(a, w_bad, bias_bad))
        clean = _run(spec, nat, w, bias, None, None, True, terms, 'dense')
        got = _run(spec, nat, w_bad, bias_bad, None, None, True, terms, 'first-half', partner=p)
        assert torch.equal(_bits(got[:, 0::2]), _bits(p))
        _check('partner', got[:, 1::2].contiguous(), clean, cls, True)
        if spec[1] % 64 == 0:                                            # the head's launch of the plain kernel on padded weights
            clean = _run(spec, nat, w, bias, None, None, False, terms, 'dense', head=True)
            got = _run(spec, nat, w_bad, bias_bad, None, None, False, terms, 'dense', head=True)
            _check('head', got, clean, cls, False)


@pytest.mark.parametrize('terms', TERMS)
def test_stem_non_finite_pixels_reach_the_8x8_window_and_no_further(terms):
    """The stem's K-step is a window ROW of 8 pixels x 4 channels against zero weights in the eighth row and column (and the
    fourth channel, which is zero in memory): a non-finite pixel there meets 0 x Inf.  A departure from the GEMM contract that is
    written down rather than paid for with a select per element (the stem takes images): where the 7x7 window holds the pixel
    the contract's classes apply; where only the 8x8 window does, the result is NaN or the clean run's; everything else is bit
    for bit the clean run's."""
    spec = ('stem',)
    nat, a, w, bias, _, _ = xc.randn_problem(spec, 17, False, False)
    x = nat[0]
    B, _, H, W = x.shape
    _, ho, wo = xc.out_shape(spec)
    places = [((0, 1, 0, 0), NAN), ((0, 2, 20, 31), INF), ((1, 0, H - 1, W - 1), -INF), ((1, 1, 8, 12), NAN)]
    x_bad = xc.plant(x, places)
    cls = xc.nonfinite_class(xc.ref32(xc.im2col_stem(x_bad), w, bias))
    wide = torch.zeros((B, ho, wo), dtype=torch.bool)                    # outputs whose 8x8 window holds a planted pixel
    for (b, _, y, xx), _ in places:
        for oy in range(ho):
            for ox in range(wo):
                if 2 * oy - 3 <= y <= 2 * oy + 4 and 2 * ox - 3 <= xx <= 2 * ox + 4:
                    wide[b, oy, ox] = True
    wide = wide.reshape(-1, 1).expand(-1, w.shape[0])
    assert bool(((cls != xc.FINITE) <= wide).all()) and bool((wide & (cls == xc.FINITE)).any()) and bool((~wide).any())
    leak = wide & (cls == xc.FINITE)
    allowed = torch.where(leak, torch.full_like(cls, xc.NAN), cls)
    for relu in (False, True):
        for layout in _layouts(spec):
            clean = _run(spec, [x], w, bias, None, None, relu, terms, layout)
            assert bool(clean.isfinite().all())
            got = _run(spec, [x_bad], w, bias, None, None, relu, terms, layout)
            _check((relu, layout), got, clean, allowed, relu, zeroed=leak)


@pytest.mark.parametrize('order', [0, 1])
def test_winograd_non_finite_inputs_stay_in_their_windows(order):
    """Variant 4: a NaN, a +Inf and a -Inf pixel in three places of two images (a corner of the first tile, the last pixel, the
    inside).  F(2x2, 3x3) reads a 4x4 input tile for 2x2 outputs, but ``B^T d B`` and ``A^T M A`` only add and subtract: a tile row
    that an output's window does not hold never enters that output.  So the contract is the GEMM modes': with ``ref32`` torch's
    float32 convolution, where it is finite the result is bit for bit the clean run's -- in the same tile too -- and where it is
    NaN or +-Inf the result is NaN or that infinity (an infinite V leaves the split as NaN); with ReLU NaN, 0 or +Inf."""
    _winograd_non_finite_inputs(xc.WINO[0], order)


@pytest.mark.parametrize('order', [0, 1])
def test_winograd_wide_non_finite_inputs_stay_in_their_windows(order):
    """The same contract, against the same references (torch's float32 convolution, ``nonfinite_class``), for variant 5.  Its
    padding is no select but a load past the buffer descriptor's range: the corner pixel and the last pixel are where that zero
    meets an infinity in ``B^T d B`` -- and must stay a zero (Inf - 0, never Inf x 0 or Inf - Inf) wherever the reference is
    finite.  40 tiles in two blocks of 32: the planted pixels lie in block 0 (tile 0), block 0's last tiles and block 1."""
    _winograd_non_finite_inputs(xc.WINO_WIDE[0], order)


def _winograd_non_finite_inputs(shape, order):
    x, f, bias = xc.winograd_randn_case(shape, 15)
    B, C, H, W = x.shape
    places = [((0, 3, 0, 0), NAN), ((0, C - 1, H - 1, W - 1), INF), ((1, 0, 3, 4), -INF)]
    x_bad = xc.plant(x, places)
    cls = xc.nonfinite_class(torch.nn.functional.conv2d(x_bad, f, bias, padding=1))
    window = torch.zeros((B, 1, H, W), dtype=torch.bool)
    for (b, _, y, xx), _ in places:
        window[b, 0, max(y - 1, 0):y + 2, max(xx - 1, 0):xx + 2] = True
    assert torch.equal(cls != xc.FINITE, window.expand(B, f.shape[0], H, W))
    for relu in (False, True):
        clean = _run_wino(x, f, bias, relu, order)
        got = _run_wino(x_bad, f, bias, relu, order)
        assert bool(clean.isfinite().all())
        _check(('winograd', relu), got, clean, cls, relu)


@pytest.mark.parametrize('order', [0, 1])
def test_winograd_non_finite_filter_and_bias_stay_in_their_channels(order):
    """NaN, +Inf and -Inf in three filters (one tap of one input channel each), +Inf in the bias of a fourth.  ``G g G^T`` spreads
    a non-finite tap over the sixteen positions of that (c_out, c_in) pair and nowhere else: the output CHANNEL is non-finite, at
    the borders too (where the tap meets the padding the im2col reference has 0 x Inf = NaN as well); every other channel is
    bit for bit the clean run's."""
    _winograd_non_finite_filter_and_bias(xc.WINO[0], order)


@pytest.mark.parametrize('order', [0, 1])
def test_winograd_wide_non_finite_filter_and_bias_stay_in_their_channels(order):
    """The same for variant 5, whose workgroup holds all 128 channels as four accumulator blocks of 32 and rotates the filter
    fragments through four register sets: channels 1 and 3 (block 0), 64 (block 2) and 127 (block 3) are non-finite, every other
    channel -- in the same block, the same fragment, the same 64-channel output half -- is bit for bit the clean run's."""
    _winograd_non_finite_filter_and_bias(xc.WINO_WIDE[0], order)


def _winograd_non_finite_filter_and_bias(shape, order):
    x, f, bias = xc.winograd_randn_case(shape, 16)
    B, C, H, W = x.shape
    O = f.shape[0]
    f_bad = xc.plant(f, [((1, 0, 0, 0), NAN), ((O // 2, C - 1, 1, 1), INF), ((O - 1, 5, 2, 2), -INF)])
    bias_bad = xc.plant(bias, [((3,), INF)])
    ref32 = xc.ref32(xc.im2col_3x3(x, 1), xc.weight_rows(f_bad), bias_bad)
    cls = xc.nonfinite_class(xc.image_of(ref32, B, H, W))
    assert sorted(set((cls != xc.FINITE).any(0).any(1).any(1).nonzero().flatten().tolist())) == sorted({1, 3, O // 2, O - 1})
    for relu in (False, True):
        clean = _run_wino(x, f, bias, relu, order)
        got = _run_wino(x, f_bad, bias_bad, relu, order)
        assert bool(clean.isfinite().all())
        _check(('winograd filter', relu), got, clean, cls, relu)
