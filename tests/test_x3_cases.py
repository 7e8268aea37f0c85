"""The expectations of tests/test_gpu_x3_edges.py follow from the split-operand arithmetic, not from the kernels: everything here
runs on the CPU against ``x3_common.model`` (three bfloat16 pieces per operand, six or nine piece products).  The split itself, the
known answers (selection weights, one-hot activations, integers inside a bit budget that is ASSERTED), the scaling cases' range,
the wide-range bar, and four mutants of the arithmetic that each fail a named measure -- the proof that the new measures can fail."""
import pytest

torch = pytest.importorskip('torch')

import x3_common as xc  # noqa: E402

TERMS = [6, 9]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the split ---------------------------------------------------------------------------------------------------------------------------

def test_split3_is_split_weight_bit_for_bit_on_random_bit_patterns():
    from openpifpaf_amd import fused
    g = xc.gen(1)
    t = torch.randint(-2 ** 31, 2 ** 31, (64, 1024), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    p = xc.split3(t)
    w3 = fused.split_weight(t)
    assert w3.dtype == torch.bfloat16 and tuple(w3.shape) == (3, 64, 1024)
    assert torch.equal(w3.view(torch.int16), p.to(torch.bfloat16).view(torch.int16))
    fin = t.isfinite()
    # every piece IS a bfloat16 number from |t| = 2^-110 up (and for zero); below, the number has bits under 2^-133, the smallest
    # subnormal bfloat16: the float32 pieces still sum to it, their bfloat16 forms are off by less than 2^-133 together
    big = fin & ((t.abs() >= 2.0 ** -110) | (t == 0))
    assert bool((_bits(p)[:, big] & 0xffff == 0).all()) and bool((t[fin & ~big] != 0).any())
    lost = (p.double() - p.to(torch.bfloat16).double())[:, fin & ~big].abs().sum(0)
    assert float(lost.max()) < 2.0 ** -133 and float(lost.max()) > 0
    back = (p[0] + p[1]) + p[2]
    zero = t == 0
    assert torch.equal(_bits(back)[fin & ~zero], _bits(t)[fin & ~zero])   # (a zero comes back as +0.0, see below)
    assert bool((back[zero] == 0).all())
    assert torch.equal(p.double().sum(0)[fin], t.double()[fin])
    assert bool(back[~fin].isnan().all())                                 # Inf and NaN alike: the pieces no longer sum to the number


def test_split_of_special_values_is_pinned():
    inf, nan = float('inf'), float('nan')
    quiet_low = torch.tensor([0x7f800001], dtype=torch.int32).view(torch.float32)      # a NaN whose payload is in the low 16 bits
    t = torch.cat((torch.tensor([inf, -inf, nan, -0.0, 0.0]), quiet_low))
    p = xc.split3(t)
    assert p[0, 0] == inf and p[0, 1] == -inf and bool(p[1:, :2].isnan().all())         # +-Inf -> (+-Inf, NaN, NaN): Inf - Inf
    assert bool(p[:, 2].isnan().all())
    assert p[0, 5] == inf and bool(p[1:, 5].isnan().all())                              # its high half is Inf's: (Inf, NaN, NaN)
    assert _bits(p[:, 3]).tolist() == [-2 ** 31, 0, 0] and _bits(p[:, 4]).tolist() == [0, 0, 0]     # -0.0 -> (-0.0, +0.0, +0.0)
    # subnormal float32 numbers and normal ones below 2^-110: the split stays exact, the low pieces are subnormal bfloat16 numbers
    a = xc.subnormal_piece_rows(64, 32, xc.gen(2))
    q = xc.split3(a)
    assert torch.equal(_bits((q[0] + q[1]) + q[2]), _bits(a))
    assert bool((_bits(q[:2]) & 0xffff == 0).all())                      # (the third piece may hold bits below 2^-133: see above)
    tiny = 2.0 ** -126
    rows = torch.arange(64)
    small, sub = a[rows % 4 == 1], a[rows % 16 == 3]
    assert bool((small.abs() >= tiny).all()) and bool((small.abs() < 2.0 ** -104).all())
    assert bool((sub.abs() < tiny).all()) and bool((sub != 0).all())
    low_rows = (rows % 4 == 1) & (xc.small_row_exponent(64) <= -111)    # a3 < 2^-16 |a| < 2^-126: a subnormal bfloat16 number
    third = q[2, low_rows]
    assert bool(low_rows.any()) and bool((third.abs() < tiny).all()) and float((third != 0).float().mean()) > 0.9
    assert bool(xc.representable_small_rows(64).any())


# ---- known answers -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('terms', TERMS)
def test_selection_weight_returns_the_operand_exactly(terms):
    """w = 1.0 has the pieces (1, 0, 0) and all three products a_i x 1 are among the six: every K column, exponents over 2^+-100."""
    g = xc.gen(3)
    m, k, n = 286, 192, 64
    a = xc.full_significand((m, k), g, -100, 100)
    seen = torch.zeros(k, dtype=torch.bool)
    for off in xc.selection_offsets(n, k):
        cols = xc.selection_columns(n, k, off, g)
        seen[cols] = True
        assert torch.equal(xc.model(a, xc.selection_weight(cols, k), terms), a[:, cols].double())
    assert bool(seen.all())
    x = xc.full_significand((3, 64, 9, 7), g)                            # the 3x3 mode's operand: padding is +0.0, every tap
    for stride in (1, 2, 3):
        col = xc.im2col_3x3(x, stride)
        for off in xc.selection_offsets(64, 576):
            cols = xc.selection_columns(64, 576, off, g)
            assert torch.equal(xc.model(col, xc.selection_weight(cols, 576), terms), col[:, cols].double())


@pytest.mark.parametrize('terms', TERMS)
def test_one_hot_activation_returns_the_weight_exactly(terms):
    g = xc.gen(4)
    m, k, n = 286, 174, 128
    w = xc.full_significand((n, k), g, -100, 100)
    assert torch.equal(xc.model(xc.one_hot(m, k), w, terms), w[:, torch.arange(m) % k].t().double())


def _is_multiple(t, unit):
    return bool((torch.remainder(t.double(), unit) == 0).all())


@pytest.mark.parametrize('with_res,with_pro', [(False, False), (True, True)])
@pytest.mark.parametrize('spec', xc.GEMM_SPECS, ids=xc.spec_id)
def test_integer_cases_stay_inside_their_bit_budget(spec, with_res, with_pro):
    """Every piece is an integer, the pieces' magnitudes add up to the number's (truncation keeps the sign), so every partial sum
    of every piece product in ANY order is an integer below ``S = sum |a||w| + |bias| + |res| < 2^24``: exact in float32."""
    _, a, w, bias, res, ab = xc.integer_problem(spec, 5, with_res, with_pro)
    ab = None if ab is None else xc.prologue_bias(spec, ab)
    a_eff = xc.operand32(a, ab)
    assert torch.equal(a_eff.double(), xc.operand(a, ab))                 # the prologue is exact
    pa, pw = xc.split3(a_eff), xc.split3(w)
    for t in (pa, pw, bias) + (() if res is None else (res,)):
        assert _is_multiple(t, 0.25) and _is_multiple(t, 1.0)
    assert torch.equal(pa.abs().sum(0), a_eff.abs()) and torch.equal(pw.abs().sum(0), w.abs())
    assert bool((pa[1] != 0).any()) and bool((pw[1] != 0).any())          # the values need two pieces
    S = xc.scale_of(a, w, bias, res, ab)
    assert float(S.max()) < 2.0 ** 24
    exact = a_eff.to(torch.int64) @ w.to(torch.int64).t()
    for terms in TERMS:
        assert torch.equal(xc.model(a_eff, w, terms), exact.double())     # (the third pieces are zero: six terms lose nothing)
    full = exact + bias.to(torch.int64) + (0 if res is None else res.to(torch.int64))
    assert torch.equal(xc.ref64(a, w, bias, res, ab), full.double()) and float(full.abs().max()) < 2.0 ** 24


@pytest.mark.parametrize('shape', xc.WINO + xc.WINO_WIDE, ids=str)
def test_winograd_integer_case_stays_inside_its_bit_budget(shape):
    """16-bit inputs, one power-of-two tap per output channel: the input transform (both passes), U, every partial sum of U V over
    the channels and every partial sum of the output transform are multiples of 2^-2 below 2^24; U is ONE piece, so the six kept
    products hold all three pieces of V; and the expected output is the float64 algorithm's, exactly."""
    from openpifpaf_amd import winograd
    x, f, want = xc.winograd_integer_case(shape, 6)
    half, v, u, m_abs, m, y_abs = xc.winograd_intermediates(x, f)
    for t in (half, v, u, m_abs, m, y_abs):
        assert _is_multiple(t, 0.25) and float(t.abs().max()) < 2.0 ** 24
    assert bool((x.abs() >= 2 ** 8).any())                               # the inputs need two pieces, V up to three
    pu = xc.split3(u.float())
    assert torch.equal(u.float().double(), u) and bool((pu[1:] == 0).all())
    assert torch.equal(winograd.reference_f23(x, f), want)
    assert torch.equal(torch.nn.functional.conv2d(x.double(), f.double(), padding=1), want)


# ---- scaling -----------------------------------------------------------------------------------------------------------------------------

def _scaling_range_ok(a_eff, w, bias, res, s, t):
    """Neither overflow nor underflow under (2^s, 2^t): every piece of the scaled operands is a normal number, every non-zero partial
    sum of piece products is a multiple of 2^(lowest bit of a + lowest bit of w) >= 2^-126 and so are the bias and the residual,
    and the largest magnitude any partial sum can reach stays below 2^127."""
    la, lw = float(xc.lowest_bit(a_eff).min()), float(xc.lowest_bit(w).min())
    ok = la + s >= -126 and lw + t >= -126 and la + lw + s + t >= -126
    for extra in (bias, res):
        if extra is not None:
            ok = ok and float(xc.lowest_bit(extra).min()) + s + t >= -126
    S = xc.scale_of(a_eff, w, bias, res)
    top = max(float(S.max()) * 2.0 ** (s + t), float(a_eff.abs().max()) * 2.0 ** s, float(w.abs().max()) * 2.0 ** t)
    return ok and top < 2.0 ** 127


@pytest.mark.parametrize('s,t', xc.SCALINGS)
@pytest.mark.parametrize('spec', xc.GEMM_SPECS, ids=xc.spec_id)
def test_scaling_cases_neither_overflow_nor_underflow(spec, s, t):
    for with_res, with_pro in ((False, False), (True, True)):
        _, a, w, bias, res, ab = xc.randn_problem(spec, 7, with_res, with_pro)
        ab = None if ab is None else xc.prologue_bias(spec, ab)
        assert _scaling_range_ok(xc.operand32(a, ab), w, bias, res, s, t)
        if ab is not None:                                               # the prologue's own sum scales exactly too
            assert torch.equal(xc.operand32(a * 2.0 ** s, ab * 2.0 ** s), xc.operand32(a, ab) * 2.0 ** s)
            assert float(xc.lowest_bit(ab[ab != 0]).min()) + s >= -126


@pytest.mark.parametrize('s,t', xc.SCALINGS)
@pytest.mark.parametrize('shape', xc.WINO + xc.WINO_WIDE, ids=str)
def test_winograd_scaling_cases_neither_overflow_nor_underflow(shape, s, t):
    """V is a sum of inputs (a multiple of their lowest bit), U = G g G^T rounded to float32 once: the same condition on (x, U)."""
    x, f, bias = xc.winograd_randn_case(shape, 8)
    _, v, u, m_abs, _, y_abs = xc.winograd_intermediates(x, f)
    u32 = u.float()
    assert torch.equal((xc.winograd_intermediates(x * 2.0 ** s, f * 2.0 ** t)[2]).float(), u32 * 2.0 ** t)
    lx, lu = float(xc.lowest_bit(x).min()), float(xc.lowest_bit(u32).min())
    assert lx + s >= -126 and lu + t >= -126 and lx + lu + s + t >= -126
    assert float(xc.lowest_bit(bias).min()) + s + t >= -126
    assert float(y_abs.max()) * 2.0 ** (s + t) < 2.0 ** 126 and float(v.abs().max()) * 2.0 ** s < 2.0 ** 127


# ---- the wide-range bar ------------------------------------------------------------------------------------------------------------------

def _torch_conv(spec, nat, w, bias):
    """torch's own float32 convolution(s) of the case on the CPU -> [B, N, ho, wo]."""
    F = torch.nn.functional
    K, N = xc.dims(spec)
    if spec[0] == 'conv3':
        return F.conv2d(nat[0], xc.weight_4d(w, 64, 3), bias, stride=spec[1], padding=1)
    if spec[0] == 'pair':
        k1 = spec[1]
        return F.conv2d(nat[0], w[:, :k1].reshape(N, k1, 1, 1), bias) + F.conv2d(nat[1], w[:, k1:].reshape(N, K - k1, 1, 1), stride=spec[4])
    return F.conv2d(nat[0], w.view(N, K, 1, 1), bias)


@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', [('plain', 192, 64), ('conv3', 1), ('pair', 32, 96, 64, 2), ('unit', 174, 128)], ids=xc.spec_id)
def test_wide_range_bar_holds_for_the_model_and_for_torch_float32(spec, terms):
    """``err_c <= 2 e0_c + 2^-23`` with e0_c taken from the other of the two: the model with the kernels' float32 accumulators
    (``x3_common.model_f32``), and torch's float32 convolution on the CPU -- the bar the GPU test uses is one that a correct
    float32 product meets on these operands, and one that does not let a worse one through.  (The model rounded to float32 ONCE
    is below both: printed, and held to the same bar against torch.)"""
    nat, a, w, bias = xc.wide_problem(spec, 9)
    ref, S = xc.ref64(a, w, bias), xc.scale_of(a, w, bias)
    e_model = xc.err_c(xc.model_f32(a, w, terms) + bias, ref, S)
    e_once = xc.err_c((xc.model(a, w, terms) + bias.double()).float(), ref, S)
    e_torch = xc.err_c(xc.rows_of(_torch_conv(spec, nat, w, bias)), ref, S)
    print('X3CASE wide %s terms=%d | model rounded once %.3e' % (xc.spec_id(spec), terms, e_once))
    assert e_once <= 2 * e_torch + 2.0 ** -23
    print('X3CASE wide %s terms=%d | model %.3e torch float32 %.3e' % (xc.spec_id(spec), terms, e_model, e_torch))
    assert e_model <= 2 * e_torch + 2.0 ** -23 and e_torch <= 2 * e_model + 2.0 ** -23, (e_model, e_torch)


# ---- mutants: each fails a named measure ----------------------------------------------------------------------------------------------------

def _drop_piece(pa, pw):                      # the third piece of A's last K column is lost (where tails and selects live)
    pa = pa.clone()
    pa[2, :, -1] = 0
    return pa, pw


def _swap_planes(pa, pw):                     # A's planes 2 and 3 change places (a wrong LDS plane offset)
    return pa[[0, 2, 1]], pw


def _swap_columns(pa, pw):                    # A's K columns 4 and 5 change places (a wrong swizzle)
    idx = torch.arange(pa.shape[2])
    idx[4], idx[5] = 5, 4
    return pa[:, :, idx], pw


def _mutant(name):
    mutate = {'piece dropped in one K column': _drop_piece, 'planes 2 and 3 swapped': _swap_planes,
              'K columns k and k+1 swapped': _swap_columns, 'small rows returned as 0': None}[name]

    def run(a, w, terms):
        out = xc.model(a, w, terms, mutate)
        if mutate is None:
            out = torch.where(a.abs().max(1, keepdim=True).values < 2.0 ** 20, torch.zeros_like(out), out)
        return out
    return run


def _measures(run, terms):
    """-> {measure: passed} for an implementation ``run(a, w, terms)`` of the product, on this file's own cases."""
    g = xc.gen(10)
    out = {}
    a = xc.full_significand((286, 192), g)
    cols = xc.selection_columns(64, 192, 128, g)                          # columns 128..191: K - 1 among them
    out['selection'] = torch.equal(run(a, xc.selection_weight(cols, 192), terms), a[:, cols].double())
    w = xc.full_significand((64, 192), g)
    out['one-hot'] = torch.equal(run(xc.one_hot(286, 192), w, terms), w[:, torch.arange(286) % 192].t().double())
    _, ai, wi, _, _, _ = xc.integer_problem(('plain', 192, 64), 5, False, False)
    out['integers'] = torch.equal(run(ai, wi, terms), (ai.to(torch.int64) @ wi.to(torch.int64).t()).double())
    _, aw, ww, _ = xc.wide_problem(('plain', 192, 64), 9)
    ref, S = xc.ref64(aw, ww), xc.scale_of(aw, ww)
    e0 = xc.err_c(xc.ref32(aw, ww), ref, S)
    out['wide range'] = xc.err_c(run(aw, ww, terms).float(), ref, S) <= 2 * e0 + xc.EXTRA[terms]
    # the measure the suite had: the error over the largest magnitude of the whole output
    d = (run(aw, ww, terms).float().double() - ref).abs()
    out['(old) max over max |ref|'] = float(d.max() / ref.abs().max()) < 2e-6
    return out


@pytest.mark.parametrize('terms', TERMS)
def test_the_model_itself_passes_every_measure(terms):
    assert all(_measures(lambda a, w, t: xc.model(a, w, t), terms).values())


@pytest.mark.parametrize('name,terms,fails', [
    ('piece dropped in one K column', 6, ('selection', 'wide range')), ('piece dropped in one K column', 9, ('selection', 'wide range')),
    # (with nine terms the two planes' products are all summed: the swap is no error there, and the kernels' nine-term order is
    #  symmetric in them; with six it loses a2 w2 and keeps a3 w2)
    ('planes 2 and 3 swapped', 6, ('integers', 'wide range')),
    ('small rows returned as 0', 6, ('wide range',)), ('small rows returned as 0', 9, ('wide range',)),
    ('K columns k and k+1 swapped', 6, ('one-hot', 'integers', 'wide range')),
    ('K columns k and k+1 swapped', 9, ('one-hot', 'integers', 'wide range'))])
def test_mutants_fail_a_named_measure(name, terms, fails):
    got = _measures(_mutant(name), terms)
    print('X3CASE mutant %-32s terms=%d | %s' % (name, terms, ' '.join('%s=%s' % (k, 'pass' if v else 'FAIL') for k, v in got.items())))
    for measure in fails:
        assert not got[measure], (name, measure)


# ---- the Winograd measure ----------------------------------------------------------------------------------------------------------------

def _wino_case(shape):
    x, f = xc.wino_wide_case(shape, 11)
    ref = torch.nn.functional.conv2d(x.double(), f.double(), padding=1)
    B, _, H, W = x.shape
    S = xc.image_of(xc.scale_of(xc.im2col_3x3(x, 1), xc.weight_rows(f)), B, H, W)
    return x, f, ref, S, xc.winograd_scale(x, f)


@pytest.mark.parametrize('shape', xc.WINO + xc.WINO_WIDE, ids=str)
def test_winograd_measure_is_the_algorithms_own_and_its_bar_can_be_met(shape):
    """F(2x2, 3x3) multiplies ``B^T d B`` with ``G g G^T``: sums over the 4x4 tile and over all nine taps, which the output
    transform takes apart again.  Against the convolution's own ``S`` (the 3x3 window, zero outside the image) NO float32
    Winograd meets ``2 e0_c + 2^-23`` on the wide-range case -- at the 1x1 image the output reads the centre tap alone and
    U sums up to 121 x as much -- so the Winograd tests measure against ``winograd_scale``: the same sum of magnitudes taken
    over every term the algorithm forms.  It is never below S; torch's float32 convolution (e0_c) is measured against it too;
    and the model of variant 4 meets the bar there, with e0_c from torch's CPU convolution and the other way round."""
    x, f, ref, S, Sw = _wino_case(shape)
    assert bool((Sw >= S * (1 - 1e-12)).all())
    conv32 = torch.nn.functional.conv2d(x, f, padding=1)
    mdl = xc.winograd_model_f32(x, f)
    e0, em = xc.err_c(conv32, ref, Sw), xc.err_c(mdl, ref, Sw)
    print('X3CASE winograd %s | against winograd_scale: torch float32 %.3e model %.3e | against S: torch %.3e model %.3e | max Sw/S %.1f'
          % (shape, e0, em, xc.err_c(conv32, ref, S), xc.err_c(mdl, ref, S), float((Sw / S).max())))
    assert em <= 2 * e0 + 2.0 ** -23 and e0 <= 2 * em + 2.0 ** -23, (e0, em)
    assert xc.err_c(mdl, ref, S) > 2 * xc.err_c(conv32, ref, S) + 2.0 ** -23          # (why S itself is not the measure)


def _wino_drop(pv, pu):                       # the third piece of V is lost in channel 5
    pv = pv.clone()
    pv[2, :, :, :, 5] = 0
    return pv, pu


def _wino_swap_planes(pv, pu):                # V's planes 2 and 3 change places
    return pv[[0, 2, 1]], pu


def _wino_swap_channels(pv, pu):              # V's channels 4 and 5 change places
    idx = torch.arange(pv.shape[4])
    idx[4], idx[5] = 5, 4
    return pv[:, :, :, :, idx], pu


@pytest.mark.parametrize('name,mutate', [('piece dropped in one channel', _wino_drop), ('planes 2 and 3 swapped', _wino_swap_planes),
                                         ('channels c and c+1 swapped', _wino_swap_channels), ('small images returned as 0', None)])
def test_winograd_mutants_fail_the_wide_range_measure(name, mutate):
    """The measure against ``winograd_scale`` still catches what the GEMM measures catch (shape (2, 32, 64, 7, 9))."""
    x, f, ref, _, Sw = _wino_case(xc.WINO[0])
    e0 = xc.err_c(torch.nn.functional.conv2d(x, f, padding=1), ref, Sw)
    got = xc.winograd_model_f32(x, f, mutate)
    if mutate is None:
        small = x.abs().amax((1, 2, 3)) < x.abs().max()
        got[small] = 0
    err = xc.err_c(got, ref, Sw)
    print('X3CASE winograd mutant %-28s | err_c %.3e against bar %.3e' % (name, err, 2 * e0 + 2.0 ** -23))
    assert err > 2 * e0 + 2.0 ** -23


# ---- the subnormal test can tell -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('small', ['a', 'w'])
@pytest.mark.parametrize('terms', TERMS)
@pytest.mark.parametrize('spec', [s for s in xc.SUBNORMAL_SPECS if s[0] in ('plain', 'unit')], ids=xc.spec_id)
def test_flushed_subnormal_pieces_show_in_the_telling_elements(spec, terms, small):
    """On the GPU test's own operands: with the pieces kept the telling elements are as exact as float32 allows, with every
    subnormal bfloat16 piece read as zero they are off by 1e-06 and more of S (only part of the third pieces in [2^-110, 2^-104)
    are subnormal and their losses add with either sign over K: far less than the 2^-16 one element can lose) --
    ``KEPT_BELOW`` separates the two with a factor of two to spare on either side."""
    _, a, w, tell = xc.subnormal_problem(spec, small)
    assert bool(tell.any())
    ref, S = xc.ref64(a, w), xc.scale_of(a, w)
    kept = float(((xc.model_f32(a, w, terms).double() - ref).abs() / S)[tell].max())
    flushed = float(((xc.model(a, w, terms, xc.flush_subnormal_pieces).float().double() - ref).abs() / S)[tell].max())
    print('X3CASE subnormal-%s %s terms=%d | telling elements: kept %.3e flushed %.3e' % (small, xc.spec_id(spec), terms, kept, flushed))
    assert 2 * kept < xc.KEPT_BELOW < flushed / 2, (kept, flushed)
