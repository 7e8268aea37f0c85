"""The bf16 two-source GEMM (csrc/gemm2_bf16.hip, ``opa_gemm2_bias_act_bf16``): a bfloat16 ResNet block's last 1x1 convolution and its
downsampling 1x1 convolution as one product, the folded bias and the ReLU inside, one rounding at the store.  Kernel level, through
the C entry point: ``(batch, h_in, w_in)`` = (3, 23, 19) gives M = 1311 rows at stride 1 and 360 at stride 2 (neither a multiple of the
128-row tile), (2, 7, 5) is less than one tile; ``(k1, k2, n)`` = (64, 64, 64) is one K-step per source and one 64-wide N tile,
(128, 192, 128) two and three K-steps and the 128-wide tile, (64, 128, 192) three 64-wide tiles, (0, 128, 64) the strided 1x1
convolution alone.

Known answers are demanded bit for bit: every product and sum of the first two tests is a small integer, exact in float32 and in
bfloat16 whatever the order of summation.  Random operands are held to the float32 accumulation bound of ANY summation order,
doubled (truncating adders), plus half an ulp of bfloat16 -- and to the project's relative bar, 1.05 x the error of torch's own
bfloat16 convolutions.  Every reference is float64, formed from two matrix products over explicitly gathered rows -- never torch's
GPU convolution."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(3, 23, 19), (2, 7, 5)]
STRIDES = [1, 2]
CHANNELS = [(64, 64, 64), (128, 192, 128), (64, 128, 192), (0, 128, 64)]
CASES = [pytest.param(k1, k2, n, id='k%d-k%d-n%d' % (k1, k2, n)) for k1, k2, n in CHANNELS]
GEOMETRIES = [(b, h, w, s) for b, h, w in SHAPES for s in STRIDES]
assert 3 * 23 * 19 == 1311 and 1311 % 128 != 0 and 3 * 12 * 10 == 360 and 360 % 128 != 0 and 2 * 7 * 5 < 128


def _bits(t):
    return t.contiguous().view(torch.int16)


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _rows(b, h, w, s, device='cuda'):
    """The linear index of the pixel of x [B, h, w] that row m = (b * ho + oy) * wo + ox of the product reads: (b, s oy, s ox)."""
    ho, wo = _out_hw(h, w, s)
    m = torch.arange(b * ho * wo, device=device)
    bi, oy, ox = m // (ho * wo), m // wo % ho, m % wo
    return (bi * h + s * oy) * w + s * ox


def _product64(a1, x, w, bias, s, absolute=False):
    """[A1 | x gathered at stride s] * W^T + bias in float64 as two matrix products -> [M, n]; ``absolute``: of the magnitudes (the
    bound's S).  ``a1`` [M, k1] or None, ``x`` [B, h, w, k2], ``w`` [n, k1 + k2], ``bias`` [n] or None."""
    b, h, wd, k2 = x.shape
    k1 = w.shape[1] - k2
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    total = f(x).reshape(-1, k2)[_rows(b, h, wd, s)] @ f(w)[:, k1:].t()
    if k1:
        total = total + f(a1) @ f(w)[:, :k1].t()
    return total if bias is None else total + f(bias)


def _raw(a1, k1, x, k2, b, h, w, s, a_bias, wcat, bias, out_ptr, n, relu):
    from openpifpaf_amd import _lib

    def p(t):
        return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())
    return _lib.lib().opa_gemm2_bias_act_bf16(p(a1), k1, p(x), k2, b, h, w, s, p(a_bias), p(wcat), p(bias), p(out_ptr), n, relu, None)


def _run(a1, x, w, bias, s, relu=False, a_bias=None):
    """Operands with bfloat16-exact values (any dtype) -> [M, n] bfloat16 through the C entry point."""
    b, h, wd, k2 = x.shape
    n, k1 = w.shape[0], w.shape[1] - k2
    ho, wo = _out_hw(h, wd, s)
    a1b = None if k1 == 0 else a1.to(BF).contiguous()
    xb, wb = x.to(BF).contiguous(), w.to(BF).contiguous()
    b32 = None if bias is None else bias.float().contiguous()
    ab = None if a_bias is None else a_bias.to(BF).contiguous()
    out = torch.full((b * ho * wo, n), float('nan'), device='cuda', dtype=BF)
    rc = _raw(a1b, k1, xb, k2, b, h, wd, s, ab, wb, b32, out, n, int(relu))
    torch.cuda.synchronize()
    assert rc == 0
    return out


def _select_operands(b, h, wd, s, k1, k2, n):
    """Row m of A1 holds 1.0 at channel m mod k1 and 2.0 at (7 m + 3) mod k1, pixel p of x 1.0 at p mod k2 and 2.0 at (5 p + 1) mod k2
    (the 2.0 wins where they coincide); the weights and the bias are integers in [-8, 8]."""
    g = torch.Generator(device='cuda').manual_seed(11 + k1 + 3 * k2 + n + 7 * h + s)
    w = torch.randint(-8, 9, (n, k1 + k2), device='cuda', generator=g).double()
    bias = torch.randint(-8, 9, (n,), device='cuda', generator=g).double()
    ho, wo = _out_hw(h, wd, s)
    a1 = None
    if k1:
        m = torch.arange(b * ho * wo, device='cuda')
        a1 = torch.zeros((b * ho * wo, k1), device='cuda', dtype=torch.float64)
        a1[m, m % k1] = 1.0
        a1[m, (7 * m + 3) % k1] = 2.0
    p = torch.arange(b * h * wd, device='cuda')
    x = torch.zeros((b * h * wd, k2), device='cuda', dtype=torch.float64)
    x[p, p % k2] = 1.0
    x[p, (5 * p + 1) % k2] = 2.0
    return a1, x.reshape(b, h, wd, k2), w, bias


@pytest.mark.parametrize('k1,k2,n', CASES)
def test_source_and_pixel_selection_bit_for_bit(k1, k2, n):
    """Every output is an integer of magnitude <= 2 * (1 + 2) * 8 + 8 = 56, exact in float32 and bfloat16 in any order -- a wrong
    source, row, pixel, channel or fragment order is a wrong integer.  With and without the ReLU, with and without the bias."""
    for b, h, wd, s in GEOMETRIES:
        a1, x, w, bias = _select_operands(b, h, wd, s, k1, k2, n)
        for bi in (bias, None):
            plain = _product64(a1, x, w, bi, s)
            assert float(plain.abs().max()) <= 56
            for relu in (False, True):
                want = plain.clamp(min=0) if relu else plain
                got = _run(a1, x, w, bi, s, relu)
                assert torch.equal(want.to(BF).double(), want)                          # (an integer <= 256: a bfloat16)
                assert torch.equal(_bits(got), _bits(want.to(BF))), ((b, h, wd, s), bi is not None, relu)


def _exact_operands(b, h, wd, s, k1, k2, n):
    """A1 and x in {0, 1}, w in {-1, 0, 1}, bias in [-4, 4], from numpy's generator (so that the bound below can be checked without a GPU)."""
    rng = np.random.default_rng(100000 * k1 + 100 * k2 + n + s)
    ho, wo = _out_hw(h, wd, s)
    a1 = rng.integers(0, 2, (b * ho * wo, k1))
    x = rng.integers(0, 2, (b, h, wd, k2))
    w = rng.integers(-1, 2, (n, k1 + k2))
    bias = rng.integers(-4, 5, n)
    return a1.astype(np.float64), x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64)


@pytest.mark.parametrize('k1,k2,n', CASES)
def test_dense_exact_sums_bit_for_bit(k1, k2, n):
    """Every element of A1, x and w takes part: sums of k1 + k2 products of {0, 1} x {-1, 0, 1}.  The int64 reference stays within
    +-256 (asserted; checked with numpy for these seeds: the largest magnitudes over (3, 23, 19) at stride 1 / 2 and (2, 7, 5) at
    stride 1 / 2 are 30 / 30 / 27 / 20 for (64, 64, 64), 49 / 48 / 42 / 39 for (128, 192, 128), 43 / 35 / 35 / 30 for (64, 128, 192)
    and 29 / 27 / 24 / 23 for (0, 128, 64)), where every integer is a bfloat16 and every partial sum a float32: the result must be
    that integer."""
    for b, h, wd, s in GEOMETRIES:
        a1, x, w, bias = (torch.from_numpy(t).cuda() for t in _exact_operands(b, h, wd, s, k1, k2, n))
        want = _product64(a1, x, w, bias, s).long()
        assert int(want.abs().max()) <= 256
        got = _run(a1, x, w, bias, s)
        assert torch.equal(_bits(got), _bits(want.to(BF))) and torch.equal(got.long(), want), (b, h, wd, s)


_RANDOM = {}


def _random_case(b, h, wd, s, k1, k2, n):
    """(A1, x, w, bias, a_bias) for the random cases, computed once per key and left unchanged: bfloat16-exact operands as float64."""
    key = (b, h, wd, s, k1, k2, n)
    if key not in _RANDOM:
        g = torch.Generator(device='cuda').manual_seed(1 + sum(k * 31 ** i for i, k in enumerate(key)))
        ho, wo = _out_hw(h, wd, s)
        a1 = torch.randn((b * ho * wo, k1), device='cuda', generator=g).to(BF).double()
        x = torch.randn((b, h, wd, k2), device='cuda', generator=g).to(BF).double()
        w = (torch.randn((n, k1 + k2), device='cuda', generator=g) * (2.0 / (k1 + k2)) ** 0.5).to(BF).double()
        bias = (torch.randn((n,), device='cuda', generator=g) * 0.5).to(BF).double()
        a_bias = (torch.randn((k1,), device='cuda', generator=g) * 0.5).to(BF).double()
        _RANDOM[key] = (a1, x, w, bias, a_bias)
    return _RANDOM[key]


def _assert_within_bound(what, got, a1, x, w, bias, s, relu):
    """|got - want| <= E + 2^-8 (|want| + E) for EVERY element: E = 2 (k1 + k2 + 1) 2^-24 S bounds the float32 accumulation of the
    k1 + k2 products and the bias in any order (u = 2^-24 per addition, doubled for adders that truncate), S = sum |a w| + |bias|;
    2^-8 is half an ulp of bfloat16, relative, for the one rounding; the ReLU's Lipschitz constant is 1."""
    p, sabs = _product64(a1, x, w, bias, s), _product64(a1, x, w, bias, s, absolute=True)
    want = p.clamp(min=0) if relu else p
    e = 2.0 * (w.shape[1] + 1) * 2.0 ** -24 * sabs
    excess = (got.double() - want).abs() - (e + 2.0 ** -8 * (want.abs() + e))
    print('gemm2 bf16 %s: max |error| %.3e, largest error - bound %.3e' % (what, float((got.double() - want).abs().max()), float(excess.max())))
    assert float(excess.max()) <= 0.0, what


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('k1,k2,n', CASES)
def test_random_operands_against_float64(k1, k2, n, relu):
    for b, h, wd, s in GEOMETRIES:
        a1, x, w, bias, _ = _random_case(b, h, wd, s, k1, k2, n)
        got = _run(a1, x, w, bias, s, relu)
        _assert_within_bound('%s k1=%d k2=%d n=%d relu=%d' % ((b, h, wd, s), k1, k2, n, relu), got, a1, x, w, bias, s, relu)


def _staged(a1, a_bias):
    """What the operand prologue stages for A1: bf16_rne(max(float(a) + float(a_bias[k]), 0))."""
    return (a1.to(BF).float() + a_bias.to(BF).float()).clamp(min=0).to(BF).double()


@pytest.mark.parametrize('k1,k2,n', [c for c in CASES if c.values[0] > 0])
def test_the_operand_prologue(k1, k2, n):
    """``a_bias``: A1 is raw, and relu(A1 + a_bias) rounded to bfloat16 is what is multiplied; x is staged as it is (its K-steps get no
    bias and no ReLU: x holds negative values in the random case).  The selection test with a_bias in {-1, 0} and + 1 at two channels
    -- integers of magnitude <= (3 + 2) * 8 + 3 * 8 + 8 = 72 -- bit for bit; the random test within its bound of the staged operand."""
    for b, h, wd, s in GEOMETRIES:
        a1, x, w, bias = _select_operands(b, h, wd, s, k1, k2, n)
        g = torch.Generator(device='cuda').manual_seed(5 + k1 + n + s)
        a_bias = -torch.randint(0, 2, (k1,), device='cuda', generator=g).double()
        a_bias[5], a_bias[k1 - 3] = 1.0, 1.0
        staged = _staged(a1, a_bias)
        assert not torch.equal(staged, a1) and float(staged.min()) == 0.0 and bool((a1 + a_bias < 0).any())
        plain = _product64(staged, x, w, bias, s)
        assert float(plain.abs().max()) <= 72
        for relu in (False, True):
            want = plain.clamp(min=0) if relu else plain
            got = _run(a1, x, w, bias, s, relu, a_bias)
            assert torch.equal(want.to(BF).double(), want)
            assert torch.equal(_bits(got), _bits(want.to(BF))), ((b, h, wd, s), relu)
        a1, x, w, bias, a_bias = _random_case(b, h, wd, s, k1, k2, n)
        assert bool((x < 0).any()) and bool((a1 + a_bias < 0).any())
        for relu in (False, True):
            got = _run(a1, x, w, bias, s, relu, a_bias)
            _assert_within_bound('PRO %s k1=%d k2=%d n=%d relu=%d' % ((b, h, wd, s), k1, k2, n, relu), got, _staged(a1, a_bias), x, w, bias, s, relu)


def _rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt())


@pytest.mark.parametrize('k1,k2,n', CASES)
def test_rms_error_no_worse_than_torch_bfloat16(k1, k2, n):
    """The project's relative bar (``test_gpu_unit_gemm.py``): the rms error against float64 is no more than 1.05 x that of
    ``relu(conv2d(h, W3) + conv2d(x, Wd, stride=s) + bias)`` in torch's own bfloat16 on the same operands."""
    conv2d = torch.nn.functional.conv2d
    for b, h, wd, s in GEOMETRIES:
        a1, x, w, bias, _ = _random_case(b, h, wd, s, k1, k2, n)
        ref = _product64(a1, x, w, bias, s).clamp(min=0)
        got = _run(a1, x, w, bias, s, True)
        ho, wo = _out_hw(h, wd, s)
        wb = w.to(BF)
        theirs = conv2d(x.to(BF).permute(0, 3, 1, 2), wb[:, k1:].reshape(n, k2, 1, 1).contiguous(), stride=s)
        if k1:
            theirs = conv2d(a1.to(BF).reshape(b, ho, wo, k1).permute(0, 3, 1, 2), wb[:, :k1].reshape(n, k1, 1, 1).contiguous()) + theirs
        theirs = torch.relu(theirs + bias.to(BF).view(1, n, 1, 1)).permute(0, 2, 3, 1).reshape(-1, n)
        e_got, e_theirs = _rms(got, ref), _rms(theirs, ref)
        print('gemm2 bf16 %s k1=%d k2=%d n=%d: rms %.3e | torch bfloat16 rms %.3e' % ((b, h, wd, s), k1, k2, n, e_got, e_theirs))
        assert e_got <= 1.05 * e_theirs, ((b, h, wd, s), e_got, e_theirs)


@pytest.mark.parametrize('k1,k2,n', CASES)
def test_non_finite_values(k1, k2, n):
    """A NaN or +-Inf in one element of A1, of x (at a pixel the stride reads) or of the weight shows in exactly the output elements
    whose float64 reference is not finite -- with the ReLU as well, where the reference's -Inf is 0 and NaN stays NaN (a select) --
    and every other element keeps the bits of the clean run."""
    for b, h, wd, s in GEOMETRIES:
        a1, x, w, bias, _ = _random_case(b, h, wd, s, k1, k2, n)
        m = b * _out_hw(h, wd, s)[0] * _out_hw(h, wd, s)[1]
        pixel = int(_rows(b, h, wd, s)[m // 2])
        clean = {relu: _run(a1, x, w, bias, s, relu) for relu in (False, True)}
        assert clean[False].isfinite().all()
        for value in (float('nan'), float('inf'), float('-inf')):
            for where in ('a1', 'x', 'w-a1', 'w-x'):
                if k1 == 0 and where in ('a1', 'w-a1'):
                    continue
                sa, sx, sw = (None if a1 is None or k1 == 0 else a1.clone()), x.clone(), w.clone()
                if where == 'a1':
                    sa[m - 1, 3] = value
                elif where == 'x':
                    sx.view(-1, k2)[pixel, k2 - 5] = value
                else:
                    sw[n // 2 + 1, 7 if where == 'w-a1' else k1 + 9] = value
                sums = _product64(sa, sx, sw, bias, s)
                reached = ~sums.isfinite()                                               # the elements the value reaches
                assert 0 < int(reached.sum()) < reached.numel()
                for relu in (False, True):
                    ref = sums.clamp(min=0) if relu else sums                          # (-Inf -> 0, NaN stays NaN)
                    bad = ~ref.isfinite()
                    got = _run(sa, sx, sw, bias, s, relu)
                    assert torch.equal(~got.isfinite(), bad), ((b, h, wd, s), value, where, relu)
                    assert torch.equal(got.isnan(), ref.isnan()), ((b, h, wd, s), value, where, relu)
                    assert bool((got[reached & ~bad] == 0).all())                       # the ReLU of -Inf
                    assert torch.equal(_bits(got[~reached]), _bits(clean[relu][~reached])), ((b, h, wd, s), value, where, relu)


@pytest.mark.parametrize('k1,k2,n', CASES)
def test_guard_rows_and_determinism(k1, k2, n):
    """``out`` is carved from a larger buffer with 128 sentinel rows before and behind it, and they stay; two calls on equal inputs give
    equal bits; relu = 1 is ``where(out < 0, 0, out)`` of the relu = 0 result bit for bit (the select commutes with the rounding)."""
    guard, sentinel = 128, 12345.0
    for b, h, wd, s in GEOMETRIES:
        a1, x, w, bias, a_bias = _random_case(b, h, wd, s, k1, k2, n)
        m = b * _out_hw(h, wd, s)[0] * _out_hw(h, wd, s)[1]
        a1b, xb, wb, b32 = (None if k1 == 0 else a1.to(BF).contiguous()), x.to(BF).contiguous(), w.to(BF).contiguous(), bias.float().contiguous()
        ab = None if k1 == 0 else a_bias.to(BF).contiguous()
        outs = {}
        for pro in ((None, ab) if k1 else (None,)):
            for relu in (0, 1):
                for again in (0, 1):
                    buf = torch.full((guard + m + guard, n), sentinel, device='cuda', dtype=BF)
                    assert buf[guard:].data_ptr() % 16 == 0
                    rc = _raw(a1b, k1, xb, k2, b, h, wd, s, pro, wb, b32, buf[guard:].data_ptr(), n, relu)
                    torch.cuda.synchronize()
                    assert rc == 0
                    assert (buf[:guard] == sentinel).all() and (buf[guard + m:] == sentinel).all(), ((b, h, wd, s), pro is not None, relu)
                    out = buf[guard:guard + m].clone()
                    assert torch.equal(_bits(outs.setdefault((pro is not None, relu), out)), _bits(out))
        for pro in ((False, True) if k1 else (False,)):
            plain, relued = outs[(pro, 0)], outs[(pro, 1)]
            assert plain.isfinite().all() and bool((plain < 0).any())
            assert torch.equal(_bits(relued), _bits(torch.where(plain < 0, torch.zeros_like(plain), plain)))
        assert torch.equal(_bits(outs[(False, 0)]), _bits(_run(a1, x, w, bias, s)))


def test_an_empty_call_and_a_refused_one_launch_nothing():
    b, h, wd, s, k1, k2, n = 2, 7, 5, 1, 64, 64, 64
    a1, x, w, bias, a_bias = _random_case(b, h, wd, s, k1, k2, n)
    a1b, xb, wb, b32, ab = a1.to(BF).contiguous(), x.to(BF).contiguous(), w.to(BF).contiguous(), bias.float().contiguous(), a_bias.to(BF).contiguous()
    out = torch.full((b * h * wd, n), 12345.0, device='cuda', dtype=BF)

    def raw(a1_=a1b, k1_=k1, x_=xb, k2_=k2, batch=b, hh=h, ww=wd, ss=s, ab_=None, nn=n):
        return _raw(a1_, k1_, x_, k2_, batch, hh, ww, ss, ab_, wb, b32, out, nn, 1)
    assert raw(batch=0) == 0 and raw(hh=0) == 0 and raw(ww=0) == 0
    for case in (dict(x_=xb.data_ptr() + 2), dict(x_=None), dict(a1_=None), dict(k1_=0), dict(a1_=None, k1_=0, ab_=ab), dict(k1_=32), dict(k2_=63),
                 dict(nn=32), dict(ss=3), dict(ss=0), dict(batch=-1), dict(batch=2 ** 20, hh=2 ** 10)):
        assert raw(**case) != 0, case
    torch.cuda.synchronize()
    assert (out == 12345.0).all()
