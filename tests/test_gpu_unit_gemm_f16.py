"""The unit mode of the 16-bit GEMM in FLOAT16 (csrc/gemm_unit_bf16.hip instantiated with ``TileElem<1>``, ``opa_gemm_unit_actp_f16``): the
1x1 convolutions of a ShuffleNetV2K cast with ``.half()`` -- any even K and N, the operand a channel slice on a 4-byte boundary, the
result stored dense or into its shuffled position next to a partner the same kernel copies, one rounding at the store.  Kernel level,
``M = 3 x 23 x 19 = 1311`` and the five shapes of ``test_gpu_unit_gemm_bf16.py``: a K shorter than one K-step (24), a K tail and a
4-byte-only slice offset (174: 348 bytes), no tail at all (256), an N tail (340) and more than one N tile (1392).

Known answers are demanded bit for bit: every product and sum of the first two tests is a small integer, exact in float32 and in
float16 (every integer up to 2048 is one) whatever the order of summation.  Random operands are held to the float32 accumulation
bound of ANY summation order, doubled (truncating adders), plus half an ulp of float16 (2^-11 relative, 2^-25 absolute below 2^-14)
-- and to the project's relative bar, 1.05 x the error of torch's own float16 convolution.  Float16's own ground: a subnormal
activation, the last finite value and the first sums that become +-inf, a partner's NaN payload / -0.0 / inf / subnormal bits."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import test_gpu_unit_gemm as f32                         # noqa: E402  (``_conv``: the operands of the float32 unit mode's tests)

CL = torch.channels_last
B, H, W, M = f32.B, f32.H, f32.W, f32.M
SHAPES = [(24, 174), (174, 174), (256, 256), (1392, 340), (1392, 1392)]
F16 = torch.float16
assert M == 1311 and M % 128 != 0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rows(t):
    """[B, C, H, W] -> [M, C] (values)."""
    return t.permute(0, 2, 3, 1).reshape(M, t.shape[1])


def _image(rows):
    """[M, C] -> [B, C, H, W] channels_last, same dtype."""
    return rows.reshape(B, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def _conv_of(w, bias):
    """A float16 1x1 convolution with the weight ``w`` [N, K] and ``bias`` [N] (values exact in float16)."""
    n, k = w.shape
    conv = torch.nn.Conv2d(k, n, 1).cuda().to(F16).requires_grad_(False)
    conv.weight.copy_(w.view(n, k, 1, 1))
    conv.bias.copy_(bias)
    assert torch.equal(conv.weight.double().view(n, k), w.double()) and torch.equal(conv.bias.double(), bias.double())
    return conv


def _half_of(t, half, fill=float('nan')):
    """``t`` [B, C, H, W] float16 as the first (0) / second (1) half of the channels of a [B, 2C, H, W] channels-last tensor whose
    other half holds ``fill``; the bits of ``t`` are copied as they are."""
    c = t.shape[1]
    big = torch.full((B, 2 * c, H, W), fill, device='cuda', dtype=F16).contiguous(memory_format=CL)
    view = big[:, half * c:(half + 1) * c]
    view.view(torch.int16).copy_(t.view(torch.int16))
    assert view.data_ptr() == big.data_ptr() + half * c * 2 and view.data_ptr() % 4 == 0
    return view


def _gemm(conv, x, **kw):
    from openpifpaf_amd import fused
    old, fused.UNIT_F16 = fused.UNIT_F16, True
    try:
        assert fused.unit_conv_f16_supported(conv, x, kw.get('partner'), kw.get('residual'))
        assert fused.unit_mode_of(x) is fused.UNIT_MODE_F16
    finally:
        fused.UNIT_F16 = old
    kw.setdefault('act', 0)
    out = fused.conv1x1_unit_f16(conv, x, **kw)
    torch.cuda.synchronize()
    assert out.dtype == F16 and out.is_contiguous(memory_format=CL)
    return out


def _third(n, seed, special=True):
    """A partner [B, n, H, W] float16 (dense channels-last) with a NaN that carries a payload, -0.0, inf and a subnormal among its bits."""
    torch.manual_seed(seed)
    p = torch.randn(B, n, H, W, device='cuda').to(F16).contiguous(memory_format=CL)
    if special:
        bits = p.view(torch.int16)
        bits[0, 0, 0, 0], bits[1, n - 1, 2, 3], bits[2, 1, H - 1, W - 1], bits[0, 3, 1, 1] = 0x7E55, -0x8000, 0x7C00, 0x0001
        assert p[0, 0, 0, 0].isnan() and p[2, 1, H - 1, W - 1].isinf() and float(p[0, 3, 1, 1]) == 2.0 ** -24
    return p


@pytest.mark.parametrize('k,n', SHAPES)
def test_column_selection_bit_for_bit(k, n):
    """Row m of A holds 1.0 at column m mod K and 2.0 at (7 m + 3) mod K (the 2.0 wins where they coincide), W and the bias random
    integers in [-8, 8]: out[m] = W[:, c1] + 2 W[:, c2] + bias, an integer of magnitude <= 32 (<= 40 with the residual) -- a wrong
    column, row, K-step or fragment order is a wrong integer.  Dense, as either half of a tensor whose other half is NaN, with a
    partner, with a residual."""
    g = torch.Generator(device='cuda').manual_seed(11 + k + n)
    w = torch.randint(-8, 9, (n, k), device='cuda', generator=g)
    bias = torch.randint(-8, 9, (n,), device='cuda', generator=g)
    res = torch.randint(-8, 9, (M, n), device='cuda', generator=g)
    m = torch.arange(M, device='cuda')
    c1, c2 = m % k, (7 * m + 3) % k
    a = torch.zeros((M, k), device='cuda')
    a[m, c1] = 1.0
    a[m, c2] = 2.0
    wt = w.t()
    want = wt[c1] * (c1 != c2).unsqueeze(1) + 2 * wt[c2] + bias                    # int64 [M, N]
    assert int(want.abs().max()) <= 32 and int((want + res).abs().max()) <= 40
    conv = _conv_of(w.to(F16), bias.to(F16))
    x = _image(a.to(F16)).contiguous(memory_format=CL)
    want_h, want_res = want.to(F16), (want + res).to(F16)
    assert torch.equal(want_h.long(), want) and torch.equal(want_res.long(), want + res)
    assert torch.equal(_bits(_rows(_gemm(conv, x))), _bits(want_h))
    for half in (1, 0):
        assert torch.equal(_bits(_rows(_gemm(conv, _half_of(x, half)))), _bits(want_h)), half
    p = _third(n, 5)
    got = _rows(_gemm(conv, x, partner=_half_of(p, 1))).reshape(M, n, 2)
    assert torch.equal(_bits(got[:, :, 0]), _bits(_rows(p))) and torch.equal(_bits(got[:, :, 1]), _bits(want_h))
    r = _half_of(_image(res.to(F16)), 0)
    assert torch.equal(_bits(_rows(_gemm(conv, _half_of(x, 0), residual=r))), _bits(want_res))


def _exact_operands(k, n):
    """a in {0, 1}, w in {-1, 0, 1}, bias in [-4, 4], from numpy's generator: the operands of ``test_gpu_unit_gemm_bf16.py``."""
    rng = np.random.default_rng(1000 * k + n)
    a = rng.integers(0, 2, (M, k)).astype(np.float32)
    w = rng.integers(-1, 2, (n, k)).astype(np.float32)
    bias = rng.integers(-4, 5, (n,)).astype(np.float32)
    return a, w, bias


@pytest.mark.parametrize('k,n', SHAPES)
def test_dense_exact_sums_bit_for_bit(k, n):
    """Every element of A and W takes part: sums of up to K products of {0, 1} x {-1, 0, 1}.  The int64 reference stays within
    +-256 (asserted), where every integer is a float16 and every partial sum a float32: the result must be that integer."""
    a, w, bias = (torch.from_numpy(t).cuda() for t in _exact_operands(k, n))
    want = (a.double() @ w.double().t() + bias.double()).long()
    assert int(want.abs().max()) <= 256
    got = _rows(_gemm(_conv_of(w.to(F16), bias.to(F16)), _image(a.to(F16)).contiguous(memory_format=CL)))
    assert torch.equal(_bits(got), _bits(want.to(F16))) and torch.equal(got.long(), want)


def _random_case(k, n):
    conv32, x32 = f32._conv(k, n)
    conv = _conv_of(conv32.weight.view(n, k).to(F16), conv32.bias.to(F16))
    return conv, x32.to(F16).contiguous(memory_format=CL)


_REFERENCE = {}


def _reference(k, n):
    """(p, S) in float64 for the random case, computed once per shape: p = sum a w + bias, S = sum |a w| + |bias|, [M, N]."""
    if (k, n) not in _REFERENCE:
        conv, x = _random_case(k, n)
        a, w, b = _rows(x).double(), conv.weight.double().view(n, k), conv.bias.double()
        _REFERENCE[(k, n)] = (a @ w.t() + b, a.abs() @ w.abs().t() + b.abs())
    return _REFERENCE[(k, n)]


def _act64(p, code, param):
    if code == 0:
        return p
    if code == 1:
        return p.clamp(min=0)
    if code == 2:
        return p * (p + 3).clamp(0, 6) / 6
    if code == 3:
        return torch.where(p < 0, p * param, p)
    return p.clamp(0, param)


# (code, parameter, with a residual)
ACTS = [(0, 0.0, False), (1, 0.0, False), (2, 0.0, False), (3, 0.01, False), (3, 2.5, False), (4, 0.5, False),
        (0, 0.0, True), (1, 0.0, True), (2, 0.0, True)]


@pytest.mark.parametrize('code,param,with_residual', ACTS)
@pytest.mark.parametrize('k,n', SHAPES)
def test_random_operands_against_float64(k, n, code, param, with_residual):
    """|got - act(p)| <= L E + 2^-11 (|act(p)| + L E) + 2^-25 for EVERY element: E = 2 (K + 2) 2^-24 S bounds the float32 accumulation
    of the K products, the bias and the residual in any order (u = 2^-24 per addition, doubled for adders that truncate), L is the
    activation's Lipschitz constant (1, 1, 1.5, max(1, slope), 1), 2^-11 half an ulp of float16, relative, for the one rounding, and
    2^-25 half the subnormal spacing, for results below 2^-14."""
    conv, x = _random_case(k, n)
    p, s = _reference(k, n)
    kw = {}
    if with_residual:
        r = _third(n, 9, special=False)
        kw['residual'] = _half_of(r, 1)
        p, s = p + _rows(r).double(), s + _rows(r).double().abs()
    got = _rows(_gemm(conv, x, act=code, act_param=param, **kw)).double()
    want = _act64(p, code, param)
    lip = {0: 1.0, 1: 1.0, 2: 1.5, 3: max(1.0, param), 4: 1.0}[code]
    e = lip * 2.0 * (k + 2) * 2.0 ** -24 * s
    excess = (got - want).abs() - (e + 2.0 ** -11 * (want.abs() + e) + 2.0 ** -25)
    print('unit gemm f16 K=%d N=%d act=%d(%g) residual=%d: max |error| %.3e, largest error - bound %.3e'
          % (k, n, code, param, with_residual, float((got - want).abs().max()), float(excess.max())))
    assert float(excess.max()) <= 0.0


@pytest.mark.parametrize('k,n', SHAPES)
def test_rms_error_no_worse_than_torch_float16(k, n):
    """The project's relative bar (``test_gpu_unit_gemm_bf16.py``): the rms error against float64 is no more than 1.05 x that of torch's
    own float16 convolution + ReLU on the same operands."""
    conv, x = _random_case(k, n)
    ref = _reference(k, n)[0].clamp(min=0)
    got = _rows(_gemm(conv, x, act=1))
    theirs = _rows(torch.relu(torch.nn.functional.conv2d(x, conv.weight, conv.bias)))
    e_got, e_theirs = f32._errors(got, ref), f32._errors(theirs, ref)
    print('unit gemm f16 K=%d N=%d: rms %.3e max %.3e | torch float16 rms %.3e max %.3e' % ((k, n) + e_got + e_theirs))
    assert e_got[0] <= 1.05 * e_theirs[0], (e_got, e_theirs)


@pytest.mark.parametrize('k,n', SHAPES)
def test_channel_slices_sentinels_partner_bits_and_activations(k, n):
    """The operand as either half next to NaN equals the dense call bit for bit; a sentinel outside [M, N] / [M, 2N] stays; the
    partner's bits pass through (a NaN with a payload, -0.0, inf and a subnormal among them); codes 1 and 4 are relu / clamp(., 0, cap)
    of the code-0 result bit for bit (both commute with the rounding); two calls give equal bits."""
    from openpifpaf_amd import _lib, fused
    conv, x = _random_case(k, n)
    dense = _gemm(conv, x)
    assert dense.isfinite().all()
    assert torch.equal(_bits(dense), _bits(_gemm(conv, x)))
    for half in (1, 0):
        assert torch.equal(_bits(_gemm(conv, _half_of(x, half))), _bits(dense)), half
    assert torch.equal(_bits(_gemm(conv, x, act=1)), _bits(torch.where(dense < 0, torch.zeros_like(dense), dense)))
    assert torch.equal(_bits(_gemm(conv, x, act=4, act_param=0.5)), _bits(torch.where(dense < 0, torch.zeros_like(dense), dense.clamp(max=0.5))))
    # the raw entry point into a buffer with a sentinel around the output
    wp, bp = fused._unit_weight_f16_of(conv)
    assert wp.dtype == F16 and bp.dtype == torch.float32
    p = _third(n, 7)
    partner = _half_of(p, 1)
    assert torch.equal(_bits(partner), _bits(p))
    pad, sentinel = 4096, 12345.0
    for third, width in ((None, n), (partner, 2 * n)):
        buf = torch.full((pad + M * width + pad,), sentinel, device='cuda', dtype=F16)
        assert (buf.data_ptr() + pad * 2) % 16 == 0
        rc = _lib.lib().opa_gemm_unit_actp_f16(
            ctypes.c_void_p(x.data_ptr()), k, ctypes.c_void_p(wp.data_ptr()), ctypes.c_void_p(bp.data_ptr()),
            ctypes.c_void_p(third.data_ptr()) if third is not None else None, 2 * n if third is not None else 0, None, 0,
            ctypes.c_void_p(buf.data_ptr() + pad * 2), M, n, k, 0, 0.0, None)
        torch.cuda.synchronize()
        assert rc == 0
        assert (buf[:pad] == sentinel).all() and (buf[pad + M * width:] == sentinel).all()
        out = buf[pad:pad + M * width]
        if third is None:
            assert torch.equal(_bits(out.view(M, n)), _bits(_rows(dense)))
        else:
            out = out.view(M, n, 2)
            assert torch.equal(_bits(out[:, :, 0]), _bits(_rows(p))) and torch.equal(_bits(out[:, :, 1]), _bits(_rows(dense)))
            again = _rows(_gemm(conv, x, partner=partner)).reshape(M, n, 2)
            assert torch.equal(_bits(again), _bits(out))


@pytest.mark.parametrize('k,n', SHAPES)
def test_a_subnormal_activation_contributes_exactly(k, n):
    """Row m of A holds 2^-20 -- a SUBNORMAL float16 -- at column m mod K and zeros elsewhere, every weight is 2^10 and every bias 1:
    the one product is exactly 2^-10 and every output element 1 + 2^-10, one unit of float16 above 1 (the f16 MFMA keeps subnormal
    activations, as ``test_gpu_tile_f16.py`` found for the tile kernels)."""
    m = torch.arange(M, device='cuda')
    a = torch.zeros((M, k), device='cuda', dtype=torch.float64)
    a[m, m % k] = 2.0 ** -20
    assert torch.equal(a.to(F16).double(), a)
    conv = _conv_of(torch.full((n, k), 2.0 ** 10, device='cuda', dtype=F16), torch.ones(n, device='cuda', dtype=F16))
    got = _rows(_gemm(conv, _image(a.to(F16)).contiguous(memory_format=CL)))
    want = torch.full((M, n), 1.0 + 2.0 ** -10, device='cuda', dtype=torch.float64).to(F16)
    assert float(want[0, 0]) == 1.0 + 2.0 ** -10
    assert torch.equal(_bits(got), _bits(want)), got.flatten()[:8]


def test_the_store_at_the_end_of_float16s_range():
    """Rows whose exact sums are 65504 (the last finite float16: stays), 65519 (rounds down to 65504), 65520 (the tie that becomes inf),
    -65520 (-inf) and 131008 (far beyond: inf): every partial sum is an integer below 2^24, exact in float32 in any order, so the
    stored bits must be ``tensor.to(torch.float16)`` of the exact sum.  With the ReLU -inf becomes 0 and inf stays."""
    k, n = 24, 174
    rows = torch.tensor([[1, 1, 0, 0], [1, 1, 0, 1], [1, 1, 1, 0], [-1, -1, -1, 0], [2, 2, 0, 0]], device='cuda', dtype=torch.float64)
    a = torch.zeros((M, k), device='cuda', dtype=torch.float64)
    a[:, :4] = rows[torch.arange(M, device='cuda') % 5]
    w = torch.zeros((n, k), device='cuda', dtype=torch.float64)
    w[:, 0], w[:, 1], w[:, 2], w[:, 3] = 32752.0, 32752.0, 16.0, 15.0
    assert torch.equal(w.to(F16).double(), w)
    exact = a @ w.t()
    assert sorted(set(exact[:5, 0].tolist())) == [-65520.0, 65504.0, 65519.0, 65520.0, 131008.0]
    want = exact.float().to(F16)
    assert want[:5, 0].tolist() == [65504.0, 65504.0, float('inf'), -float('inf'), float('inf')]
    conv = _conv_of(w.to(F16), torch.zeros(n, device='cuda', dtype=F16))
    x = _image(a.to(F16)).contiguous(memory_format=CL)
    assert torch.equal(_bits(_rows(_gemm(conv, x))), _bits(want))
    assert torch.equal(_bits(_rows(_gemm(conv, x, act=1))), _bits(exact.clamp(min=0).float().to(F16)))


def test_an_empty_call_and_a_refused_one_launch_nothing():
    from openpifpaf_amd import _lib, fused
    conv, x = _random_case(174, 174)
    wp, bp = fused._unit_weight_f16_of(conv)
    out = torch.full((M * 174,), 12345.0, device='cuda', dtype=F16)

    def raw(a, m=M, n=174, k=174, pitch=174):
        return _lib.lib().opa_gemm_unit_actp_f16(ctypes.c_void_p(a), pitch, ctypes.c_void_p(wp.data_ptr()), ctypes.c_void_p(bp.data_ptr()),
                                                 None, 0, None, 0, ctypes.c_void_p(out.data_ptr()), m, n, k, 1, 0.0, None)
    assert raw(x.data_ptr(), m=0) == 0
    for case in (dict(a=x.data_ptr() + 2), dict(a=x.data_ptr(), n=173), dict(a=x.data_ptr(), k=173), dict(a=x.data_ptr(), pitch=172),
                 dict(a=x.data_ptr(), m=2 ** 31)):
        assert raw(**case) != 0, case
    torch.cuda.synchronize()
    assert (out == 12345.0).all()
