"""The bf16 GROUPED 3x3 implicit GEMM (csrc/gconv3x3_bf16.hip, ``opa_gconv3x3_act_bf16``): conv2 of a ResNeXt bottleneck cast to
bfloat16 -- as many output as input channels C, group width CG, stride 1 or 2, dilation = padding 1, 2 or 4, the folded bias and the
ReLU inside, one rounding at the store.  Kernel level: ``(B, h, w)`` = (3, 23, 19) gives M = 1311 rows at stride 1 and 360 at stride 2
(neither a multiple of the 128-row tile), (2, 7, 5) is less than one tile, and (1, 3, 3) at dilation 4 leaves only the centre tap
inside the image; ``(C, CG)`` covers one and three N-tiles, both instantiations (CG <= 32: two of the four k-substeps per wave,
CG = 64: all four) and every width.

Known answers are demanded bit for bit: every product and sum of the first two tests is a small integer, exact in float32 and in
bfloat16 whatever the order of summation.  Random operands are held to the float32 accumulation bound of ANY summation order of the
9 * 64 + 2 additions the kernel performs (those of exact zeros add no error), doubled (truncating adders), plus half an ulp of
bfloat16 -- and to the project's relative bar, 1.05 x the error of torch's own bfloat16 grouped convolution.  Every reference is
float64, formed from nine shifted per-group matrix products -- never torch's GPU convolution."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
SHAPES = [(3, 23, 19), (2, 7, 5), (1, 3, 3)]
CHANNELS = [(64, 4), (64, 8), (64, 16), (64, 32), (192, 4), (192, 8), (192, 16), (192, 32), (192, 64)]         # (C, CG)
MODES = [(1, 1), (2, 1), (1, 2), (1, 4)]                 # (stride, dilation)
CASES = [pytest.param(c, cg, s, d, id='c%d-cg%d-s%d-d%d' % (c, cg, s, d)) for c, cg in CHANNELS for s, d in MODES]
assert 3 * 23 * 19 == 1311 and 1311 % 128 != 0 and 3 * 12 * 10 == 360 and 360 % 128 != 0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _taps(x, s, d):
    """``x`` [B, h, w, C] -> the nine shifted views [B, ho, wo, C] (tap 3 ky + kx; zeros in the padding), the plain definition."""
    b, h, w, c = x.shape
    ho, wo = _out_hw(h, w, s)
    xp = torch.zeros((b, h + 2 * d, w + 2 * d, c), dtype=x.dtype, device=x.device)
    xp[:, d:d + h, d:d + w] = x
    return [xp[:, ky * d:ky * d + s * (ho - 1) + 1:s, kx * d:kx * d + s * (wo - 1) + 1:s] for ky in range(3) for kx in range(3)]


def _gconv64(x, w, s, d, absolute=False):
    """sum over the taps of the per-group products [M, G, CG] x [G, CG, CG] in float64 -> [M, C]; ``absolute``: of the magnitudes (the
    bound's S).  ``w`` [C, 3, 3, CG]: output channel co reads the CG input channels of its group co // CG."""
    x, w = x.double(), w.double()
    if absolute:
        x, w = x.abs(), w.abs()
    c, cg = w.shape[0], w.shape[3]
    total = None
    for tap, view in enumerate(_taps(x, s, d)):
        part = torch.einsum('mgi,goi->mgo', view.reshape(-1, c // cg, cg), w[:, tap // 3, tap % 3].reshape(c // cg, cg, cg))
        total = part if total is None else total + part
    return total.reshape(-1, c)


def _conv_of(w, s, d):
    """A bfloat16 grouped 3x3 convolution with the weight ``w`` [C, 3, 3, CG] (values exact in bfloat16), stride s, dilation = padding d."""
    c, cg = w.shape[0], w.shape[3]
    conv = torch.nn.Conv2d(c, c, 3, s, d, dilation=d, groups=c // cg, bias=False).cuda().to(BF).requires_grad_(False)
    conv.weight.copy_(w.permute(0, 3, 1, 2))
    assert torch.equal(conv.weight.double(), w.permute(0, 3, 1, 2).double())
    return conv


def _image(rows_nhwc):
    """[B, h, w, C] (contiguous) -> the [B, C, h, w] channels-last view of the same memory."""
    return rows_nhwc.contiguous().permute(0, 3, 1, 2)


def _run(x, w, bias, s, d, relu=False):
    """``x`` [B, h, w, C], ``w`` [C, 3, 3, CG], ``bias`` [C] or None (all bfloat16-exact) -> [M, C] bfloat16."""
    from openpifpaf_amd import fused
    b, h, wd, c = x.shape
    ho, wo = _out_hw(h, wd, s)
    conv, xi = _conv_of(w, s, d), _image(x.to(BF))
    bi = None if bias is None else bias.to(BF)
    old, fused.GCONV_BF16 = fused.GCONV_BF16, True
    try:
        assert fused.gconv3x3_bf16_supported(conv, xi, bi)
    finally:
        fused.GCONV_BF16 = old
    out = fused.gconv3x3_bias_act_bf16(conv, xi, bi, relu=relu)
    torch.cuda.synchronize()
    assert out.dtype == BF and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (b, c, ho, wo)
    return out.permute(0, 2, 3, 1).reshape(-1, c)


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_tap_selection_bit_for_bit(c, cg, s, d):
    """Pixel p (linear index) holds 1.0 at channel p mod C and 2.0 at (7 p + 3) mod C (the 2.0 wins where they coincide); w and the
    bias are integers in [-8, 8]: every output is an integer of magnitude <= 9 * 24 + 8 = 224 (asserted), exact in float32 and
    bfloat16 in any order -- a wrong tap, pixel, channel base, group boundary or fragment order is a wrong integer, and so is an
    off-group weight that leaked into the packing or a skipped k-substep that was needed.  With and without the ReLU."""
    for b, h, wd in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(11 + c + cg + 7 * h)
        w = torch.randint(-8, 9, (c, 3, 3, cg), device='cuda', generator=g).double()
        bias = torch.randint(-8, 9, (c,), device='cuda', generator=g).double()
        p = torch.arange(b * h * wd, device='cuda')
        x = torch.zeros((b * h * wd, c), device='cuda', dtype=torch.float64)
        x[p, p % c] = 1.0
        x[p, (7 * p + 3) % c] = 2.0
        x = x.reshape(b, h, wd, c)
        plain = _gconv64(x, w, s, d) + bias
        assert float(plain.abs().max()) <= 9 * 24 + 8 and torch.equal(plain, plain.round())
        for relu in (False, True):
            want = plain.clamp(min=0) if relu else plain
            got = _run(x, w, bias, s, d, relu)
            assert torch.equal(want.to(BF).double(), want)                      # (an integer <= 256: a bfloat16)
            assert torch.equal(_bits(got), _bits(want.to(BF))), ((b, h, wd), relu)


def _exact_operands(b, h, wd, c, cg):
    """x in {0, 1}, w in {-1, 0, 1}, bias in [-4, 4], from numpy's generator (so that the bound below can be checked without a GPU)."""
    rng = np.random.default_rng(1000 * c + cg)
    x = rng.integers(0, 2, (b, h, wd, c))
    w = rng.integers(-1, 2, (c, 3, 3, cg))
    bias = rng.integers(-4, 5, c)
    return x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64)


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_dense_exact_sums_bit_for_bit(c, cg, s, d):
    """Every element of x and w takes part: sums of up to 9 CG <= 576 products of {0, 1} x {-1, 0, 1} (variance 1/3 each: sigma <= 14;
    the dense kernel's test measured a maximum of 59 at K = 576).  The int64 reference stays within +-256 (asserted; checked with
    numpy on the CPU for (3, 23, 19) and these seeds: the largest magnitudes over the four (stride, dilation) pairs are
    EXACT_MAXIMA below), where every integer is a bfloat16 and every partial sum a float32: the result must be that integer."""
    for b, h, wd in SHAPES:
        x, w, bias = (torch.from_numpy(t).cuda() for t in _exact_operands(b, h, wd, c, cg))
        want = (_gconv64(x, w, s, d) + bias).long()
        assert int(want.abs().max()) <= 256
        if (b, h, wd) == SHAPES[0]:
            assert int(want.abs().max()) == EXACT_MAXIMA[(c, cg)][MODES.index((s, d))]
        got = _run(x, w, bias, s, d)
        assert torch.equal(_bits(got), _bits(want.to(BF))) and torch.equal(got.long(), want), (b, h, wd)


# max |reference| of test_dense_exact_sums_bit_for_bit at (3, 23, 19) per (C, CG), for (s, d) = (1, 1), (2, 1), (1, 2), (1, 4): numpy, CPU
EXACT_MAXIMA = {
    (64, 4): (17, 17, 17, 17), (64, 8): (21, 20, 22, 22), (64, 16): (29, 29, 31, 30), (64, 32): (44, 44, 41, 41),
    (192, 4): (18, 17, 17, 17), (192, 8): (25, 24, 25, 25), (192, 16): (30, 28, 28, 29), (192, 32): (50, 43, 45, 47),
    (192, 64): (65, 57, 57, 56),
}

_RANDOM = {}


def _random_case(b, h, wd, c, cg, s, d):
    """(x, w, bias, p, S) for the random case, computed once per key and left unchanged: bfloat16-exact operands as float64,
    p = sum x w + bias and S = sum |x w| + |bias| over the group in float64, [M, C]."""
    key = (b, h, wd, c, cg, s, d)
    if key not in _RANDOM:
        g = torch.Generator(device='cuda').manual_seed(1 + sum(k * 31 ** i for i, k in enumerate(key)))
        x = torch.randn((b, h, wd, c), device='cuda', generator=g).to(BF).double()
        w = (torch.randn((c, 3, 3, cg), device='cuda', generator=g) * (2.0 / (9 * cg)) ** 0.5).to(BF).double()
        bias = (torch.randn((c,), device='cuda', generator=g) * 0.5).to(BF).double()
        _RANDOM[key] = (x, w, bias, _gconv64(x, w, s, d) + bias, _gconv64(x, w, s, d, absolute=True) + bias.abs())
    return _RANDOM[key]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_random_operands_against_float64(c, cg, s, d, relu):
    """|got - want| <= E + 2^-8 (|want| + E) for EVERY element: E = 2 (9 * 64 + 2) 2^-24 S bounds the float32 accumulation of the
    9 * 64 products the kernel adds per output (those with an off-group zero weight add nothing and no error) and the bias in any
    order (u = 2^-24 per addition, doubled for adders that truncate), S = sum |x w| + |bias| over the group; 2^-8 is half an ulp of
    bfloat16, relative, for the one rounding; the ReLU's Lipschitz constant is 1."""
    for b, h, wd in SHAPES:
        x, w, bias, p, sabs = _random_case(b, h, wd, c, cg, s, d)
        want = p.clamp(min=0) if relu else p
        got = _run(x, w, bias, s, d, relu).double()
        e = 2.0 * (9 * 64 + 2) * 2.0 ** -24 * sabs
        excess = (got - want).abs() - (e + 2.0 ** -8 * (want.abs() + e))
        print('gconv3x3 bf16 %s C=%d CG=%d s=%d d=%d relu=%d: max |error| %.3e, largest error - bound %.3e'
              % ((b, h, wd), c, cg, s, d, relu, float((got - want).abs().max()), float(excess.max())))
        assert float(excess.max()) <= 0.0, (b, h, wd)


def _rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt())


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_rms_error_no_worse_than_torch_bfloat16(c, cg, s, d):
    """The project's relative bar (``test_gpu_unit_gemm.py``, ``test_gpu_conv3x3_bf16.py``): the rms error against float64 is no more
    than 1.05 x that of torch's own bfloat16 ``conv2d(..., groups=)`` + bias + ReLU on the same operands."""
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, c, cg, s, d)
        ref = p.clamp(min=0)
        got = _run(x, w, bias, s, d, True)
        conv = _conv_of(w, s, d)
        theirs = torch.relu(torch.nn.functional.conv2d(_image(x.to(BF)), conv.weight, bias.to(BF), stride=s, padding=d, dilation=d,
                                                       groups=c // cg))
        theirs = theirs.permute(0, 2, 3, 1).reshape(-1, c)
        e_got, e_theirs = _rms(got, ref), _rms(theirs, ref)
        print('gconv3x3 bf16 %s C=%d CG=%d s=%d d=%d: rms %.3e | torch bfloat16 rms %.3e' % ((b, h, wd), c, cg, s, d, e_got, e_theirs))
        assert e_got <= 1.05 * e_theirs, ((b, h, wd), e_got, e_theirs)


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_non_finite_values_reach_what_the_contract_states(c, cg, s, d):
    """One NaN at a corner pixel (channel 3) and one Inf at an interior pixel (channel C - 27: the other 32-channel half of the last
    chunk).  The stated contract (csrc/gconv3x3_bf16.hip): every output of the special value's OWN GROUP at a pixel whose window holds
    it is non-finite -- NaN where the NaN is held, also under the ReLU (a select); every output outside the window, or outside the
    special channel's 32-aligned block (CG <= 16) or group (CG >= 32), has the bits of the clean run: the padding is not loaded, so
    nothing multiplies a zero with them there; the remaining outputs of the block (CG <= 16 only: zeros that the MFMA does multiply)
    are each either the clean bits or NaN -- which, the test does not fix."""
    reach = 32 if cg <= 16 else cg
    for b, h, wd in SHAPES:
        x, w, bias, _, _ = _random_case(b, h, wd, c, cg, s, d)
        clean = _run(x, w, bias, s, d)
        assert clean.isfinite().all()
        where = {'nan': ((0, 0, 0), 3), 'inf': ((b - 1, h // 2, wd // 2), c - 27)}
        special = x.clone()
        special[where['nan'][0] + (3,)] = float('nan')
        special[where['inf'][0] + (c - 27,)] = float('inf')
        m = clean.shape[0]
        cols = torch.arange(c, device='cuda')
        own = torch.zeros((m, c), dtype=torch.bool, device='cuda')           # the own group at the pixels that hold the value
        block = torch.zeros((m, c), dtype=torch.bool, device='cuda')         # what the value may reach
        held = {}
        for name, (pixel, ch) in where.items():
            mark = torch.zeros(x.shape[:3] + (1,), dtype=torch.float64, device='cuda')
            mark[pixel] = 1.0
            held[name] = sum(view.reshape(-1) for view in _taps(mark, s, d)) > 0       # [M]: the window holds the pixel
            assert 0 < int(held[name].sum())
            own |= held[name][:, None] & (cols // cg == ch // cg)[None, :]
            block |= held[name][:, None] & (cols // reach == ch // reach)[None, :]
        assert bool((own & block == own).all()) and int(block.sum()) < block.numel()
        nan_own = held['nan'][:, None] & (cols // cg == 3 // cg)[None, :]
        got, with_relu = _run(special, w, bias, s, d), _run(special, w, bias, s, d, True)
        assert not got[own].isfinite().any(), (b, h, wd)
        assert got[nan_own].isnan().all() and with_relu[nan_own].isnan().all(), (b, h, wd)
        clean_relu = torch.where(clean < 0, torch.zeros_like(clean), clean)
        assert torch.equal(_bits(got[~block]), _bits(clean[~block])), (b, h, wd)
        assert torch.equal(_bits(with_relu[~block]), _bits(clean_relu[~block])), (b, h, wd)
        rest = block & ~own
        assert bool((got[rest].isnan() | (_bits(got[rest]) == _bits(clean[rest]))).all()), (b, h, wd)
        assert bool((with_relu[rest].isnan() | (_bits(with_relu[rest]) == _bits(clean_relu[rest]))).all()), (b, h, wd)
        assert int(rest.sum()) == 0 or cg <= 16


def _raw(x, w9, b32, out_ptr, b, h, wd, c, cg, s, d, relu):
    from openpifpaf_amd import _lib
    return _lib.lib().opa_gconv3x3_act_bf16(
        ctypes.c_void_p(x), ctypes.c_void_p(w9.data_ptr()), ctypes.c_void_p(b32.data_ptr()) if b32 is not None else None,
        ctypes.c_void_p(out_ptr), b, h, wd, c, cg, s, d, relu, None)


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_sentinels_repeatability_relu_and_a_null_bias(c, cg, s, d):
    """The raw entry point writes into a buffer with 4096 sentinel elements on both sides, and they stay; two calls give equal bits;
    relu = 1 is ``where(out < 0, 0, out)`` of the relu = 0 result bit for bit (the select commutes with the rounding); a NULL bias is
    a zero bias bit for bit."""
    from openpifpaf_amd import fused
    pad, sentinel = 4096, 12345.0
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, c, cg, s, d)
        m = p.shape[0]
        w9, b32 = fused.gconv3x3_bf16_weight_of(_conv_of(w, s, d), bias.to(BF))
        assert tuple(w9.shape) == (c, 9, 64) and b32.dtype == torch.float32
        xb = x.to(BF).contiguous()
        outs = {}
        for name, bias_dev in (('bias', b32), ('null', None), ('zero', torch.zeros_like(b32))):
            for relu in (0, 1):
                for again in (0, 1):
                    buf = torch.full((pad + m * c + pad,), sentinel, device='cuda', dtype=BF)
                    assert (buf.data_ptr() + pad * 2) % 16 == 0
                    rc = _raw(xb.data_ptr(), w9, bias_dev, buf.data_ptr() + pad * 2, b, h, wd, c, cg, s, d, relu)
                    torch.cuda.synchronize()
                    assert rc == 0
                    assert (buf[:pad] == sentinel).all() and (buf[pad + m * c:] == sentinel).all()
                    out = buf[pad:pad + m * c].view(m, c).clone()
                    assert torch.equal(_bits(outs.setdefault((name, relu), out)), _bits(out))
        for name in ('bias', 'null'):
            plain, relued = outs[(name, 0)], outs[(name, 1)]
            assert plain.isfinite().all() and bool((plain < 0).any())
            assert torch.equal(_bits(relued), _bits(torch.where(plain < 0, torch.zeros_like(plain), plain)))
        for relu in (0, 1):
            assert torch.equal(_bits(outs[('null', relu)]), _bits(outs[('zero', relu)]))
        assert torch.equal(_bits(outs[('bias', 0)]), _bits(_run(x, w, bias, s, d)))       # the launcher hands over the same call
        assert torch.equal(_bits(outs[('null', 1)]), _bits(_run(x, w, None, s, d, True)))


def test_an_empty_call_and_a_refused_one_launch_nothing():
    from openpifpaf_amd import fused
    b, h, wd, c, cg = 2, 7, 5, 192, 4
    x, w, bias, _, _ = _random_case(b, h, wd, c, cg, 1, 1)
    w9, b32 = fused.gconv3x3_bf16_weight_of(_conv_of(w, 1, 1), bias.to(BF))
    xb = x.to(BF).contiguous()
    out = torch.full((b * h * wd * c,), 12345.0, device='cuda', dtype=BF)

    def raw(x_ptr=xb.data_ptr(), out_ptr=out.data_ptr(), batch=b, hh=h, ww=wd, cc=c, width=cg, s=1, d=1):
        return _raw(x_ptr, w9, b32, out_ptr, batch, hh, ww, cc, width, s, d, 1)
    assert raw(batch=0) == 0 and raw(hh=0) == 0 and raw(ww=0) == 0
    for case in (dict(x_ptr=xb.data_ptr() + 2), dict(out_ptr=out.data_ptr() + 8), dict(x_ptr=0), dict(out_ptr=0), dict(cc=96), dict(width=12),
                 dict(cc=64, width=64), dict(s=3), dict(d=3), dict(s=2, d=2), dict(batch=-1), dict(batch=2 ** 20, hh=2 ** 10)):
        assert raw(**case) != 0, case
    torch.cuda.synchronize()
    assert (out == 12345.0).all()
