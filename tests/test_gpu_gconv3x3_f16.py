"""The GROUPED 3x3 implicit GEMM instantiated for float16 (csrc/gconv3x3_bf16.hip with DT = 1 on v_mfma_f32_32x32x16_f16,
``opa_gconv3x3_act_f16``, behind ``fused.GCONV_F16``): conv2 of a ResNeXt bottleneck cast with ``.half()``.  Shapes and cases are
``test_gpu_gconv3x3_bf16.py``'s: ``(B, h, w)`` = (3, 23, 19) gives M = 1311 rows at stride 1 and 360 at stride 2 (neither a multiple
of the 128-row tile), (2, 7, 5) is less than one tile, and (1, 3, 3) at dilation 4 leaves only the centre tap inside the image;
``(C, CG)`` covers one and three N-tiles, both instantiations (CG <= 32: two of the four k-substeps per wave, CG = 64: all four) and
every width.

Known answers are demanded bit for bit, among them integers that only float16 holds (odd ones between 257 and 2047).  Random
operands are held, per element, to ``|got - ref| <= 2 n 2^-24 S + ulp16(ref) / 2``: n = 9 * 64 + 2 additions in float32 in any order,
doubled (truncating adders), S the float64 sum of magnitudes with the bias, ulp16(v) = 2^(max(floor(log2 |v|), -14) - 10) for the one
rounding of the store -- derived, not measured -- and to the project's relative bar, 1.05 x the error of torch's own float16 grouped
convolution.  The store is checked at float16's edges (65504, the tie 65520 -> inf, subnormal results) against
``accumulator.to(torch.float16)`` computed on the CPU.  Every reference is float64, formed from nine shifted per-group matrix
products -- never torch's GPU convolution."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CL = torch.channels_last
F16 = torch.float16
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
    """A float16 grouped 3x3 convolution with the weight ``w`` [C, 3, 3, CG] (values exact in float16), stride s, dilation = padding d."""
    c, cg = w.shape[0], w.shape[3]
    conv = torch.nn.Conv2d(c, c, 3, s, d, dilation=d, groups=c // cg, bias=False).cuda().to(F16).requires_grad_(False)
    conv.weight.copy_(w.permute(0, 3, 1, 2))
    assert torch.equal(conv.weight.double(), w.permute(0, 3, 1, 2).double())
    return conv


def _image(rows_nhwc):
    """[B, h, w, C] (contiguous) -> the [B, C, h, w] channels-last view of the same memory."""
    return rows_nhwc.contiguous().permute(0, 3, 1, 2)


def _run(x, w, bias, s, d, relu=False):
    """``x`` [B, h, w, C], ``w`` [C, 3, 3, CG], ``bias`` [C] or None (all float16-exact) -> [M, C] float16."""
    from openpifpaf_amd import fused
    b, h, wd, c = x.shape
    ho, wo = _out_hw(h, wd, s)
    conv, xi = _conv_of(w, s, d), _image(x.to(F16))
    bi = None if bias is None else bias.to(F16)
    old, fused.GCONV_F16 = fused.GCONV_F16, True
    try:
        assert fused.gconv3x3_bf16_supported(conv, xi, bi)
    finally:
        fused.GCONV_F16 = old
    out = fused.gconv3x3_bias_act_bf16(conv, xi, bi, relu=relu)
    torch.cuda.synchronize()
    assert out.dtype == F16 and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (b, c, ho, wo)
    return out.permute(0, 2, 3, 1).reshape(-1, c)


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_tap_selection_bit_for_bit(c, cg, s, d):
    """Pixel p (linear index) holds 1.0 at channel p mod C and 2.0 at (7 p + 3) mod C (the 2.0 wins where they coincide); w and the
    bias are integers in [-8, 8]: every output is an integer of magnitude <= 9 * 24 + 8 = 224 (asserted), exact in float32 and
    float16 in any order -- a wrong tap, pixel, channel base, group boundary or fragment order is a wrong integer, and so is an
    off-group weight that leaked into the packing or a skipped k-substep that was needed.  With and without the ReLU.  A second pass
    takes a bias only float16 holds -- odd integers of magnitude 257 .. 1823 --: every output is then an integer of magnitude
    <= 216 + 1823 < 2048, still exact in float16 and in no coarser format, and odd results above 256 do occur (asserted)."""
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
        odd = (2 * torch.randint(128, 912, (c,), device='cuda', generator=g) + 1).double()               # 257 .. 1823
        odd = odd * (2 * torch.randint(0, 2, (c,), device='cuda', generator=g) - 1).double()
        wide = _gconv64(x, w, s, d) + odd
        assert float(odd.abs().min()) >= 257 and float(wide.abs().max()) <= 2047 and torch.equal(wide, wide.round())
        assert bool(((wide.abs() > 256) & (wide % 2 == 1)).any()) and not torch.equal(wide.to(torch.bfloat16).double(), wide)
        for relu in (False, True):
            for ref, bias_used in ((plain, bias), (wide, odd)):
                want = ref.clamp(min=0) if relu else ref
                got = _run(x, w, bias_used, s, d, relu)
                assert torch.equal(want.to(F16).double(), want)                  # (an integer <= 2048: a float16)
                assert torch.equal(_bits(got), _bits(want.to(F16))), ((b, h, wd), relu)


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
    EXACT_MAXIMA below), where every integer is a float16 and every partial sum a float32: the result must be that integer."""
    for b, h, wd in SHAPES:
        x, w, bias = (torch.from_numpy(t).cuda() for t in _exact_operands(b, h, wd, c, cg))
        want = (_gconv64(x, w, s, d) + bias).long()
        assert int(want.abs().max()) <= 256
        if (b, h, wd) == SHAPES[0]:
            assert int(want.abs().max()) == EXACT_MAXIMA[(c, cg)][MODES.index((s, d))]
        got = _run(x, w, bias, s, d)
        assert torch.equal(_bits(got), _bits(want.to(F16))) and torch.equal(got.long(), want), (b, h, wd)


# max |reference| of test_dense_exact_sums_bit_for_bit at (3, 23, 19) per (C, CG), for (s, d) = (1, 1), (2, 1), (1, 2), (1, 4): numpy, CPU
EXACT_MAXIMA = {
    (64, 4): (17, 17, 17, 17), (64, 8): (21, 20, 22, 22), (64, 16): (29, 29, 31, 30), (64, 32): (44, 44, 41, 41),
    (192, 4): (18, 17, 17, 17), (192, 8): (25, 24, 25, 25), (192, 16): (30, 28, 28, 29), (192, 32): (50, 43, 45, 47),
    (192, 64): (65, 57, 57, 56),
}

_RANDOM = {}


def _random_case(b, h, wd, c, cg, s, d):
    """(x, w, bias, p, S) for the random case, computed once per key and left unchanged: float16-exact operands as float64,
    p = sum x w + bias and S = sum |x w| + |bias| over the group in float64, [M, C]."""
    key = (b, h, wd, c, cg, s, d)
    if key not in _RANDOM:
        g = torch.Generator(device='cuda').manual_seed(1 + sum(k * 31 ** i for i, k in enumerate(key)))
        x = torch.randn((b, h, wd, c), device='cuda', generator=g).to(F16).double()
        w = (torch.randn((c, 3, 3, cg), device='cuda', generator=g) * (2.0 / (9 * cg)) ** 0.5).to(F16).double()
        bias = (torch.randn((c,), device='cuda', generator=g) * 0.5).to(F16).double()
        _RANDOM[key] = (x, w, bias, _gconv64(x, w, s, d) + bias, _gconv64(x, w, s, d, absolute=True) + bias.abs())
    return _RANDOM[key]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_random_operands_against_float64(c, cg, s, d, relu):
    """|got - want| <= E + ulp16(want) / 2 for EVERY element: E = 2 (9 * 64 + 2) 2^-24 S bounds the float32 accumulation of the
    9 * 64 products the kernel adds per output (those with an off-group zero weight add nothing and no error) and the bias in any
    order (u = 2^-24 per addition, doubled for adders that truncate), S = sum |x w| + |bias| over the group;
    ulp16(v) = 2^(max(floor(log2 |v|), -14) - 10) is float16's spacing at v (the subnormal spacing below 2^-14), half of it for the
    one rounding; the ReLU's Lipschitz constant is 1.  The operands are scaled so that no result comes near +-65504 (asserted)."""
    for b, h, wd in SHAPES:
        x, w, bias, p, sabs = _random_case(b, h, wd, c, cg, s, d)
        want = p.clamp(min=0) if relu else p
        got = _run(x, w, bias, s, d, relu).double()
        e = 2.0 * (9 * 64 + 2) * 2.0 ** -24 * sabs
        assert float(p.abs().max()) + float(e.max()) < 60000
        excess = (got - want).abs() - (e + 0.5 * _ulp16(want))
        print('gconv3x3 f16 %s C=%d CG=%d s=%d d=%d relu=%d: max |error| %.3e, largest error - bound %.3e'
              % ((b, h, wd), c, cg, s, d, relu, float((got - want).abs().max()), float(excess.max())))
        assert float(excess.max()) <= 0.0, (b, h, wd)


def _ulp16(v):
    """float16's spacing at ``v`` (float64 tensor): 2^(max(floor(log2 |v|), -14) - 10); at zero the subnormal spacing 2^-24."""
    exponent = torch.frexp(v.abs())[1].double() - 1                             # floor(log2 |v|); frexp(0) gives exponent 0
    return torch.exp2(torch.where(v == 0, torch.full_like(v, -14.0), exponent.clamp(min=-14.0)) - 10)


def _rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt())


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_rms_error_no_worse_than_torch_float16(c, cg, s, d):
    """The project's relative bar (``test_gpu_unit_gemm.py``, ``test_gpu_conv3x3_bf16.py``): the rms error against float64 is no more
    than 1.05 x that of torch's own float16 ``conv2d(..., groups=)`` + bias + ReLU on the same operands."""
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, c, cg, s, d)
        ref = p.clamp(min=0)
        got = _run(x, w, bias, s, d, True)
        conv = _conv_of(w, s, d)
        theirs = torch.relu(torch.nn.functional.conv2d(_image(x.to(F16)), conv.weight, bias.to(F16), stride=s, padding=d, dilation=d,
                                                       groups=c // cg))
        theirs = theirs.permute(0, 2, 3, 1).reshape(-1, c)
        e_got, e_theirs = _rms(got, ref), _rms(theirs, ref)
        print('gconv3x3 f16 %s C=%d CG=%d s=%d d=%d: rms %.3e | torch float16 rms %.3e' % ((b, h, wd), c, cg, s, d, e_got, e_theirs))
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


def _diagonal(c, cg, wv):
    """[C, 3, 3, CG] float64: output channel co reads input channel co alone, at the centre tap, with the weight ``wv[co]``."""
    w = torch.zeros((c, 3, 3, cg), dtype=torch.float64, device='cuda')
    co = torch.arange(c, device='cuda')
    w[co, 1, 1, co % cg] = wv
    return w


def _run32(x, w, bias32, s, d, relu=False):
    """``_run`` with a FLOAT32 bias handed over as it is (the predicate takes one; the kernel's bias is float32 anyway)."""
    from openpifpaf_amd import fused
    conv, xi = _conv_of(w, s, d), _image(x.to(F16))
    old, fused.GCONV_F16 = fused.GCONV_F16, True
    try:
        assert fused.gconv3x3_bf16_supported(conv, xi, bias32)
    finally:
        fused.GCONV_F16 = old
    out = fused.gconv3x3_bias_act_bf16(conv, xi, bias32, relu=relu)
    torch.cuda.synchronize()
    return out.permute(0, 2, 3, 1).reshape(-1, x.shape[3])


# (x, w, bias): float16 operands and a float32 bias whose accumulator x * w + bias is EXACT in float32 (one product of two float16s,
# one addition whose result has at most 17 significant bits), at float16's edges
EDGES = [
    (2.0, 32752.0, 0.0),                    # 65504, the largest float16
    (2.0, 32752.0, 15.0),                   # 65519 -> 65504
    (2.0, 32752.0, 16.0),                   # 65520, the tie -> even -> inf
    (-2.0, 32752.0, -16.0),                 # -65520 -> -inf (ReLU: 0)
    (2.0, 32752.0, 17.0),                   # 65521 -> inf
    (2047.0, 1.0, 0.0), (1.0, 1025.0, 0.0),                                                 # odd integers only float16 holds
    (3.0, 683.0, 0.0), (3.0, 683.0, 2.0),                                                   # 2049 -> 2048 (tie to even), 2051 -> 2052
    (2.0 ** -12, 2.0 ** -12, 0.0), (3 * 2.0 ** -12, 2.0 ** -12, 0.0), (1023 * 2.0 ** -12, 2.0 ** -12, 0.0),   # k 2^-24, subnormal results
    (2.0 ** -12, 2.0 ** -12, 2.0 ** -25), (3 * 2.0 ** -12, 2.0 ** -12, 2.0 ** -25),         # ties between subnormals: 1.5 -> 2, 3.5 -> 4 units
    (2.0 ** -12, 2.0 ** -12, -2.0 ** -25), (0.0, 1.0, 2.0 ** -25), (0.0, 1.0, 2.0 ** -25 + 2.0 ** -40),   # 0.5 -> 0, 0.5 -> 0, just above -> 1 unit
    (1024 * 2.0 ** -12, 2.0 ** -12, -2.0 ** -25),                                           # 2^-14 - 2^-25: the tie at the smallest normal
]


@pytest.mark.parametrize('c,cg', CHANNELS)
def test_the_store_at_the_edges_of_float16(c, cg):
    """Channel co takes ``EDGES[co % len(EDGES)]``: x = its first value at every pixel of that channel, a diagonal centre-tap weight
    of its second, a float32 bias of its third.  The float32 accumulator is exact (asserted in float64), so the output must be
    ``accumulator.to(torch.float16)`` as the CPU computes it, bit for bit: round to nearest even, beyond 65504 +-inf, subnormal
    results kept.  With the ReLU the negative ones are +0."""
    b, h, wd = SHAPES[1]
    rows = torch.tensor(EDGES, dtype=torch.float64)[torch.arange(c) % len(EDGES)]
    xv, wv, bv = rows[:, 0], rows[:, 1], rows[:, 2]
    for v in (xv, wv):
        assert torch.equal(v.to(F16).double(), v)
    acc64 = xv * wv + bv
    acc32 = (xv.float() * wv.float() + bv.float())
    assert torch.equal(acc32.double(), acc64) and torch.equal(bv.float().double(), bv)
    want = acc32.to(F16)                                                        # the CPU's conversion
    assert bool(want.isinf().any()) and bool(((want != 0) & (want.abs() < 2.0 ** -14)).any()) and float(want[0]) == 65504.0
    x = xv.cuda().expand(b, h, wd, c).contiguous()
    for s, d in MODES[:2]:
        m = b * _out_hw(h, wd, s)[0] * _out_hw(h, wd, s)[1]
        got = _run32(x, _diagonal(c, cg, wv.cuda()), bv.float().cuda(), s, d)
        assert torch.equal(_bits(got.cpu()), _bits(want.expand(m, c))), (s, d)
        got = _run32(x, _diagonal(c, cg, wv.cuda()), bv.float().cuda(), s, d, True)
        relued = torch.where(acc32 < 0, torch.zeros_like(acc32), acc32).to(F16)
        assert torch.equal(_bits(got.cpu()), _bits(relued.expand(m, c))), (s, d)


@pytest.mark.parametrize('c,cg', CHANNELS)
def test_subnormal_operands(c, cg):
    """A subnormal ACTIVATION 2^-20 against a weight 2^10 contributes its exact 2^-10 (the A operand's subnormals are
    kept).  A subnormal WEIGHT 2^-20 against an activation 2^10: kept (2^-10) or flushed (0) are both accepted, but the same in
    EVERY element; which one is printed."""
    b, h, wd = SHAPES[1]
    ones = torch.ones(c, dtype=torch.float64, device='cuda')
    x = (ones * 2.0 ** -20).expand(b, h, wd, c).contiguous()
    got = _run(x, _diagonal(c, cg, ones * 2.0 ** 10), None, 1, 1)
    assert torch.equal(got.double(), torch.full_like(got, 2.0 ** -10).double())
    x = (ones * 2.0 ** 10).expand(b, h, wd, c).contiguous()
    got = _run(x, _diagonal(c, cg, ones * 2.0 ** -20), None, 1, 1).double()
    kept, flushed = bool((got == 2.0 ** -10).all()), bool((got == 0).all())
    print('gconv3x3 f16 C=%d CG=%d: a subnormal weight 2^-20 against 2^10 is %s' % (c, cg, 'KEPT' if kept else 'FLUSHED' if flushed else 'MIXED'))
    assert kept or flushed


def _raw(x, w9, b32, out_ptr, b, h, wd, c, cg, s, d, relu):
    from openpifpaf_amd import _lib
    return _lib.lib().opa_gconv3x3_act_f16(
        ctypes.c_void_p(x), ctypes.c_void_p(w9.data_ptr()), ctypes.c_void_p(b32.data_ptr()) if b32 is not None else None,
        ctypes.c_void_p(out_ptr), b, h, wd, c, cg, s, d, relu, None)


@pytest.mark.parametrize('c,cg,s,d', CASES)
def test_sentinels_repeatability_relu_and_a_null_bias(c, cg, s, d):
    """The raw entry point writes into a buffer with 4096 sentinel elements on both sides, and they stay; two calls give equal bits;
    relu = 1 is ``where(out < 0, 0, out)`` of the relu = 0 result bit for bit (the select commutes with the rounding); a NULL bias is
    a zero bias bit for bit."""
    from openpifpaf_amd import fused
    pad, sentinel = 4096, 12344.0
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, c, cg, s, d)
        m = p.shape[0]
        w9, b32 = fused.gconv3x3_bf16_weight_of(_conv_of(w, s, d), bias.to(F16))
        assert tuple(w9.shape) == (c, 9, 64) and b32.dtype == torch.float32
        xb = x.to(F16).contiguous()
        outs = {}
        for name, bias_dev in (('bias', b32), ('null', None), ('zero', torch.zeros_like(b32))):
            for relu in (0, 1):
                for again in (0, 1):
                    buf = torch.full((pad + m * c + pad,), sentinel, device='cuda', dtype=F16)
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
    w9, b32 = fused.gconv3x3_bf16_weight_of(_conv_of(w, 1, 1), bias.to(F16))
    xb = x.to(F16).contiguous()
    out = torch.full((b * h * wd * c,), 12344.0, device='cuda', dtype=F16)

    def raw(x_ptr=xb.data_ptr(), out_ptr=out.data_ptr(), batch=b, hh=h, ww=wd, cc=c, width=cg, s=1, d=1):
        return _raw(x_ptr, w9, b32, out_ptr, batch, hh, ww, cc, width, s, d, 1)
    assert raw(batch=0) == 0 and raw(hh=0) == 0 and raw(ww=0) == 0
    for case in (dict(x_ptr=xb.data_ptr() + 2), dict(out_ptr=out.data_ptr() + 8), dict(x_ptr=0), dict(out_ptr=0), dict(cc=96), dict(width=12),
                 dict(cc=64, width=64), dict(s=3), dict(d=3), dict(s=2, d=2), dict(batch=-1), dict(batch=2 ** 20, hh=2 ** 10)):
        assert raw(**case) != 0, case
    torch.cuda.synchronize()
    assert (out == 12344.0).all()
