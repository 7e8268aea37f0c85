"""Every leaf of the three GEMM families' launch dispatch once, through the Python launchers, against exact expectations:
csrc/gemm_epilogue.hip (bfloat16) and csrc/gemm_f32.hip (float32 MFMA), ``<BN, RES, RELU, PRO>`` each, and csrc/gemm_f32x3.hip's
``launch_x3`` -- plain, pair and taps over both term counts, and the unit mode's thirteen (third operand, activation) combinations.
The kernels are the same bytes whatever the host code around them looks like (``tools/kernel_fingerprint.py``); what this file
checks is the MAPPING of run-time arguments onto them: a flag that reaches the wrong template parameter, a mode whose
``X3Second`` fields are not filled, a swapped activation.

Operands are integers, so every expected value is exact and the comparison is ``torch.equal`` against an int64 computation
(hardswish, whose division need not be correctly rounded, within one float32 ulp of the float64 value).  Every case first asserts
that its own variants -- with and without residual, ReLU, prologue; the activation codes -- have DIFFERENT expected tensors, so
that a launch that took another leaf cannot pass.  Integers cannot tell six terms from nine: ``test_terms_*`` does, with one
product whose seventh-to-ninth piece products sum to 2^-27.

What no result shows is the tile width BN: a 64-wide and a 128-wide tile compute the same numbers.  N = 64 can only take the
64-wide tile, N = 128 takes the 128-wide one by the two rules that stand as one line each in ``launch_x3`` (plain
``N % 128 == 0``; unit ``N % 128 == 0 && terms == 6``) and in the other two files' launchers; both widths run here.

M = 129 is one full 128-row tile and a one-row tile, K = 64 two K-steps -- the whole peeled loop of a block tail."""
import contextlib
import functools
import itertools

import pytest

torch = pytest.importorskip('torch')

import x3_common as xc  # noqa: E402

gpu = pytest.mark.gpu
CL = torch.channels_last
HW = (3, 43)                                    # M = 129 pixels of one image
SLOPE, CAP = 0.25, 3.0                          # exact on integers: a quarter, and a cap that is one
SIX, NINE = float.fromhex('0x1.81p-9'), float.fromhex('0x1.81004p-9')


# ---- expectations (CPU, int64) ------------------------------------------------------------------------------------------------------

def _product(a, w, bias, res=None, a_bias=None):
    """``[M, K] x [N, K]`` integers as float32 -> int64 ``[M, N]`` before the activation."""
    a = a.long()
    if a_bias is not None:
        a = (a + a_bias.long()).clamp_min(0)
    out = a @ w.long().t() + bias.long()
    return out if res is None else out + res.long()


def _all_different(tensors, what):
    for (i, s), (j, t) in itertools.combinations(enumerate(tensors), 2):
        assert not torch.equal(s, t), '%s: variants %d and %d expect the same tensor' % (what, i, j)


def _activated(pre, act):
    """int64 pre-activation -> the exact expectation in float64 (hardswish: the float64 value of x clamp(x + 3, 0, 6) / 6)."""
    x = pre.double()
    if act == 0:
        return x
    if act == 1:
        return x.clamp_min(0)
    if act == 2:
        return x * (x + 3).clamp(0, 6) / 6
    return torch.where(x < 0, x * SLOPE, x) if act == 3 else x.clamp(0, CAP)


def _assert_result(got, want64, act, what):
    if act != 2:
        want = want64.float()
        assert torch.equal(want.double(), want64), what + ': the expectation is not a float32 number'
        assert torch.equal(got, want), '%s: %d elements differ' % (what, int((got != want).sum()))
        return
    _, e = torch.frexp(want64)                                              # |want| in [2^(e-1), 2^e): a float32 ulp is 2^(e-24)
    ulp = torch.where(want64 == 0, torch.zeros_like(want64), torch.exp2(e.double() - 24))
    worst = ((got.double() - want64).abs() - ulp).max()
    assert worst <= 0, '%s: hardswish is %g beyond one ulp' % (what, float(worst))


def _both_signs(pre, beyond=0):
    return bool((pre < -beyond).any()) and bool((pre > beyond).any())


# ---- operands --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _plain_problem(n, small):
    """M = 129, K = 64 -> (a, w, bias, res, a_bias), integers as float32.  ``small`` (the bfloat16 family): every stored value is a
    bfloat16 integer -- |a| <= 7, |a_bias| <= 3, four weights of |w| <= 3 per row, |bias| <= 31, |res| <= 63: an output is at most
    4 x 10 x 3 + 31 + 63 = 214 <= 256.  Otherwise ``xc.integer_problem``'s budget: 9-bit operands, 32 weights per row, below 2^24."""
    g = xc.gen(7 + n + small)
    m, k = HW[0] * HW[1], 64
    if small:
        a, w = xc.integers((m, k), g, 3), xc.sparse_integer_weight(n, k, g, bits=2, nnz=4)
        bias, res, a_bias = xc.integers((n,), g, 5), xc.integers((m, n), g, 6), xc.integers((k,), g, 2)
    else:
        a, w = xc.integers((m, k), g, 9), xc.sparse_integer_weight(n, k, g)
        bias, res, a_bias = xc.integers((n,), g, 20), xc.integers((m, n), g, 20), xc.integers((k,), g, 8)
    assert bool(res.any()) and bool(a_bias.any())
    return a, w, bias, res, a_bias


def _image(rows, b=1, hw=HW, dtype=torch.float32):
    """``[M, C]`` -> ``[B, C, H, W]`` channels_last on the GPU."""
    return xc.image_of(rows, b, *hw).to(dtype).cuda().contiguous(memory_format=CL)


@contextlib.contextmanager
def _terms(terms):
    from openpifpaf_amd import fused
    old, fused.X3_TERMS = fused.X3_TERMS, terms
    try:
        yield
    finally:
        fused.X3_TERMS = old


def _conv(w4d, stride=1, padding=0, dilation=1, bias=None):
    n, c, k, _ = w4d.shape
    conv = torch.nn.Conv2d(c, n, k, stride, padding, dilation, bias=bias is not None).cuda().requires_grad_(False)
    conv.weight.copy_(w4d)
    if bias is not None:
        conv.bias.copy_(bias)
    return conv


def _rows(out):
    torch.cuda.synchronize()
    assert out.is_contiguous(memory_format=CL)
    return xc.rows_of(out.float().cpu())


# ---- <BN, RES, RELU, PRO>: the bfloat16 and the float32 MFMA GEMM, the split-operand GEMM with six and nine terms ---------------------------

FLAGS = list(itertools.product((False, True), repeat=3))                    # (res, relu, pro)


@gpu
@pytest.mark.parametrize('n', [64, 128])
@pytest.mark.parametrize('family', ['bf16', 'f32', 'x3-6', 'x3-9'])
def test_plain_leaves(family, n):
    from openpifpaf_amd import fused
    a, w, bias, res, a_bias = _plain_problem(n, family == 'bf16')
    dtype = torch.bfloat16 if family == 'bf16' else torch.float32
    pres = [_product(a, w, bias, res if r else None, a_bias if p else None) for r, _, p in FLAGS]
    assert all(_both_signs(pre) for pre in pres)
    wants = [_activated(pre, int(relu)) for pre, (_, relu, _) in zip(pres, FLAGS)]
    _all_different(wants, family)
    if family == 'bf16':
        assert max(float(t.abs().max()) for t in pres) <= 256
    x, r_d = _image(a, dtype=dtype), _image(res, dtype=dtype)
    w_d, bias_d, ab_d = w.to(dtype).cuda(), bias.to(dtype).cuda(), a_bias.to(dtype).cuda()
    w3 = fused.split_weight(w_d) if family.startswith('x3') else None
    assert fused.conv1x1_supported(x, w_d, bias_d, r_d, ab_d)
    with torch.no_grad():
        for (with_res, relu, pro), want in zip(FLAGS, wants):
            rest = (bias_d, r_d if with_res else None, relu, ab_d if pro else None)
            if w3 is None:
                out = fused.conv1x1_bias_act(x, w_d, *rest)
            else:
                out = fused.conv1x1_bias_act_x3(x, w3, *rest, int(family[3:]))
            assert out.dtype == dtype and tuple(out.shape) == (1, n) + HW
            _assert_result(_rows(out), want, int(relu), '%s N %d res %d relu %d pro %d' % (family, n, with_res, relu, pro))


# ---- the pair: two activations along K, no residual ---------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('n', [64, 128])
def test_pair_leaves(n, stride, terms):
    from openpifpaf_amd import fused
    spec = ('pair', 32, 32, n, stride)                                      # k1 = k2 = 32 on a 3 x 9 x 7 input
    variants = list(itertools.product((False, True), repeat=2))             # (relu, pro)
    problems = {pro: xc.integer_problem(spec, 11 + n + stride, False, pro) for pro in (False, True)}
    wants = []
    for relu, pro in variants:
        _, a, w, bias, _, a_bias = problems[pro]
        pre = _product(a, w, bias, None, None if a_bias is None else xc.prologue_bias(spec, a_bias))
        assert _both_signs(pre) and (a_bias is None or bool(a_bias.any()))
        wants.append(_activated(pre, int(relu)))
    _all_different(wants, 'pair')
    with torch.no_grad(), _terms(terms):
        for (relu, pro), want in zip(variants, wants):
            nat, _, w, bias, _, a_bias = problems[pro]
            conv, dconv = _conv(w[:, :32].reshape(n, 32, 1, 1)), _conv(w[:, 32:].reshape(n, 32, 1, 1), stride)
            h, x, bias_d = nat[0].cuda().contiguous(memory_format=CL), nat[1].cuda().contiguous(memory_format=CL), bias.cuda()
            ab = None if a_bias is None else a_bias.cuda()
            assert fused.pair_supported(conv, dconv, h, x, bias_d, ab)
            out = fused.conv1x1_pair_bias_act_x3(conv, dconv, h, x, bias_d, relu, ab)
            _assert_result(_rows(out), want, int(relu), 'pair N %d stride %d terms %d relu %d pro %d' % (n, stride, terms, relu, pro))


# ---- taps: the three launchers that fill X3Second for an implicit GEMM ----------------------------------------------------------------------

# (launcher, input [B, C, H, W], kernel, stride, padding, dilation)
TAPS = {'conv3x3-s2': ('conv3x3_bias_act_x3', (1, 64, 5, 5), 3, 2, 1, 1),
        'conv3x3-d2': ('conv3x3_dilated_bias_act_x3', (1, 64, 5, 5), 3, 1, 2, 2),
        'stem7x7': ('stem7x7_bias_act_x3', (2, 3, 9, 9), 7, 2, 3, 1)}


@gpu
@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('n', [64, 128])
@pytest.mark.parametrize('which', sorted(TAPS))
def test_taps_leaves(which, n, terms):
    from openpifpaf_amd import fused
    launcher, shape, ksize, stride, padding, dilation = TAPS[which]
    g = xc.gen(23 + n)
    x = xc.integers(shape, g, 9)
    w4d = xc.sparse_integer_weight(n, shape[1] * ksize * ksize, g).reshape(n, shape[1], ksize, ksize)
    bias = xc.integers((n,), g, 20)
    cols = torch.nn.functional.unfold(x, ksize, dilation, padding, stride)  # [B, C k k, pixels], zeros in the padding
    pre = _product(cols.transpose(1, 2).reshape(-1, cols.shape[1]), w4d.reshape(n, -1), bias)
    assert _both_signs(pre)
    conv, bias_d = _conv(w4d, stride, padding, dilation), bias.cuda()
    x_d = x.cuda() if which == 'stem7x7' else x.cuda().contiguous(memory_format=CL)
    supported = {'conv3x3-s2': fused.conv3x3_x3_supported, 'conv3x3-d2': fused.conv3x3_dilated_x3_supported,
                 'stem7x7': fused.stem_x3_supported}[which]
    with torch.no_grad(), _terms(terms):
        assert supported(conv, x_d, bias_d)
        for relu in (False, True):
            out = getattr(fused, launcher)(conv, x_d, bias_d, relu)
            assert out.shape[1] == n and out.shape[0] * out.shape[2] * out.shape[3] == pre.shape[0]
            _assert_result(_rows(out), _activated(pre, int(relu)), int(relu), '%s N %d terms %d relu %d' % (which, n, terms, relu))


# ---- the unit mode: thirteen combinations of third operand and activation code ---------------------------------------------------------------

UNIT_ACTS = {'none': (0, 1, 2, 3, 4), 'partner': (0, 1, 2, 3, 4), 'residual': (0, 1, 2)}


@gpu
@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('k,n', [(6, 10), (72, 128)])
def test_unit_leaves(k, n, terms):
    from openpifpaf_amd import _lib, fused
    g = xc.gen(31 + n)
    m = HW[0] * HW[1]
    # 5-bit activations, 3-bit weights, every column in use: |sum| < 72 x 31 x 7 < 2^14; small enough for hardswish's products too
    a, w, bias = xc.integers((m, k), g, 5), xc.integers((n, k), g, 3), xc.integers((n,), g, 8)
    third = xc.integers((m, n), g, 10)
    assert bool(third.any())
    conv, x, third_d = _conv(w.reshape(n, k, 1, 1), bias=bias), _image(a), _image(third)
    with torch.no_grad():
        for kind, acts in UNIT_ACTS.items():
            pre = _product(a, w, bias, third if kind == 'residual' else None)
            assert _both_signs(pre, beyond=CAP)
            wants = [_activated(pre, act) for act in acts]
            _all_different(wants, 'unit ' + kind)
            extra = {} if kind == 'none' else {kind: third_d}
            assert fused.unit_conv_x3_supported(conv, x, **extra)
            for act, want in zip(acts, wants):
                what = 'unit K %d N %d terms %d %s act %d' % (k, n, terms, kind, act)
                out = fused.conv1x1_unit_x3(conv, x, act=act, terms=terms, act_param={3: SLOPE, 4: CAP}.get(act, 0.0), **extra)
                rows = _rows(out)
                if kind == 'partner':                                       # channel_shuffle(cat((partner, y), 1), 2)
                    assert tuple(out.shape) == (1, 2 * n) + HW
                    assert torch.equal(rows[:, 0::2], third), what + ': the partner did not pass through'
                    rows = rows[:, 1::2]
                else:
                    assert tuple(out.shape) == (1, n) + HW
                _assert_result(rows.contiguous(), want, act, what)
        for act, param in ((3, SLOPE), (4, CAP)):                           # no instantiation: refused, nothing launched
            with pytest.raises(_lib.NativeError):
                fused.conv1x1_unit_x3(conv, x, act=act, terms=terms, act_param=param, residual=third_d)
        torch.cuda.synchronize()


# ---- six terms or nine ----------------------------------------------------------------------------------------------------------------------

def _terms_probe(n, k=64):
    """(1 + 2^-9 + 2^-18) (1 + 2^-10 + 2^-19) - 1 in every element: the leading product cancels against -1 x 1, the six kept
    corrections sum to 0x1.81p-9, the three that six terms drop (a2 w3 + a3 w2 = 2^-27, a3 w3 = 2^-37: below the sum's last bit)
    add exactly 2^-27."""
    a, w = torch.zeros((HW[0] * HW[1], k)), torch.zeros((n, k))
    a[:, 0], a[:, 1] = 1 + 2.0 ** -9 + 2.0 ** -18, -1.0
    w[:, 0], w[:, 1] = 1 + 2.0 ** -10 + 2.0 ** -19, 1.0
    return a, w


def test_terms_probe_model():
    """The probe's two values follow from the kernel's arithmetic as ``x3_common.model_f32`` restates it."""
    a, w = _terms_probe(2)
    assert NINE - SIX == 2.0 ** -27
    for terms, value in ((6, SIX), (9, NINE)):
        assert torch.equal(xc.model_f32(a[:3], w, terms), torch.full((3, 2), value))


@gpu
@pytest.mark.parametrize('n', [64, 128])
@pytest.mark.parametrize('kernel', ['plain', 'unit'])
def test_terms_reach_the_kernel(kernel, n):
    from openpifpaf_amd import fused
    a, w = _terms_probe(n)
    x = _image(a)
    with torch.no_grad():
        for terms, value in ((6, SIX), (9, NINE)):
            if kernel == 'plain':
                out = fused.conv1x1_bias_act_x3(x, fused.split_weight(w.cuda()), torch.zeros(n, device='cuda'), None, False, None, terms)
            else:
                out = fused.conv1x1_unit_x3(_conv(w.reshape(n, 64, 1, 1)), x, relu=False, terms=terms)
            assert torch.equal(_rows(out), torch.full((a.shape[0], n), value)), '%s N %d terms %d' % (kernel, n, terms)
