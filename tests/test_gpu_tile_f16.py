"""The float16 instantiations of the three kernels on the shared 16-bit MFMA tile (csrc/bf16_tile.hpp, ``TileElem<1>`` on
v_mfma_f32_32x32x16_f16): the 1x1 GEMM with the fused epilogue (csrc/gemm_epilogue.hip, ``opa_gemm_bias_act_f16`` /
``opa_gemm_pro_bias_act_f16``), the 3x3 implicit GEMM (csrc/conv3x3_bf16.hip, ``opa_conv3x3_act_f16``) and the block tail +
downsampling product (csrc/gemm2_bf16.hip, ``opa_gemm2_bias_act_f16``), through their ``fused`` launchers and once each through the
raw entry point.  Shapes and operand constructions are the bfloat16 twins' (``test_gpu_conv3x3_bf16.py``, ``test_gpu_gemm2_bf16.py``);
the plain GEMM runs M in {1311, 70, 9} x (K, N) in {(64, 64), (128, 192)}.

Every kernel here computes ``act(A * W^T + bias (+ residual))`` for a matrix A that it gathers itself -- rows of a matrix, nine taps
of an image, a row of the inner activation next to a strided pixel of the block's input.  Each ``_Kernel`` below gathers that A
EXPLICITLY in float64 (``cols``), so every reference is a float64 matrix product (for the 3x3: the sum of the nine taps' products),
never torch's GPU convolution.

What float16 adds to the twins' tests: known answers that bfloat16 cannot hold (odd integers above 256, bit for bit), the store at
the edges of float16's range (ties, the last finite value, the first that becomes inf, subnormal results, bit for bit against
``tensor.to(torch.float16)`` on the CPU), and what the f16 MFMA does with SUBNORMAL OPERANDS, which no document says: the test accepts
kept or flushed, the same for every element of every kernel, and prints which."""
import ctypes

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CL = torch.channels_last
F16, BF = torch.float16, torch.bfloat16
SUFFIX = {F16: '_f16', BF: '_bf16'}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _image(rows_nhwc):
    """[B, h, w, C] (contiguous) -> the [B, C, h, w] channels-last view of the same memory."""
    return rows_nhwc.contiguous().permute(0, 3, 1, 2)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


class _Kernel:
    """One launch geometry of one kernel.  ``inputs``: the shapes of the activation tensors, ``wshape`` the weight's; ``cols(*inputs)``
    -> A [M, K] and ``wmat(w)`` -> [N, K] in the operands' dtype (a gather: no arithmetic); ``run`` through the ``fused`` launcher and
    ``raw`` through the C entry point -> [M, N].  ``bias_dtype(dt)``: float32 where the kernel's bias is, else ``dt``."""
    has_residual = has_prologue = False

    def bias_dtype(self, dt):
        return torch.float32


class _Gemm(_Kernel):
    has_residual = has_prologue = True

    def __init__(self, m, k, n):
        self.m, self.k, self.n, self.id = m, k, n, 'gemm-m%d-k%d-n%d' % (m, k, n)
        self.inputs, self.wshape, self.pro_channels = [(m, k)], (n, k), k

    def bias_dtype(self, dt):
        return dt

    def cols(self, a):
        return a

    def wmat(self, w):
        return w

    def _view(self, t):
        return None if t is None else t.contiguous().view(1, t.shape[0], 1, t.shape[1]).permute(0, 3, 1, 2)    # [1, C, M, 1] channels-last

    def run(self, dt, inputs, w, bias, residual=None, relu=False, a_bias=None):
        from openpifpaf_amd import fused
        x, r = self._view(inputs[0].to(dt)), self._view(None if residual is None else residual.to(dt))
        wd, bi, ab = w.to(dt).contiguous(), bias.to(dt), None if a_bias is None else a_bias.to(dt)
        old, fused.F16 = fused.F16, True
        try:
            assert fused.conv1x1_supported(x, wd.view(self.n, self.k, 1, 1), bi, r, ab)
        finally:
            fused.F16 = old
        out = fused.conv1x1_bias_act(x, wd, bi, r, relu, ab)
        torch.cuda.synchronize()
        assert out.dtype == dt and tuple(out.shape) == (1, self.n, self.m, 1)
        return out.permute(0, 2, 3, 1).reshape(-1, self.n)

    def raw(self, dt, inputs, w, bias, residual, relu, a_bias, out_ptr):
        from openpifpaf_amd import _lib
        a, wd, bi = inputs[0].to(dt).contiguous(), w.to(dt).contiguous(), bias.to(dt)
        r = None if residual is None else residual.to(dt).contiguous()
        tail = (_ptr(wd), _ptr(bi), _ptr(r), _ptr(out_ptr), self.m, self.n, self.k, int(relu), None)
        if a_bias is None:
            return _lib.lib().opa_gemm_bias_act_f16(_ptr(a), *tail)
        ab = a_bias.to(dt)
        return _lib.lib().opa_gemm_pro_bias_act_f16(_ptr(a), _ptr(ab), *tail)


class _Conv3(_Kernel):
    has_residual = True

    def __init__(self, b, h, w, c, n, s, d):
        self.geo, self.c, self.n, self.s, self.d = (b, h, w), c, n, s, d
        self.id = 'conv3-%dx%dx%d-c%d-n%d-s%d-d%d' % (b, h, w, c, n, s, d)
        ho, wo = _out_hw(h, w, s)
        self.m, self.k, self.inputs, self.wshape = b * ho * wo, 9 * c, [(b, h, w, c)], (n, 3, 3, c)

    def cols(self, x):
        """The nine shifted views (tap 3 ky + kx; zeros in the padding) side by side: [M, 9 C], the plain definition."""
        (b, h, w), s, d = self.geo, self.s, self.d
        ho, wo = _out_hw(h, w, s)
        xp = torch.zeros((b, h + 2 * d, w + 2 * d, self.c), dtype=x.dtype, device=x.device)
        xp[:, d:d + h, d:d + w] = x
        taps = [xp[:, ky * d:ky * d + s * (ho - 1) + 1:s, kx * d:kx * d + s * (wo - 1) + 1:s] for ky in range(3) for kx in range(3)]
        return torch.cat([t.reshape(-1, self.c) for t in taps], dim=1)

    def wmat(self, w):
        return w.reshape(self.n, 9 * self.c)

    def conv(self, dt, w):
        conv = torch.nn.Conv2d(self.c, self.n, 3, self.s, self.d, dilation=self.d, bias=False).cuda().to(dt).requires_grad_(False)
        conv.weight.copy_(w.permute(0, 3, 1, 2))
        return conv

    def run(self, dt, inputs, w, bias, residual=None, relu=False, a_bias=None):
        from openpifpaf_amd import fused
        (b, h, wd), n = self.geo, self.n
        ho, wo = _out_hw(h, wd, self.s)
        conv, xi = self.conv(dt, w), _image(inputs[0].to(dt))
        bi = None if bias is None else bias.float()
        ri = None if residual is None else _image(residual.to(dt).reshape(b, ho, wo, n))
        old = fused.F16, fused.CONV3_BF16
        fused.F16 = fused.CONV3_BF16 = True
        try:
            assert fused.conv3x3_bf16_supported(conv, xi, bi, ri)
        finally:
            fused.F16, fused.CONV3_BF16 = old
        out = fused.conv3x3_bias_act_bf16(conv, xi, bi, ri, relu=relu)
        torch.cuda.synchronize()
        assert out.dtype == dt and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (b, n, ho, wo)
        return out.permute(0, 2, 3, 1).reshape(-1, n)

    def raw(self, dt, inputs, w, bias, residual, relu, a_bias, out_ptr):
        from openpifpaf_amd import _lib
        x, w9 = inputs[0].to(dt).contiguous(), w.to(dt).reshape(self.n, 9, self.c).contiguous()
        b32, r = bias.float().contiguous(), None if residual is None else residual.to(dt).contiguous()
        return _lib.lib().opa_conv3x3_act_f16(_ptr(x), _ptr(w9), _ptr(b32), _ptr(r), _ptr(out_ptr), *self.geo, self.c, self.n, self.s, self.d,
                                              int(relu), None)


class _Gemm2(_Kernel):
    def __init__(self, b, h, w, s, k1, k2, n):
        self.geo, self.s, self.k1, self.k2, self.n = (b, h, w), s, k1, k2, n
        self.id = 'gemm2-%dx%dx%d-s%d-k%d-k%d-n%d' % (b, h, w, s, k1, k2, n)
        ho, wo = _out_hw(h, w, s)
        self.m, self.k, self.wshape = b * ho * wo, k1 + k2, (n, k1 + k2)
        self.inputs = ([(self.m, k1)] if k1 else []) + [(b, h, w, k2)]
        self.has_prologue, self.pro_channels = k1 > 0, k1

    def rows(self, device):
        """The linear index of the pixel of x [B, h, w] that row m = (b * ho + oy) * wo + ox of the product reads: (b, s oy, s ox)."""
        (b, h, w), s = self.geo, self.s
        ho, wo = _out_hw(h, w, s)
        m = torch.arange(b * ho * wo, device=device)
        return (m // (ho * wo) * h + s * (m // wo % ho)) * w + s * (m % wo)

    def cols(self, *inputs):
        x = inputs[-1]
        gathered = x.reshape(-1, self.k2)[self.rows(x.device)]
        return torch.cat((inputs[0], gathered), dim=1) if self.k1 else gathered

    def wmat(self, w):
        return w

    def convs(self, dt, w):
        dconv = torch.nn.Conv2d(self.k2, self.n, 1, self.s, bias=False).cuda().to(dt).requires_grad_(False)
        dconv.weight.copy_(w[:, self.k1:].reshape(self.n, self.k2, 1, 1))
        if not self.k1:
            return None, dconv
        conv = torch.nn.Conv2d(self.k1, self.n, 1, bias=False).cuda().to(dt).requires_grad_(False)
        conv.weight.copy_(w[:, :self.k1].reshape(self.n, self.k1, 1, 1))
        return conv, dconv

    def run(self, dt, inputs, w, bias, residual=None, relu=False, a_bias=None):
        from openpifpaf_amd import fused
        assert residual is None
        (b, h, wd), n = self.geo, self.n
        ho, wo = _out_hw(h, wd, self.s)
        conv, dconv = self.convs(dt, w)
        x = _image(inputs[-1].to(dt))
        old = fused.F16, fused.PAIR_BF16
        fused.F16 = fused.PAIR_BF16 = True
        try:
            if self.k1:
                hh = _image(inputs[0].to(dt).reshape(b, ho, wo, self.k1))
                bi, ab = None if bias is None else bias.float(), None if a_bias is None else a_bias.to(dt)
                assert fused.pair_bf16_supported(conv, dconv, hh, x, bi, ab)
            else:
                assert fused.conv1x1_strided_bf16_supported(dconv, x)
        finally:
            fused.F16, fused.PAIR_BF16 = old
        if self.k1:
            out = fused.conv1x1_pair_bias_act_bf16(conv, dconv, hh, x, bi, relu, ab)
        else:
            assert bias is None and not relu
            out = fused.conv1x1_strided_bf16(dconv, x)
        torch.cuda.synchronize()
        assert out.dtype == dt and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (b, n, ho, wo)
        return out.permute(0, 2, 3, 1).reshape(-1, n)

    def raw(self, dt, inputs, w, bias, residual, relu, a_bias, out_ptr):
        from openpifpaf_amd import _lib
        a1 = inputs[0].to(dt).contiguous() if self.k1 else None
        x, wd = inputs[-1].to(dt).contiguous(), w.to(dt).contiguous()
        b32, ab = None if bias is None else bias.float().contiguous(), None if a_bias is None else a_bias.to(dt)
        return _lib.lib().opa_gemm2_bias_act_f16(_ptr(a1), self.k1, _ptr(x), self.k2, *self.geo, self.s, _ptr(ab), _ptr(wd), _ptr(b32),
                                                 _ptr(out_ptr), self.n, int(relu), None)


GEMMS = [_Gemm(m, k, n) for m in (1311, 70, 9) for k, n in ((64, 64), (128, 192))]
CONVS = [_Conv3(b, h, w, c, n, s, d) for b, h, w in ((3, 23, 19), (2, 7, 5), (1, 3, 3)) for c, n in ((64, 64), (128, 192))
         for s, d in ((1, 1), (2, 1), (1, 2), (1, 4))]
PAIRS = [_Gemm2(b, h, w, s, k1, k2, n) for b, h, w in ((3, 23, 19), (2, 7, 5)) for s in (1, 2)
         for k1, k2, n in ((64, 64, 64), (128, 192, 128), (64, 128, 192), (0, 128, 64))]
KERNELS = GEMMS + CONVS + PAIRS
ALL = [pytest.param(k, id=k.id) for k in KERNELS]
# one geometry per kernel and N-tile width for the tests whose subject is the store, not the gather
STORE = [pytest.param(k, id=k.id) for k in (GEMMS[0], GEMMS[1], GEMMS[5], CONVS[0], CONVS[5], CONVS[23], PAIRS[0], PAIRS[1], PAIRS[6], PAIRS[11])]
assert 3 * 23 * 19 == 1311 and 1311 % 128 != 0 and 3 * 12 * 10 == 360 and 360 % 128 != 0 and 2 * 7 * 5 < 128


def _seed(kernel, salt):
    return salt + sum(ord(ch) * 31 ** (i % 5) for i, ch in enumerate(kernel.id)) % (2 ** 31)


def _want(kernel, inputs, w, bias, residual=None, relu=False, a_bias=None, absolute=False):
    """The float64 reference [M, N] from float64 operands; ``absolute``: of the magnitudes (the bound's S).  With ``a_bias`` the first
    input is what the prologue makes of it, ``max(x + a_bias, 0)``, which the caller has made sure is exact in the element type."""
    inputs = [t.double() for t in inputs]
    if a_bias is not None:
        inputs[0] = (inputs[0] + a_bias.double()).clamp(min=0)
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    total = f(kernel.cols(*inputs)) @ f(kernel.wmat(w.double())).t()
    if bias is not None:
        total = total + f(bias.double())
    if residual is not None:
        total = total + f(residual.double())
    return total.clamp(min=0) if relu and not absolute else total


def _variants(kernel):
    """(with residual, relu, with prologue) that the kernel has; the strided 1x1 alone (k1 = 0) has neither bias nor ReLU."""
    if isinstance(kernel, _Gemm2) and not kernel.k1:
        return [(False, False, False)]
    return [(res, relu, pro) for res in ((False, True) if kernel.has_residual else (False,)) for relu in (False, True)
            for pro in ((False, True) if kernel.has_prologue else (False,))]


def _integer_case(kernel, bias_range, select):
    """Integer operands, asymmetric between A and W.  ``select``: row r of every input holds 1 at channel r mod C and 2 at
    (7 r + 3) mod C, the weights are integers in [-8, 8] (the twins' tap / source selection); else the inputs are in {0, 1} and the
    weights in {-1, 0, 1} (the twins' dense sums).  The bias is an integer in ``[-bias_range, bias_range]``, the residual in [-8, 8],
    ``a_bias`` in [-2, 1] (so that the prologue's ReLU cuts)."""
    g = torch.Generator(device='cuda').manual_seed(_seed(kernel, 11 + bias_range + select))
    inputs = []
    for shape in kernel.inputs:
        rows, c = int(torch.tensor(shape[:-1]).prod()), shape[-1]
        if select:
            r = torch.arange(rows, device='cuda')
            t = torch.zeros((rows, c), device='cuda', dtype=torch.float64)
            t[r, r % c] = 1.0
            t[r, (7 * r + 3) % c] = 2.0
        else:
            t = torch.randint(0, 2, (rows, c), device='cuda', generator=g).double()
        inputs.append(t.reshape(shape))
    w = torch.randint(-8, 9, kernel.wshape, device='cuda', generator=g).double() if select else \
        torch.randint(-1, 2, kernel.wshape, device='cuda', generator=g).double()
    bias = torch.randint(-bias_range, bias_range + 1, (kernel.n,), device='cuda', generator=g).double()
    res = torch.randint(-8, 9, (kernel.m, kernel.n), device='cuda', generator=g).double()
    a_bias = torch.randint(-2, 2, (kernel.pro_channels,), device='cuda', generator=g).double() if kernel.has_prologue else None
    return inputs, w, bias, res, a_bias


@pytest.mark.parametrize('select', [True, False], ids=['select', 'dense'])
@pytest.mark.parametrize('kernel', ALL)
def test_known_integers_beyond_bfloat16_bit_for_bit(kernel, select):
    """The twins' selection and dense exact-sum cases with the bias drawn from [-1000, 1000]: every product and partial sum is an
    integer of magnitude <= 2047 (asserted on the float64 reference: the 3x3 twin records 89 as the largest dense |sum|, the selection
    case stays below 9 * 24 + 8), where every integer is a float16 and every partial sum a float32 in any order -- the result must be
    that integer.  The results hold odd integers above 256 (asserted), which bfloat16 cannot: a kernel that rounded through bfloat16
    fails.  A and W differ in kind (sparse {1, 2} or {0, 1} against signed integers), so an exchanged operand or fragment order shows."""
    inputs, w, bias, res, a_bias = _integer_case(kernel, 1000, select)
    for with_res, relu, pro in _variants(kernel):
        strided_alone = isinstance(kernel, _Gemm2) and not kernel.k1
        bi = None if strided_alone else bias
        r, ab = res if with_res else None, a_bias if pro else None
        want = _want(kernel, inputs, w, bi, r, relu, ab)
        magnitude = _want(kernel, inputs, w, bi, r, False, ab, absolute=True)
        assert float(magnitude.max()) <= 2047 and torch.equal(want, want.round())
        if not strided_alone:
            odd = (want.abs() > 256) & (want.long() % 2 == 1)
            assert bool(odd.any()) and not torch.equal(want.to(BF).double(), want)
        got = kernel.run(F16, inputs, w, bi, r, relu, ab)
        assert torch.equal(_bits(got), _bits(want.to(F16))) and torch.equal(got.double(), want), (kernel.id, with_res, relu, pro)


@pytest.mark.parametrize('kernel', STORE)
def test_float16_and_bfloat16_kernels_agree_on_small_integers(kernel):
    """Operands and results that are integers of magnitude <= 256 (the dense case with the twins' bias in [-4, 4]) are exact in both
    element types: the f16 and bf16 instantiations give equal values element for element."""
    inputs, w, bias, res, a_bias = _integer_case(kernel, 4, False)
    for with_res, relu, pro in _variants(kernel):
        bi = None if isinstance(kernel, _Gemm2) and not kernel.k1 else bias
        r, ab = res if with_res else None, a_bias if pro else None
        want = _want(kernel, inputs, w, bi, r, relu, ab)
        plain = _want(kernel, inputs, w, bi, r, False, ab)
        assert float(plain.abs().max()) <= 256 and float(_want(kernel, inputs, w, bi, r, False, ab, absolute=True).max()) <= 2047
        half, brain = kernel.run(F16, inputs, w, bi, r, relu, ab), kernel.run(BF, inputs, w, bi, r, relu, ab)
        assert torch.equal(half.double(), want) and torch.equal(brain.double(), half.double()), (kernel.id, with_res, relu, pro)


def _pieces(value):
    """A float32 ``value`` as a sum of at most three NORMAL float16 numbers, exact in float32 in any order (asserted by the caller)."""
    out, rest = [], float(torch.tensor(value, dtype=torch.float32))
    while rest != 0.0 and len(out) < 3:
        piece = float(torch.tensor(max(min(rest, 65504.0), -65504.0), dtype=torch.float32).to(F16))
        out.append(piece)
        rest = float(torch.tensor(rest, dtype=torch.float32) - torch.tensor(piece, dtype=torch.float32))
    assert rest == 0.0, value
    return out


# the sums, as (what multiplies the weights: the activations' common value, [weights]): every operand is a NORMAL float16
EDGE_SUMS = [(1.0, _pieces(v)) for v in (2049.0, 2051.0, 65504.0, 65519.99, 65520.0, 1e5, -1e5)] + [
    (2.0 ** -12, [2.0 ** -12]),                              # 2^-24: the smallest subnormal
    (2.0 ** -12, [2.0 ** -13]),                              # 2^-25: a tie with zero, to even
    (2.0 ** -12, [(1 + 2.0 ** -10) * 2.0 ** -13]),           # 1.001 * 2^-25 to float16's precision: above the tie
    (2.0 ** -12, [-(2.0 ** -13)]),                           # -2^-25: -0
    (1.0, [float('inf')]), (1.0, [float('nan')])]
# ... and the literal values of the list through the float32 bias of the kernels that have one, the product being zero
EDGE_BIASES = [65519.99, 1.001 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 65520.0]


def test_the_edge_values_round_as_stated_on_the_cpu():
    """What ``tensor.to(torch.float16)`` makes of the list, the yardstick of the next test: 2048, 2052, 65504, 65504, inf, inf, -inf,
    2^-24, 0, 2^-24, -0."""
    sums = [sum(torch.tensor(a, dtype=torch.float32) * torch.tensor(p, dtype=torch.float32) for p in ws) for a, ws in EDGE_SUMS[:11]]
    got = torch.stack(sums).to(F16)
    want = torch.tensor([2048.0, 2052.0, 65504.0, 65504.0, float('inf'), float('inf'), -float('inf'), 2.0 ** -24, 0.0, 2.0 ** -24, -0.0],
                        dtype=F16)
    assert torch.equal(_bits(got), _bits(want))
    assert float(torch.tensor(65519.99, dtype=torch.float32)) == sum(_pieces(65519.99)) and len(_pieces(65519.99)) == 3


@pytest.mark.parametrize('kernel', STORE)
def test_the_store_at_the_edges_of_float16_bit_for_bit(kernel):
    """Output column j takes edge case j mod 13: channels 0 .. 2 of the activation (of the centre tap; of x for the pair kernel) hold
    the case's common value at every pixel, every other channel is zero, and row j of W holds the case's pieces in those channels --
    one-hot operands, so the float32 sum is exact and equal to the listed value whatever the order, and a non-finite weight meets no
    zero.  The result must have the bits of ``tensor.to(torch.float16)`` of that float32 sum, computed on the CPU; NaN stays NaN.
    With and without the ReLU (``where(x < 0, 0, x)`` of it: NaN stays NaN, -0 stays -0 as in the twins' select).  The activations'
    value differs between cases, so the cases of equal value share a launch: two launches per ReLU setting.  Behind them the literal
    values 65519.99 and 1.001 * 2^-25, which no sum of float16 products forms, arrive through the float32 bias of the kernels that
    have one, the product being zero."""
    for act_value in sorted({a for a, _ in EDGE_SUMS}):
        cases = [ws for a, ws in EDGE_SUMS if a == act_value]
        inputs = [torch.zeros(shape, device='cuda', dtype=torch.float64) for shape in kernel.inputs]
        inputs[-1][..., :3] = act_value
        w = torch.zeros(kernel.wshape, device='cuda', dtype=torch.float64)
        centre = w[:, 1, 1] if isinstance(kernel, _Conv3) else w[:, kernel.k - inputs[-1].shape[-1]:]
        sums = torch.zeros(kernel.n, dtype=torch.float32)
        for j in range(kernel.n):
            for i, piece in enumerate(cases[j % len(cases)]):
                centre[j, i] = piece
                sums[j] += torch.tensor(act_value, dtype=torch.float32) * torch.tensor(piece, dtype=torch.float32)
        zero_bias = None if isinstance(kernel, _Gemm2) and not kernel.k1 else torch.zeros(kernel.n, device='cuda', dtype=torch.float64)
        for relu in ((False,) if zero_bias is None else (False, True)):
            got = kernel.run(F16, inputs, w, zero_bias, None, relu)
            want32 = torch.where(sums < 0, torch.zeros_like(sums), sums) if relu else sums
            want = want32.to(F16).cuda().unsqueeze(0).expand(kernel.m, -1)
            nan = want.isnan()
            assert torch.equal(got.isnan(), nan), (kernel.id, act_value, relu)
            assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (kernel.id, act_value, relu)
    if kernel.bias_dtype(F16) == torch.float32 and not (isinstance(kernel, _Gemm2) and not kernel.k1):
        inputs = [torch.zeros(shape, device='cuda', dtype=torch.float64) for shape in kernel.inputs]
        w = torch.zeros(kernel.wshape, device='cuda', dtype=torch.float64)
        bias = torch.tensor([EDGE_BIASES[j % len(EDGE_BIASES)] for j in range(kernel.n)], dtype=torch.float32)
        for relu in (False, True):
            got = kernel.run(F16, inputs, w, bias.cuda(), None, relu)
            want32 = torch.where(bias < 0, torch.zeros_like(bias), bias) if relu else bias
            assert torch.equal(_bits(got), _bits(want32.to(F16).cuda().unsqueeze(0).expand(kernel.m, -1))), (kernel.id, relu)


_RANDOM = {}


def _random_case(kernel):
    """(inputs, w, bias, residual, a_bias) for the random case, computed once per kernel and left unchanged: float16-exact operands as
    float64.  The raw first input of the prologue is the same tensor: ``max(x + a_bias, 0)`` is rounded by the reference as
    ``opa_bias_act`` rounds it (one rounding to float16 of the float32 sum, which float64 forms exactly)."""
    if kernel.id not in _RANDOM:
        g = torch.Generator(device='cuda').manual_seed(_seed(kernel, 1))
        inputs = [torch.randn(shape, device='cuda', generator=g).to(F16).double() for shape in kernel.inputs]
        w = (torch.randn(kernel.wshape, device='cuda', generator=g) * (2.0 / kernel.k) ** 0.5).to(F16).double()
        bias = (torch.randn((kernel.n,), device='cuda', generator=g) * 0.5).to(F16).double()
        res = torch.randn((kernel.m, kernel.n), device='cuda', generator=g).to(F16).double()
        a_bias = (torch.randn((kernel.pro_channels,), device='cuda', generator=g) * 0.5).to(F16).double() if kernel.has_prologue else None
        _RANDOM[kernel.id] = (inputs, w, bias, res, a_bias)
    return _RANDOM[kernel.id]


def _staged(inputs, a_bias):
    """What the prologue stages: f16_rne(max(float32(x) + float32(a_bias), 0)) -- the float32 sum of two float16 numbers rounded to
    float32 first, then to float16, as the kernel and ``opa_bias_act`` do."""
    first = (inputs[0].float() + a_bias.float()).clamp(min=0).to(F16).double()
    return [first] + list(inputs[1:])


@pytest.mark.parametrize('kernel', ALL)
def test_random_operands_against_float64(kernel):
    """|got - want| <= E + 2^-11 (|want| + E) + 2^-25 for EVERY element: E = 2 (K + 2) 2^-24 S bounds the float32 accumulation of the
    K products, the bias and the residual in any order (u = 2^-24 per addition, doubled for adders that truncate), S = sum |a w| +
    |bias| (+ |residual|) -- the twins' bound; 2^-11 is half an ulp of float16, relative, for the one rounding; 2^-25 is half the
    subnormal spacing, for results below 2^-14; the ReLU's Lipschitz constant is 1.  The plain GEMM's bias is a float16, exact."""
    inputs, w, bias, res, a_bias = _random_case(kernel)
    for with_res, relu, pro in _variants(kernel):
        bi = None if isinstance(kernel, _Gemm2) and not kernel.k1 else bias
        r = res if with_res else None
        ref_inputs = _staged(inputs, a_bias) if pro else inputs
        want = _want(kernel, ref_inputs, w, bi, r, relu)
        sabs = _want(kernel, ref_inputs, w, bi, r, absolute=True)
        got = kernel.run(F16, inputs, w, bi, r, relu, a_bias if pro else None).double()
        e = 2.0 * (kernel.k + 2) * 2.0 ** -24 * sabs
        excess = (got - want).abs() - (e + 2.0 ** -11 * (want.abs() + e) + 2.0 ** -25)
        print('%s residual=%d relu=%d prologue=%d: max |error| %.3e, largest error - bound %.3e'
              % (kernel.id, with_res, relu, pro, float((got - want).abs().max()), float(excess.max())))
        assert float(excess.max()) <= 0.0, (kernel.id, with_res, relu, pro)


def _rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt())


@pytest.mark.parametrize('kernel', ALL)
def test_rms_error_no_worse_than_torch_float16(kernel):
    """The project's relative bar: the rms error against float64 is no more than 1.05 x that of torch's own float16 ``conv2d`` + bias
    + ReLU on the same operands (the pair: torch's two convolutions, summed by torch in float16)."""
    from torch.nn.functional import conv2d
    inputs, w, bias, _, _ = _random_case(kernel)
    alone = isinstance(kernel, _Gemm2) and not kernel.k1
    bi, relu = (None, False) if alone else (bias, True)
    ref = _want(kernel, inputs, w, bi, None, relu)
    got = kernel.run(F16, inputs, w, bi, None, relu)
    wh = w.to(F16)
    if isinstance(kernel, _Gemm):
        theirs = conv2d(kernel._view(inputs[0].to(F16)), wh.view(kernel.n, kernel.k, 1, 1), bias.to(F16))
    elif isinstance(kernel, _Conv3):
        theirs = conv2d(_image(inputs[0].to(F16)), wh.permute(0, 3, 1, 2), bias.to(F16), stride=kernel.s, padding=kernel.d, dilation=kernel.d)
    else:
        (b, h, wd), s, k1 = kernel.geo, kernel.s, kernel.k1
        theirs = conv2d(_image(inputs[-1].to(F16)), wh[:, k1:].reshape(kernel.n, kernel.k2, 1, 1), stride=s)
        if k1:
            ho, wo = _out_hw(h, wd, s)
            theirs = theirs + conv2d(_image(inputs[0].to(F16).reshape(b, ho, wo, k1)), wh[:, :k1].reshape(kernel.n, k1, 1, 1), bias.to(F16))
    theirs = (torch.relu(theirs) if relu else theirs).permute(0, 2, 3, 1).reshape(-1, kernel.n)
    e_got, e_theirs = _rms(got, ref), _rms(theirs, ref)
    print('%s: rms %.3e | torch float16 rms %.3e' % (kernel.id, e_got, e_theirs))
    assert e_got <= 1.05 * e_theirs, (kernel.id, e_got, e_theirs)


@pytest.mark.parametrize('kernel', ALL)
def test_non_finite_pixels_reach_their_windows_only(kernel):
    """One NaN element in the first row / corner pixel and one Inf element in the interior of every input: exactly the outputs whose
    row of A holds one of them are non-finite, every other output has the bits of the clean run -- the 3x3's padding and the rows
    behind M are not loaded, so nothing multiplies a zero with them.  With the ReLU the NaN stays NaN (a select)."""
    inputs, w, bias, _, _ = _random_case(kernel)
    alone = isinstance(kernel, _Gemm2) and not kernel.k1
    bi = None if alone else bias
    clean = kernel.run(F16, inputs, w, bi)
    assert clean.isfinite().all()
    special, nan_marks, marks = [], [], []
    for t in inputs:
        flat, nm, mk = t.clone().reshape(-1, t.shape[-1]), torch.zeros_like(t).reshape(-1, t.shape[-1]), torch.zeros_like(t).reshape(-1, t.shape[-1])
        flat[0, 3], nm[0, 3], mk[0, 3] = float('nan'), 1.0, 1.0
        flat[flat.shape[0] // 2, 5], mk[flat.shape[0] // 2, 5] = float('inf'), 1.0
        special.append(flat.reshape(t.shape)), nan_marks.append(nm.reshape(t.shape)), marks.append(mk.reshape(t.shape))
    held, holds_nan = kernel.cols(*marks).sum(1) > 0, kernel.cols(*nan_marks).sum(1) > 0
    assert 0 < int(held.sum()) and (int(held.sum()) < held.numel() or held.numel() <= 9) and bool(holds_nan.any())
    got = kernel.run(F16, special, w, bi)
    assert torch.equal(~got.isfinite(), held.unsqueeze(1).expand(-1, kernel.n)), kernel.id
    assert got[holds_nan].isnan().all()
    assert torch.equal(_bits(got[~held]), _bits(clean[~held])), kernel.id
    if not alone:
        with_relu = kernel.run(F16, special, w, bi, None, True)
        assert with_relu[holds_nan].isnan().all()
        assert torch.equal(_bits(with_relu[~held]), _bits(torch.where(clean < 0, torch.zeros_like(clean), clean)[~held]))


@pytest.mark.parametrize('kernel', ALL)
def test_sentinels_repeatability_and_relu(kernel):
    """The raw entry point writes into a buffer with 4096 sentinel elements on both sides, and they stay; two calls give equal bits;
    relu = 1 is ``where(out < 0, 0, out)`` of the relu = 0 result bit for bit (the select commutes with the rounding); the launcher
    hands over the same call."""
    pad, sentinel = 4096, 12345.0
    inputs, w, bias, res, a_bias = _random_case(kernel)
    alone = isinstance(kernel, _Gemm2) and not kernel.k1
    m, n, outs = kernel.m, kernel.n, {}
    for with_res, relu, pro in _variants(kernel):
        for again in (0, 1):
            buf = torch.full((pad + m * n + pad,), sentinel, device='cuda', dtype=F16)
            assert (buf.data_ptr() + pad * 2) % 16 == 0
            rc = kernel.raw(F16, inputs, w, None if alone else bias, res if with_res else None, relu, a_bias if pro else None,
                            buf.data_ptr() + pad * 2)
            torch.cuda.synchronize()
            assert rc == 0
            assert (buf[:pad] == sentinel).all() and (buf[pad + m * n:] == sentinel).all()
            out = buf[pad:pad + m * n].view(m, n).clone()
            assert torch.equal(_bits(outs.setdefault((with_res, relu, pro), out)), _bits(out))
    for (with_res, relu, pro), relued in outs.items():
        if relu:
            plain = outs[(with_res, False, pro)]
            assert plain.isfinite().all() and bool((plain < 0).any())
            assert torch.equal(_bits(relued), _bits(torch.where(plain < 0, torch.zeros_like(plain), plain)))
    first = _variants(kernel)[0]
    assert torch.equal(_bits(outs[first]), _bits(kernel.run(F16, inputs, w, None if alone else bias)))


@pytest.mark.parametrize('kernel', [pytest.param(k, id=k.id) for k in KERNELS if k.has_prologue])
def test_the_prologue_is_opa_bias_act_then_the_kernel(kernel):
    """``relu(x + a_bias)`` in float32, one rounding to float16, applied while the operand is staged: bit for bit the result of
    running ``opa_bias_act`` with dtype 1 on the operand first and then the kernel without the prologue."""
    from openpifpaf_amd import fused
    inputs, w, bias, _, a_bias = _random_case(kernel)
    fusedrun = kernel.run(F16, inputs, w, bias, None, True, a_bias)
    first = inputs[0].to(F16).reshape(-1, kernel.pro_channels).contiguous()
    staged = first.view(1, first.shape[0], 1, first.shape[1]).permute(0, 3, 1, 2)
    assert staged.is_cuda and fused.bias_act_(staged, a_bias.to(F16)) is staged
    torch.cuda.synchronize()
    assert torch.equal(first.double(), _staged(inputs, a_bias)[0].reshape(first.shape))        # (the pass itself, against the definition)
    two_steps = kernel.run(F16, [first.double().reshape(inputs[0].shape)] + list(inputs[1:]), w, bias, None, True)
    assert torch.equal(_bits(fusedrun), _bits(two_steps)), kernel.id


def test_subnormal_float16_operands_one_answer_for_every_kernel():
    """x = 2^-20 -- a SUBNORMAL float16 -- in every activation element, w = 2^10, products exactly 2^-10: the documents say that the
    MFMA's C/D never flush and that float32 inputs follow the mode, and nothing about 16-bit inputs.  Either answer is accepted -- the
    exact one (row sum of A's non-zero elements x 2^-10, the bias none) or the flushed one (the contribution missing: zero) -- but the
    SAME one for every element of every kernel; it is printed, and DESIGN.md records it.  (Subnormal RESULTS are another matter: they
    must be exact, ``test_the_store_at_the_edges_of_float16_bit_for_bit``.)"""
    findings = {}
    for kernel in (GEMMS[0], GEMMS[5], CONVS[0], CONVS[5], CONVS[23], PAIRS[0], PAIRS[6], PAIRS[11]):
        inputs = [torch.full(shape, 2.0 ** -20, device='cuda', dtype=torch.float64) for shape in kernel.inputs]
        assert all(torch.equal(t.to(F16).double(), t) for t in inputs)
        w = torch.full(kernel.wshape, 2.0 ** 10, device='cuda', dtype=torch.float64)
        zero = None if isinstance(kernel, _Gemm2) and not kernel.k1 else torch.zeros(kernel.n, device='cuda', dtype=torch.float64)
        got = kernel.run(F16, inputs, w, zero)
        exact = _want(kernel, inputs, w, zero).to(F16)           # taps inside the image x c_in x 2^-10 <= 1152 x 2^-10: exact in float16
        assert torch.equal(exact.double(), _want(kernel, inputs, w, zero))
        kept, flushed = torch.equal(_bits(got), _bits(exact)), bool((got == 0).all())
        assert kept != flushed, (kernel.id, got.flatten()[:8])
        findings[kernel.id] = 'kept' if kept else 'flushed'
    print('v_mfma_f32_32x32x16_f16 with subnormal float16 A operands: %s' % sorted(set(findings.values())), findings)
    assert len(set(findings.values())) == 1, findings
