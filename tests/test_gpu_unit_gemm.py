"""The unit mode of the split-operand GEMM (csrc/gemm_f32x3.hip, ``opa_gemm_unit_bias_act_f32x3``): the 1x1 convolutions of the
ShuffleNetV2K units -- any even K and N, the operand a channel slice of a wider tensor, the result stored dense or into its
shuffled position next to a partner that the same kernel copies.  Kernel level, real widths (k16: 24 / 174 / 348 / 696 / 1392,
k30: 32 / 256, a head: 340), ``M = 3 x 23 x 19`` (no multiple of the 128-row tile), inputs as in ``test_gpu_gemm_x3.py``."""
import ctypes

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CL = torch.channels_last
B, H, W = 3, 23, 19
M = B * H * W
SHAPES = [(174, 174), (348, 348), (696, 696), (24, 174), (1392, 1392), (256, 256), (32, 256), (1392, 340)]
SENTINEL = 12345.5
assert M % 128 != 0


def _conv(k, n, seed=3):
    """-> (conv with the weights of ``test_gpu_gemm_x3._case``, a post-ReLU activation [B, k, H, W] channels_last)."""
    torch.manual_seed(seed)
    x = torch.randn(B, k, H, W, device='cuda').clamp_(min=0).contiguous(memory_format=CL)
    conv = torch.nn.Conv2d(k, n, 1).cuda().requires_grad_(False)
    conv.weight.copy_((torch.randn(n, k, device='cuda') * (2.0 / k) ** 0.5).view(n, k, 1, 1))
    conv.bias.copy_(torch.randn(n, device='cuda') * 0.1)
    return conv, x


def _call(conv, a_ptr, a_pitch, out_ptr, partner_ptr=None, partner_pitch=0, relu=1, terms=6, m=M, n=None, k=None):
    """The C entry point, raw -> its return code."""
    from openpifpaf_amd import _lib, fused
    w3, bp = fused._unit_weight_of(conv)
    rc = _lib.lib().opa_gemm_unit_bias_act_f32x3(
        ctypes.c_void_p(a_ptr), a_pitch, ctypes.c_void_p(w3.data_ptr()), ctypes.c_void_p(bp.data_ptr()),
        ctypes.c_void_p(partner_ptr) if partner_ptr else None, partner_pitch, ctypes.c_void_p(out_ptr),
        m, conv.out_channels if n is None else n, conv.in_channels if k is None else k, relu, terms, None)
    torch.cuda.synchronize()
    return rc


def _dense(conv, x, terms):
    """The dense mode on a dense operand -> [M, N]."""
    out = torch.empty((M, conv.out_channels), device='cuda')
    assert _call(conv, x.data_ptr(), conv.in_channels, out.data_ptr(), terms=terms) == 0
    return out


def _rows(t):
    """[B, C, H, W] -> [M, C] (values)."""
    return t.permute(0, 2, 3, 1).reshape(M, t.shape[1])


def _errors(got, ref):
    d = got.double() - ref
    scale = float(ref.abs().max())
    return float((d * d).mean().sqrt()) / scale, float(d.abs().max()) / scale


def _half_of(t, half, fill=float('nan')):
    """``t`` [B, C, H, W] as the first (0) / second (1) half of the channels of a [B, 2C, H, W] channels-last tensor whose other half
    holds ``fill``."""
    c = t.shape[1]
    big = torch.full((B, 2 * c, H, W), fill, device='cuda').contiguous(memory_format=CL)
    view = big[:, half * c:(half + 1) * c]
    view.copy_(t)
    assert view.data_ptr() == big.data_ptr() + half * c * 4 and not view.is_contiguous(memory_format=CL)
    return view


@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('k,n', SHAPES)
def test_against_float64_and_torch_float32(k, n, terms):
    """rms < 2e-7 and max < 2e-6 of max |ref| (the bars ``test_gpu_gemm_x3.py`` holds this kernel to), and the rms no more than
    1.05 x that of torch's own float32 convolution on the same dense operands + 1e-9."""
    conv, x = _conv(k, n)
    got = _dense(conv, x, terms)
    ref = _rows(torch.nn.functional.conv2d(x.double(), conv.weight.double(), conv.bias.double()).clamp_(min=0))
    theirs = _rows(torch.relu(torch.nn.functional.conv2d(x, conv.weight, conv.bias)))
    e_got, e_theirs = _errors(got, ref), _errors(theirs, ref)
    print('unit gemm K=%d N=%d terms=%d: rms %.3e max %.3e | torch float32 rms %.3e max %.3e' % ((k, n, terms) + e_got + e_theirs))
    assert e_got[0] < 2e-7 and e_got[1] < 2e-6, e_got
    assert e_got[0] <= 1.05 * e_theirs[0] + 1e-9, (e_got, e_theirs)


@pytest.mark.parametrize('half', [1, 0], ids=['second-half', 'first-half'])
@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('k,n', SHAPES)
def test_operand_as_a_channel_slice_next_to_nan(k, n, terms, half):
    """The operand as one half of the channels of a wider tensor whose other half is NaN: finite, and bit for bit the result from a
    dense copy of the slice (the K tail: what lies behind column K of a row is the next pixel or this pixel's other half; k16's
    stage-2 slice starts 696 bytes into the pixel, 8 bytes off a 16-byte boundary)."""
    from openpifpaf_amd import fused
    conv, x = _conv(k, n)
    old, fused.X3_TERMS = fused.X3_TERMS, terms
    try:
        view = _half_of(x, half)
        assert fused.unit_conv_x3_supported(conv, view) and fused._pixel_stride(view) == 2 * k
        got = fused.conv1x1_unit_x3(conv, view)
        want = fused.conv1x1_unit_x3(conv, x)
    finally:
        fused.X3_TERMS = old
    assert tuple(got.shape) == (B, n, H, W) and got.is_contiguous(memory_format=CL)
    assert got.isfinite().all()
    assert torch.equal(got, want)
    assert torch.equal(_rows(want), _dense(conv, x, terms))


@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('k,n', SHAPES)
def test_dense_store_stays_inside_its_rows(k, n, terms):
    """The output lives inside a larger buffer filled with a sentinel: nothing outside [M, N] is written (the row pitch is N: a
    store one column too far lands in the next pixel, which the comparison with the plain call sees)."""
    conv, x = _conv(k, n)
    pad = 4096
    buf = torch.full((pad + M * n + pad,), SENTINEL, device='cuda')
    assert (buf.data_ptr() + pad * 4) % 16 == 0
    assert _call(conv, x.data_ptr(), k, buf.data_ptr() + pad * 4, terms=terms) == 0
    assert (buf[:pad] == SENTINEL).all() and (buf[pad + M * n:] == SENTINEL).all()
    assert torch.equal(buf[pad:pad + M * n].view(M, n), _dense(conv, x, terms))


@pytest.mark.parametrize('partner_half', [0, 1], ids=['partner-first-half', 'partner-second-half'])
@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('k,n', SHAPES)
def test_interleaved_store_with_a_partner(k, n, terms, partner_half):
    """out[m, 2c] = partner[m, c] bit for bit (the partner a slice with NaN neighbours, some of its own values NaN and -0.0),
    out[m, 2c + 1] = the dense-mode result of the same operands bit for bit; the sentinel outside [M, 2N] is untouched."""
    conv, x = _conv(k, n)
    torch.manual_seed(7)
    p = torch.randn(B, n, H, W, device='cuda')
    p[0, 0, 0, 0], p[1, n - 1, 2, 3], p[2, 1, H - 1, W - 1] = float('nan'), -0.0, float('inf')
    partner = _half_of(p, partner_half)
    pad = 4096
    buf = torch.full((pad + M * 2 * n + pad,), SENTINEL, device='cuda')
    assert _call(conv, x.data_ptr(), k, buf.data_ptr() + pad * 4, partner.data_ptr(), 2 * n, terms=terms) == 0
    assert (buf[:pad] == SENTINEL).all() and (buf[pad + M * 2 * n:] == SENTINEL).all()
    out = buf[pad:pad + M * 2 * n].view(M, n, 2)
    assert torch.equal(out[:, :, 0].contiguous().view(torch.int32), _rows(p).contiguous().view(torch.int32))
    assert torch.equal(out[:, :, 1], _dense(conv, x, terms))
    # ... and through the Python launcher: channel_shuffle(cat((partner, y), 1), 2), channels_last
    from openpifpaf_amd import fused
    old, fused.X3_TERMS = fused.X3_TERMS, terms
    try:
        assert fused.unit_conv_x3_supported(conv, x, partner)
        got = fused.conv1x1_unit_x3(conv, x, partner=partner)
    finally:
        fused.X3_TERMS = old
    assert tuple(got.shape) == (B, 2 * n, H, W) and got.is_contiguous(memory_format=CL)
    assert torch.equal(_rows(got).contiguous().view(torch.int32), out.reshape(M, 2 * n).contiguous().view(torch.int32))


# (K, N) multiples of 64 and the terms with which both kernels take the same tile width: N_pad % 128 == 0 -> 128 with six terms
# in both; with nine terms the unit mode takes 64 everywhere (no scratch), the plain kernel 64 only where N % 128 != 0
@pytest.mark.parametrize('k,n,terms', [(256, 256, 6), (64, 192, 6), (64, 192, 9), (128, 64, 6), (128, 64, 9), (1408, 320, 9), (512, 512, 6)])
def test_same_bits_as_the_plain_kernel_on_its_own_shapes(k, n, terms):
    """Dense, 16-byte aligned, multiples of 64: the same products in the same order as ``fused.conv1x1_bias_act_x3``."""
    from openpifpaf_amd import fused
    conv, x = _conv(k, n)
    w3 = fused.split_weight(conv.weight.reshape(n, k))
    for relu in (True, False):
        want = fused.conv1x1_bias_act_x3(x, w3, conv.bias, None, relu, None, terms)
        got = torch.empty((M, n), device='cuda')
        assert _call(conv, x.data_ptr(), k, got.data_ptr(), relu=int(relu), terms=terms) == 0
        assert torch.equal(got, _rows(want))


def test_rejects_what_it_cannot_run():
    from openpifpaf_amd import _lib
    conv, x = _conv(174, 174)
    out = torch.full((M * 2 * 174 + 8,), SENTINEL, device='cuda')
    partner = torch.zeros((M, 174), device='cuda')
    a, o, p = x.data_ptr(), out.data_ptr(), partner.data_ptr()
    assert _call(conv, a, 174, o, m=0) == 0                        # OPA_OK, nothing to do
    bad = [dict(n=173), dict(k=173), dict(a_pitch=172), dict(a_pitch=175), dict(terms=7), dict(terms=0), dict(m=2 ** 31),
           dict(a_ptr=a + 4), dict(out_ptr=o + 8), dict(partner_ptr=p, partner_pitch=172), dict(partner_ptr=p, partner_pitch=175),
           dict(partner_ptr=p + 4, partner_pitch=174), dict(m=-1)]
    for case in bad:
        args = dict(a_ptr=a, a_pitch=174, out_ptr=o)
        args.update(case)
        assert _call(conv, **args) != 0, case
    from openpifpaf_amd import fused
    w3, bp = fused._unit_weight_of(conv)
    lib = _lib.lib()

    def raw(w_ptr, b_ptr):
        return lib.opa_gemm_unit_bias_act_f32x3(ctypes.c_void_p(a), 174, ctypes.c_void_p(w_ptr), ctypes.c_void_p(b_ptr), None, 0,
                                                ctypes.c_void_p(o), M, 174, 174, 1, 6, None)
    assert raw(w3.data_ptr() + 8, bp.data_ptr()) != 0 and raw(w3.data_ptr(), bp.data_ptr() + 8) != 0
    assert raw(None, bp.data_ptr()) != 0 and raw(w3.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                 # nothing was launched
