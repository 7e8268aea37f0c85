"""Variant 4 of csrc/winograd.hip on the GPU (F(2x2, 3x3) on the bf16 MFMA pipe with exactly split operands): against a float64
convolution (max error below 2e-5 of the output's largest magnitude, rms at most 1.25x variant 2's on the same inputs), both
workgroup orders, ragged sizes, bias + ReLU, the whole trunk against the variant-2 trunk, and the C ABI's refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 64, 8, 8), (2, 32, 64, 7, 9), (3, 64, 128, 21, 21), (2, 64, 64, 41, 40), (1, 128, 128, 5, 3),
          (1, 16, 64, 1, 1), (5, 48, 192, 16, 13)]


def _inputs(B, C, O, H, W, bias, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, C, H, W), generator=g).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn((O, C, 3, 3), generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()
    b = torch.randn((O,), generator=g).cuda() if bias else None
    return x, w, b


def _errors(y, x, w, b, relu):
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double() if b is not None else None, padding=1)
    if relu:
        ref = ref.relu()
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    d = y.double() - ref
    scale = ref.abs().max().item()
    return d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / scale


def _case(B, C, O, H, W, order, bias=False, relu=False, seed=0):
    from openpifpaf_amd import winograd
    x, w, b = _inputs(B, C, O, H, W, bias, seed)
    y4 = winograd.conv3x3_x3(x, winograd.split_filter(w), O, bias=b, relu=relu, order=order)
    y2 = winograd.conv3x3(x, winograd.transform_filter(w, 2), O, bias=b, relu=relu, variant=2, order=order)
    return _errors(y4, x, w, b, relu), _errors(y2, x, w, b, relu)


@pytest.mark.parametrize('shape', SHAPES)
def test_variant4_equals_the_convolution(shape):
    for order in (0, 1):
        (max4, rms4), (_, rms2) = _case(*shape, order)
        assert max4 < 2e-5, (shape, order, max4)
        assert rms4 <= 1.25 * rms2, (shape, order, rms4, rms2)


@pytest.mark.parametrize('bias,relu', [(True, True), (True, False), (False, True)])
def test_variant4_bias_and_relu(bias, relu):
    for order in (0, 1):
        (max4, rms4), (_, rms2) = _case(2, 32, 64, 11, 13, order, bias=bias, relu=relu, seed=3)
        assert max4 < 2e-5 and rms4 <= 1.25 * rms2, (order, max4, rms4, rms2)


def test_variant4_bad_arguments_and_unknown_variants_are_refused():
    from openpifpaf_amd import winograd
    x, w, _ = _inputs(1, 32, 64, 8, 8, False, 5)
    u3 = winograd.split_filter(w)
    u = winograd.transform_filter(w, 2)
    with pytest.raises(Exception):                   # c_in not a multiple of 16
        winograd.conv3x3_x3(x[:, :24].contiguous(memory_format=torch.channels_last), u3, 64)
    with pytest.raises(Exception):                   # c_out not a multiple of 64
        winograd.conv3x3_x3(x, u3, 32)
    for variant in (0, 2, 3, 5, 11, 24):             # the split-operand entry runs variant 4 only
        with pytest.raises(Exception):
            winograd.conv3x3_x3(x, u3, 64, variant=variant)
    for variant in (4, 5, 21):                       # the float32 entry refuses what it cannot run
        with pytest.raises(Exception):
            winograd.conv3x3(x, u, 64, variant=variant)
    torch.cuda.synchronize()
    assert winograd.conv3x3_x3(x, u3, 64).isfinite().all()     # (and the library still works)


def _trunk_pair(name, batch, seed):
    from openpifpaf_amd import network, winograd
    net = network.optimize_for_inference_(network.factory(name)).cuda().to(memory_format=torch.channels_last)
    x = torch.randn((batch, 3, 321, 321), generator=torch.Generator().manual_seed(seed)).cuda().contiguous(memory_format=torch.channels_last)
    old_mode, old_x3 = winograd.set_mode('winograd'), winograd.X3
    try:
        with torch.no_grad():
            winograd.X3 = True
            a = net(x)
            winograd.X3 = False
            b = net(x)
    finally:
        winograd.set_mode(old_mode)
        winograd.X3 = old_x3
    for fa, fb in zip(a, b):
        raw_a, raw_b = torch.nan_to_num(fa), torch.nan_to_num(fb)
        assert not torch.equal(raw_a, raw_b)                  # (it did take the other kernel)
        assert (raw_a - raw_b).abs().max().item() <= 1e-4 * raw_b.abs().max().item()


def test_resnet50_fields_variant4_against_variant2():
    _trunk_pair('resnet50', 2, 1)


def test_resnet18_fields_variant4_against_variant2():
    _trunk_pair('resnet18', 16, 2)
