"""The reference's five ResNet options (``network.Resnet``; reference ``network/basenetworks.py:71-183``) without a GPU: strides,
features, module structure and state-dict keys of every variant, the defaults against the network as it was before the options,
conv + BN folding, a float64 model of the tap formula the dilated implicit GEMM is written against, the identity the pool kernel
rests on, the command line, and the argument checks of ``opa_conv3x3_dilated_f32x3`` and ``opa_maxpool3x3_bias_act``."""
import argparse
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import fused, network
from openpifpaf_amd.predictor import Predictor

import trunk_common as tc

# options -> (overall stride, out_features relative to the default, output H x W on [1, 3, 65, 49])
VARIANTS = {
    'default': ({}, 16, 1, (5, 4)),
    'pool0': (dict(pool0_stride=2), 32, 1, (3, 2)),
    'dilation2': (dict(block5_dilation=2), 8, 1, (9, 7)),
    'conv2': (dict(input_conv2_stride=2), 32, 1, (3, 2)),
    'four-stage': (dict(remove_last_block=True), 8, 2, (9, 7)),
    'stem1': (dict(input_conv_stride=1), 8, 1, (9, 7)),
    'pool0+dilation2': (dict(pool0_stride=2, block5_dilation=2), 16, 1, (5, 4)),
}
DEFAULTS = dict(pool0_stride=0, input_conv_stride=2, input_conv2_stride=0, block5_dilation=1, remove_last_block=False)
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')


def _parent_keys_resnet50():
    """The state-dict keys of ``Resnet('resnet50')`` before the options existed, written out from the architecture."""
    keys = ['input_block.0.weight'] + ['input_block.1.' + k for k in BN_KEYS]
    for stage, blocks in zip((2, 3, 4, 5), (3, 4, 6, 3)):
        for i in range(blocks):
            p = 'block%d.%d.' % (stage, i)
            for j in (1, 2, 3):
                keys += [p + 'conv%d.weight' % j] + [p + 'bn%d.%s' % (j, k) for k in BN_KEYS]
            if i == 0:
                keys += [p + 'downsample.0.weight'] + [p + 'downsample.1.' + k for k in BN_KEYS]
    return keys


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', ['resnet18', 'resnet50'])
def test_structure(name, variant):
    options, stride, shrink, hw = VARIANTS[variant]
    base = network.Resnet(name, **options).eval()
    features = (512 if name == 'resnet18' else 2048) // shrink
    assert base.stride == stride and base.out_features == features
    with torch.no_grad():
        y = base(torch.randn(1, 3, 65, 49))
    assert tuple(y.shape) == (1, features) + hw
    keys = list(base.state_dict())
    plain = list(network.Resnet(name, **DEFAULTS).state_dict())
    stem = base.input_block[0]
    assert stem.stride == ((1, 1) if 'input_conv_stride' in options else (2, 2)) and stem.kernel_size == (7, 7)
    if 'pool0_stride' in options:
        pool = base.input_block[3]
        assert isinstance(pool, nn.MaxPool2d) and (pool.kernel_size, pool.stride, pool.padding) == (3, 2, 1)
        assert not list(pool.parameters()) and len(base.input_block) == 4
    if 'input_conv2_stride' in options:
        conv2 = base.input_block[3]
        assert isinstance(conv2[0], nn.Conv2d) and isinstance(conv2[1], nn.BatchNorm2d) and isinstance(conv2[2], nn.ReLU)
        assert (conv2[0].in_channels, conv2[0].out_channels, conv2[0].kernel_size, conv2[0].stride, conv2[0].padding, conv2[0].bias) == \
            (64, 64, (3, 3), (2, 2), (1, 1), None)
        assert sorted(set(keys) - set(plain)) == sorted(['input_block.3.0.weight'] + ['input_block.3.1.' + k for k in BN_KEYS])
    elif 'remove_last_block' in options:
        assert base.block5 is None and keys == [k for k in plain if not k.startswith('block5.')]
    else:
        assert keys == plain                               # the pool, a dilation and a stem stride add and rename nothing
    if 'pool0_stride' not in options and 'input_conv2_stride' not in options:
        assert len(base.input_block) == 3
    if base.block5 is not None:
        d = options.get('block5_dilation', 1)
        convs = [(n, m) for n, m in base.block5.named_modules() if isinstance(m, nn.Conv2d)]
        assert any('downsample' in n for n, _ in convs)
        for n, m in convs:
            first = n.startswith('0.') and (n.endswith('downsample.0') or n.endswith('conv2' if name == 'resnet50' else 'conv1'))
            if d != 1:
                assert m.stride == (1, 1), n
                assert (m.dilation, m.padding) == (((d, d), (d, d)) if m.kernel_size == (3, 3) else ((1, 1), (0, 0))), n
            else:
                assert m.stride == ((2, 2) if first else (1, 1)) and m.dilation == (1, 1), n
    # nothing outside block 5 is dilated
    for stage in (base.block2, base.block3, base.block4):
        assert all(m.dilation == (1, 1) for m in stage.modules() if isinstance(m, nn.Conv2d))


def test_second_input_convolution_and_pool_exclude_each_other():
    with pytest.raises(AssertionError):
        network.Resnet('resnet50', pool0_stride=2, input_conv2_stride=2)
    with pytest.raises(AssertionError):
        network.Resnet('resnet18', remove_last_block=True, block5_dilation=2)


def test_defaults_are_the_network_as_it_was():
    assert {k: getattr(network.Resnet, k) for k in DEFAULTS} == DEFAULTS
    torch.manual_seed(11)
    a = network.Resnet('resnet50').eval()
    torch.manual_seed(11)
    b = network.Resnet('resnet50', **DEFAULTS).eval()
    assert list(a.state_dict()) == _parent_keys_resnet50() == list(b.state_dict())
    assert [type(m) for m in a.input_block] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU] and a.stride == 16 and a.out_features == 2048
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    x = torch.randn((1, 3, 33, 33), generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    # the factory's seeded network too: the same weights whether or not the keywords are spelled out
    net = network.factory('resnet50', seed=3).base_net
    torch.manual_seed(3)
    again = network.Resnet('resnet50', **DEFAULTS)
    assert torch.equal(net.block5[2].conv3.weight, again.block5[2].conv3.weight)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', ['resnet18', 'resnet50'])
def test_folding_on_the_cpu(name, variant):
    options = VARIANTS[variant][0]
    net = tc.randomize_(network.Resnet(name, **options), 3)
    x = torch.randn((2, 3, 33, 33), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = net(x)
        opt = network.optimize_for_inference_(copy.deepcopy(net))
        assert not any(isinstance(m, nn.BatchNorm2d) for m in opt.modules()) and opt.fused
        assert all(m.bias is None for m in opt.modules() if isinstance(m, nn.Conv2d))
        assert hasattr(opt, 'fb0_2') == ('input_conv2_stride' in options)
        h = torch.randn(1, 64, 5, 5).contiguous(memory_format=torch.channels_last)
        dil = nn.Conv2d(64, 64, 3, 1, 2, 2, bias=False)
        assert not fused.conv3x3_dilated_x3_supported(dil, h, torch.zeros(64))           # the CPU declines both
        assert not fused.maxpool3x3_supported(h) and not fused.maxpool3x3_supported(h, torch.zeros(64))
        assert not any(k.split('.')[-1].startswith('_opa') for k in opt.state_dict())
        got = opt(x)
    assert got.shape == ref.shape and float(ref.abs().max()) > 0
    assert float((ref - got).abs().max()) <= 1e-4 * float(ref.abs().max())


def _tap_model(x, w3, bias, s, d):
    """The implicit GEMM's formula on a channels-last array: column block t = 3 ky + kx of K = 9 C holds the channels of input pixel
    (s y - d + d ky, s x - d + d kx), zeros in the padding; ``w3`` is ``[N, (ky, kx, c)]`` as ``fused.split_weight_3x3`` orders it."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, d, d, d, d))                   # [B, H + 2d, W + 2d, C]
    cols = [xp[:, ky * d:ky * d + (Ho - 1) * s + 1:s, kx * d:kx * d + (Wo - 1) * s + 1:s] for ky in range(3) for kx in range(3)]
    a = torch.cat(cols, dim=3).reshape(B * Ho * Wo, 9 * C)
    return (a @ w3.t() + bias).reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize('hw', [(6, 7), (1, 1)])
@pytest.mark.parametrize('d,s', [(2, 1), (3, 1), (2, 2)])
def test_tap_formula_is_the_dilated_convolution(d, s, hw):
    g = torch.Generator().manual_seed(10 * d + s)
    C, N = 5, 4
    weight = torch.randn((N, C, 3, 3), generator=g, dtype=torch.float64)
    x = torch.randn((2, C) + hw, generator=g, dtype=torch.float64)
    bias = torch.randn(N, generator=g, dtype=torch.float64)
    want = F.conv2d(x, weight, bias, stride=s, padding=d, dilation=d)
    got = _tap_model(x, weight.permute(0, 2, 3, 1).reshape(N, 9 * C), bias, s, d)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the operand's order is the one the model multiplies with
    planes = fused.split_weight_3x3(weight.float())
    assert torch.equal(planes.float().sum(0), weight.float().permute(0, 2, 3, 1).reshape(N, 9 * C))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pool_identity(dtype):
    """``relu(maxpool(x) + b) == maxpool(relu(x + b))`` exactly: the addition, its rounding and the ReLU are non-decreasing."""
    g = torch.Generator().manual_seed(5)
    for hw in ((1, 1), (2, 5), (9, 7), (8, 23)):
        x = (torch.randn((2, 16) + hw, generator=g) * 3).to(dtype)
        b = torch.randn(16, generator=g).to(dtype)
        want = F.max_pool2d(F.relu(x + b.view(1, -1, 1, 1)), 3, 2, 1)
        pooled = F.max_pool2d(x, 3, 2, 1)
        assert torch.equal(F.relu(pooled + b.view(1, -1, 1, 1)), want)
        # ... and with the kernel's arithmetic: float32 addition, ONE rounding to the storage type
        assert torch.equal(F.relu((pooled.float() + b.float().view(1, -1, 1, 1)).to(dtype)), want)


def test_cli_sets_the_class_attributes():
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    saved = {k: getattr(network.Resnet, k) for k in DEFAULTS}
    try:
        args = parser.parse_args([])
        assert {k: getattr(args, 'resnet_' + k) for k in DEFAULTS} == DEFAULTS
        args = parser.parse_args(['--resnet-pool0-stride', '2', '--resnet-input-conv-stride', '1', '--resnet-block5-dilation', '2'])
        Predictor.configure(args)
        assert (network.Resnet.pool0_stride, network.Resnet.input_conv_stride, network.Resnet.block5_dilation) == (2, 1, 2)
        assert network.Resnet.input_conv2_stride == 0 and network.Resnet.remove_last_block is False
        base = network.factory('resnet18').base_net
        assert base.stride == 8 and base.block5[0].conv1.dilation == (2, 2) and isinstance(base.input_block[3], nn.MaxPool2d)
        args = parser.parse_args(['--resnet-input-conv2-stride', '2', '--resnet-remove-last-block'])
        Predictor.configure(args)
        assert {k: getattr(network.Resnet, k) for k in DEFAULTS} == dict(DEFAULTS, input_conv2_stride=2, remove_last_block=True)
        base = network.factory('resnet18').base_net
        assert base.stride == 16 and base.block5 is None and base.out_features == 256
        Predictor.configure(parser.parse_args([]))
        assert {k: getattr(network.Resnet, k) for k in DEFAULTS} == DEFAULTS
    finally:
        for k, v in saved.items():
            setattr(network.Resnet, k, v)


def test_entry_points_check_their_arguments():
    """Bad arguments are refused on the host, before anything is launched (so this needs no GPU): never dereferenced pointers."""
    from openpifpaf_amd import _lib
    lib, fake = _lib.lib(), 4096
    INVALID = 1
    assert lib.opa_abi_version() == 9 == _lib.ABI_VERSION

    def conv(x=fake, w3=fake, bias=fake, out=fake, batch=2, h=9, w=7, c_in=64, c_out=128, stride=1, dilation=2, relu=1, terms=6):
        return lib.opa_conv3x3_dilated_f32x3(x, w3, bias, out, batch, h, w, c_in, c_out, stride, dilation, relu, terms, None)
    for bad in (dict(x=None), dict(w3=None), dict(bias=None), dict(out=None), dict(x=fake + 4), dict(w3=fake + 8), dict(bias=fake + 4),
                dict(out=fake + 4), dict(c_in=32), dict(c_in=96), dict(c_out=96), dict(c_in=0), dict(dilation=0), dict(dilation=-1),
                dict(stride=0), dict(terms=7), dict(batch=-1), dict(h=-1)):
        assert conv(**bad) == INVALID, bad
        assert lib.opa_last_error().startswith(b'opa_conv3x3_dilated_f32x3'), bad
    # (batch h w + d (w + 1)) c_in 4 < 2^31.  The dilation's share alone (an empty call is checked like any other, and launches
    # nothing): d (15 + 1) 64 4 reaches 2^31 at d = 2^19
    assert conv(batch=0, w=15, dilation=2 ** 19 - 1) == 0
    assert conv(batch=0, w=15, dilation=2 ** 19) == INVALID and b'2 GB' in lib.opa_last_error()
    # ... and on top of a tensor: 559207 rows of 15 pixels pass the bound with d = 31 and miss it with d = 32
    h = 559207
    assert (h * 15 + 31 * 16) * 64 * 4 < 2 ** 31 <= (h * 15 + 32 * 16) * 64 * 4
    assert conv(batch=1, h=h, w=15, dilation=32) == INVALID and b'2 GB' in lib.opa_last_error()
    assert lib.opa_last_error().startswith(b'opa_conv3x3_dilated_f32x3')
    assert conv(batch=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1) == INVALID and b'2 GB' in lib.opa_last_error()
    for empty in (dict(batch=0), dict(h=0), dict(w=0)):                      # nothing to compute: OK, nothing runs
        assert conv(**empty) == 0, empty
    assert conv(batch=0, c_in=32) == INVALID                                 # (an empty call is checked like any other)
    # the undilated entry point: the same checks under its own name
    assert lib.opa_conv3x3_f32x3(fake, fake, fake, fake, 2, 9, 7, 32, 128, 1, 1, 6, None) == INVALID
    assert lib.opa_last_error().startswith(b'opa_conv3x3_f32x3:')

    def pool(x=fake, bias=fake, out=fake, dtype=0, batch=2, h=9, w=7, c=64, stride=2, relu=1):
        return lib.opa_maxpool3x3_bias_act(x, bias, out, dtype, batch, h, w, c, stride, relu, None)
    for bad in (dict(x=None), dict(out=None), dict(x=fake + 4), dict(out=fake + 8), dict(bias=fake + 4), dict(c=4), dict(c=12), dict(c=0),
                dict(stride=0), dict(stride=1), dict(stride=3), dict(dtype=1), dict(dtype=3), dict(dtype=-1), dict(batch=-1), dict(w=-1),
                dict(batch=2 ** 15, h=2 ** 8, w=2 ** 8, c=8), dict(dtype=2, batch=2 ** 16, h=2 ** 8, w=2 ** 8, c=8),
                dict(h=2 ** 31 - 1, w=2 ** 31 - 1)):
        assert pool(**bad) == INVALID, bad
        assert lib.opa_last_error().startswith(b'opa_maxpool3x3_bias_act'), bad
    assert pool(batch=2 ** 15, h=2 ** 8, w=2 ** 8, c=8) == INVALID and b'32-bit' in lib.opa_last_error()
    for empty in (dict(batch=0), dict(h=0), dict(w=0), dict(batch=0, bias=None)):
        assert pool(**empty) == 0, empty
    assert pool(batch=0, c=4) == INVALID and pool(batch=0, stride=1) == INVALID
