"""ResNet-152 and ResNeXt-50 (32x4d) / -101 (32x8d) (``network.Resnet``) without a GPU: the architecture restated from torchvision's
width rule (reference ``network/factory.py:51-79``), parameter counts, key names and shapes of the state dict (no checkpoint can be
loaded offline), conv + BN folding, the operand of the grouped 3x3 kernel (``fused.gconv_weight_of``) and the formula that kernel
is written against, the command line, and the argument checks of ``opa_gconv3x3_bias_act_f32``."""
import argparse
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import fused, network
from openpifpaf_amd.predictor import Predictor

import trunk_common as tc

# name: (block counts, groups, group width of block2, parameters of base_net)
NAMES = {'resnet152': ([3, 8, 36, 3], 1, 64, 58143808), 'resnext50': ([3, 4, 6, 3], 32, 4, 22979904),
         'resnext101': ([3, 4, 23, 3], 32, 8, 86742336)}


@pytest.mark.parametrize('name', list(NAMES))
def test_structure_and_output_shape(name):
    counts, groups, cg, _ = NAMES[name]
    base = network.factory(name).base_net
    assert isinstance(base, network.Resnet) and base.stride == 16 and base.out_features == 2048
    stages = [base.block2, base.block3, base.block4, base.block5]
    assert [len(s) for s in stages] == counts
    for i, stage in enumerate(stages):
        for j, block in enumerate(stage):
            assert isinstance(block, network._Bottleneck) and block.conv2.groups == groups
            assert block.conv2.in_channels == block.conv2.out_channels == (cg * groups << i)
            assert block.conv2.stride == ((2, 2) if j == 0 and i > 0 else (1, 1)) and block.conv3.out_channels == 256 << i
            assert (block.downsample is not None) == (j == 0)
    with torch.no_grad():
        y = base(torch.randn(1, 3, 65, 49))
    assert tuple(y.shape) == (1, 2048, 5, 4)


@pytest.mark.parametrize('name,want', [(n, v[3]) for n, v in NAMES.items()] + [('resnet50', 23508032)])
def test_parameter_counts(name, want):
    """torchvision's totals minus the 2 049 000 parameters of its classifier."""
    assert sum(p.numel() for p in network.factory(name).base_net.parameters()) == want


def test_default_bottleneck_is_the_plain_one():
    block = network._Bottleneck(256, 64)
    assert block.conv1.out_channels == 64 and block.conv2.groups == 1 and tuple(block.conv2.weight.shape) == (64, 64, 3, 3)
    assert tuple(block.conv3.weight.shape) == (256, 64, 1, 1) and block.bn1.num_features == block.bn2.num_features == 64
    wide = network._Bottleneck(256, 64, groups=32, base_width=8)
    assert tuple(wide.conv1.weight.shape) == (256, 256, 1, 1) and tuple(wide.conv2.weight.shape) == (256, 8, 3, 3)   # int(64 * 8 / 64) * 32


def test_state_dict_keys_and_shapes():
    """torchvision's names below ``base_net``: what a reference checkpoint holds (names and shapes only)."""
    sd50, sd101 = network.factory('resnext50').state_dict(), network.factory('resnext101').state_dict()
    want = {'block2.0.conv2.weight': ((128, 4, 3, 3), (256, 8, 3, 3)), 'block5.2.conv2.weight': ((1024, 32, 3, 3), (2048, 64, 3, 3)),
            'block5.2.conv3.weight': ((2048, 1024, 1, 1), (2048, 2048, 1, 1)),
            'block2.0.downsample.0.weight': ((256, 64, 1, 1), (256, 64, 1, 1)), 'block2.0.bn2.running_var': ((128,), (256,)),
            'input_block.0.weight': ((64, 3, 7, 7), (64, 3, 7, 7))}
    for key, (s50, s101) in want.items():
        assert tuple(sd50['base_net.' + key].shape) == s50 and tuple(sd101['base_net.' + key].shape) == s101, key
    for sd in (sd50, sd101, network.factory('resnet152').state_dict()):
        for key in sd:                                     # no key of the project's own in an unoptimized network
            if key.startswith('base_net.'):
                assert key.split('.')[-1] in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'), key
    assert 'base_net.block4.35.conv3.weight' in network.factory('resnet152').state_dict()


def test_folding_on_the_cpu(monkeypatch):
    net = tc.randomize_(network.factory('resnext50'), 3)
    x = torch.randn((2, 3, 33, 33), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = net(x)
        for on in (True, False):
            monkeypatch.setattr(fused, 'GCONV', on)
            opt = network.optimize_for_inference_(copy.deepcopy(net))
            assert not any(isinstance(m, nn.BatchNorm2d) for m in opt.modules())
            blocks = [m for m in opt.modules() if isinstance(m, network._Bottleneck)]
            assert len(blocks) == 16 and all(m.fused and m.conv2.bias is None for m in blocks)
            h = torch.randn(1, 128, 5, 5).contiguous(memory_format=torch.channels_last)
            assert not fused.gconv3x3_supported(blocks[0].conv2, h, blocks[0].fb2)          # the CPU declines
            assert not any(k.split('.')[-1].startswith('_opa') for k in opt.state_dict())
            got = opt(x)
            for r, g in zip(ref, got):
                assert float((r - g).abs().max()) <= 1e-4 * float(r.abs().max())
    assert all(float(r.abs().max()) > 0 for r in ref)


@pytest.mark.parametrize('cg,groups', [(4, 32), (8, 3), (64, 2)])
def test_operand_follows_the_weight(cg, groups):
    C = cg * groups
    conv = tc.randomize_(nn.Conv2d(C, C, 3, 1, 1, groups=groups, bias=False), cg)

    def want():
        return conv.weight.detach().permute(2, 3, 1, 0).reshape(9, cg, C)
    wt = fused.gconv_weight_of(conv)
    assert tuple(wt.shape) == (9, cg, C) and wt.is_contiguous() and torch.equal(wt, want())
    assert wt[5, 1, 3] == conv.weight[3, 1, 1, 2]
    assert fused.gconv_weight_of(conv) is wt
    with torch.no_grad():
        conv.weight.mul_(2.0)                               # in place
    old = wt.clone()
    wt2 = fused.gconv_weight_of(conv)
    assert wt2 is wt and torch.equal(wt2, want()) and torch.equal(wt2, old * 2.0)        # the kept tensor, overwritten in place
    other = tc.randomize_(nn.Conv2d(C, C, 3, 1, 1, groups=groups, bias=False), cg + 100)
    conv.load_state_dict(other.state_dict())
    assert torch.equal(fused.gconv_weight_of(conv), other.weight.detach().permute(2, 3, 1, 0).reshape(9, cg, C))
    assert not any(k.startswith('_opa') for k in conv.state_dict())


def _model(x, wt, bias, cg, s):
    """The kernel's formula on a channels-last array: out[b,y,x,co] = bias[co] + sum_{t,ci} x[b, y*s-1+ky, x*s-1+kx, (co/cg)*cg+ci] * wt[t][ci][co]."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))                 # [B, H + 2, W + 2, C]
    out = bias.reshape(1, 1, 1, C).repeat(B, Ho, Wo, 1)
    src = (torch.arange(C) // cg) * cg                                      # first input channel of co's group
    for t in range(9):
        ky, kx = divmod(t, 3)
        win = xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]     # [B, Ho, Wo, C]
        for ci in range(cg):
            out = out + win[..., src + ci] * wt[t, ci]
    return out.permute(0, 3, 1, 2)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('cg', [4, 8, 16, 32])
def test_formula_is_the_grouped_convolution(cg, stride):
    groups = 3
    C = cg * groups
    g = torch.Generator().manual_seed(cg + stride)
    conv = nn.Conv2d(C, C, 3, stride, 1, groups=groups, bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64))
    x = torch.randn((2, C, 6, 7), generator=g, dtype=torch.float64)
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    want = F.conv2d(x, conv.weight, bias, stride, 1, groups=groups)
    got = _model(x, fused.gconv_weight_of(conv), bias, cg, stride)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_supported_declines_what_the_kernel_does_not_take(monkeypatch):
    monkeypatch.setattr(fused, 'GCONV', True)
    conv = nn.Conv2d(128, 128, 3, 1, 1, groups=32, bias=False)
    x = torch.randn(1, 128, 5, 5).contiguous(memory_format=torch.channels_last)
    assert not fused.gconv3x3_supported(conv, x, torch.zeros(128))           # not on the GPU


def test_cli_offers_the_three_names():
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    for name in NAMES:
        assert parser.parse_args(['--basenet', name]).basenet == name
    assert set(NAMES) <= set(network.BASE_FACTORIES)


def test_entry_point_checks_its_arguments():
    """Bad arguments are refused on the host, before anything is launched (so this needs no GPU): never dereferenced pointers."""
    from openpifpaf_amd import _lib
    lib, fake = _lib.lib(), 4096
    INVALID = 1

    def call(x=fake, xs=128, wt=fake, bias=fake, out=fake, os=128, batch=2, h=9, w=7, c=128, cg=4, stride=1):
        return lib.opa_gconv3x3_bias_act_f32(x, xs, wt, bias, out, os, batch, h, w, c, cg, stride, 1, None)
    for bad in (dict(cg=2), dict(cg=12), dict(cg=128, c=256, xs=256, os=256), dict(c=132, xs=132, os=132, cg=8), dict(stride=0),
                dict(stride=3), dict(xs=124), dict(os=124), dict(xs=130), dict(os=134), dict(x=fake + 4), dict(wt=fake + 8),
                dict(out=fake + 4), dict(bias=fake + 4), dict(x=None), dict(wt=None), dict(out=None), dict(batch=65536),
                dict(batch=-1), dict(c=0)):
        assert call(**bad) == INVALID, bad
        assert lib.opa_last_error().startswith(b'opa_gconv3x3_bias_act_f32'), bad
    assert call(batch=65536) == INVALID and b'grid.y' in lib.opa_last_error()
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1) == INVALID and b'grid.x' in lib.opa_last_error()
    for empty in (dict(batch=0), dict(h=0), dict(w=0)):                      # nothing to compute: OK, nothing runs
        assert call(**empty) == 0, empty
    assert call(batch=0, cg=5) == INVALID                                    # (an empty call is checked like any other)
