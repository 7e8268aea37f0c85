"""MobileNetV3 large / small (``network.MobileNetV3``) without a GPU: the architecture restated from the paper's tables with
torchvision's module tree (reference ``network/basenetworks.py:432-446``: torchvision's ``features`` with the first stride set to 1),
key names and shapes of the state dict (no checkpoint can be loaded offline), conv + BN folding, and the command line."""
import argparse
import copy

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network
from openpifpaf_amd.predictor import Predictor

import trunk_common as tc

NAMES = {'mobilenetv3large': (960, 17), 'mobilenetv3small': (576, 13)}


@pytest.mark.parametrize('name', list(NAMES))
def test_structure_and_output_shape(name):
    out_features, n_modules = NAMES[name]
    net = network.factory(name)
    base = net.base_net
    assert isinstance(base, network.MobileNetV3) and base.stride == 16 and base.out_features == out_features
    assert len(base.backbone) == n_modules
    stem = base.backbone[0][0]
    assert stem.stride == (1, 1) and stem.kernel_size == (3, 3) and stem.padding == (1, 1) and stem.bias is None
    assert isinstance(base.backbone[0][2], nn.Hardswish) and isinstance(base.backbone[-1][2], nn.Hardswish)
    with torch.no_grad():
        y = base(torch.randn(1, 3, 65, 49))
    assert tuple(y.shape) == (1, out_features, 5, 4)
    bns = [m for m in base.modules() if isinstance(m, nn.BatchNorm2d)]
    assert bns and all(m.eps == 1e-3 and m.momentum == 0.01 for m in bns)
    assert all(m.bias is None for m in base.modules() if isinstance(m, nn.Conv2d) and m.kernel_size != (1, 1))


def test_state_dict_keys_and_shapes():
    """torchvision's names below ``base_net.backbone``: what a reference checkpoint holds (names and shapes only)."""
    large = network.factory('mobilenetv3large').state_dict()
    small = network.factory('mobilenetv3small').state_dict()
    want_large = {'backbone.0.0.weight': (16, 3, 3, 3), 'backbone.0.1.running_var': (16,), 'backbone.1.block.0.0.weight': (16, 1, 3, 3),
                  'backbone.1.block.1.0.weight': (16, 16, 1, 1), 'backbone.2.block.0.0.weight': (64, 16, 1, 1),
                  'backbone.4.block.2.fc1.weight': (24, 72, 1, 1), 'backbone.4.block.2.fc1.bias': (24,),
                  'backbone.4.block.2.fc2.weight': (72, 24, 1, 1), 'backbone.5.block.2.fc1.weight': (32, 120, 1, 1),
                  'backbone.15.block.2.fc1.weight': (240, 960, 1, 1), 'backbone.16.0.weight': (960, 160, 1, 1)}
    want_small = {'backbone.1.block.1.fc1.weight': (8, 16, 1, 1), 'backbone.1.block.2.0.weight': (16, 16, 1, 1),
                  'backbone.4.block.2.fc1.weight': (24, 96, 1, 1), 'backbone.12.0.weight': (576, 96, 1, 1),
                  'backbone.12.1.weight': (576,)}
    for sd, want in ((large, want_large), (small, want_small)):
        for key, shape in want.items():
            assert tuple(sd['base_net.' + key].shape) == shape, key
    # nothing but torchvision's parameters and buffers: no key of our own in an unoptimized network
    for sd in (large, small):
        for key in sd:
            if key.startswith('base_net.'):
                assert key.split('.')[-1] in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'), key


@pytest.mark.parametrize('name,want', [('mobilenetv3large', [1, 3, 5, 6, 8, 9, 10, 12, 14, 15]), ('mobilenetv3small', [3, 5, 6, 8, 10, 11])])
def test_residuals(name, want):
    backbone = network.factory(name).base_net.backbone
    assert [i for i, m in enumerate(backbone) if isinstance(m, network._MBV3Block) and m.use_res_connect] == want
    assert all(isinstance(m, network._MBV3Block) for m in list(backbone)[1:-1])


def test_make_divisible():
    assert [network._make_divisible(v // 4, 8) for v in (16, 72, 96, 120, 240, 288, 480, 576, 672, 960)] == \
        [8, 24, 24, 32, 64, 72, 120, 144, 168, 240]


@pytest.mark.parametrize('name', list(NAMES))
def test_folding_on_the_cpu(name, monkeypatch):
    net = tc.randomize_(network.factory(name), 3)
    x = torch.randn((2, 3, 33, 33), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = net(x)
        for mbv3 in (True, False):
            monkeypatch.setattr(fused, 'MBV3', mbv3)
            opt = network.optimize_for_inference_(copy.deepcopy(net))
            assert not any(isinstance(m, nn.BatchNorm2d) for m in opt.modules())
            assert all(m.fused for m in opt.modules() if isinstance(m, (network._MBV3Block, network.MobileNetV3)))
            got = opt(x)
            for r, g in zip(ref, got):
                assert float((r - g).abs().max()) <= 1e-4 * float(r.abs().max())
    assert all(float(r.abs().max()) > 0 for r in ref)


def test_route_declines_on_the_cpu_and_when_switched_off(monkeypatch):
    block = network.optimize_for_inference_(tc.randomize_(network._MBV3Block(112, 3, 672, 112, True, True, 1), 0))
    x = torch.randn(1, 112, 5, 5).contiguous(memory_format=torch.channels_last)
    assert block.fused and not block._route_supported(x)
    assert block.expand is block.block[0][0] and block.depthwise is block.block[1][0] and block.se is block.block[2]
    assert block.project is block.block[3][0]
    bare = network._MBV3Block(16, 3, 16, 16, False, False, 1)
    assert bare.expand is None and bare.se is None and bare.depthwise is bare.block[0][0] and bare.project is bare.block[1][0]
    with pytest.raises(AssertionError):
        bare.enable_fused_()                                          # batch norms not folded
    # the predicates of the new kernels decline what is not on the GPU
    se = block.se
    assert fused._se_convs_ok(se.fc1, se.fc2) and not fused.se_gate_supported(x.new_zeros(1, 672, 5, 5), se.fc1, se.fc2)
    assert not fused.scale_channels_supported(x, torch.ones(1, 112))
    assert not fused._se_convs_ok(se.fc1, nn.Conv2d(168, 672, 1, bias=False)) and not fused._se_convs_ok(se.fc2, se.fc2)
    assert not fused.unit_conv_x3_supported(block.project, x.new_zeros(1, 672, 5, 5), residual=x)


def test_taps_follow_the_weight():
    block = network.optimize_for_inference_(tc.randomize_(network._MBV3Block(24, 5, 72, 40, True, False, 2), 0))
    dw = block.depthwise
    taps = block.taps_of(dw)
    assert tuple(taps.shape) == (25, 72) and torch.equal(taps, dw.weight.detach().reshape(72, 25).t())
    assert block.taps_of(dw) is taps
    with torch.no_grad():
        dw.weight.mul_(2.0)
    assert torch.equal(block.taps_of(dw), dw.weight.detach().reshape(72, 25).t())


def test_cli_offers_both_names():
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    for name in NAMES:
        assert parser.parse_args(['--basenet', name]).basenet == name
    assert set(NAMES) <= set(network.BASE_FACTORIES)


def test_new_entry_points_check_their_arguments():
    """Bad arguments are refused on the host, before anything is launched (so this needs no GPU): never dereferenced pointers."""
    from openpifpaf_amd import _lib
    lib, fake = _lib.lib(), 4096
    INVALID, WORKSPACE = 1, 4
    # a residual together with a partner; an activation code that does not exist; odd N; a residual pitch shorter than N
    assert lib.opa_gemm_unit_act_f32x3(fake, 72, fake, fake, fake, 40, fake, 40, fake, 286, 40, 72, 0, 6, None) == INVALID
    assert b'residual' in lib.opa_last_error()
    assert lib.opa_gemm_unit_act_f32x3(fake, 72, fake, fake, None, 0, None, 0, fake, 286, 40, 72, 3, 6, None) == INVALID
    assert lib.opa_gemm_unit_act_f32x3(fake, 72, fake, fake, None, 0, fake, 40, fake, 286, 39, 72, 0, 6, None) == INVALID
    assert lib.opa_gemm_unit_act_f32x3(fake, 72, fake, fake, None, 0, fake, 38, fake, 286, 40, 72, 0, 6, None) == INVALID
    assert lib.opa_gemm_unit_act_f32x3(fake, 72, fake, fake, None, 0, fake + 4, 40, fake, 286, 40, 72, 0, 6, None) == INVALID
    assert lib.opa_gemm_unit_act_f32x3(fake, 72, fake, fake, None, 0, fake, 40, fake, 0, 40, 72, 2, 6, None) == 0      # m == 0: nothing runs
    assert lib.opa_dwconv_act(fake, 8, fake, None, fake, 8, 1, 4, 4, 8, 3, 1, 0, 3, None) == INVALID
    assert lib.opa_dwconv_act(fake, 8, fake, None, fake, 8, 1, 4, 4, 8, 4, 1, 0, 2, None) == INVALID                   # k = 4
    assert lib.opa_dwconv_act(fake, 8, fake, None, fake, 8, 65536, 4, 4, 8, 3, 1, 0, 2, None) == INVALID               # grid.y
    # squeeze-and-excitation: the workspace's size, channel counts and pitches that are no multiple of 4, alignment, limits
    assert lib.opa_se_workspace_bytes(2, 161 * 161, 72) == 2 * 51 * 72 * 8 and lib.opa_se_workspace_bytes(3, 1, 960) == 3 * 960 * 8
    assert lib.opa_se_workspace_bytes(3, 512, 8) == 3 * 8 * 8 and lib.opa_se_workspace_bytes(3, 513, 8) == 2 * 3 * 8 * 8
    assert lib.opa_se_pool(fake, 72, 2, 25, 72, fake, 2 * 72 * 8 - 1, None) == WORKSPACE
    assert lib.opa_se_pool(fake, 74, 2, 25, 74, fake, 1 << 20, None) == INVALID
    assert lib.opa_se_pool(fake, 74, 2, 25, 72, fake, 1 << 20, None) == INVALID
    assert lib.opa_se_pool(fake, 68, 2, 25, 72, fake, 1 << 20, None) == INVALID
    assert lib.opa_se_pool(fake + 8, 72, 2, 25, 72, fake, 1 << 20, None) == INVALID
    assert lib.opa_se_pool(fake, 72, 65536, 25, 72, fake, 1 << 40, None) == INVALID
    assert lib.opa_se_gate(fake, 2 * 72 * 8, 2, 25, 72, 4097, fake, fake, fake, fake, fake, None, None) == INVALID
    assert lib.opa_se_gate(fake, 2 * 72 * 8 - 1, 2, 25, 72, 24, fake, fake, fake, fake, fake, None, None) == WORKSPACE
    assert lib.opa_se_gate(fake, 2 * 72 * 8, 2, 25, 72, 24, fake, None, fake, fake, fake, None, None) == INVALID
    assert lib.opa_se_scale(fake, 72, 2, 25, 72, None, None) == INVALID
    assert lib.opa_se_scale(fake, 72, 2, 25, 70, fake, None) == INVALID
