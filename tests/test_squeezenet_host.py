"""SqueezeNet 1.1 (``network.SqueezeNet``) without a GPU: the architecture restated with torchvision's module tree (reference
``network/basenetworks.py:461-487``: torchvision's ``squeezenet1_1().features`` with padding 1 on the stem and on the ceil-mode
max-pools), key names and shapes of the state dict (no checkpoint can be loaded offline), the optimized forward on the CPU, the
derived operand of the Fire expand kernel, the ceil-mode output sizes, the argument checks of both new C entry points, and the
command line."""
import argparse
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import fused, network
from openpifpaf_amd.predictor import Predictor

import trunk_common as tc

# index in ``backbone`` -> (in, squeeze, expand 1x1, expand 3x3)
FIRES = {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 6: (128, 32, 128, 128), 7: (256, 32, 128, 128),
         9: (256, 48, 192, 192), 10: (384, 48, 192, 192), 11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}


def _want_state_dict():
    """The 50 keys below ``backbone`` and their shapes, written out from torchvision's ``squeezenet1_1().features``."""
    want = {'backbone.0.weight': (64, 3, 3, 3), 'backbone.0.bias': (64,)}
    for i, (inp, s, e1, e3) in FIRES.items():
        want['backbone.%d.squeeze.weight' % i] = (s, inp, 1, 1)
        want['backbone.%d.squeeze.bias' % i] = (s,)
        want['backbone.%d.expand1x1.weight' % i] = (e1, s, 1, 1)
        want['backbone.%d.expand1x1.bias' % i] = (e1,)
        want['backbone.%d.expand3x3.weight' % i] = (e3, s, 3, 3)
        want['backbone.%d.expand3x3.bias' % i] = (e3,)
    return want


def test_structure():
    base = network.factory('squeezenet').base_net
    assert isinstance(base, network.SqueezeNet) and base.stride == 16 and base.out_features == 512
    sd = base.state_dict()
    want = _want_state_dict()
    assert len(want) == 50 and {k: tuple(v.shape) for k, v in sd.items()} == want
    # torchvision's published 1 235 496 parameters of squeezenet1_1 minus its classifier (Conv2d(512, 1000, 1): 513 000)
    assert sum(p.numel() for p in base.parameters()) == 722496 == 1235496 - 513000
    assert sum(isinstance(m, nn.Conv2d) for m in base.modules()) == 25
    assert all(m.bias is not None for m in base.modules() if isinstance(m, nn.Conv2d))
    assert not any(isinstance(m, nn.BatchNorm2d) for m in base.modules())
    pools = [(i, m) for i, m in enumerate(base.backbone) if isinstance(m, nn.MaxPool2d)]
    assert [i for i, _ in pools] == [2, 5, 8]
    for _, m in pools:
        assert m.padding == 1 and m.ceil_mode and m.kernel_size == 3 and m.stride == 2
    stem = base.backbone[0]
    assert stem.padding == (1, 1) and stem.stride == (2, 2) and stem.kernel_size == (3, 3) and isinstance(base.backbone[1], nn.ReLU)
    assert [i for i, m in enumerate(base.backbone) if isinstance(m, network._Fire)] == list(FIRES)
    # torchvision's initialisation: zero biases, weights that are not
    assert all(not m.bias.any() and m.weight.any() for m in base.modules() if isinstance(m, nn.Conv2d))
    assert 'names and shapes only' in ' '.join(network.SqueezeNet.__doc__.split())


@pytest.mark.parametrize('shape', [(1, 3, 65, 49), (1, 3, 64, 50)])
def test_output_shape(shape):
    net = network.factory('squeezenet')
    with torch.no_grad():
        x = torch.randn(shape)
        assert tuple(net.base_net(x).shape) == (1, 512, 5, 4)
        cif, caf = net(x)
    assert tuple(cif.shape) == (1, 17, 5, 9, 7) and tuple(caf.shape) == (1, 19, 8, 9, 7)


def test_sizes_at_641():
    base = network.SqueezeNet()
    sizes, hw = [], 641
    for m in base.backbone:
        if isinstance(m, nn.MaxPool2d):
            hw = fused.maxpool3x3_out_hw(hw, hw, True)[0]
            sizes.append(hw)
        elif isinstance(m, nn.Conv2d):
            hw = (hw + 2 - 3) // 2 + 1
            sizes.append(hw)
    assert sizes == [321, 161, 81, 41]


def test_optimizing_on_the_cpu(monkeypatch):
    net = tc.randomize_(network.factory('squeezenet'), 3)
    x = torch.randn((2, 3, 34, 33), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref = net(x)
        for fire in (True, False):
            monkeypatch.setattr(fused, 'FIRE', fire)
            opt = network.optimize_for_inference_(copy.deepcopy(net))
            fires = [m for m in opt.modules() if isinstance(m, (network._Fire, network.SqueezeNet))]
            assert len(fires) == 9 and all(m.fused for m in fires)
            assert list(opt.state_dict()) == list(net.state_dict())
            got = opt(x.contiguous(memory_format=torch.channels_last))
            for r, g in zip(ref, got):
                assert float((r - g).abs().max()) <= 1e-4 * float(r.abs().max())
    assert all(float(r.abs().max()) > 0 for r in ref)


def test_route_declines_on_the_cpu_and_when_switched_off(monkeypatch):
    block = network.optimize_for_inference_(tc.randomize_(network._Fire(256, 48, 192, 192), 0))
    x = torch.randn(1, 256, 5, 5).contiguous(memory_format=torch.channels_last)
    h = torch.randn(1, 48, 5, 5).contiguous(memory_format=torch.channels_last)
    assert fused.FIRE is False, 'the route ships switched off'
    assert fused.FIRE_TERMS == 9, 'six terms shrink the output of 17 layers in series: profiles/squeezenet/terms.log'
    for fire in (True, False):
        monkeypatch.setattr(fused, 'FIRE', fire)
        with torch.no_grad():
            assert block.fused and not block._route_supported(x)
            assert not fused.fire_expand_supported(block.expand1x1, block.expand3x3, h)
    # what depends on the convolutions alone: squeeze widths of 16 ... 64 in steps of 16, output channels in multiples of 64
    assert fused._fire_convs_ok(block.expand1x1, block.expand3x3)
    for s, e1, e3 in ((8, 64, 64), (24, 64, 64), (80, 64, 64), (16, 32, 64), (16, 64, 96)):
        bad = network._Fire(64, s, e1, e3)
        assert not fused._fire_convs_ok(bad.expand1x1, bad.expand3x3), (s, e1, e3)
    assert not fused._fire_convs_ok(block.expand1x1, nn.Conv2d(48, 192, 3, padding=1, stride=2))
    assert not fused._fire_convs_ok(block.expand1x1, nn.Conv2d(48, 192, 3, padding=0))
    assert not fused._fire_convs_ok(block.expand1x1, nn.Conv2d(32, 192, 3, padding=1))


def test_derived_weight_follows_the_weight():
    """One block of three bf16 planes whose sum is the weight, in the kernel's fragment order; the same object until a weight or a bias
    changes -- in place or through ``load_state_dict`` (a stale snapshot would survive both)."""
    fire = tc.randomize_(network._Fire(128, 32, 128, 128), 0)
    e1, e3 = fire.expand1x1, fire.expand3x3
    w3, bias = fused.fire_weight_of(e1, e3)
    assert tuple(w3.shape) == (3, (128 + 9 * 128) * 32) and w3.dtype == torch.bfloat16 and w3.is_contiguous()
    assert torch.equal(bias, torch.cat((e1.bias, e3.bias)).detach())
    assert fused.fire_weight_of(e1, e3)[0] is w3

    def decoded(block):
        """The fragments back as ([e1, s], [e3, 3, 3, s]): fragment (32-row block, K-step) = 64 lanes x 8, lane l = row l % 32, columns 8 (l // 32) ..."""
        w = (block[0].float() + block[1].float()) + block[2].float()
        a = w[:128 * 32].reshape(4, 2, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(128, 32)
        b = w[128 * 32:].reshape(4, 18, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(128, 3, 3, 32)
        return a, b
    a, b = decoded(w3)
    assert torch.equal(a, e1.weight.detach().reshape(128, 32)) and torch.equal(b, e3.weight.detach().permute(0, 2, 3, 1))
    old = w3.clone()
    with torch.no_grad():
        e3.weight.mul_(2.0)
    w3b, bias_b = fused.fire_weight_of(e1, e3)
    # (the kept tensors, overwritten in place: an address a HIP graph holds sees the new weights)
    assert w3b is w3 and bias_b is bias and not torch.equal(w3b, old) and torch.equal(decoded(w3b)[1], e3.weight.detach().permute(0, 2, 3, 1))
    with torch.no_grad():
        e1.bias.add_(1.0)
    assert torch.equal(fused.fire_weight_of(e1, e3)[1], torch.cat((e1.bias, e3.bias)).detach())
    other = tc.randomize_(network._Fire(128, 32, 128, 128), 1)
    fire.load_state_dict(other.state_dict())
    w3c, bias_c = fused.fire_weight_of(e1, e3)
    a, b = decoded(w3c)
    assert torch.equal(a, other.expand1x1.weight.detach().reshape(128, 32))
    assert torch.equal(b, other.expand3x3.weight.detach().permute(0, 2, 3, 1))
    assert torch.equal(bias_c, torch.cat((other.expand1x1.bias, other.expand3x3.bias)).detach())
    assert fused.fire_weight_of(e1, e3)[0] is w3c


def test_ceil_mode_output_sizes():
    sizes = (1, 2, 3, 4, 7, 8, 9, 16, 17)
    for h in sizes:
        for w in sizes:
            x = torch.zeros(1, 1, h, w)
            assert fused.maxpool3x3_out_hw(h, w, True) == tuple(F.max_pool2d(x, 3, 2, 1, ceil_mode=True).shape[2:]), (h, w)
            assert fused.maxpool3x3_out_hw(h, w) == tuple(F.max_pool2d(x, 3, 2, 1).shape[2:]), (h, w)
    assert [fused.maxpool3x3_out_hw(h, h, True)[0] for h in (33, 34, 641, 642)] == [17, 18, 321, 322]


def test_new_entry_points_check_their_arguments():
    """Bad arguments are refused on the host, before anything is launched (so this needs no GPU): never dereferenced pointers."""
    from openpifpaf_amd import _lib
    lib, fake = _lib.lib(), 4096
    INVALID = 1

    def refused(name, *args):
        assert getattr(lib, name)(*args) == INVALID, (name, args)
        assert lib.opa_last_error().startswith(name.encode() + b': '), lib.opa_last_error()
        return lib.opa_last_error()
    fire = 'opa_fire_expand_f32x3'
    for s in (8, 24, 80):
        assert b'c_squeeze' in refused(fire, fake, fake, fake, fake, 2, 9, 7, s, 64, 64, 6, None)
    assert b'c_e1' in refused(fire, fake, fake, fake, fake, 2, 9, 7, 16, 32, 64, 6, None)
    assert b'c_e1' in refused(fire, fake, fake, fake, fake, 2, 9, 7, 16, 64, 96, 6, None)
    refused(fire, fake, fake, fake, fake, 2, 9, 7, 16, 64, 64, 7, None)                             # terms
    refused(fire, None, fake, fake, fake, 2, 9, 7, 16, 64, 64, 6, None)
    refused(fire, fake, fake, None, fake, 2, 9, 7, 16, 64, 64, 6, None)                             # the bias is required
    refused(fire, fake, fake, fake, fake, -1, 9, 7, 16, 64, 64, 6, None)
    for i in range(4):
        pointers = [fake + (8 if j == i else 0) for j in range(4)]
        assert b'aligned' in refused(fire, *pointers, 2, 9, 7, 16, 64, 64, 6, None)
    # 2 GB: the output of 2^22 pixels x 128 channels x 4 bytes; one pixel less passes this check (and is refused by nothing else:
    # it would launch, so it is not called); the input alone at 64 channels
    assert b'2 GB' in refused(fire, fake, fake, fake, fake, 1, 2048, 2048, 16, 64, 64, 6, None)
    assert b'2 GB' in refused(fire, fake, fake, fake, fake, 4, 2048, 2048, 64, 64, 64, 6, None)
    for empty in ((0, 9, 7), (2, 0, 7), (2, 9, 0)):
        assert lib.opa_fire_expand_f32x3(fake, fake, fake, fake, *empty, 16, 64, 64, 6, None) == 0                       # nothing runs
    pool = 'opa_maxpool3x3_ceil_bias_act'
    assert refused(pool, None, None, fake, 0, 2, 8, 8, 64, 2, 0, None).endswith(b'bad arguments')
    assert b'dtype' in refused(pool, fake, None, fake, 1, 2, 8, 8, 64, 2, 0, None)
    assert b'stride' in refused(pool, fake, None, fake, 0, 2, 8, 8, 64, 1, 0, None)
    assert b'multiple of 8' in refused(pool, fake, None, fake, 0, 2, 8, 8, 12, 2, 0, None)
    assert b'aligned' in refused(pool, fake + 8, None, fake, 0, 2, 8, 8, 64, 2, 0, None)
    assert b'aligned' in refused(pool, fake, fake + 4, fake, 0, 2, 8, 8, 64, 2, 0, None)
    assert b'2 GB' in refused(pool, fake, None, fake, 0, 8, 2048, 2048, 16, 2, 0, None)
    assert b'2 GB' in refused(pool, fake, None, fake, 2, 16, 2048, 2048, 16, 2, 0, None)
    for empty in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert lib.opa_maxpool3x3_ceil_bias_act(fake, None, fake, 0, *empty, 64, 2, 0, None) == 0
    # the floor-mode entry point answers under its own name, as before
    assert lib.opa_maxpool3x3_bias_act(fake, None, fake, 0, 2, 8, 8, 12, 2, 0, None) == INVALID
    assert lib.opa_last_error() == b'opa_maxpool3x3_bias_act: c must be a multiple of 8'


def test_cli_offers_the_name():
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    assert parser.parse_args(['--basenet', 'squeezenet']).basenet == 'squeezenet'
    assert 'squeezenet' in network.BASE_FACTORIES
