"""Shared by the trunk's route tests (test_trunk_dispatch_model.py, test_trunk_operands.py, test_gpu_trunk_routes.py): modules
with BatchNorm statistics far from the identity, their float64 reference and the error measure."""
import copy

import torch
from torch import nn

from openpifpaf_amd import network


def randomize_(module, seed):
    """Kaiming weights like ``network.Resnet`` gives its convolutions, and BatchNorm statistics / affine terms drawn at random:
    the folded biases ``fb*`` are of the activations' own size (a bias applied twice, or not at all, moves the output by
    order one -- with the zero bias of a fresh BatchNorm it would move nothing)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1] // m.groups
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                m.bias.copy_(torch.randn(n, generator=g) * 0.5)
    return module.eval()


def bottleneck(inplanes, planes, stride, downsample, seed):
    ds = None
    if downsample:
        ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
    else:
        assert stride == 1 and inplanes == planes * 4
    return randomize_(network._Bottleneck(inplanes, planes, stride, ds), seed)


def basic_block(inplanes, planes, stride, downsample, seed):
    ds = None
    if downsample:
        ds = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
    return randomize_(network._BasicBlock(inplanes, planes, stride, ds), seed)


def optimized(module):
    """A copy of the unfused ``module`` with conv + BN folded and the fused forward switched on."""
    return network.optimize_for_inference_(copy.deepcopy(module))


def errors(got, ref64):
    """(max, rms) of ``got - ref64`` relative to ``max |ref64|``."""
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    d = got.double() - ref64.to(got.device)
    scale = ref64.abs().max().item()
    return d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / scale
