"""Shared by the trunk's route tests (test_trunk_dispatch_model.py, test_trunk_operands.py, test_gpu_trunk_routes.py and the
backbone families' test_gpu_*.py): modules with BatchNorm statistics far from the identity, their float64 reference, the error
measure and its budget, and the launch recorder behind every ``rec`` fixture."""
import copy

import torch
from torch import nn

from openpifpaf_amd import fused, network


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


# ---- the route tests on the GPU (test_gpu_*.py): one error budget, one launch recorder ---------------------------------------------

def gen(seed):
    return torch.Generator().manual_seed(seed)


def e0(fn, ref64):
    """(max, rms) error of torch's own float32 computation ``fn`` against ``ref64``: the median of nine calls."""
    errs = [errors(fn(), ref64) for _ in range(9)]
    return tuple(sorted(e[i] for e in errs)[4] for i in (0, 1))


def report(tag, what, err, e0, k=2, extra=(0.0, 0.0), show_k=False):
    """Prints the line that ``profiles/*/route_errors.log`` keep and says whether ``err <= k * e0 + extra``, as a maximum and as an rms."""
    print('%s %s | e0 max %.3e rms %.3e | err max %.3e rms %.3e | err/e0 max %.2f rms %.2f%s'
          % (tag, what, e0[0], e0[1], err[0], err[1], err[0] / max(e0[0], 1e-30), err[1] / max(e0[1], 1e-30),
             ' | k=%d' % k if show_k else ''))
    return err[0] <= k * e0[0] + extra[0] and err[1] <= k * e0[1] + extra[1]


class Recorder:
    """``trace``: the label of every wrapped launcher of ``fused`` and ``miopen:<name>`` for every watched ``nn.Conv2d``, in call
    order; ``timed``: how often something tried to time a kernel."""

    def __init__(self):
        self.trace, self.timed = [], 0

    def watch(self, module):
        for name, m in module.named_modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_hook(lambda mod, args, out, name=name: self.trace.append('miopen:' + name))
        return module


class PinnedGemm3(dict):
    """A choice table that answers every float32 key of ``conv_bias_act`` with 'gemm3' and stays empty."""

    def get(self, key, default=None):
        if len(key) == 6 and key[0] == 'torch.float32':
            return 'gemm3'
        return super().get(key, default)


def recorder(monkeypatch, launchers, switches=(), force_pick=None, table=None):
    """The body of a ``rec`` fixture -> ``Recorder``.  Every launcher of ``fused`` in ``launchers`` (attribute -> label) appends its
    label to the trace; timing raises; ``switches`` are on, ``FORCE_PICK`` is ``force_pick``, ``X3_TERMS`` 6 and the choice table is
    ``table`` (default: an empty one).  ``monkeypatch`` undoes all of it."""
    r = Recorder()
    for attr, label in launchers.items():
        def wrapper(*args, _real=getattr(fused, attr), _label=label, **kwargs):
            r.trace.append(_label)
            return _real(*args, **kwargs)
        monkeypatch.setattr(fused, attr, wrapper)

    def time_ms(fn, reps=3):
        r.timed += 1
        raise AssertionError('a route timed something')
    monkeypatch.setattr(fused, '_time_ms', time_ms)
    monkeypatch.setattr(fused, 'FORCE_PICK', force_pick)
    monkeypatch.setattr(fused, 'X3_TERMS', 6)
    for attr in switches:
        monkeypatch.setattr(fused, attr, True)
    monkeypatch.setattr(fused, '_CHOICE', {} if table is None else table)
    return r


def forward_checks(opt, x, rec):
    """-> (output of the first call, launch trace of the second); first == second == fresh clone, bit for bit, where no MIOpen step
    is on the route; x unchanged."""
    x0 = x.clone()
    with torch.no_grad():
        first = opt(x)
        rec.trace.clear()
        second = opt(x)
        trace = list(rec.trace)
        assert torch.equal(x, x0), 'the forward wrote into its input'
        third = opt(x0.clone(memory_format=torch.preserve_format))
    assert first.isfinite().all()
    if not any(t.startswith('miopen:') for t in trace):
        assert torch.equal(first, second) and torch.equal(first, third)
    return first, trace
