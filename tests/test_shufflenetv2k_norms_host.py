"""The reference's ``--shufflenetv2k-instance-norm`` / ``--shufflenetv2k-group-norm`` (``network.ShuffleNetV2K(layer_norm=...)``; reference
``network/basenetworks.py:250-259, 376-400``) without a GPU: module types, group counts and state-dict keys, the defaults against the
network without the keyword, both norms against the reference's own class in float64 (``tests/golden/shufflenetv2k_norms.npz``, written
by ``tests/golden/make_golden_shufflenetv2k_norms.py``) before and after ``optimize_for_inference_``, what folds and what stays, the three
routes that skip the module between a convolution and its activation declining for a group norm -- with ``fused.GN`` off and on --,
everything ``group_norm_supported`` declines, the switch's default and the command line."""
import argparse
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import _lib, fused, network
from openpifpaf_amd.predictor import Predictor

import trunk_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shufflenetv2k_norms.npz')
TINY = ([1, 1, 1], [24, 232, 64, 256, 24])
# variant -> the keywords
VARIANTS = {'instance': dict(layer_norm='instance'), 'group': dict(layer_norm='group'), 'group_leaky': dict(layer_norm='group', leaky_relu=True)}
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')
CL = torch.channels_last


def _groups(c):
    return (32 if c % 32 == 0 else 29) if c > 100 else 4


def _norm_positions(net):
    """-> [(the Sequential, index)] of every place a ShuffleNetV2K has a norm."""
    places = [(net.input_block, 1)] + [(m, 1) for m in list(net.input_block)[3:]]
    for stage in (net.stage2, net.stage3, net.stage4):
        for unit in stage:
            if unit.branch1 is not None:
                places += [(unit.branch1, 1), (unit.branch1, 3)]
            places += [(unit.branch2, 1), (unit.branch2, 4), (unit.branch2, 6)]
    return places + [(net.conv5, 1)]


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _golden_net(golden, variant):
    net = network.ShuffleNetV2K('tiny', config=TINY, **VARIANTS[variant]).double().eval()
    w_of = str(golden[variant + '/w_from']) if variant + '/w_from' in golden.files else variant
    keys, sizes, flat = [str(k) for k in golden[variant + '/keys']], golden[variant + '/sizes'], golden[w_of + '/w']
    state = net.state_dict()
    assert keys == [k for k in state if not k.endswith('num_batches_tracked')], 'the key names differ from the reference\'s'
    assert int(sizes.sum()) == len(flat)
    at = 0
    for key, size in zip(keys, sizes):
        assert state[key].numel() == size, key
        state[key] = torch.from_numpy(flat[at:at + size].astype(np.float64)).reshape(state[key].shape)
        at += int(size)
    net.load_state_dict(state, strict=True)
    return net


# ---- structure ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['shufflenetv2k16', 'shufflenetv2k30'])
def test_module_types_group_counts_and_keys(name):
    plain = network.ShuffleNetV2K(name)
    inst, group = network.ShuffleNetV2K(name, layer_norm='instance'), network.ShuffleNetV2K(name, layer_norm='group', input_conv2_stride=2)
    assert (plain.layer_norm, inst.layer_norm, group.layer_norm) == (None, 'instance', 'group')
    assert list(inst.state_dict()) == list(plain.state_dict())              # the same five keys per norm, the same positions
    for (seq, i), (pseq, pi) in zip(_norm_positions(inst), _norm_positions(plain)):
        m, c = seq[i], pseq[pi].num_features
        assert i == pi and type(m) is nn.InstanceNorm2d and type(pseq[pi]) is nn.BatchNorm2d
        assert (m.num_features, m.affine, m.track_running_stats, m.eps, m.momentum) == (c, True, True, 1e-5, 0.1)
    widths = set()
    for seq, i in _norm_positions(group):
        m, c = seq[i], seq[i - 1].out_channels
        assert type(m) is nn.GroupNorm and (m.num_channels, m.num_groups, m.eps, m.affine) == (c, _groups(c), 1e-5, True)
        widths.add((c, m.num_groups))
    want = {'shufflenetv2k16': {(24, 4), (174, 29), (348, 29), (696, 29), (1392, 29)},
            'shufflenetv2k30': {(32, 4), (256, 32), (512, 32), (1024, 32), (2048, 32)}}[name]
    assert widths == want
    with_conv2 = network.ShuffleNetV2K(name, input_conv2_stride=2)
    assert list(group.state_dict()) == [k for k in with_conv2.state_dict() if not k.endswith(BN_KEYS[2:])]
    # no other module differs
    assert [type(m) for m in plain.modules() if not isinstance(m, nn.BatchNorm2d)] == [type(m) for m in inst.modules() if not isinstance(m, nn.InstanceNorm2d)]
    unit = network._InvertedResidualK(24, 232, True, layer_norm='group')
    assert [type(m) for m in unit.branch2] == [nn.Conv2d, nn.GroupNorm, nn.ReLU, nn.Conv2d, nn.GroupNorm, nn.Conv2d, nn.GroupNorm, nn.ReLU]
    assert unit.branch2[1].num_groups == 29 and unit.branch1[1].num_groups == 4
    assert 'layer_norm' in network.ShuffleNetV2K.OPTIONS and network.ShuffleNetV2K.layer_norm is None
    with pytest.raises(ValueError):
        network.ShuffleNetV2K(name, layer_norm='layer')


def test_the_keys_are_the_goldens(golden):
    for variant, options in VARIANTS.items():
        net = network.ShuffleNetV2K('tiny', config=TINY, **options)
        assert [k for k in net.state_dict() if not k.endswith('num_batches_tracked')] == [str(k) for k in golden[variant + '/keys']]
        assert {m.eps for m in net.modules() if isinstance(m, (nn.InstanceNorm2d, nn.GroupNorm))} == {float(golden[variant + '/eps'][0])}


def test_x5_stem_is_not_divisible():
    """42 channels in 4 groups: torch's own ``ValueError``, as in the reference."""
    with pytest.raises(ValueError, match='divisible'):
        network.ShuffleNetV2K('shufflenetv2kx5', layer_norm='group')
    assert network.ShuffleNetV2K('shufflenetv2kx5', layer_norm='instance').input_block[1].num_features == 42


def test_defaults_are_the_network_without_the_keyword():
    torch.manual_seed(11)
    a = network.ShuffleNetV2K('shufflenetv2k16').eval()
    torch.manual_seed(11)
    b = network.ShuffleNetV2K('shufflenetv2k16', layer_norm=None).eval()
    assert not any(isinstance(m, (nn.InstanceNorm2d, nn.GroupNorm)) for m in a.modules())
    assert sum(isinstance(m, nn.BatchNorm2d) for m in a.modules()) == len(_norm_positions(a))
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    x = torch.randn((1, 3, 33, 33), generator=tc.gen(12))
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    # the norms draw nothing: the seeded convolutions are the same under every norm
    torch.manual_seed(11)
    c = network.ShuffleNetV2K('shufflenetv2k16', layer_norm='group')
    assert torch.equal(a.conv5[0].weight, c.conv5[0].weight) and torch.equal(a.stage3[2].branch2[3].weight, c.stage3[2].branch2[3].weight)


# ---- against the reference's class -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', list(VARIANTS))
def test_against_the_reference_class(golden, variant):
    """The in-tree float64 network with the reference's weights against the reference's float64 output: ``max |delta| <= 1e-9 max
    |ref|`` (the bound of ``test_shufflenetv2k_options_host.py``), and the same after ``optimize_for_inference_`` on the CPU: the instance
    norms folded -- an ``Identity`` wherever a norm was --, the group norms where they were."""
    assert golden['x'].dtype == np.float32 and all(golden[k].dtype.kind in 'fiU' for k in golden.files)
    net = _golden_net(golden, variant)
    x = torch.from_numpy(golden['x']).double()
    ref = torch.from_numpy(golden[variant + '/out'])
    assert ref.dtype == torch.float64
    with torch.no_grad():
        got = net(x)
        opt = network.optimize_for_inference_(copy.deepcopy(net))
        assert opt.fused and opt.stage4[0].fused
        folded = opt(x)
    kinds = [type(seq[i]) for seq, i in _norm_positions(opt)]
    assert len(kinds) == 17 and set(kinds) == ({nn.Identity} if variant == 'instance' else {nn.GroupNorm})
    if variant == 'instance':
        assert not any(isinstance(m, (nn.InstanceNorm2d, nn.BatchNorm2d, nn.GroupNorm)) for m in opt.modules())
        assert all(seq[i - 1].bias is not None for seq, i in _norm_positions(opt))
    else:
        assert all(seq[i - 1].bias is None for seq, i in _norm_positions(opt))
        assert [k for k in opt.state_dict() if 'w_taps' not in k] == list(net.state_dict())
    scale = float(ref.abs().max())
    assert got.shape == ref.shape and scale > 1
    for what, t in (('unfused', got), ('optimized', folded)):
        delta = float((t - ref).abs().max())
        print('SHUFFLENORM golden %s %s max |delta| %.3e of max |ref| %.3e' % (variant, what, delta, scale))
        assert delta <= 1e-9 * scale, (what, delta, scale)


def test_the_golden_outputs_need_their_norms(golden):
    """The batch-norm network with the instance variant's weights IS that variant in ``eval()``; the group variant's output is not
    the output of the same convolutions without their norms."""
    inst = _golden_net(golden, 'instance')
    plain = network.ShuffleNetV2K('tiny', config=TINY).double().eval()
    plain.load_state_dict(inst.state_dict())
    x = torch.from_numpy(golden['x']).double()
    group = _golden_net(golden, 'group')
    bare = copy.deepcopy(group)
    for seq, i in _norm_positions(bare):
        seq[i] = nn.Identity()
    with torch.no_grad():
        ref = torch.from_numpy(golden['instance/out'])
        assert float((plain(x) - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
        ref = torch.from_numpy(golden['group/out'])
        assert float((bare(x) - ref).abs().max()) > 1e-2 * float(ref.abs().max())


def test_only_an_eval_instance_norm_with_affine_and_running_statistics_folds():
    def seq(norm):
        return nn.Sequential(nn.Conv2d(4, 8, 1, bias=False), norm, nn.ReLU()).eval()
    for norm, folds in ((nn.InstanceNorm2d(8, affine=True, track_running_stats=True), True), (nn.InstanceNorm2d(8, affine=True), False),
                        (nn.InstanceNorm2d(8, track_running_stats=True), False), (nn.InstanceNorm2d(8), False), (nn.GroupNorm(4, 8), False),
                        (nn.BatchNorm2d(8), True)):
        m = seq(norm)
        assert network._folds(m[1]) is folds
        network.fuse_conv_bn_(m)
        assert isinstance(m[1], nn.Identity) is folds and (m[1] is norm) is not folds
    training = nn.InstanceNorm2d(8, affine=True, track_running_stats=True).train()
    assert not network._folds(training)
    # the folded convolution computes what the module did
    m = seq(nn.InstanceNorm2d(8, affine=True, track_running_stats=True))
    with torch.no_grad():
        m[1].running_mean.normal_(generator=tc.gen(1)); m[1].running_var.uniform_(0.5, 2.0, generator=tc.gen(2))
        m[1].weight.uniform_(0.5, 1.5, generator=tc.gen(3)); m[1].bias.normal_(generator=tc.gen(4))
        x = torch.randn((2, 4, 5, 3), generator=tc.gen(5))
        want = m.double()(x.double())
        got = network.fuse_conv_bn_(m)(x.double())
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- the routes that skip the module between a convolution and its activation ----------------------------------------------------------

class _OnDevice(torch.Tensor):
    is_cuda = True


def _randomize_norms_(net, seed):
    g = tc.gen(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.GroupNorm, nn.InstanceNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
    return net


def _cl(y):
    """Dense channels-last, as every kernel writes its output."""
    return y.contiguous(memory_format=CL)


def _apply(y, act, param):
    return {0: lambda: y, 1: lambda: torch.relu(y), 3: lambda: F.leaky_relu(y, param)}[int(act)]()


@pytest.fixture
def kernels(monkeypatch):
    """torch on the host in place of every launcher a ShuffleNetV2K route calls, each recording its label and activation code; every
    switch of these routes on but ``GN``, which the tests set; the predicates see a CPU tensor that says it is on the GPU."""
    calls = []

    def unit(conv, x, relu=True, partner=None, residual=None, act=None, terms=None, act_param=0.0):
        code = int(bool(relu)) if act is None else act
        calls.append(('unit', code))
        y = _apply(F.conv2d(x, conv.weight, conv.bias), code, act_param)
        return _cl(y if partner is None else network._channel_shuffle(torch.cat((partner, y), 1), 2))

    def dwconv(x, w_taps, bias, kernel_size, stride, relu=False, act=None, dilation=1, act_param=0.0):
        calls.append(('dwconv', int(bool(relu)) if act is None else act))
        c = x.shape[1]
        return _cl(F.conv2d(x, w_taps.t().reshape(c, 1, kernel_size, kernel_size), bias, stride, kernel_size // 2 * dilation, dilation, c))

    def stem(conv, x, act=fused.ACT_NONE, act_param=0.0):
        calls.append(('stem', act))
        return _cl(_apply(F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding), act, act_param))

    def group_norm(norm, x, act=fused.ACT_NONE, act_param=0.0, out=None):
        calls.append(('gn', act))
        y = _apply(F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps), act, act_param)
        return _cl(y) if out is None else out.copy_(y)

    def interleave(a, b):
        calls.append(('interleave', 0))
        return _cl(network._channel_shuffle(torch.cat((a, b), 1), 2))
    for name, fn in (('conv1x1_unit_x3', unit), ('dwconv_bias_act', dwconv), ('stem_conv3x3_bias_act', stem), ('group_norm_act', group_norm),
                     ('channel_interleave', interleave)):
        monkeypatch.setattr(fused, name, fn)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    for switch in ('X3_UNIT', 'UNIT_LEAKY', 'STEM'):
        monkeypatch.setattr(fused, switch, True)
    monkeypatch.setattr(fused, 'X3_TERMS', 6)
    monkeypatch.setattr(fused, 'FORCE_PICK', 'x3')
    monkeypatch.setattr(fused, '_CHOICE', {})
    return calls


def _nets(leaky=False):
    """-> (the group-norm network, the batch-norm network of the same convolutions), optimized, and their unfused originals"""
    torch.manual_seed(5)
    group = _randomize_norms_(tc.randomize_(network.ShuffleNetV2K('tiny', config=TINY, layer_norm='group', leaky_relu=leaky), 5), 6)
    torch.manual_seed(5)
    batch = tc.randomize_(network.ShuffleNetV2K('tiny', config=TINY, leaky_relu=leaky), 5)
    return network.optimize_for_inference_(copy.deepcopy(group)), network.optimize_for_inference_(copy.deepcopy(batch)), group, batch


@pytest.mark.parametrize('leaky', [False, True], ids=['relu', 'leaky'])
@pytest.mark.parametrize('gn', [False, True], ids=['GN-off', 'GN-on'])
def test_the_skipping_routes_decline_for_a_group_norm(kernels, monkeypatch, gn, leaky):
    """``_forward_unit``, ``_conv5_forward`` and ``_stem_route`` apply convolution + activation and skip the module between them.  For
    the folded batch-norm network they run (so the patches leave them able to); for the group-norm network none does, with ``GN`` off
    and on: no launcher ever gets an activation code in front of a norm, and the whole forward is the unfused network's."""
    monkeypatch.setattr(fused, 'GN', gn)
    group, batch, group0, batch0 = _nets(leaky)
    x = torch.randn((2, 3, 33, 25), generator=tc.gen(7)).contiguous(memory_format=CL).as_subclass(_OnDevice)
    code = 3 if leaky else 1
    with torch.no_grad():
        # the batch-norm network: all three routes
        h = batch.input_block(x)
        assert batch.stage2[0]._unit_route_supported(h)
        del kernels[:]
        got = batch(x)
        assert kernels[0] == ('stem', code) and kernels[-1] == ('unit', code) and ('unit', code) in kernels[1:-1]
        assert not [c for c in kernels if c[0] in ('gn', 'interleave')]
        want = batch0(x.as_subclass(torch.Tensor))
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
        # the group-norm network
        h = group.input_block(x)
        for stage in (group.stage2, group.stage3, group.stage4):
            assert not stage[0]._unit_route_supported(h) and stage[0]._convs_supported(h)
            h = stage(h)
        assert network._stem_route(batch, batch.input_block[0], batch.input_block[2], x, norm=batch.input_block[1]) is not None
        del kernels[:]
        routed = network._stem_route(group, group.input_block[0], group.input_block[2], x, norm=group.input_block[1])
        assert (routed is None) is (not gn) and kernels == ([('stem', 0), ('gn', code)] if gn else [])
        del kernels[:]
        got = group(x)
        trace = list(kernels)
        want = group0(x.as_subclass(torch.Tensor))
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), 'a norm was skipped'
    assert not [c for c in trace if c[0] in ('unit', 'stem', 'dwconv') and c[1] != 0], trace          # never an activation before the norm
    norms = len(_norm_positions(group))
    if gn:
        assert [c[0] for c in trace].count('gn') == norms == 17 and trace[:2] == [('stem', 0), ('gn', code)] and trace[-2:] == [('unit', 0), ('gn', code)]
        assert sorted(c[1] for c in trace if c[0] == 'gn') == [0] * 6 + [code] * 11               # behind a depthwise convolution: no activation
        assert [c[0] for c in trace].count('unit') == 10 and [c[0] for c in trace].count('dwconv') == 6
    else:
        assert not [c for c in trace if c[0] in ('gn', 'unit', 'stem')], trace                        # torch's convolutions and norms
        assert [c[0] for c in trace].count('dwconv') == 6 and [c[0] for c in trace].count('interleave') == 3


def test_conv5_declines_on_its_own(kernels, monkeypatch):
    group, batch, _, _ = _nets()
    x = torch.randn((1, 256, 3, 2), generator=tc.gen(8)).contiguous(memory_format=CL).as_subclass(_OnDevice)
    with torch.no_grad():
        network._conv5_forward(batch, x)
        assert kernels == [('unit', 1)]
        for gn, want in ((False, []), (True, [('unit', 0), ('gn', 1)])):
            monkeypatch.setattr(fused, 'GN', gn)
            del kernels[:]
            got = network._conv5_forward(group, x)
            assert kernels == want
            assert float((got - group.conv5(x)).abs().max()) <= 1e-5


def test_an_unsupported_norm_runs_through_torch(kernels, monkeypatch):
    """``GN`` on, but the norm's groups hold an odd number of channels: the convolution through the GEMM, the norm through torch."""
    monkeypatch.setattr(fused, 'GN', True)
    norm = nn.GroupNorm(4, 12)
    t = torch.randn((1, 12, 3, 2), generator=tc.gen(9)).contiguous(memory_format=CL).as_subclass(_OnDevice)
    with torch.no_grad():
        assert not fused.group_norm_supported(norm, t) and fused.group_norm_supported(nn.GroupNorm(3, 12), t)
        got = network._norm_act(norm, nn.ReLU(), t.clone())
        assert kernels == [] and torch.equal(got, torch.relu(F.group_norm(t, 4, norm.weight, norm.bias, norm.eps)))
        got = network._norm_act(nn.GroupNorm(3, 12), None, t.clone())
        assert kernels == [('gn', 0)]


# ---- group_norm_supported --------------------------------------------------------------------------------------------------------------

def _t(channels=24, dtype=torch.float32, hw=(9, 7)):
    return torch.zeros((2, channels) + hw, dtype=dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def test_supported_declines(monkeypatch):
    """Every reason on its own; the first case is the device."""
    monkeypatch.setattr(_lib, 'available', lambda: True)
    gn = nn.GroupNorm(4, 24)
    with torch.no_grad():
        assert fused.group_norm_supported(gn, _t()), 'the base case is not accepted: the cases below would show nothing'
        assert fused.group_norm_supported(nn.GroupNorm(4, 24, affine=False), _t())
        assert fused.group_norm_supported(nn.GroupNorm(29, 174), _t(348)[:, 174:])                      # a channel slice, 8-byte aligned
        assert not fused.group_norm_supported(gn, torch.zeros(2, 24, 9, 7).contiguous(memory_format=CL))  # a CPU tensor
        assert not fused.group_norm_supported(gn, _t(dtype=torch.bfloat16))
        assert not fused.group_norm_supported(gn, _t(dtype=torch.float64))
        with monkeypatch.context() as m:                                                                # autocast
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not fused.group_norm_supported(gn, _t())
        assert not fused.group_norm_supported(gn, _t().requires_grad_())
        # layouts the kernel does not take: NCHW, three dimensions, an odd pitch, a slice on a 4-byte boundary, other channels
        assert not fused.group_norm_supported(gn, torch.zeros(2, 24, 9, 7).as_subclass(_OnDevice))
        assert not fused.group_norm_supported(gn, _t()[0])
        assert not fused.group_norm_supported(gn, _t(25)[:, :24])
        assert not fused.group_norm_supported(gn, _t(26)[:, 1:25])
        assert not fused.group_norm_supported(gn, _t(32))
        assert not fused.group_norm_supported(gn, torch.zeros(2, 24, 0, 7).as_subclass(_OnDevice))
        # an odd number of channels per group
        assert not fused.group_norm_supported(nn.GroupNorm(8, 24), _t()) and not fused.group_norm_supported(nn.GroupNorm(24, 24), _t())
        assert fused.group_norm_supported(nn.GroupNorm(12, 24), _t())
        # another module, other parameters
        assert not fused.group_norm_supported(nn.BatchNorm2d(24), _t()) and not fused.group_norm_supported(nn.InstanceNorm2d(24), _t())
        assert not fused.group_norm_supported(nn.GroupNorm(4, 24).double(), _t())
        assert not fused.group_norm_supported(nn.GroupNorm(4, 24, eps=float('inf')), _t())
        assert not fused.group_norm_supported(nn.GroupNorm(4, 24, eps=-1.0), _t())
        # a group wider than the coefficients kernel's LDS holds
        assert not fused.group_norm_supported(nn.GroupNorm(1, 4098), _t(4098, hw=(1, 1)))
        assert fused.group_norm_supported(nn.GroupNorm(1, 2048), _t(2048, hw=(1, 1)))
        # a library without the symbol, no library
        with monkeypatch.context() as m:
            m.setattr(_lib, 'lib', lambda: object())
            assert not fused.group_norm_supported(gn, _t())
        monkeypatch.setattr(_lib, 'available', lambda: False)
        assert not fused.group_norm_supported(gn, _t())
    # parameters that autograd follows, with gradients enabled
    monkeypatch.setattr(_lib, 'available', lambda: True)
    assert not fused.group_norm_supported(gn, _t())
    assert fused.group_norm_supported(nn.GroupNorm(4, 24).requires_grad_(False), _t())


def test_the_switch_is_read_once_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(int(fused.GN))'
    for env, want in (({}, '0'), ({'OPA_GN': '1'}, '1'), ({'OPA_GN': '0'}, '0')):
        clean = {k: v for k, v in os.environ.items() if k != 'OPA_GN'}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])
    if 'OPA_GN' not in os.environ:
        assert fused.GN is False
    assert fused.GN_CHUNK_PIXELS == 512


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    for symbol in ('opa_groupnorm_workspace_bytes', 'opa_groupnorm_actp'):
        assert symbol + '(' in header and symbol in _lib.SYMBOLS and hasattr(_lib.lib(), symbol)
    assert '#define OPA_GN_CHUNK_PIXELS %d' % fused.GN_CHUNK_PIXELS in header
    lib = _lib.lib()
    assert lib.opa_groupnorm_workspace_bytes(2, 1000, 24) == 2 * 2 * 24 * 16 + 2 * 24 * 8
    assert lib.opa_groupnorm_workspace_bytes(1, 512, 8) == 8 * 16 + 8 * 8 and lib.opa_groupnorm_workspace_bytes(1, 513, 8) == 2 * 8 * 16 + 8 * 8
    for bad in ((0, 5, 8), (-1, 5, 8), (1, 0, 8), (1, -3, 8), (1, 5, 0), (1, 5, -8)):
        assert lib.opa_groupnorm_workspace_bytes(*bad) == 0


# ---- the command line -------------------------------------------------------------------------------------------------------------------

def test_cli():
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    saved = network.ShuffleNetV2K.layer_norm
    try:
        assert parser.parse_args([]).shufflenetv2k_layer_norm is None
        Predictor.configure(parser.parse_args([]))
        assert network.ShuffleNetV2K.layer_norm is None
        Predictor.configure(parser.parse_args(['--shufflenetv2k-instance-norm']))
        assert network.ShuffleNetV2K.layer_norm == 'instance'
        assert isinstance(network.factory('shufflenetv2k16').base_net.input_block[1], nn.InstanceNorm2d)
        Predictor.configure(parser.parse_args(['--shufflenetv2k-group-norm', '--shufflenetv2k-leaky-relu']))
        assert network.ShuffleNetV2K.layer_norm == 'group' and network.ShuffleNetV2K.leaky_relu is True
        base = network.factory('shufflenetv2k16').base_net
        assert isinstance(base.conv5[1], nn.GroupNorm) and base.conv5[1].num_groups == 29 and isinstance(base.conv5[2], nn.LeakyReLU)
        assert network.ShuffleNetV2K('shufflenetv2k16', layer_norm='instance').layer_norm == 'instance'      # the keyword wins
        with pytest.raises(SystemExit):
            parser.parse_args(['--shufflenetv2k-instance-norm', '--shufflenetv2k-group-norm'])
        Predictor.configure(parser.parse_args([]))
        assert network.ShuffleNetV2K.layer_norm is None and network.ShuffleNetV2K.leaky_relu is False
        assert isinstance(network.factory('shufflenetv2k16').base_net.input_block[1], nn.BatchNorm2d)
        dests = [a.dest for a in parser._actions if a.option_strings and a.option_strings[0] in ('--shufflenetv2k-instance-norm', '--shufflenetv2k-group-norm')]
        assert dests == ['shufflenetv2k_layer_norm'] * 2
    finally:
        network.ShuffleNetV2K.layer_norm = saved
        network.ShuffleNetV2K.leaky_relu = False
