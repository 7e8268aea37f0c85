"""The ShuffleNetV2K unit and ``conv5`` on the split-operand GEMM's unit mode, one MODULE at a time (real kernels, MI355X), built
like ``test_gpu_trunk_routes.py``: the module unfused, in ``eval()``, with random BatchNorm statistics; ``ref64`` its ``double()`` copy;
``e0`` the error of the SAME unfused float32 module (PyTorch / MIOpen; the median of nine calls) against ``ref64``; the module under
test its folded + ``enable_fused_()`` copy, channels_last.  ``err = max |got - ref64| / max |ref64|`` and the same as an rms.

1. ``err <= 2 * e0`` (max and rms; 2 = two errors of size ``e0``), seeds 0, 1, 2; the per-seed lines go to
   ``profiles/unit_gemm/route_errors.log`` (printed here as ``UNITROUTE`` lines);
2. the second call's launch trace is exactly ``unit, dwconv, unit`` (a first unit: ``dwconv, unit, unit, dwconv, unit``);
3. first call == second call == a call on a fresh clone, bit for bit (no MIOpen on the route); the input is unchanged;
4. the default decision (empty table): by size alone, never timed; the switches; bfloat16; a first call under capture;
5. the operands after a parameter event; the whole k16 network with the route forced on against the route off."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network

import trunk_common as tc

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
CL = torch.channels_last
_LAUNCHERS = {'conv1x1_unit_x3': 'unit', 'dwconv_bias_act': 'dwconv', 'channel_interleave': 'interleave', 'bias_act_': 'bias_act',
              'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3', 'head_conv_x3': 'head_x3', 'head_epilogue': 'head_epilogue'}


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder; the switches and the choice table saved and restored; the table starts EMPTY, nothing forced."""
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_UNIT',))


def _make(inp, oup, first, stride, seed):
    return tc.randomize_(network._InvertedResidualK(inp, oup, first, stride=stride), seed)


# the real widths: k16 stage 2 (split), k16 stage 2 and 3 (first units), k30 stage 2 (split)
UNITS = {'k16-348': (348, 348, False, 1), 'k16-first-24': (24, 348, True, 2), 'k16-first-348': (348, 696, True, 2),
         'k30-512': (512, 512, False, 1)}
NEW = {False: ['unit', 'dwconv', 'unit'], True: ['dwconv', 'unit', 'unit', 'dwconv', 'unit']}
OLD = {False: ['miopen:branch2.0', 'dwconv', 'miopen:branch2.5', 'interleave'],
       True: ['dwconv', 'miopen:branch1.2', 'miopen:branch2.0', 'dwconv', 'miopen:branch2.5', 'interleave']}


def _key(spec, shape):
    inp, oup, first, stride = spec
    m = shape[0] * ((shape[2] - 1) // stride + 1) * ((shape[3] - 1) // stride + 1)
    return ('torch.float32/unit', m, oup // 2, oup // 2, True, False)


@functools.lru_cache(maxsize=None)
def _reference(spec, shape, seed):
    """-> (the unfused module on the CPU, x, ref64, e0)."""
    module = _make(*spec, seed)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1000 + seed)).relu().cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(module).double().cuda()(x.double())
        plain = copy.deepcopy(module).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0


def _optimized(module, rec, dtype=torch.float32):
    return rec.watch(tc.optimized(module).cuda().to(dtype).to(memory_format=CL))


@pytest.mark.parametrize('unit', list(UNITS))
def test_unit_on_the_split_operand_gemm(rec, unit):
    spec = UNITS[unit]
    shape = (3, spec[0], 15, 11)
    rows = []
    for seed in SEEDS:
        module, x, ref64, e0 = _reference(spec, shape, seed)
        opt = _optimized(module, rec)
        table = {_key(spec, shape): 'x3'}
        fused.set_choices(table, replace=True)
        got, trace = tc.forward_checks(opt, x, rec)
        assert trace == NEW[spec[2]], trace
        assert fused.choices() == table and rec.timed == 0
        assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape
        err = tc.errors(got, ref64)
        print('UNITROUTE %s float32 forced | %s | seed %d | e0 max %.3e rms %.3e | err max %.3e rms %.3e | err/e0 max %.2f rms %.2f'
              % (unit, ' '.join(trace), seed, e0[0], e0[1], err[0], err[1], err[0] / e0[0], err[1] / e0[1]))
        rows.append((seed, err, e0))
        # ... and the table's other side IS today's route, launch for launch
        fused.set_choices({_key(spec, shape): 'conv'}, replace=True)
        _, trace = tc.forward_checks(opt, x, rec)
        assert trace == OLD[spec[2]], trace
    bad = [(seed, err, e0) for seed, err, e0 in rows if err[0] > 2 * e0[0] or err[1] > 2 * e0[1]]
    assert not bad, bad


def test_default_decision_is_by_size_and_never_timed(rec):
    spec = UNITS['k16-348']
    module = _make(*spec, 0)
    small = torch.randn((3, 348, 15, 11), generator=torch.Generator().manual_seed(1)).relu().cuda().contiguous(memory_format=CL)
    large = torch.randn((2, 348, 96, 96), generator=torch.Generator().manual_seed(2)).relu().cuda().contiguous(memory_format=CL)
    assert 2 * 96 * 96 == 18432
    opt = _optimized(module, rec)
    _, trace = tc.forward_checks(opt, small, rec)
    assert trace == OLD[False] and fused.choices() == {_key(spec, small.shape): 'conv'}, (trace, fused.choices())
    got, trace = tc.forward_checks(opt, large, rec)
    assert trace == NEW[False] and fused.choices()[_key(spec, large.shape)] == 'x3' and rec.timed == 0, trace
    # X3_UNIT off: today's trace at any size, no decision asked for
    fused.set_choices({}, replace=True)
    fused.X3_UNIT = False
    off, trace = tc.forward_checks(opt, large, rec)
    assert trace == OLD[False] and fused.choices() == {} and rec.timed == 0
    assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max()) and not torch.equal(off, got)
    fused.X3_UNIT = True
    # what the predicate declines on the GPU, next to a positive control
    conv, x2 = opt.branch2[0], small.chunk(2, dim=1)[1]
    assert fused.unit_conv_x3_supported(conv, x2) and fused.unit_conv_x3_supported(conv, x2, small.chunk(2, dim=1)[0])
    assert not fused.unit_conv_x3_supported(conv, x2.bfloat16()) and not fused.unit_conv_x3_supported(conv, small[:, 1:175])
    assert not fused.unit_conv_x3_supported(conv, x2.contiguous()) and not fused.unit_conv_x3_supported(conv, x2, small[:, :172])
    assert not fused.unit_conv_x3_supported(conv, x2.clone(memory_format=torch.preserve_format).requires_grad_(True))
    assert not fused.unit_conv_x3_supported(nn.Conv2d(174, 173, 1).cuda(), x2)
    # bfloat16: today's trace even with the route forced
    fused.FORCE_PICK = 'x3'
    opt16 = _optimized(module, rec, torch.bfloat16)
    _, trace = tc.forward_checks(opt16, large.bfloat16().contiguous(memory_format=CL), rec)
    assert trace == OLD[False] and rec.timed == 0, trace


def test_first_call_under_capture(rec):
    """18 432 pixels, empty table, the FIRST call inside a stream capture: the new route by size; the replay equals the eager run
    with the remembered choice bit for bit."""
    spec = UNITS['k16-348']
    for seed in SEEDS:
        opt = _optimized(_make(*spec, seed), rec)
        x = torch.randn((2, 348, 96, 96), generator=torch.Generator().manual_seed(seed)).relu().cuda().contiguous(memory_format=CL)
        x0 = x.clone()
        fused.set_choices({}, replace=True)
        rec.trace.clear()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            with torch.no_grad():
                y = opt(x)
        trace = list(rec.trace)
        graph.replay()
        torch.cuda.synchronize()
        got = y.clone()
        with torch.no_grad():
            eager = opt(x)
        graph.replay()
        torch.cuda.synchronize()
        assert trace == NEW[False] and rec.timed == 0 and fused.choices() == {_key(spec, x.shape): 'x3'}, trace
        assert torch.equal(got, eager) and torch.equal(y, got) and torch.equal(x, x0) and got.isfinite().all()


def _event(opt, other, name):
    with torch.no_grad():
        if name == 'load_state_dict':
            opt.load_state_dict(other.state_dict(), strict=True)
        elif name == 'in_place':
            for p in opt.parameters():
                p.mul_(1.25)
        else:
            opt.to(torch.bfloat16).float()


@pytest.mark.parametrize('event', ['load_state_dict', 'in_place', 'bfloat16_round_trip'])
@pytest.mark.parametrize('unit', ['k16-348', 'k16-first-24'])
def test_forward_after_a_parameter_event(rec, unit, event):
    """A forward (which fills the operand caches), the event, a forward: bit for bit the output of a freshly optimized unit that
    holds the same parameters."""
    spec = UNITS[unit]
    x = torch.randn((3, spec[0], 15, 11), generator=torch.Generator().manual_seed(5)).relu().cuda().contiguous(memory_format=CL)
    fused.FORCE_PICK = 'x3'
    opt = tc.optimized(_make(*spec, 0)).cuda().to(memory_format=CL)
    other = tc.optimized(_make(*spec, 1)).cuda().to(memory_format=CL)
    with torch.no_grad():
        before = opt(x)
        _event(opt, other, event)
        rec.trace.clear()
        after = opt(x)
        assert rec.trace == NEW[spec[2]], rec.trace
        fresh = tc.optimized(_make(*spec, 0)).cuda().to(memory_format=CL)
        fresh.load_state_dict(opt.state_dict(), strict=True)
        want = fresh(x)
    assert not torch.equal(before, after)
    assert torch.equal(after, want), 'stale operand: max |delta| %.3g' % (after - want).abs().max().item()


def test_shufflenetv2k16_with_and_without_the_unit_route(rec):
    """The whole float32 network: the heads with the route forced on agree with the route off within 1e-4 of each head's largest
    magnitude (the bar of ``test_resnet50_trunk_with_and_without_the_split_operand_kernel``), and the new launcher really ran:
    3 first units x 3 + 13 units x 2 + conv5 + the two heads (1392 input channels: no multiple of 64) = 38 times."""
    torch.manual_seed(5)
    net = network.factory('shufflenetv2k16').cuda()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    network.optimize_for_inference_(net)
    net = net.to(memory_format=CL)
    x = torch.randn((2, 3, 161, 193), device='cuda').contiguous(memory_format=CL)
    with torch.no_grad():
        fused.FORCE_PICK = 'conv'
        a = net(x)
        assert 'unit' not in rec.trace
        rec.trace.clear()
        fused.FORCE_PICK = 'x3'
        b = net(x)
        units = rec.trace.count('unit')
    assert units == 38 and 'head_x3' not in rec.trace, (units, rec.trace)
    assert 'interleave' not in rec.trace and 'bias_act' not in rec.trace
    for u, v in zip(a, b):
        assert float((u - v).abs().max()) <= 1e-4 * float(u.abs().max()), float((u - v).abs().max())
    assert not all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('which', [0, 1], ids=['cif', 'caf'])
def test_head_with_1392_input_channels(rec, which):
    """``CompositeField4`` behind k16 (1392 input channels, ``head_conv_x3`` declines): the dense unit mode, 340 / 684 output
    channels stored without a padded pitch; against the float64 head at ``2 * e0`` like the units; today's route below the size line."""
    from openpifpaf_amd import headmeta
    meta = headmeta.cocokp_metas()[which]
    for seed in SEEDS:
        head = tc.randomize_(network.CompositeField4(meta, 1392), seed)
        head.fused_epilogue = False
        x = torch.randn((3, 1392, 21, 19), generator=torch.Generator().manual_seed(2000 + seed)).relu().cuda().contiguous(memory_format=CL)
        assert not fused.head_conv_x3_supported(head.conv, x)
        with torch.no_grad():
            ref64 = copy.deepcopy(head).double().cuda()(x.double())
            opt = rec.watch(copy.deepcopy(head).cuda().to(memory_format=CL))
            fused.FORCE_PICK = 'conv'
            errs = [tc.errors(opt(x), ref64) for _ in range(9)]
            e0 = tuple(sorted(e[i] for e in errs)[4] for i in (0, 1))
            fused.FORCE_PICK = None
            fused.set_choices({}, replace=True)
            _, trace = tc.forward_checks(opt, x, rec)
            assert trace == ['miopen:conv'] and rec.timed == 0, trace              # 1197 pixels: by size
            fused.set_choices({('torch.float32/unit', 3 * 21 * 19, 1392, head.conv.out_channels, False, False): 'x3'}, replace=True)
            got, trace = tc.forward_checks(opt, x, rec)
        assert trace == ['unit'] and rec.timed == 0, trace
        err = tc.errors(got, ref64)
        print('UNITROUTE head-%s float32 forced | %s | seed %d | e0 max %.3e rms %.3e | err max %.3e rms %.3e | err/e0 max %.2f rms %.2f'
              % (('cif', 'caf')[which], ' '.join(trace), seed, e0[0], e0[1], err[0], err[1], err[0] / e0[0], err[1] / e0[1]))
        assert err[0] <= 2 * e0[0] and err[1] <= 2 * e0[1], (err, e0)
