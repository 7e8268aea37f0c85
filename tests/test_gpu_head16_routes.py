"""Whole networks with the 16-bit head route (``fused.HEAD16``: csrc/head16.hip), with the method of ``test_gpu_f16_routes.py``:
``network.factory('resnet18')`` and ``'resnet50'`` with random BatchNorm statistics, optimized, cast to bfloat16 (both) and float16
(resnet18), channels_last, input 2 x 3 x 97 x 65, ``OPA_CONV1X1=gemm`` (real kernels, MI355X).  The trunk's own 16-bit switches are on
(bfloat16: ``CONV3_BF16``, ``PAIR_BF16``, ``STEM7_BF16``; float16: ``F16``), so that the trunk repeats bit for bit and both sides of every
comparison read the same trunk output.

(a) ``HEAD16`` on: the forward launches the new symbol twice -- once per head -- and calls no head's ``nn.Conv2d``, no
    ``opa_head_epilogue``; off: the parent's launches -- both heads' ``nn.Conv2d``, ``opa_head_epilogue`` twice, the new symbol never.
(b) per head, ``e_on`` / ``e_off``: the rms error of the fields against the float32 forward of the same weights upcast, relative to
    that forward's rms, route on / off ON THE SAME TRUNK OUTPUT.  Both hold the same propagated trunk error; the route off adds the
    rounding of the convolution's output to 16 bits, independent of it, so the expectation is ``e_on < e_off``.  Asserted:
    ``e_on <= 1.005 * e_off`` -- the half percent is for the cross term's sampling noise over about 10^5 elements.  Printed as
    ``HEAD16ROUTE`` lines; one run is kept as profiles/head16/route_errors.log.
(c) the whole forward with the route on repeats bit for bit (the heads torch runs do not, ``test_gpu_f16_routes.py``)."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F16, BF16 = torch.float16, torch.bfloat16
CASES = {'resnet18-bfloat16': ('resnet18', BF16), 'resnet50-bfloat16': ('resnet50', BF16), 'resnet18-float16': ('resnet18', F16)}
TRUNK_SWITCHES = {BF16: ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16'), F16: ('F16',)}
NEW = {BF16: 'opa_head_conv_fields_bf16', F16: 'opa_head_conv_fields_f16'}


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the plain 1x1 choice pinned to the GEMM,
    nothing timed; every 16-bit switch off and restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    monkeypatch.setenv('OPA_CONV1X1', 'gemm')
    monkeypatch.setattr(fused, '_CHOICE', {})
    for name in ('HEAD16', 'F16', 'CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16', 'GCONV_BF16', 'UNIT_BF16'):
        monkeypatch.setattr(fused, name, False)
    return symbols


@functools.lru_cache(maxsize=None)
def _case(case):
    """-> (the optimized network cast to the case's dtype, x, the head fields of its float32 copy on x upcast, as float64); computed
    once and left unchanged."""
    name, dt = CASES[case]
    net = network.factory(name, seed=0).cuda()
    torch.manual_seed(100)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    network.optimize_for_inference_(net)
    x = torch.randn((2, 3, 97, 65), device='cuda').to(dt).contiguous(memory_format=CL)
    cast = net.to(dt).to(memory_format=CL).requires_grad_(False)
    table = fused.choices()                                            # (the float32 forward may enter its decisions: put the table back)
    try:
        with torch.no_grad():
            ref = tuple(f.double() for f in copy.deepcopy(cast).float()(x.float()))
    finally:
        fused.set_choices(table, replace=True)
    assert all(f.isfinite().all() for f in ref)
    return cast, x, ref


def _switches(monkeypatch, dt, head16):
    for name in TRUNK_SWITCHES[dt]:
        monkeypatch.setattr(fused, name, True)
    monkeypatch.setattr(fused, 'HEAD16', head16)


def _run(module, x):
    with torch.no_grad():
        out = module(x)
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_heads_run_on_the_new_kernel_and_not_with_the_switch_off(launches, monkeypatch, case):
    net, x, ref = _case(case)
    dt = CASES[case][1]
    convs = {m: n for n, m in net.named_modules() if isinstance(m, nn.Conv2d)}
    called = []
    hooks = [m.register_forward_hook(lambda mod, args, out: called.append(convs[mod])) for m in convs]
    try:
        _switches(monkeypatch, dt, True)
        del launches[:]
        out = _run(net, x)
        on, called_on = list(launches), list(called)
        assert on.count(NEW[dt]) == 2 and 'opa_head_epilogue' not in on
        assert not [n for n in called_on if n.startswith('head_nets.')]
        assert len(out) == len(ref) and all(f.dtype == torch.float32 and f.shape == r.shape and f.isfinite().all() for f, r in zip(out, ref))
        again = _run(net, x)                                           # (c) the whole forward repeats bit for bit
        assert all(torch.equal(_bits(f), _bits(g)) for f, g in zip(out, again))
        _switches(monkeypatch, dt, False)
        del launches[:], called[:]
        off = _run(net, x)
        assert not [s for s in launches if s.startswith('opa_head_conv_fields')] and launches.count('opa_head_epilogue') == 2
        assert sorted(n for n in called if n.startswith('head_nets.')) == ['head_nets.0.conv', 'head_nets.1.conv']
        assert [s for s in launches if s != 'opa_head_epilogue'] == [s for s in on if s != NEW[dt]]              # the trunk's launches as they were
        assert [n for n in called if not n.startswith('head_nets.')] == called_on
        assert all(f.shape == g.shape and g.isfinite().all() for f, g in zip(out, off))
    finally:
        for h in hooks:
            h.remove()


def _rms_error(got, ref):
    return (float(((got.double() - ref) ** 2).sum()) / float((ref ** 2).sum())) ** 0.5


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_fields_are_no_further_from_float32_than_with_the_switch_off(launches, monkeypatch, case):
    net, x, ref = _case(case)
    dt = CASES[case][1]
    _switches(monkeypatch, dt, False)
    features = _run(net.base_net, x)                                   # ONE trunk output for both sides
    assert torch.equal(features.contiguous().view(torch.int16), _run(net.base_net, x).contiguous().view(torch.int16))
    rows = []
    for i, head in enumerate(net.head_nets):
        monkeypatch.setattr(fused, 'HEAD16', False)
        e_off = _rms_error(_run(head, features), ref[i])
        monkeypatch.setattr(fused, 'HEAD16', True)
        del launches[:]
        e_on = _rms_error(_run(head, features), ref[i])
        assert launches == [NEW[dt]]
        print('HEAD16ROUTE %s | head %d (%s) | e_off (torch conv + opa_head_epilogue) %.5e | e_on (one kernel) %.5e | e_on / e_off %.4f'
              % (case, i, head.meta.name, e_off, e_on, e_on / e_off))
        rows.append((i, e_on, e_off))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > 1.005 * r[2]]
    assert not bad, bad
