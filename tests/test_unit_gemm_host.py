"""Host side of the ShuffleNetV2K unit route (``fused.conv1x1_unit_x3``, ``opa_gemm_unit_bias_act_f32x3``), without a GPU: the
derived weight operand, the decision (table, then size, never timing) and what the predicate declines."""
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network

import trunk_common as tc


def _net(seed):
    return network.optimize_for_inference_(tc.randomize_(network.factory('shufflenetv2k16', seed=seed), 10 + seed))


def _unit_convs(net):
    """Every convolution the unit route hands to the GEMM: the 1x1 convolutions of the units and conv5."""
    convs = [(name, m) for name, m in net.base_net.named_modules()
             if isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.groups == 1]
    assert len(convs) == 3 * 3 + 13 * 2 + 1, len(convs)
    return convs


def _fresh(conv):
    """``_unit_weight_of`` restated: -> (w3, bias)."""
    n, k = conv.out_channels, conv.in_channels
    npad, kpad = (n + 63) // 64 * 64, (k + 63) // 64 * 64
    wp = torch.zeros(npad, kpad)
    wp[:n, :k] = conv.weight.detach().float().reshape(n, k)
    bp = torch.zeros(npad)
    if conv.bias is not None:
        bp[:n] = conv.bias.detach().float()
    return fused.split_weight(wp), bp, wp


def test_unit_weight_shapes_padding_and_exact_split():
    net = _net(0)
    widths = set()
    for name, conv in _unit_convs(net):
        n, k = conv.out_channels, conv.in_channels
        widths.add((k, n))
        w3, bp = fused._unit_weight_of(conv)
        npad, kpad = (n + 63) // 64 * 64, (k + 63) // 64 * 64
        assert w3.dtype == torch.bfloat16 and tuple(w3.shape) == (3, npad, kpad) and w3.is_contiguous(), name
        assert bp.dtype == torch.float32 and tuple(bp.shape) == (npad,)
        assert not w3[:, n:].float().any() and not w3[:, :, k:].float().any() and not bp[n:].any()
        _, _, wp = _fresh(conv)
        assert torch.equal((w3[0].float() + w3[1].float()) + w3[2].float(), wp) and torch.equal(w3.float().sum(0), wp)
        assert torch.equal(bp[:n], conv.bias.detach())
        assert fused._unit_weight_of(conv)[0] is w3                   # cached
    assert {(24, 174), (174, 174), (348, 348), (696, 696), (1392, 1392)} <= widths, widths
    bare = nn.Conv2d(24, 174, 1, bias=False)
    assert not fused._unit_weight_of(bare)[1].any()                   # zeros where the convolution has no bias


def _load_other(net):
    net.load_state_dict(_net(1).state_dict(), strict=True)


def _scale_in_place(net):
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.5)


def _bfloat16_round_trip(net):
    net.to(torch.bfloat16).float()


def _replace_bias(net):
    for _, conv in _unit_convs(net):
        old = conv.bias
        new = nn.Parameter(torch.randn(conv.out_channels, generator=torch.Generator().manual_seed(7)))
        with torch.no_grad():
            while new._version < old._version:
                new.add_(0.0)
        conv.bias = new


@pytest.mark.parametrize('event', [_load_other, _scale_in_place, _bfloat16_round_trip, _replace_bias], ids=lambda f: f.__name__.strip('_'))
def test_unit_weight_follows_the_parameters(event):
    net = _net(0)
    keys = set(net.state_dict())
    before = [(name, [t.clone() for t in fused._unit_weight_of(conv)]) for name, conv in _unit_convs(net)]     # (fills the caches)
    event(net)
    changed = 0
    for (name, conv), (_, old) in zip(_unit_convs(net), before):
        w3, bp = fused._unit_weight_of(conv)
        want3, wantb, _ = _fresh(conv)
        assert torch.equal(w3, want3) and torch.equal(bp, wantb), name
        changed += int(not (torch.equal(w3, old[0]) and torch.equal(bp, old[1])))
    assert changed == len(before)                                     # (the event did change every one of them)
    assert set(net.state_dict()) == keys and not any('_opa' in k for k in keys)
    assert all(conv.bias is not None for _, conv in _unit_convs(net))  # the folded convolutions keep their bias parameter


def test_enable_fused_of_the_network_changes_no_parameter_or_buffer():
    net = network.fuse_conv_bn_(tc.randomize_(network.factory('shufflenetv2k16', seed=0), 3))
    base = net.base_net
    state = {k: v.clone() for k, v in base.state_dict().items()}
    assert not base.fused
    base.enable_fused_()
    assert base.fused and set(base.state_dict()) == set(state) and all(torch.equal(v, state[k]) for k, v in base.state_dict().items())


@pytest.fixture
def decision(monkeypatch):
    def no_timing(*args, **kwargs):
        raise AssertionError('the unit decision timed something')
    monkeypatch.setattr(fused, '_time_ms', no_timing)
    monkeypatch.setattr(fused, 'FORCE_PICK', None)
    saved = fused.choices()
    fused.set_choices({}, replace=True)
    yield lambda m, partner=True: fused.pick('unit', m, 174, 174, partner, False, lambda: 'x3', lambda: 'conv', timing=False)
    fused.set_choices(saved, replace=True)


@pytest.mark.parametrize('capturing', [False, True])
@pytest.mark.parametrize('ranks', [1, 4])
def test_the_unit_decision(decision, monkeypatch, capturing, ranks):
    """Table entry first, else by size ('x3' from 16384 pixels), ``FORCE_PICK`` over both; nothing is ever timed."""
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: capturing)
    monkeypatch.setattr(fused, '_in_multi_rank_job', lambda: ranks > 1)
    assert decision(16383) == 'conv' and decision(16384) == 'x3' and decision(1) == 'conv' and decision(10 ** 6) == 'x3'
    key = ('torch.float32/unit', 16383, 174, 174, True, False)
    assert fused.choices()[key] == 'conv' and fused.choices()[('torch.float32/unit', 16384, 174, 174, True, False)] == 'x3'
    fused.set_choices({key: 'x3', ('torch.float32/unit', 20000, 174, 174, False, False): 'conv'}, replace=True)
    assert decision(16383) == 'x3' and decision(20000, partner=False) == 'conv' and decision(20000) == 'x3'
    monkeypatch.setattr(fused, 'FORCE_PICK', 'conv')
    assert decision(16383) == 'conv' and decision(10 ** 6) == 'conv'
    monkeypatch.setattr(fused, 'FORCE_PICK', 'x3')
    assert decision(20000, partner=False) == 'x3' and decision(1) == 'x3'


def test_pick_still_times_by_default(monkeypatch):
    """``timing`` defaults to today's behaviour: an unknown shape outside a capture, one rank, is timed."""
    calls = []
    monkeypatch.setattr(fused, '_time_ms', lambda fn, reps=3: calls.append(fn()) or (1.0 if fn() == 'x3' else 2.0))
    monkeypatch.setattr(fused, 'FORCE_PICK', None)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    monkeypatch.setattr(fused, '_in_multi_rank_job', lambda: False)
    saved = fused.choices()
    try:
        fused.set_choices({}, replace=True)
        assert fused.pick('head', 10, 64, 64, False, False, lambda: 'x3', lambda: 'conv') == 'x3' and len(calls) == 2
    finally:
        fused.set_choices(saved, replace=True)


def test_what_the_predicate_declines(monkeypatch):
    monkeypatch.setattr(fused, 'X3_UNIT', True)
    monkeypatch.setattr(fused, 'X3_TERMS', 6)
    cl = torch.channels_last
    conv_ok, operand_ok = (functools.partial(f, fused.UNIT_MODE_X3) for f in (fused._unit_conv_ok, fused._unit_operand_ok))
    conv = nn.Conv2d(174, 174, 1).requires_grad_(False)
    x = torch.randn(2, 348, 5, 7).contiguous(memory_format=cl)
    x1, x2 = x.chunk(2, dim=1)
    assert conv_ok(conv) and operand_ok(x2, 174) and operand_ok(x1, 174)     # the positive controls
    assert fused._pixel_stride(x2) == 348 and x2.data_ptr() % 16 == 8
    assert not fused.unit_conv_x3_supported(conv, x2)                 # not on the GPU
    assert not conv_ok(nn.Conv2d(174, 173, 1)) and not conv_ok(nn.Conv2d(173, 174, 1))         # odd widths
    assert not conv_ok(nn.Conv2d(174, 174, 3, padding=1)) and not conv_ok(nn.Conv2d(174, 174, 1, stride=2))
    assert not conv_ok(nn.Conv2d(174, 174, 1, groups=2)) and not conv_ok(nn.Conv2d(174, 174, 1).bfloat16())
    assert not operand_ok(x2.bfloat16(), 174)             # bfloat16
    assert not operand_ok(torch.randn(2, 174, 5, 7), 174)  # channels outermost
    assert not operand_ok(x2, 172) and not operand_ok(x[:, 1:175], 174)                         # 4 bytes off
    assert not operand_ok(x2.clone(memory_format=torch.preserve_format).requires_grad_(True), 174)
    monkeypatch.setattr(fused, 'X3_UNIT', False)
    assert not conv_ok(conv)
    monkeypatch.setattr(fused, 'X3_UNIT', True)
    monkeypatch.setattr(fused, 'X3_TERMS', 0)
    assert not conv_ok(conv)
