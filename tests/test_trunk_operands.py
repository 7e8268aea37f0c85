"""Every operand the trunk hands to a kernel is DERIVED from a parameter (a transformed, split, padded or transposed copy).  After
the parameter changes -- ``load_state_dict`` into an optimized network, an in-place update, a dtype round trip, a Parameter
replaced by a new one -- the operand of the next launch must be the one derived from the current parameter, not a snapshot.
CPU only: the lookups (``fused._*_of``, ``winograd.filter_of`` / ``split_filter_of``, ``_InvertedResidualK.taps_of``) run without
a launch; each is compared with an independent restatement of the derivation."""
import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network, winograd

import trunk_common as tc


def _net(name, seed):
    return network.optimize_for_inference_(tc.randomize_(network.factory(name, seed=seed), 10 + seed))


def _pad_rows(t, n):
    out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=torch.float32)
    out[:t.shape[0]] = t
    return out


def _operands(net):
    """[(name, what the next launch would be handed, the same derived here from the current parameters)]"""
    out = []
    for name, m in net.named_modules():
        if isinstance(m, (network._Bottleneck, network._BasicBlock)):
            for attr, conv in (('wino_u', m.conv2), ('wino_u1', m.conv1), ('wino_u2', m.conv2)):
                if hasattr(m, attr):
                    out.append((name + '.' + attr, getattr(m, attr).float(), winograd.transform_filter(conv.weight.float(), 2)))
                    if conv.weight.dtype == torch.float32:
                        out.append((name + '.' + attr + '/split', winograd.split_filter_of(conv), winograd.split_filter(conv.weight)))
        if isinstance(m, network._Bottleneck) and m.conv1.weight.dtype == torch.float32:
            for conv in (m.conv1, m.conv3):
                w2d = conv.weight.reshape(conv.out_channels, conv.in_channels)
                out.append((name + '/w3', fused._split_weight_of(conv, w2d), fused.split_weight(w2d.detach().clone())))
            if m.conv2.stride != (1, 1):
                w = m.conv2.weight.detach()
                out.append((name + '.conv2/w3_3x3', fused._split_weight_3x3_of(m.conv2),
                            fused.split_weight(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1))))
            if m.downsample is not None:
                dconv = m.downsample[0]
                both = torch.cat((m.conv3.weight.detach().flatten(1), dconv.weight.detach().flatten(1)), dim=1)
                for a_bias in (None, m.fb2):
                    w3, ab = fused._pair_weight_of(m.conv3, dconv, a_bias)
                    out.append((name + '/pair', w3, fused.split_weight(both)))
                    if a_bias is not None:
                        out.append((name + '/pair a_bias', ab, torch.cat((m.fb2.detach().float(), torch.zeros(dconv.in_channels)))))
        if isinstance(m, network.Resnet) and m.input_block[0].weight.dtype == torch.float32:
            w = m.input_block[0].weight.detach()
            wp = torch.zeros((w.shape[0], 8, 8, 4))
            wp[:, :7, :7, :3] = w.permute(0, 2, 3, 1)
            out.append((name + '/stem', fused._stem_weight_of(m.input_block[0]), fused.split_weight(wp.reshape(w.shape[0], 256))))
        if isinstance(m, network.CompositeField4) and m.conv.weight.dtype == torch.float32:
            n, k = m.conv.out_channels, m.conv.in_channels
            npad, kpad = (n + 63) // 64 * 64, (k + 63) // 64 * 64       # (k16's heads have 1392 input channels: the unit mode's K tail)
            w3, bp = fused._unit_weight_of(m.conv)
            wp = torch.zeros((npad, kpad))
            wp[:n, :k] = m.conv.weight.detach().flatten(1)
            out.append((name + '/head w3', w3, fused.split_weight(wp)))
            out.append((name + '/head bias', bp, _pad_rows(m.conv.bias.detach(), npad)))
        if isinstance(m, nn.Conv2d) and hasattr(m, 'w_taps'):
            k = m.kernel_size[0]
            out.append((name + '.w_taps', network._InvertedResidualK.taps_of(m), m.weight.detach().reshape(m.out_channels, k * k).t()))
    return out


def _load_other(net, name):
    net.load_state_dict(_net(name, 1).state_dict(), strict=True)


def _scale_in_place(net, name):
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.5)
        for n, b in net.named_buffers():
            if n.rsplit('.', 1)[-1].startswith('fb'):
                b.add_(0.25)


def _bfloat16_round_trip(net, name):
    net.to(torch.bfloat16).float()


def _replace_head_bias(net, name):
    for head in net.head_nets:
        old = head.conv.bias
        new = nn.Parameter(torch.randn(head.conv.out_channels, generator=torch.Generator().manual_seed(7)))
        with torch.no_grad():
            while new._version < old._version:         # (a key that held the bias's version counter alone would not see it)
                new.add_(0.0)
        head.conv.bias = new


EVENTS = {'load_state_dict': _load_other, 'in_place': _scale_in_place, 'bfloat16_round_trip': _bfloat16_round_trip,
          'head_bias_replaced': _replace_head_bias}
EXPECTED = {'resnet50': ('wino_u', '/split', '/w3', '/w3_3x3', '/pair', '/pair a_bias', '/stem', '/head w3', '/head bias'),
            'resnet18': ('wino_u1', 'wino_u2', '/split', '/stem', '/head w3', '/head bias'),
            'shufflenetv2k16': ('.w_taps', '/head w3', '/head bias')}


@pytest.mark.parametrize('event', list(EVENTS))
@pytest.mark.parametrize('name', list(EXPECTED))
def test_operands_follow_the_parameters(name, event):
    net = _net(name, 0)
    before = [(n, got.clone(), want) for n, got, want in _operands(net)]          # (fills every cache)
    assert all(any(n.endswith(kind) for n, _, _ in before) for kind in EXPECTED[name]), [n for n, _, _ in before]
    assert all(torch.equal(got, want) for _, got, want in before), [n for n, got, want in before if not torch.equal(got, want)]
    EVENTS[event](net, name)
    after = _operands(net)
    assert [n for n, _, _ in after] == [n for n, _, _ in before]
    stale = [n for n, got, want in after if got.shape != want.shape or not torch.equal(got, want)]
    assert not stale, stale
    changed = sum(1 for (_, a, _), (_, b, _) in zip(before, after) if not torch.equal(a, b))
    assert changed >= (2 if event == 'head_bias_replaced' else len(after) - 2), (changed, len(after))     # (the event did change them)


def test_state_of_an_optimized_network_keeps_its_keys():
    """Checkpoints written from an optimized network before the operands became derived hold ``w_taps`` and no ``wino_u*``:
    they load with ``strict=True``, and a new one has the same keys."""
    keys = set(_net('shufflenetv2k16', 0).state_dict())
    assert any(k.endswith('.w_taps') for k in keys) and not any('_opa' in k for k in keys)
    keys50 = set(_net('resnet50', 0).state_dict())
    assert not any('wino' in k or '_opa' in k for k in keys50) and any(k.endswith('.fb2') for k in keys50)
    net = _net('resnet50', 0)
    _operands(net)
    assert set(net.state_dict()) == keys50                            # (the caches are no part of it either)


def test_in_place_events_are_seen_by_the_block_attributes_too():
    block = tc.optimized(tc.bottleneck(256, 64, 1, False, 0))
    first = block.wino_u
    assert block.wino_u is first                                      # cached
    old = first.clone()
    with torch.no_grad():
        block.conv2.weight.mul_(2.0)
    assert torch.equal(block.wino_u, winograd.transform_filter(block.conv2.weight, 2)) and not torch.equal(block.wino_u, old)
    assert block.wino_u is first                                      # ... and overwritten where it is kept: a HIP graph may hold its address
    assert not hasattr(tc.bottleneck(256, 64, 1, False, 0), 'wino_u')                  # not optimized
    assert not hasattr(tc.optimized(tc.bottleneck(64, 64, 2, True, 0)), 'wino_u')      # strided
