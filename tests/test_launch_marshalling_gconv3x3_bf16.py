"""What ``fused.gconv3x3_bias_act_bf16`` hands to the C ABI (``opa_gconv3x3_act_bf16``), argument by argument, without a GPU -- recorded
like ``test_launch_marshalling.py`` records its cases (on the harness of ``abi_tables.py``) and compared with
``golden/launch_marshalling_gconv3x3_bf16.json`` (``golden/make_golden_abi.py launch_marshalling_gconv3x3_bf16``).

Operands: a dense channels-last bfloat16 tensor; with and without the folded bias, every (stride, dilation) the kernel takes, a group
width of each instantiation (4: the half-K one, 64: the full one), ``relu`` on and off.  The pointers handed over are the tensor's own
(``x``: no copy), the derived operands the launcher keeps on the module (``w``: ``[C][9][64]`` bfloat16, ``bias``: FLOAT32) and the
output it allocates (``new0``)."""
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm

GOLDEN = at.golden('launch_marshalling_gconv3x3_bf16')
BF16 = torch.bfloat16
SYMBOL = 'opa_gconv3x3_act_bf16'
B, H, W = 2, 7, 5
C = 128
MODES = [(1, 1), (2, 1), (1, 2), (1, 4)]            # (stride, dilation)
WIDTHS = [4, 64]


def _out_hw(s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def _conv(cg, s, d):
    return nn.Conv2d(C, C, 3, s, d, dilation=d, groups=C // cg, bias=False).to(BF16).requires_grad_(False)


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor})}"""
    out = {}
    for s, d in MODES:
        for cg in WIDTHS:
            for has_bias in (True, False):
                for relu in (True, False):
                    conv, x = _conv(cg, s, d), tlm._act(B, C, H, W, BF16)
                    bias = torch.zeros(C, dtype=BF16) if has_bias else None
                    out['gconv3x3_bf16/s%dd%d/cg%d/bias%d/relu%d' % (s, d, cg, has_bias, relu)] = (
                        lambda conv=conv, x=x, bias=bias, relu=relu: fused.gconv3x3_bias_act_bf16(conv, x, bias, relu=relu),
                        {'x': x}, lambda conv=conv: tlm._cached_on(conv, 'w', 'bias'))
    # ``relu`` left to its default
    conv, x, bias = _conv(8, 1, 1), tlm._act(B, C, H, W, BF16), torch.zeros(C, dtype=BF16)
    out['gconv3x3_bf16/s1d1/cg8/bias1/relu-default'] = (
        lambda: fused.gconv3x3_bias_act_bf16(conv, x, bias), {'x': x}, lambda: tlm._cached_on(conv, 'w', 'bias'))
    return out


def _check(case_id, out):
    s = int(case_id.split('/')[1][1])
    assert out.dtype == BF16 and out.is_contiguous(memory_format=torch.channels_last), case_id
    assert tuple(out.shape) == (B, C) + _out_hw(s), case_id


def record_all():
    """-> {case id: [[symbol, [arguments]], ...]}"""
    return at.record_all(cases(), check=_check)


def test_every_launch_hands_over_what_the_golden_file_says():
    got = at.marshalling(cases(), GOLDEN, check=_check)
    assert all([name for name, _ in calls] == [SYMBOL] for calls in got.values())


def test_the_arguments_are_the_tensors_and_the_convolutions_own():
    """x, w, bias, out, batch, h_in, w_in, channels, group_width, stride, dilation, relu, stream"""
    for case_id, ((_, row),) in record_all().items():
        _, mode, width, has_bias, relu = case_id.split('/')
        s, d, cg = int(mode[1]), int(mode[3]), int(width[2:])
        assert row[:2] == ['x', 'w'] and row[3] == 'new0', (case_id, row)
        assert row[2] == ('bias' if has_bias == 'bias1' else 'null'), (case_id, row)
        assert row[4:] == [B, H, W, C, cg, s, d, 0 if relu == 'relu0' else 1, 'stream'], (case_id, row)
