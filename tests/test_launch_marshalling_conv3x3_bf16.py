"""What ``fused.conv3x3_bias_act_bf16`` hands to the C ABI (``opa_conv3x3_act_bf16``), argument by argument, without a GPU -- recorded
like ``test_launch_marshalling.py`` records its cases (on the harness of ``abi_tables.py``) and compared with
``golden/launch_marshalling_conv3x3_bf16.json`` (``golden/make_golden_abi.py launch_marshalling_conv3x3_bf16``).

Operands: a dense channels-last bfloat16 tensor; with and without the folded bias, with and without a residual, every (stride,
dilation) the kernel takes, ``relu`` on and off.  The pointers handed over are the tensor's own (``x``, ``residual``: no copy), the
derived operands the launcher keeps on the module (``w``: ``[N][9][C]`` bfloat16, ``bias``: FLOAT32) and the output it allocates
(``new0``)."""
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm

GOLDEN = at.golden('launch_marshalling_conv3x3_bf16')
BF16 = torch.bfloat16
SYMBOL = 'opa_conv3x3_act_bf16'
B, H, W = 2, 7, 5
C, N = 64, 128
MODES = [(1, 1), (2, 1), (1, 2), (1, 4)]            # (stride, dilation)


def _out_hw(s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor})}"""
    out = {}
    for s, d in MODES:
        for has_bias in (True, False):
            for has_residual in (True, False):
                for relu in (True, False):
                    conv = nn.Conv2d(C, N, 3, s, d, dilation=d, bias=False).to(BF16).requires_grad_(False)
                    x = tlm._act(B, C, H, W, BF16)
                    bias = torch.zeros(N, dtype=BF16) if has_bias else None
                    residual = tlm._act(B, N, *_out_hw(s), BF16) if has_residual else None
                    tensors = {'x': x}
                    if has_residual:
                        tensors['residual'] = residual
                    out['conv3x3_bf16/s%dd%d/bias%d/residual%d/relu%d' % (s, d, has_bias, has_residual, relu)] = (
                        lambda conv=conv, x=x, bias=bias, residual=residual, relu=relu: fused.conv3x3_bias_act_bf16(conv, x, bias, residual, relu=relu),
                        tensors, lambda conv=conv: tlm._cached_on(conv, 'w', 'bias'))
    # ``relu`` left to its default
    conv = nn.Conv2d(C, N, 3, 1, 1, bias=False).to(BF16).requires_grad_(False)
    x, bias = tlm._act(B, C, H, W, BF16), torch.zeros(N, dtype=BF16)
    out['conv3x3_bf16/s1d1/bias1/residual0/relu-default'] = (
        lambda: fused.conv3x3_bias_act_bf16(conv, x, bias), {'x': x}, lambda: tlm._cached_on(conv, 'w', 'bias'))
    return out


def _check(case_id, out):
    s = int(case_id.split('/')[1][1])
    assert out.dtype == BF16 and out.is_contiguous(memory_format=torch.channels_last), case_id
    assert tuple(out.shape) == (B, N) + _out_hw(s), case_id


def record_all():
    """-> {case id: [[symbol, [arguments]], ...]}"""
    return at.record_all(cases(), check=_check)


def test_every_launch_hands_over_what_the_golden_file_says():
    got = at.marshalling(cases(), GOLDEN, check=_check)
    assert all([name for name, _ in calls] == [SYMBOL] for calls in got.values())


def test_the_arguments_are_the_tensors_and_the_convolutions_own():
    """x, w, bias, residual, out, batch, h_in, w_in, c_in, c_out, stride, dilation, relu, stream"""
    for case_id, ((_, row),) in record_all().items():
        _, mode, has_bias, has_residual, relu = case_id.split('/')
        s, d = int(mode[1]), int(mode[3])
        assert row[:2] == ['x', 'w'] and row[4] == 'new0', (case_id, row)
        assert row[2] == ('bias' if has_bias == 'bias1' else 'null') and row[3] == ('residual' if has_residual == 'residual1' else 'null'), (case_id, row)
        assert row[5:] == [B, H, W, C, N, s, d, 0 if relu == 'relu0' else 1, 'stream'], (case_id, row)
