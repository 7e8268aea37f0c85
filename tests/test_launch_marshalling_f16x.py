"""What ``fused.gconv3x3_bias_act_bf16`` and ``fused.stem7x7_bias_act_bf16`` hand to the C ABI for FLOAT16 operands
(``opa_gconv3x3_act_f16``, ``opa_stem7x7_act_f16``), argument by argument, without a GPU -- recorded like
``test_launch_marshalling.py`` records its cases, on the harness of ``abi_tables.py``.

The grouped convolution's cases are ``test_launch_marshalling_gconv3x3_bf16.py``'s with float16 tensors; what is recorded must be
that file's golden table (``golden/launch_marshalling_gconv3x3_bf16.json``) with only the symbol's name replaced: the same pointers in
the same places (``x``: the tensor's own, no copy; ``w`` / ``bias``: the derived operands kept on the module; ``new0``: the output the
launcher allocates), the same integers.  The stem has no such table for bfloat16; what is expected of it stands here: the four
element strides of ``x`` as the view has them, whatever the layout, and nothing copied."""
import json

import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm
import test_launch_marshalling_gconv3x3_bf16 as twin

F16 = torch.float16
CL = torch.channels_last
B, H, W, C = twin.B, twin.H, twin.W, twin.C


def _gconv(cg, s, d):
    return nn.Conv2d(C, C, 3, s, d, dilation=d, groups=C // cg, bias=False).to(F16).requires_grad_(False)


def gconv_cases():
    """The twin's cases, id for id (the ids keep the twin's spelling: they are the golden table's keys), with float16 tensors"""
    out = {}
    for s, d in twin.MODES:
        for cg in twin.WIDTHS:
            for has_bias in (True, False):
                for relu in (True, False):
                    conv, x = _gconv(cg, s, d), tlm._act(B, C, H, W, F16)
                    bias = torch.zeros(C, dtype=F16) if has_bias else None
                    out['gconv3x3_bf16/s%dd%d/cg%d/bias%d/relu%d' % (s, d, cg, has_bias, relu)] = (
                        lambda conv=conv, x=x, bias=bias, relu=relu: fused.gconv3x3_bias_act_bf16(conv, x, bias, relu=relu),
                        {'x': x}, lambda conv=conv: tlm._cached_on(conv, 'w', 'bias'))
    conv, x, bias = _gconv(8, 1, 1), tlm._act(B, C, H, W, F16), torch.zeros(C, dtype=F16)
    out['gconv3x3_bf16/s1d1/cg8/bias1/relu-default'] = (
        lambda: fused.gconv3x3_bias_act_bf16(conv, x, bias), {'x': x}, lambda: tlm._cached_on(conv, 'w', 'bias'))
    return out


def _gconv_check(case_id, out):
    s = int(case_id.split('/')[1][1])
    assert out.dtype == F16 and out.is_contiguous(memory_format=CL), case_id
    assert tuple(out.shape) == (B, C) + twin._out_hw(s), case_id


def test_the_grouped_launches_are_the_twins_golden_table_under_the_float16_name():
    assert sorted(gconv_cases()) == sorted(twin.cases())
    got = at.record_all(gconv_cases(), check=_gconv_check)
    with open(twin.GOLDEN) as f:
        want = json.load(f)['cases']
    assert sorted(got) == sorted(want) and len(want) == 33
    for case_id, calls in want.items():
        assert [name for name, _ in calls] == [twin.SYMBOL]
        assert got[case_id] == [['opa_gconv3x3_act_f16', row] for _, row in calls], case_id


def test_the_grouped_arguments_are_the_tensors_and_the_convolutions_own():
    """x, w, bias, out, batch, h_in, w_in, channels, group_width, stride, dilation, relu, stream; the derived operands float16 / float32"""
    for case_id, (call, _, derived) in gconv_cases().items():
        ((name, row),) = at.record_all({case_id: (call, _, derived)}, check=_gconv_check)[case_id]
        _, mode, width, has_bias, relu = case_id.split('/')
        s, d, cg = int(mode[1]), int(mode[3]), int(width[2:])
        assert name == 'opa_gconv3x3_act_f16'
        assert row[:2] == ['x', 'w'] and row[3] == 'new0', (case_id, row)
        assert row[2] == ('bias' if has_bias == 'bias1' else 'null'), (case_id, row)
        assert row[4:] == [B, H, W, C, cg, s, d, 0 if relu == 'relu0' else 1, 'stream'], (case_id, row)
        operands = derived()
        assert operands['w'].dtype == F16 and tuple(operands['w'].shape) == (C, 9, 64)
        assert 'bias' not in operands or operands['bias'].dtype == torch.float32


SB, SH, SW, SN = 2, 9, 6, 64


def _image(layout):
    x = torch.zeros((SB, 3, SH, SW), dtype=F16)
    if layout == 'nchw':
        return x
    if layout == 'cl':
        return x.contiguous(memory_format=CL)
    big = torch.zeros((SB, 3, SH + 5, SW + 4), dtype=F16).contiguous(memory_format=CL)
    return big[:, :, 2:2 + SH, 1:1 + SW]


def stem_cases():
    out = {}
    for layout in ('nchw', 'cl', 'crop'):
        for s in (1, 2):
            for has_bias in (True, False):
                for relu in (True, False):
                    conv = nn.Conv2d(3, SN, 7, s, 3, bias=False).to(F16).requires_grad_(False)
                    x, bias = _image(layout), torch.zeros(SN, dtype=F16) if has_bias else None
                    out['stem7x7/%s/s%d/bias%d/relu%d' % (layout, s, has_bias, relu)] = (
                        lambda conv=conv, x=x, bias=bias, relu=relu: fused.stem7x7_bias_act_bf16(conv, x, bias, relu=relu),
                        {'x': x}, lambda conv=conv: tlm._cached_on(conv, 'w', 'bias'))
    conv, x = nn.Conv2d(3, 128, 7, 2, 3, bias=False).to(F16).requires_grad_(False), _image('nchw')
    out['stem7x7/nchw/s2/bias0/relu-default'] = (lambda: fused.stem7x7_bias_act_bf16(conv, x, None), {'x': x},
                                                  lambda: tlm._cached_on(conv, 'w', 'bias'))
    return out


def test_the_stem_hands_over_the_views_strides_and_copies_nothing():
    """x, x_batch_stride, x_channel_stride, x_row_stride, x_pixel_stride, w, bias, out, batch, h, w, c_out, stride, relu, stream"""
    strides = {'nchw': [3 * SH * SW, SH * SW, SW, 1], 'cl': [SH * SW * 3, 1, SW * 3, 3],
               'crop': [(SH + 5) * (SW + 4) * 3, 1, (SW + 4) * 3, 3]}

    def check(case_id, out):
        s, n = int(case_id.split('/')[2][1]), 128 if case_id.endswith('default') else SN
        assert out.dtype == F16 and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (SB, n, (SH - 1) // s + 1, (SW - 1) // s + 1)
    cases = stem_cases()
    got = at.record_all(cases, check=check)
    assert len(got) == 25
    for case_id, calls in got.items():
        ((name, row),) = calls
        _, layout, mode, has_bias, relu = case_id.split('/')
        n = 128 if relu == 'relu-default' else SN
        assert name == 'opa_stem7x7_act_f16', case_id
        assert row[0] == 'x' and row[1:5] == strides[layout], (case_id, row)                 # the view's own pointer and strides
        assert row[5] == 'w' and row[6] == ('bias' if has_bias == 'bias1' else 'null') and row[7] == 'new0', (case_id, row)
        assert row[8:] == [SB, SH, SW, n, int(mode[1]), 0 if relu == 'relu0' else 1, 'stream'], (case_id, row)
        operands = cases[case_id][2]()
        assert operands['w'].dtype == F16 and tuple(operands['w'].shape) == (n, 192)
        assert 'bias' not in operands or operands['bias'].dtype == torch.float32
