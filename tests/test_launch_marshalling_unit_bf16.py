"""What ``fused.conv1x1_unit_bf16`` hands to the C ABI (``opa_gemm_unit_actp_bf16``), argument by argument, without a GPU -- recorded like
``test_launch_marshalling.py`` records its cases (on the harness of ``abi_tables.py``) and compared with ``golden/launch_marshalling_unit_bf16.json`` (``golden/make_golden_abi.py launch_marshalling_unit_bf16``).

Operands: a dense channels-last bfloat16 tensor and a channel slice of a wider one; alone, with a partner, with a residual; every
activation code.  The pitches handed over must be the VIEWS' own, in bf16 elements, and the pointers their first elements: the
launcher makes no copy.  The derived operands are the padded bfloat16 weight and the padded FLOAT32 bias."""
import ctypes
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm

GOLDEN = at.golden('launch_marshalling_unit_bf16')
BF16 = torch.bfloat16
SYMBOL = 'opa_gemm_unit_actp_bf16'
B, H, W = 2, 3, 5
K, N = 72, 40
ACTS = {'none': (fused.ACT_NONE, 0.0), 'relu': (fused.ACT_RELU, 0.0), 'hardswish': (fused.ACT_HARDSWISH, 0.0),
        'leaky0.01': (fused.ACT_LEAKY_RELU, 0.01), 'relu6': (fused.ACT_RELU6, 6.0)}


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor})}"""
    out = {}
    for layout in ('dense', 'slices'):
        for has_bias in (True, False):
            conv = nn.Conv2d(K, N, 1, bias=has_bias).to(BF16)
            make = tlm._act if layout == 'dense' else tlm._slice
            x = make(B, K, H, W, BF16)
            third = make(B, N, H, W, BF16) if layout == 'dense' else tlm._slice(B, N, H, W, BF16, extra=10, start=4)
            for what in ('alone', 'partner', 'residual'):
                for act_name, (act, param) in ACTS.items():
                    if what == 'residual' and act > 2:                       # (refused by the entry point: no caller)
                        continue
                    kwargs = {} if what == 'alone' else {what: third}
                    tensors = dict({'x': x}, **kwargs)
                    out['unit_bf16/%s/bias%d/%s/%s' % (layout, has_bias, what, act_name)] = (
                        lambda conv=conv, x=x, act=act, param=param, kwargs=kwargs: fused.conv1x1_unit_bf16(conv, x, act=act, act_param=param, **kwargs),
                        tensors, lambda conv=conv: tlm._cached_on(conv, 'w_padded', 'bias_padded'))
            # ``relu=`` instead of ``act=``
            out['unit_bf16/%s/bias%d/alone/relu-keyword' % (layout, has_bias)] = (
                lambda conv=conv, x=x: fused.conv1x1_unit_bf16(conv, x), {'x': x}, lambda conv=conv: tlm._cached_on(conv, 'w_padded', 'bias_padded'))
            out['unit_bf16/%s/bias%d/alone/relu-false' % (layout, has_bias)] = (
                lambda conv=conv, x=x: fused.conv1x1_unit_bf16(conv, x, relu=False), {'x': x},
                lambda conv=conv: tlm._cached_on(conv, 'w_padded', 'bias_padded'))
    return out


def _check(case_id, out):
    assert out.dtype == BF16 and out.is_contiguous(memory_format=torch.channels_last), case_id
    assert tuple(out.shape) == (B, 2 * N if '/partner/' in case_id else N, H, W), case_id


def record_all():
    """-> {case id: [[symbol, [arguments]], ...]}"""
    return at.record_all(cases(), check=_check)


def test_every_launch_hands_over_what_the_golden_file_says():
    got = at.marshalling(cases(), GOLDEN, check=_check)
    assert all([name for name, _ in calls] == [SYMBOL] for calls in got.values())


def test_the_pitches_are_the_views_and_nothing_is_copied():
    """a, a pitch, w, bias, partner, its pitch, residual, its pitch, out, m, n, k, act, act_param, stream"""
    x = tlm._slice(B, K, H, W, BF16)                                   # (what the 'slices' cases hand over: 4 bytes into a wider pixel)
    assert x.data_ptr() % 4 == 0 and (x.data_ptr() - x.untyped_storage().data_ptr()) == 4 and fused._pixel_stride(x) == K + 6
    for case_id, ((_, row),) in record_all().items():
        _, layout, _, what, act_name = case_id.split('/')
        act, param = {'relu-keyword': (1, 0.0), 'relu-false': (0, 0.0)}.get(act_name) or ACTS[act_name]
        x_pitch, third_pitch = (K, N) if layout == 'dense' else (K + 6, N + 10)
        assert row[:4] == ['x', x_pitch, 'w_padded', 'bias_padded'], (case_id, row)
        assert row[4:6] == (['partner', third_pitch] if what == 'partner' else ['null', 0]), (case_id, row)
        assert row[6:8] == (['residual', third_pitch] if what == 'residual' else ['null', 0]), (case_id, row)
        assert row[8] == 'new0' and row[9:12] == [B * H * W, N, K], (case_id, row)
        assert row[12:] == [act, ctypes.c_float(param).value, 'stream'], (case_id, row)
