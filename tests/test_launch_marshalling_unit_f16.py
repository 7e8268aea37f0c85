"""What ``fused.conv1x1_unit_f16`` and ``fused.dwconv_bias_act`` on a float16 tensor hand to the C ABI (``opa_gemm_unit_actp_f16``,
``opa_dwconv_actp_f16``), argument by argument, without a GPU -- recorded like ``test_launch_marshalling_unit_bf16.py`` records its cases
(on the harness of ``abi_tables.py``) and compared with ``golden/launch_marshalling_unit_f16.json``
(``golden/make_golden_abi.py launch_marshalling_unit_f16``).

The GEMM: a dense channels-last float16 tensor and a channel slice of a wider one; alone, with a partner, with a residual; every
activation code, the LeakyReLU's slope among them.  The pitches handed over must be the VIEWS' own, in elements, and the pointers their
first elements: the launcher makes no copy.  The derived operands are the padded float16 weight and the padded FLOAT32 bias.  The
stencil: a plain 3 x 3, a dilated 5 x 5, a 7 x 7 and ReLU6 -- every window and every code goes to the ONE float16 symbol, which takes
no dtype."""
import ctypes
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm

GOLDEN = at.golden('launch_marshalling_unit_f16')
F16 = torch.float16
GEMM, STENCIL = 'opa_gemm_unit_actp_f16', 'opa_dwconv_actp_f16'
B, H, W = 2, 3, 5
K, N = 72, 40
C = 8
ACTS = {'none': (fused.ACT_NONE, 0.0), 'relu': (fused.ACT_RELU, 0.0), 'hardswish': (fused.ACT_HARDSWISH, 0.0),
        'leaky0.01': (fused.ACT_LEAKY_RELU, 0.01), 'relu6': (fused.ACT_RELU6, 6.0)}
# (kernel size, stride, dilation, activation, its parameter)
STENCILS = {'3x3': (3, 1, 1, 'relu'), '3x3-stride2': (3, 2, 1, 'none'), '5x5-dilated2': (5, 1, 2, 'relu'), '7x7': (7, 1, 1, 'hardswish'),
            '7x7-dilated4': (7, 1, 4, 'none'), '5x5-relu6': (5, 2, 1, 'relu6'), '3x3-dilated2-relu6': (3, 1, 2, 'relu6')}


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor})}"""
    out = {}
    for layout in ('dense', 'slices'):
        make = tlm._act if layout == 'dense' else tlm._slice
        for has_bias in (True, False):
            conv = nn.Conv2d(K, N, 1, bias=has_bias).to(F16)
            x = make(B, K, H, W, F16)
            third = make(B, N, H, W, F16) if layout == 'dense' else tlm._slice(B, N, H, W, F16, extra=10, start=4)
            for what in ('alone', 'partner', 'residual'):
                for act_name, (act, param) in ACTS.items():
                    if what == 'residual' and act > 2:                       # (refused by the entry point: no caller)
                        continue
                    kwargs = {} if what == 'alone' else {what: third}
                    tensors = dict({'x': x}, **kwargs)
                    out['unit_f16/%s/bias%d/%s/%s' % (layout, has_bias, what, act_name)] = (
                        lambda conv=conv, x=x, act=act, param=param, kwargs=kwargs: fused.conv1x1_unit_f16(conv, x, act=act, act_param=param, **kwargs),
                        tensors, lambda conv=conv: tlm._cached_on(conv, 'w_padded', 'bias_padded'))
            # ``relu=`` instead of ``act=``, and the route's own call (``conv1x1_unit``: the mode of ``x``'s dtype)
            out['unit_f16/%s/bias%d/alone/relu-keyword' % (layout, has_bias)] = (
                lambda conv=conv, x=x: fused.conv1x1_unit_f16(conv, x), {'x': x}, lambda conv=conv: tlm._cached_on(conv, 'w_padded', 'bias_padded'))
            out['unit_f16/%s/bias%d/alone/relu-false' % (layout, has_bias)] = (
                lambda conv=conv, x=x: fused.conv1x1_unit(conv, x, relu=False), {'x': x},
                lambda conv=conv: tlm._cached_on(conv, 'w_padded', 'bias_padded'))
        for name, (k, s, d, act_name) in STENCILS.items():
            dx = make(B, C, 7, 6, F16)
            taps, db = torch.zeros((k * k, C), dtype=F16), torch.zeros(C, dtype=F16)
            act, param = ACTS[act_name]
            for has_bias in (True, False):
                out['dwconv_f16/%s/bias%d/%s' % (layout, has_bias, name)] = (
                    lambda dx=dx, taps=taps, bias=db if has_bias else None, k=k, s=s, d=d, act=act, param=param:
                    fused.dwconv_bias_act(dx, taps, bias, k, s, act=act, dilation=d, act_param=param),
                    dict({'x': dx, 'w_taps': taps}, **({'bias': db} if has_bias else {})))
    dx, taps, db = tlm._act(B, C, 7, 6, F16), torch.zeros((25, C), dtype=F16), torch.zeros(C, dtype=F16)
    out['dwconv_f16/defaults'] = (lambda: fused.dwconv_bias_act(dx, taps, db, 5, 1), dict(x=dx, w_taps=taps, bias=db))
    out['dwconv_f16/relu-keyword'] = (lambda: fused.dwconv_bias_act(dx, taps, db, 5, 1, True), dict(x=dx, w_taps=taps, bias=db))
    return out


def _check(case_id, out):
    assert out.dtype == F16 and out.is_contiguous(memory_format=torch.channels_last), case_id
    if case_id.startswith('unit_f16/'):
        assert tuple(out.shape) == (B, 2 * N if '/partner/' in case_id else N, H, W), case_id
    else:
        assert out.shape[:2] == (B, C), case_id


def record_all():
    """-> {case id: [[symbol, [arguments]], ...]}"""
    return at.record_all(cases(), check=_check)


def test_every_launch_hands_over_what_the_golden_file_says():
    got = at.marshalling(cases(), GOLDEN, check=_check)
    for case_id, calls in got.items():
        assert [name for name, _ in calls] == [GEMM if case_id.startswith('unit_f16/') else STENCIL], case_id


def test_the_pitches_are_the_views_and_nothing_is_copied():
    """a, a pitch, w, bias, partner, its pitch, residual, its pitch, out, m, n, k, act, act_param, stream"""
    x = tlm._slice(B, K, H, W, F16)                                   # (what the 'slices' cases hand over: 4 bytes into a wider pixel)
    assert x.data_ptr() % 4 == 0 and (x.data_ptr() - x.untyped_storage().data_ptr()) == 4 and fused._pixel_stride(x) == K + 6
    for case_id, ((_, row),) in record_all().items():
        if not case_id.startswith('unit_f16/'):
            continue
        _, layout, _, what, act_name = case_id.split('/')
        act, param = {'relu-keyword': (1, 0.0), 'relu-false': (0, 0.0)}.get(act_name) or ACTS[act_name]
        x_pitch, third_pitch = (K, N) if layout == 'dense' else (K + 6, N + 10)
        assert row[:4] == ['x', x_pitch, 'w_padded', 'bias_padded'], (case_id, row)
        assert row[4:6] == (['partner', third_pitch] if what == 'partner' else ['null', 0]), (case_id, row)
        assert row[6:8] == (['residual', third_pitch] if what == 'residual' else ['null', 0]), (case_id, row)
        assert row[8] == 'new0' and row[9:12] == [B * H * W, N, K], (case_id, row)
        assert row[12:] == [act, ctypes.c_float(param).value, 'stream'], (case_id, row)


def test_the_stencil_hands_over_the_window_the_code_and_no_dtype():
    """x, its pixel stride, w, bias, out, its pixel stride, batch, h, w, channels, k, stride, dilation, act, act_param, stream"""
    for case_id, ((_, row),) in record_all().items():
        if not case_id.startswith('dwconv_f16/') or case_id.count('/') != 3:
            continue
        _, layout, has_bias, name = case_id.split('/')
        k, s, d, act_name = STENCILS[name]
        act, param = ACTS[act_name]
        assert row[:6] == ['x', C if layout == 'dense' else C + 6, 'w_taps', 'bias' if has_bias == 'bias1' else 'null', 'new0', C], (case_id, row)
        assert row[6:] == [B, 7, 6, C, k, s, d, act, ctypes.c_float(param).value, 'stream'], (case_id, row)
    got = record_all()
    assert got['dwconv_f16/defaults'][0][1][10:15] == [5, 1, 1, 0, 0.0] and got['dwconv_f16/relu-keyword'][0][1][10:15] == [5, 1, 1, 1, 0.0]
