"""What ``fused.stem_conv3x3_bias_act`` hands to the C ABI (``opa_stem3x3_actp``), argument by argument, without a GPU -- recorded like
``test_launch_marshalling.py`` records its cases (on the harness of ``abi_tables.py``) and compared with ``golden/launch_marshalling_stem.json`` (``golden/make_golden_abi.py launch_marshalling_stem``).

Three inputs: NCHW-contiguous, channels-last, and a view cropped by one pixel on each side out of a larger tensor of either layout.
The four strides handed over must be the VIEW's own and the pointer the view's first element: the launcher makes no copy."""
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm

GOLDEN = at.golden('launch_marshalling_stem')
CL = torch.channels_last
ACTS = {'none': (fused.ACT_NONE, 0.0), 'relu': (fused.ACT_RELU, 0.0), 'hardswish': (fused.ACT_HARDSWISH, 0.0),
        'leaky0.01': (fused.ACT_LEAKY_RELU, 0.01), 'relu6': (fused.ACT_RELU6, 6.0)}
B, H, W = 2, 9, 7


def inputs():
    """-> {layout: (x, the tensor that owns its memory)}"""
    nchw, nhwc = torch.zeros((B, 3, H, W)), torch.zeros((B, 3, H, W)).contiguous(memory_format=CL)
    big_nchw, big_nhwc = torch.zeros((B, 3, H + 2, W + 2)), torch.zeros((B, 3, H + 2, W + 2)).contiguous(memory_format=CL)
    return {'nchw': (nchw, nchw), 'nhwc': (nhwc, nhwc), 'crop-nchw': (big_nchw[:, :, 1:-1, 1:-1], big_nchw),
            'crop-nhwc': (big_nhwc[:, :, 1:-1, 1:-1], big_nhwc)}


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor})}"""
    out = {}
    for layout, (x, _) in inputs().items():
        for channels, stride in ((16, 1), (24, 2), (32, 2), (42, 2), (64, 2)):
            for act_name, (act, param) in ACTS.items():
                for has_bias in (True, False):
                    if not has_bias and act_name != 'relu':
                        continue
                    conv = nn.Conv2d(3, channels, 3, stride, 1, bias=has_bias)
                    labels = {'x': x, 'bias': conv.bias} if has_bias else {'x': x}
                    out['stem/%s/c%d/stride%d/%s/bias%d' % (layout, channels, stride, act_name, has_bias)] = (
                        lambda conv=conv, x=x, act=act, param=param: fused.stem_conv3x3_bias_act(conv, x, act=act, act_param=param),
                        labels, lambda conv=conv: tlm._cached_on(conv, 'w'))
    return out


def record_all():
    """-> {case id: [[symbol, [arguments]], ...]}"""
    return at.record_all(cases())


def test_every_launch_hands_over_what_the_golden_file_says():
    got = at.marshalling(cases(), GOLDEN)
    assert all(len(calls) == 1 and calls[0][0] == 'opa_stem3x3_actp' for calls in got.values())


def test_the_strides_are_the_views_and_nothing_is_copied():
    """x, batch / channel / row / pixel stride, w, bias, out, batch, h, w, channels_out, stride, act, act_param, stream"""
    got = record_all()
    views = inputs()
    want_strides = {'nchw': [3 * H * W, H * W, W, 1], 'nhwc': [3 * H * W, 1, 3 * W, 3],
                    'crop-nchw': [3 * (H + 2) * (W + 2), (H + 2) * (W + 2), W + 2, 1], 'crop-nhwc': [3 * (H + 2) * (W + 2), 1, 3 * (W + 2), 3]}
    for layout, (x, owner) in views.items():
        assert list(x.stride()) == want_strides[layout]
        assert x.data_ptr() - owner.data_ptr() == (4 * (x.stride(2) + x.stride(3)) if layout.startswith('crop') else 0)
    for case_id, ((name, row),) in got.items():
        _, layout, channels, stride, act_name, bias = case_id.split('/')
        act, param = ACTS[act_name]
        assert row[0] == 'x' and row[1:5] == want_strides[layout], (case_id, row)           # the view's first element, its strides
        assert row[5] == 'w' and row[6] == ('bias' if bias == 'bias1' else 'null') and row[7] == 'new0', (case_id, row)
        assert row[8:13] == [B, H, W, int(channels[1:]), int(stride[6:])], (case_id, row)
        assert row[13] == act and row[14] == torch.tensor(param, dtype=torch.float32).item() and row[15] == 'stream', (case_id, row)


def test_the_output_is_dense_channels_last():
    with at.recording(), torch.no_grad():
        for layout, (x, _) in inputs().items():
            for stride in (1, 2):
                out = fused.stem_conv3x3_bias_act(nn.Conv2d(3, 24, 3, stride, 1), x)
                assert out.shape == (B, 24) + fused.stem_conv_out_hw(H, W, stride) and out.dtype == torch.float32
                assert out.is_contiguous(memory_format=CL), layout
