"""What ``fused.conv1x1_pair_bias_act_bf16`` and ``fused.conv1x1_strided_bf16`` hand to the C ABI (``opa_gemm2_bias_act_bf16``), argument
by argument, without a GPU -- recorded on the harness of ``abi_tables.py`` like ``test_launch_marshalling_conv3x3_bf16.py`` records its
cases.  What is expected is written here.

Cases: a Bottleneck pair (``h``: the block's inner activation, ``x``: its input, the folded bias) at stride 1 and 2, with the ReLU on,
off and left to its default, with and without a bias; a ``PRO`` pair (``a_bias``: conv2's owed bias); the ``k1 == 0`` call of a
BasicBlock's downsampling convolution.  The pointers handed over are the tensors' own (``h``, ``x``, ``a_bias``: no copy), the derived
operands the launcher keeps on the downsampling convolution (``wcat``: ``[N][k1 + k2]`` bfloat16, ``bias``: FLOAT32) and the output it
allocates (``new0``)."""
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at

BF16 = torch.bfloat16
CL = torch.channels_last
SYMBOL = 'opa_gemm2_bias_act_bf16'
B, H, W = 2, 7, 5
K1, K2, N = 64, 128, 256


def _out_hw(s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def _act(c, hw):
    return torch.zeros((B, c) + tuple(hw), dtype=BF16).contiguous(memory_format=CL)


def _cached_on(module, *names):
    """The one derived operand (``fused.derived``) the launcher left on ``module`` -> {label: tensor}."""
    attrs = [a for a in vars(module) if a.startswith('_opa_')]
    assert len(attrs) == 1, attrs
    value = getattr(module, attrs[0])[1]
    assert len(value) == len(names), (attrs, len(value), names)
    return {n: t for n, t in zip(names, value) if t is not None}


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor})}"""
    out = {}
    for s in (1, 2):
        for has_bias in (True, False):
            for has_a_bias in (True, False):
                for relu in (True, False, None):
                    conv = nn.Conv2d(K1, N, 1, bias=False).to(BF16).requires_grad_(False)
                    dconv = nn.Conv2d(K2, N, 1, s, bias=False).to(BF16).requires_grad_(False)
                    h, x = _act(K1, _out_hw(s)), _act(K2, (H, W))
                    bias = torch.zeros(N, dtype=BF16) if has_bias else None
                    a_bias = torch.zeros(K1, dtype=BF16) if has_a_bias else None
                    tensors = {'h': h, 'x': x}
                    if has_a_bias:
                        tensors['a_bias'] = a_bias
                    kw = {} if relu is None else {'relu': relu}
                    out['pair/s%d/bias%d/pro%d/relu%s' % (s, has_bias, has_a_bias, 'default' if relu is None else int(relu))] = (
                        lambda conv=conv, dconv=dconv, h=h, x=x, bias=bias, a_bias=a_bias, kw=kw:
                            fused.conv1x1_pair_bias_act_bf16(conv, dconv, h, x, bias, a_bias=a_bias, **kw),
                        tensors, lambda dconv=dconv: _cached_on(dconv, 'wcat', 'bias'))
        dconv = nn.Conv2d(K2, N, 1, s, bias=False).to(BF16).requires_grad_(False)
        x = _act(K2, (H, W))
        out['strided/s%d' % s] = (lambda dconv=dconv, x=x: fused.conv1x1_strided_bf16(dconv, x), {'x': x},
                                  lambda dconv=dconv: _cached_on(dconv, 'wcat', 'bias'))
    return out


def _check(case_id, out):
    s = int(case_id.split('/')[1][1])
    assert out.dtype == BF16 and out.is_contiguous(memory_format=CL), case_id
    assert tuple(out.shape) == (B, N) + _out_hw(s), case_id


def test_every_launch_hands_over_the_tensors_and_the_convolutions_own():
    """a1, k1, a2, k2, batch, h_in, w_in, stride, a_bias, wcat, bias, out, n, relu, stream"""
    got = at.record_all(cases(), check=_check)
    assert len(got) == 2 * 2 * 2 * 3 + 2
    for case_id, calls in got.items():
        ((name, row),) = calls
        assert name == SYMBOL, case_id
        kind, stride, *rest = case_id.split('/')
        s = int(stride[1])
        if kind == 'strided':                      # no first source, no bias, no ReLU
            assert row == ['null', 0, 'x', K2, B, H, W, s, 'null', 'wcat', 'null', 'new0', N, 0, 'stream'], (case_id, row)
            continue
        has_bias, pro, relu = rest
        assert row == ['h', K1, 'x', K2, B, H, W, s, 'a_bias' if pro == 'pro1' else 'null', 'wcat', 'bias' if has_bias == 'bias1' else 'null',
                       'new0', N, 0 if relu == 'relu0' else 1, 'stream'], (case_id, row)


def test_the_derived_operands_are_what_the_kernel_reads():
    torch.manual_seed(3)
    conv = nn.Conv2d(K1, N, 1, bias=False).to(BF16).requires_grad_(False)
    dconv = nn.Conv2d(K2, N, 1, 2, bias=False).to(BF16).requires_grad_(False)
    bias = torch.randn(N).to(BF16)
    with at.recording() as rec, torch.no_grad():
        fused.conv1x1_pair_bias_act_bf16(conv, dconv, _act(K1, _out_hw(2)), _act(K2, (H, W)), bias)
        wcat, b32 = dconv._opa_w_pair_bf16[1]
        (_, args), = rec.calls
        assert args[9] == wcat.data_ptr() and args[10] == b32.data_ptr()
    assert wcat.dtype == BF16 and tuple(wcat.shape) == (N, K1 + K2) and wcat.is_contiguous() and wcat.data_ptr() % 16 == 0
    assert torch.equal(wcat, torch.cat((conv.weight.reshape(N, K1), dconv.weight.reshape(N, K2)), dim=1))
    assert b32.dtype == torch.float32 and torch.equal(b32, bias.float())
