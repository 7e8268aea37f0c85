"""What ``fused.head_conv_fields16`` hands to the C ABI (``opa_head_conv_fields_bf16`` / ``opa_head_conv_fields_f16``), argument by
argument, without a GPU -- recorded on the harness of ``abi_tables.py`` like ``test_launch_marshalling_gemm2_bf16.py`` records its cases.
What is expected is written here.

Cases: a Cif, a Caf and a CifDet head (5, 8 and 6 components; CifDet's offset mask is 0b01, Caf's 0b11), with and without
upsampling, in both 16-bit types, on a 2 x 5 x 3 trunk output of 128 channels.  The pointer of ``x`` is the tensor's own (no copy), the
weight and the bias are the derived operands the launcher keeps on the convolution (``w``: ``[Np][K]`` of ``x``'s dtype, ``Np`` the
output channels rounded up to 64; ``bias``: FLOAT32 ``[Np]``), the output is the float32 ``[B, F, C, H, W]`` it allocates (``new0``)."""
import pytest
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import head16_common as hc

CL = torch.channels_last
SUFFIX = {torch.bfloat16: '_bf16', torch.float16: '_f16'}
B, H, W, K = 2, 5, 3, 128
HEADS = {'cif': 17, 'caf': 19, 'cifdet': 3}            # kind -> fields


def _cached_on(module, *names):
    """The one derived operand (``fused.derived``) the launcher left on ``module`` -> {label: tensor}."""
    attrs = [a for a in vars(module) if a.startswith('_opa_')]
    assert attrs == ['_opa_head16'], attrs
    value = getattr(module, attrs[0])[1]
    assert len(value) == len(names)
    return dict(zip(names, value))


def _head(kind, us, dtype):
    meta = hc.meta(kind, HEADS[kind], us)
    conv = nn.Conv2d(K, HEADS[kind] * hc.n_components(meta) * us * us, 1).to(dtype).requires_grad_(False)
    return meta, conv


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor})}"""
    out = {}
    for dtype in SUFFIX:
        for kind in HEADS:
            for us in (1, 2):
                meta, conv = _head(kind, us, dtype)
                x = torch.zeros((B, K, H, W), dtype=dtype).contiguous(memory_format=CL)
                out['%s/us%d/%s' % (kind, us, dtype)] = (lambda conv=conv, x=x, meta=meta: fused.head_conv_fields16(conv, x, meta), {'x': x},
                                                        lambda conv=conv: _cached_on(conv, 'w', 'bias'))
    return out


def _check(case_id, out):
    kind, us, _ = case_id.split('/')
    us = int(us[2])
    meta = hc.meta(kind, HEADS[kind], us)
    assert out.dtype == torch.float32 and out.is_contiguous(), case_id
    assert tuple(out.shape) == (B, HEADS[kind], hc.n_components(meta), H * us - (us - 1), W * us - (us - 1)), case_id


def test_every_launch_hands_over_the_tensor_and_the_convolutions_padded_operands():
    """x, w, bias, out, batch, hc, wc, k, n_fields, n_components, upsample, n_confidences, n_vectors, vector_offset_mask, n_scales, stream"""
    got = at.record_all(cases(), check=_check)
    assert len(got) == 2 * 3 * 2
    counts = {'cif': (5, 1, 1, 0b1, 1), 'caf': (8, 1, 2, 0b11, 2), 'cifdet': (6, 1, 2, 0b01, 0)}   # C, confidences, vectors, mask, scales
    for case_id, calls in got.items():
        ((name, row),) = calls                                                                  # ONE launch
        kind, us, dtype = case_id.split('/')
        n_comp, n_conf, n_vec, mask, n_scales = counts[kind]
        assert name == 'opa_head_conv_fields' + SUFFIX[getattr(torch, dtype.split('.')[1])], case_id
        assert row == ['x', 'w', 'bias', 'new0', B, H, W, K, HEADS[kind], n_comp, int(us[2]), n_conf, n_vec, mask, n_scales, 'stream'], (case_id, row)


@pytest.mark.parametrize('dtype', list(SUFFIX), ids=str)
def test_the_derived_operands_are_what_the_kernel_reads(dtype):
    torch.manual_seed(3)
    meta, conv = _head('cif', 2, dtype)                 # N = 340 -> Np = 384
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape))
        conv.bias.copy_(torch.randn(conv.bias.shape))
    x = torch.zeros((B, K, H, W), dtype=dtype).contiguous(memory_format=CL)
    with at.recording() as rec, torch.no_grad():
        fused.head_conv_fields16(conv, x, meta)
        wp, bp = conv._opa_head16[1]
        (_, args), = rec.calls
        assert args[0] == x.data_ptr() and args[1] == wp.data_ptr() and args[2] == bp.data_ptr()
    assert wp.dtype == dtype and tuple(wp.shape) == (384, K) and wp.is_contiguous() and wp.data_ptr() % 16 == 0
    assert torch.equal(wp[:340], conv.weight.reshape(340, K)) and not wp[340:].any()
    assert bp.dtype == torch.float32 and tuple(bp.shape) == (384,) and bp.is_contiguous()
    assert torch.equal(bp[:340], conv.bias.float()) and not bp[340:].any()                      # (the 16-bit bias widened exactly)
    assert fused.HEAD16_TILE_N == 64 and fused.HEAD16_DECLINED == frozenset()
