"""What ``fused.group_norm_act`` hands to the C ABI (``opa_groupnorm_workspace_bytes``, ``opa_groupnorm_actp``), argument by argument,
without a GPU -- recorded like ``test_launch_marshalling.py`` records its cases (on the harness of ``abi_tables.py``) and compared with ``golden/launch_marshalling_groupnorm.json``
(``golden/make_golden_abi.py launch_marshalling_groupnorm``).

Operands: a dense channels-last tensor and the upper channel half of a tensor of twice the channels; out of place (a new dense
tensor), in place (``out`` is ``x``: the same pointer, the same pitch) and into a slice; with and without affine terms; each
activation.  The pitches handed over must be the VIEWS' own and the pointers their first elements: the launcher makes no copy."""
import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm

GOLDEN = at.golden('launch_marshalling_groupnorm')
CL = torch.channels_last
ACTS = {'none': (fused.ACT_NONE, 0.0), 'relu': (fused.ACT_RELU, 0.0), 'hardswish': (fused.ACT_HARDSWISH, 0.0),
        'leaky0.01': (fused.ACT_LEAKY_RELU, 0.01), 'relu6': (fused.ACT_RELU6, 6.0)}
B, H, W = 2, 9, 7
PAIRS = ((24, 4), (174, 29), (256, 32))
P = 512


def workspace_bytes(batch, pixels, channels):
    return batch * ((pixels + P - 1) // P) * channels * 16 + batch * channels * 8


def operand(channels, layout):
    """-> (x, the tensor that owns its memory)"""
    if layout == 'dense':
        t = torch.zeros((B, channels, H, W)).contiguous(memory_format=CL)
        return t, t
    big = torch.zeros((B, 2 * channels, H, W)).contiguous(memory_format=CL)
    return big[:, channels:], big


def cases():
    """-> {case id: (call, {label: input tensor})}"""
    out = {}
    for channels, groups in PAIRS:
        for layout in ('dense', 'slice'):
            for where in ('new', 'inplace', 'slice'):
                for act_name, (act, param) in ACTS.items():
                    for affine in (True, False):
                        if not affine and act_name != 'relu':
                            continue
                        norm = nn.GroupNorm(groups, channels, eps=1e-5 if affine else 1e-3, affine=affine)
                        x, _ = operand(channels, layout)
                        dest = {'new': None, 'inplace': x, 'slice': operand(channels, 'slice')[0]}[where]
                        labels = {'x': x}
                        if affine:
                            labels.update(gamma=norm.weight, beta=norm.bias)
                        if where == 'slice':
                            labels['out'] = dest
                        out['gn/c%d/g%d/%s/%s/%s/affine%d' % (channels, groups, layout, where, act_name, affine)] = (
                            lambda norm=norm, x=x, act=act, param=param, dest=dest: fused.group_norm_act(norm, x, act=act, act_param=param, out=dest),
                            labels)
    return out


def _before(rec):
    """The size query recorded and answered (``opa_groupnorm_workspace_bytes`` returns a size, not a status); every case allocates its
    workspace: ``new0``."""
    rec.opa_groupnorm_workspace_bytes = lambda b, p, c: rec.calls.append(('opa_groupnorm_workspace_bytes', (b, p, c))) or workspace_bytes(b, p, c)
    fused._GN_WORKSPACE.clear()


def record_all(golden=None):
    """-> {case id: [[symbol, [arguments]], ...]}, compared with the file ``golden`` where one is given"""
    try:
        return at.record_all(cases(), before=_before) if golden is None else at.marshalling(cases(), golden, before=_before)
    finally:
        fused._GN_WORKSPACE.clear()


def test_every_launch_hands_over_what_the_golden_file_says():
    got = record_all(GOLDEN)
    assert all([name for name, _ in calls] == ['opa_groupnorm_workspace_bytes', 'opa_groupnorm_actp'] for calls in got.values())


def test_the_pitches_are_the_views_and_nothing_is_copied():
    """x, x pitch, gamma, beta, out, out pitch, batch, pixels, channels, groups, eps, act, act_param, workspace, its bytes, stream"""
    for case_id, ((_, size_row), (_, row)) in record_all().items():
        _, channels, groups, layout, where, act_name, affine = case_id.split('/')
        C, G = int(channels[1:]), int(groups[1:])
        act, param = ACTS[act_name]
        pitch = C if layout == 'dense' else 2 * C
        assert size_row == [B, H * W, C], (case_id, size_row)
        assert row[0] == 'x' and row[1] == pitch, (case_id, row)
        assert row[2:4] == (['gamma', 'beta'] if affine == 'affine1' else ['null', 'null']), (case_id, row)
        # the workspace is the first tensor the launcher allocates in place and into a slice, the second behind a new output
        assert row[4:6] == {'new': ['new0', C], 'inplace': ['x', pitch], 'slice': ['out', 2 * C]}[where], (case_id, row)
        assert row[6:10] == [B, H * W, C, G], (case_id, row)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()    # noqa: E731
        assert row[10] == f32(1e-5 if affine == 'affine1' else 1e-3) and row[11] == act and row[12] == f32(param), (case_id, row)
        assert row[13] == ('new1' if where == 'new' else 'new0') and row[14] >= workspace_bytes(B, H * W, C) and row[14] % 8 == 0
        assert row[15] == 'stream', (case_id, row)


def test_the_output_and_the_workspace():
    with at.recording() as rec, torch.no_grad():
        rec.opa_groupnorm_workspace_bytes = lambda b, p, c: workspace_bytes(b, p, c)
        fused._GN_WORKSPACE.clear()
        norm = nn.GroupNorm(29, 174)
        x, owner = operand(174, 'slice')
        assert (x.data_ptr() - owner.data_ptr()) % 16 == 8                   # 174 floats in: an 8-byte boundary, no 16-byte one
        out = fused.group_norm_act(norm, x)
        assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous(memory_format=CL)
        assert fused.group_norm_act(norm, x, out=x) is x
        (ws,) = fused._GN_WORKSPACE.values()
        assert ws.dtype == torch.float64 and ws.numel() * 8 >= workspace_bytes(B, H * W, 174)
        fused.group_norm_act(nn.GroupNorm(4, 24), operand(24, 'dense')[0])              # a smaller call keeps it
        assert list(fused._GN_WORKSPACE.values())[0] is ws
        fused.group_norm_act(nn.GroupNorm(32, 2048), torch.zeros((B, 2048, H, W)).contiguous(memory_format=CL))
        (grown,) = fused._GN_WORKSPACE.values()
        assert grown is not ws and grown.numel() * 8 >= workspace_bytes(B, H * W, 2048)
        fused._GN_WORKSPACE.clear()
