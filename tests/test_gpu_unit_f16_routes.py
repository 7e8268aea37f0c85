"""ShuffleNetV2K cast with ``.half()`` on the project's kernels (``fused.UNIT_F16``): every 1x1 convolution on the 16-bit GEMM's unit mode
instantiated for float16 (csrc/gemm_unit_bf16.hip, ``opa_gemm_unit_actp_f16``), every depthwise convolution on the stencil
(csrc/dwconv.hip, ``opa_dwconv_actp_f16``).  The three tests of ``test_gpu_unit_bf16_routes.py`` for float16:
``network.factory('shufflenetv2k16')`` and ``'shufflenetv2k30'`` with the same random BatchNorm statistics, optimized, ``.half()``,
channels_last, input 2 x 3 x 97 x 65 (real kernels, MI355X).  The inputs stay inside float16's range: the largest convolution output
of the float32 forward of these networks is 2.8 - 3.8 and the largest parameter 0.5; the reference's finiteness is asserted.

1. switch on: a recorder on ``fused._launch`` counts exactly one ``opa_gemm_unit_actp_f16`` per 1x1 convolution of the stages, one for
   ``conv5`` and one per head whose input channels are no multiple of 64 (k16: 1392, both heads; k30: 2048, none), and one
   ``opa_dwconv_actp_f16`` per depthwise convolution -- the counts come from the module tree; no interleave pass; switch off: neither;
2. the forward repeats bit for bit: the trunk and every head on the kernel (a head that stays with MIOpen is asked to be finite);
3. the error bar.  ``e_on`` / ``e_off``: rms error of all head fields, route on / off, against the float32 forward of the same
   weights upcast (torch's own float32 convolutions), relative to the rms of that forward.  The yardstick is ``e_off``, torch's own
   float16 trunk; the margin is ``e_off``'s own seed-to-seed spread, max / min over the four seeds run.  Asserted: ``e_on <= spread *
   e_off`` on every seed, with the spread of THAT run.  Printed as ``UNITF16ROUTE`` lines (profiles/unit_f16/route_errors.log), with
   ``e_bf16``, the same figure of the bfloat16 network of the same weights with ``UNIT_BF16`` on, beside it: no bar, a record."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F16, BF16 = torch.float16, torch.bfloat16
GEMM, STENCIL = 'opa_gemm_unit_actp_f16', 'opa_dwconv_actp_f16'
SEEDS = (0, 1, 2, 3)
NETS = ('shufflenetv2k16', 'shufflenetv2k30')


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the switches restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    monkeypatch.setattr(fused, 'UNIT_F16', fused.UNIT_F16)
    monkeypatch.setattr(fused, 'UNIT_BF16', fused.UNIT_BF16)
    return symbols


def _float32_fields(net, x):
    """The head fields of ``net``'s float32 copy on ``x`` upcast, float64: torch's own float32 convolutions, nothing timed."""
    table, pick = fused.choices(), fused.FORCE_PICK
    fused.FORCE_PICK = 'conv'
    try:
        with torch.no_grad():
            ref = tuple(f.double() for f in copy.deepcopy(net).float()(x.float()))
    finally:
        fused.FORCE_PICK = pick
        fused.set_choices(table, replace=True)
    assert all(f.isfinite().all() for f in ref)
    return ref


@functools.lru_cache(maxsize=None)
def _base(name, seed):
    """-> (the optimized float32 network with random batch-norm statistics, x float32), computed once and left unchanged."""
    net = network.factory(name, seed=seed).cuda()
    torch.manual_seed(100 + seed)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    network.optimize_for_inference_(net)
    return net.requires_grad_(False), torch.randn((2, 3, 97, 65), device='cuda')


@functools.lru_cache(maxsize=None)
def _case(name, seed, dtype=F16):
    """-> (the network of ``dtype``, x, the head fields of its float32 copy on x upcast), computed once and left unchanged."""
    base, x32 = _base(name, seed)
    net = copy.deepcopy(base).to(dtype).to(memory_format=CL).requires_grad_(False)
    x = x32.to(dtype).contiguous(memory_format=CL)
    return net, x, _float32_fields(net, x)


def _forward(net, x, on, switch='UNIT_F16'):
    setattr(fused, switch, on)
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out


def _rms_error(got, ref):
    num = sum(float(((g.double() - r) ** 2).sum()) for g, r in zip(got, ref))
    den = sum(float((r ** 2).sum()) for r in ref)
    return (num / den) ** 0.5


def _expected_launches(net):
    base = net.base_net
    convs = [m for stage in (base.stage2, base.stage3, base.stage4) for m in stage.modules() if isinstance(m, nn.Conv2d)]
    stages = [m for m in convs if m.kernel_size == (1, 1) and m.groups == 1]
    depthwise = [m for m in convs if m.groups > 1]
    heads = [h for h in net.head_nets if h.conv.in_channels % 64 != 0]
    return len(stages), 1, len(heads), len(depthwise)


@pytest.mark.parametrize('name', NETS)
def test_one_launch_per_convolution_of_the_stages_and_none_with_the_switch_off(launches, name):
    net, x, _ = _case(name, 0)
    stages, conv5, heads, depthwise = _expected_launches(net)
    assert (stages, heads, depthwise) == {'shufflenetv2k16': (2 * 16 + 3, 2, 16 + 3), 'shufflenetv2k30': (2 * 30 + 3, 0, 30 + 3)}[name]
    del launches[:]                                                    # (the float32 reference's, where this call computed it)
    out = _forward(net, x, True)
    assert launches.count(GEMM) == stages + conv5 + heads, (launches.count(GEMM), stages, conv5, heads)
    assert launches.count(STENCIL) == depthwise
    assert 'opa_channel_interleave' not in launches                    # the shuffled store is the GEMM's
    assert not [s for s in launches if s.endswith('_bf16') or 'f32' in s or s in ('opa_dwconv_act', 'opa_dwconv_actp', 'opa_dwconv_dilated_act')]
    assert all(f.isfinite().all() for f in out)
    del launches[:]
    _forward(net, x, False)
    assert GEMM not in launches and STENCIL not in launches and 'opa_channel_interleave' in launches
    assert not [s for s in launches if s.startswith('opa_gemm') or s.startswith('opa_dwconv')]


@pytest.mark.parametrize('name', NETS)
def test_the_forward_repeats_bit_for_bit(launches, name):
    """Everything the route computes repeats bit for bit, on the same input and on a fresh clone of it: the whole trunk (the stem is
    torch's, and repeats) and every head that takes the kernel -- for k16 that is the whole forward.  A head that stays with torch
    (k30: K = 2048) is MIOpen's 16-bit convolution, which does not repeat at these shapes in bfloat16 (profiles/unit_bf16/README.md):
    such a head is asked to be finite and of the same shape, no more."""
    net, x, _ = _case(name, 1)
    saved = x.clone()
    a = _forward(net, x, True)
    b = _forward(net, x.clone(), True)
    assert torch.equal(x, saved)
    trunks = [_forward(net.base_net, t, True) for t in (x, x.clone(), x)]
    assert trunks[0].dtype == F16 and all(torch.equal(trunks[0], t) for t in trunks[1:])
    routed = [h.conv.in_channels % 64 != 0 for h in net.head_nets]
    assert routed == [name == 'shufflenetv2k16'] * 2
    for on_the_kernel, p, q in zip(routed, a, b):
        assert p.shape == q.shape and p.isfinite().all() and q.isfinite().all()
        if on_the_kernel:
            assert torch.equal(p, q)
    for h, on_the_kernel in zip(net.head_nets, routed):                # ... and from ONE trunk output
        if on_the_kernel:
            assert torch.equal(_forward(h, trunks[0], True), _forward(h, trunks[0], True))


@pytest.mark.parametrize('name', NETS)
def test_the_error_is_within_torchs_own_spread(launches, name):
    rows = []
    for seed in SEEDS:
        net, x, ref = _case(name, seed)
        e_on, e_off = _rms_error(_forward(net, x, True), ref), _rms_error(_forward(net, x, False), ref)
        brain, xb, refb = _case(name, seed, BF16)
        e_bf16 = _rms_error(_forward(brain, xb, True, 'UNIT_BF16'), refb)
        print('UNITF16ROUTE %s | seed %d | e_off (torch float16 trunk) %.4e | e_on (f16 unit GEMM + stencil) %.4e | e_on / e_off %.3f | '
              'e_bf16 (bfloat16 network, UNIT_BF16 on) %.4e | e_on / e_bf16 %.3f' % (name, seed, e_off, e_on, e_on / e_off, e_bf16, e_on / e_bf16))
        rows.append((seed, e_on, e_off))
    spread = max(r[2] for r in rows) / min(r[2] for r in rows)
    print('UNITF16ROUTE %s | spread of e_off over seeds %s: %.3f' % (name, SEEDS, spread))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > spread * r[2]]
    assert not bad, (bad, spread)
