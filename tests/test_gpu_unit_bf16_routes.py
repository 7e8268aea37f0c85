"""ShuffleNetV2K cast to bfloat16 with its 1x1 convolutions on the bf16 GEMM's unit mode (``fused.UNIT_BF16``, csrc/gemm_unit_bf16.hip):
``network.factory('shufflenetv2k16')`` and ``'shufflenetv2k30'`` with random BatchNorm statistics, optimized, ``.to(bfloat16)``,
channels_last, input 2 x 3 x 97 x 65 (real kernels, MI355X).

1. switch on: a recorder on ``fused._launch`` counts exactly one ``opa_gemm_unit_actp_bf16`` per 1x1 convolution of the stages, one
   for ``conv5`` and one per head whose input channels are no multiple of 64 (k16: 1392, both heads; k30: 2048, none) -- the count
   comes from the module tree; switch off: none;
2. the forward repeats bit for bit: the trunk and every head on the kernel (a head that stays with MIOpen does not repeat of its own);
3. the error bar.  ``e_on`` / ``e_off``: rms error of all head fields, route on / off, against the float32 forward of the same
   weights upcast, relative to the rms of that forward.  The yardstick is ``e_off``, torch's own bfloat16 trunk; the margin is
   ``e_off``'s own seed-to-seed spread, max / min over the four seeds run -- what the yardstick itself moves by when nothing but the
   random weights and input change.  Asserted: ``e_on <= spread * e_off`` on every seed, with the spread of THAT run.  Measured
   (profiles/unit_bf16/route_errors.log, printed here as ``UNITBF16ROUTE`` lines): spread 1.12 (k16) and 1.07 (k30);
   ``e_on / e_off`` 0.47 - 0.51 (k16) and 0.94 - 0.95 (k30) -- the route's error is BELOW torch's on every seed (one rounding per
   convolution where torch rounds the convolution and then the bias and the activation), so the margin is never used."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_gemm_unit_actp_bf16'
SEEDS = (0, 1, 2, 3)
NETS = ('shufflenetv2k16', 'shufflenetv2k30')


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the switch restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    monkeypatch.setattr(fused, 'UNIT_BF16', fused.UNIT_BF16)
    return symbols


@functools.lru_cache(maxsize=None)
def _case(name, seed):
    """-> (the optimized bfloat16 network, x, the head fields of its float32 copy on x upcast), computed once and left unchanged."""
    net = network.factory(name, seed=seed).cuda()
    torch.manual_seed(100 + seed)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    network.optimize_for_inference_(net)
    net = net.to(BF16).to(memory_format=CL).requires_grad_(False)
    x = torch.randn((2, 3, 97, 65), device='cuda').to(BF16).contiguous(memory_format=CL)
    table = fused.choices()                                            # (the float32 forward may enter its decisions: put the table back)
    try:
        with torch.no_grad():
            ref = tuple(f.double() for f in copy.deepcopy(net).float()(x.float()))
    finally:
        fused.set_choices(table, replace=True)
    assert all(f.isfinite().all() for f in ref)
    return net, x, ref


def _forward(net, x, on):
    fused.UNIT_BF16 = on
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
    stages = [m for stage in (base.stage2, base.stage3, base.stage4) for m in stage.modules()
              if isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.groups == 1]
    heads = [h for h in net.head_nets if h.conv.in_channels % 64 != 0]
    return len(stages), 1, len(heads)


@pytest.mark.parametrize('name', NETS)
def test_one_launch_per_pointwise_convolution_and_none_with_the_switch_off(launches, name):
    net, x, _ = _case(name, 0)
    stages, conv5, heads = _expected_launches(net)
    assert (stages, heads) == {'shufflenetv2k16': (2 * 16 + 3, 2), 'shufflenetv2k30': (2 * 30 + 3, 0)}[name]
    del launches[:]                                                    # (the float32 reference's, where this call computed it)
    out = _forward(net, x, True)
    assert launches.count(SYMBOL) == stages + conv5 + heads, (launches.count(SYMBOL), stages, conv5, heads)
    assert 'opa_channel_interleave' not in launches                    # the shuffled store is the GEMM's
    assert all(f.isfinite().all() for f in out)
    del launches[:]
    _forward(net, x, False)
    assert SYMBOL not in launches and 'opa_channel_interleave' in launches


@pytest.mark.parametrize('name', NETS)
def test_the_forward_repeats_bit_for_bit(launches, name):
    """Everything the route computes repeats bit for bit, on the same input and on a fresh clone of it: the whole trunk (the stem is
    torch's, and repeats) and every head that takes the kernel -- for k16 that is the whole forward.  A head that stays with torch
    (k30: K = 2048) is MIOpen's bfloat16 convolution, which does NOT repeat at these shapes whatever its input
    (profiles/unit_bf16/repeatability.log, ``tools/gpu/unit_bf16_times.py --parts repeat``: the figures are quoted in
    profiles/unit_bf16/README.md -- from ONE trunk output k30's heads give several different results in 20 calls, and with the route
    off the trunk itself 20 in 20): such a head is asked to be finite and of the same shape, no more."""
    net, x, _ = _case(name, 1)
    saved = x.clone()
    a = _forward(net, x, True)
    b = _forward(net, x.clone(), True)
    assert torch.equal(x, saved)
    trunks = [_forward(net.base_net, t, True) for t in (x, x.clone(), x)]
    assert trunks[0].dtype == BF16 and all(torch.equal(trunks[0], t) for t in trunks[1:])
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
        print('UNITBF16ROUTE %s | seed %d | e_off (torch bfloat16 trunk) %.4e | e_on (bf16 unit GEMM) %.4e | e_on / e_off %.3f'
              % (name, seed, e_off, e_on, e_on / e_off))
        rows.append((seed, e_on, e_off))
    spread = max(r[2] for r in rows) / min(r[2] for r in rows)
    print('UNITBF16ROUTE %s | spread of e_off over seeds %s: %.3f' % (name, SEEDS, spread))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > spread * r[2]]
    assert not bad, (bad, spread)
