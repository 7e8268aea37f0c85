"""ResNets cast to bfloat16 with their 3x3 convolutions on the bf16 implicit GEMM (``fused.CONV3_BF16``, csrc/conv3x3_bf16.hip):
``network.factory('resnet18')``, ``'resnet50'`` and the ResNet-50 with a dilated block 5 (``--resnet-block5-dilation 2``) with random
BatchNorm statistics, optimized, ``.to(bfloat16)``, channels_last, input 2 x 3 x 97 x 65 (real kernels, MI355X).

1. switch on: a recorder on ``fused._launch`` counts exactly one ``opa_conv3x3_act_bf16`` per ``nn.Conv2d`` with a 3x3 kernel and
   groups 1 in the module tree (16 for resnet18, 16 for resnet50) and no ``opa_gemm_pro_bias_act_bf16`` (conv2's bias + ReLU are the
   kernel's, nothing is left to the next GEMM's prologue); switch off: none of the symbol;
2. the outputs are finite and of the same shapes with the route on;
3. the error bar.  ``e_on`` / ``e_off``: rms error of all head fields, route on / off, against the float32 forward of the same
   weights upcast, relative to the rms of that forward.  The yardstick is ``e_off``, torch's own bfloat16 trunk; the margin is
   ``e_off``'s own seed-to-seed spread, max / min over the four seeds run -- what the yardstick itself moves by when nothing but the
   random weights and input change.  Asserted: ``e_on <= spread * e_off`` on every seed, with the spread of THAT run.  The rows are
   printed as ``CONV3BF16ROUTE`` lines; one run is kept as profiles/conv3_bf16/route_errors.log: spread 1.72 (resnet18), 1.21
   (resnet50) and 1.23 (dilated block 5); ``e_on / e_off`` 0.52 - 0.60, 0.71 - 0.82 and 0.71 - 0.85 -- the route's error is BELOW
   torch's on every seed (one rounding per convolution), so the margin is never used."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, headmeta, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_conv3x3_act_bf16'
SEEDS = (0, 1, 2, 3)
NETS = ('resnet18', 'resnet50', 'resnet50-block5-dilation2')


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the switch restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    monkeypatch.setattr(fused, 'CONV3_BF16', fused.CONV3_BF16)
    return symbols


def _build(name, seed):
    if name != 'resnet50-block5-dilation2':
        return network.factory(name, seed=seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        base = network.Resnet('resnet50', block5_dilation=2)
        net = network.Shell(base, [network.CompositeField4(m, base.out_features) for m in headmeta.cocokp_metas()])
    finally:
        torch.random.set_rng_state(state)
    return net.eval()


@functools.lru_cache(maxsize=None)
def _case(name, seed):
    """-> (the optimized bfloat16 network, x, the head fields of its float32 copy on x upcast), computed once and left unchanged."""
    net = _build(name, seed).cuda()
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
    fused.CONV3_BF16 = on
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out


def _rms_error(got, ref):
    num = sum(float(((g.double() - r) ** 2).sum()) for g, r in zip(got, ref))
    den = sum(float((r ** 2).sum()) for r in ref)
    return (num / den) ** 0.5


def _convs3x3(net):
    return [m for m in net.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1]


@pytest.mark.parametrize('name', NETS)
def test_one_launch_per_3x3_convolution_and_none_with_the_switch_off(launches, name):
    net, x, ref = _case(name, 0)
    convs = _convs3x3(net)
    assert len(convs) == 16
    if name == 'resnet50-block5-dilation2':
        assert [m.dilation for m in convs[-3:]] == [(2, 2)] * 3 and all(m.stride == (1, 1) for m in convs[-3:])
    del launches[:]                                                    # (the float32 reference's, where this call computed it)
    out = _forward(net, x, True)
    assert launches.count(SYMBOL) == len(convs), (launches.count(SYMBOL), len(convs))
    assert 'opa_gemm_pro_bias_act_bf16' not in launches
    passes_on = launches.count('opa_bias_act')
    assert len(out) == len(ref) and all(f.shape == r.shape and f.isfinite().all() for f, r in zip(out, ref))
    del launches[:]
    off = _forward(net, x, False)
    assert SYMBOL not in launches
    if name == 'resnet18':                                             # both epilogue passes of every block are the kernel's: the stem's stays
        assert (passes_on, launches.count('opa_bias_act')) == (1, 1 + len(convs))
    assert all(f.shape == g.shape for f, g in zip(out, off))


@pytest.mark.parametrize('name', NETS)
def test_the_error_is_within_torchs_own_spread(launches, name):
    rows = []
    for seed in SEEDS:
        net, x, ref = _case(name, seed)
        e_on, e_off = _rms_error(_forward(net, x, True), ref), _rms_error(_forward(net, x, False), ref)
        print('CONV3BF16ROUTE %s | seed %d | e_off (torch bfloat16 trunk) %.4e | e_on (bf16 3x3 implicit GEMM) %.4e | e_on / e_off %.3f'
              % (name, seed, e_off, e_on, e_on / e_off))
        rows.append((seed, e_on, e_off))
    spread = max(r[2] for r in rows) / min(r[2] for r in rows)
    print('CONV3BF16ROUTE %s | spread of e_off over seeds %s: %.3f' % (name, SEEDS, spread))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > spread * r[2]]
    assert not bad, (bad, spread)
