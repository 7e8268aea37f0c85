"""ResNets cast to bfloat16 with their downsampling 1x1 convolutions on the bf16 two-source GEMM (``fused.PAIR_BF16``,
csrc/gemm2_bf16.hip): ``network.factory('resnet18')``, ``'resnet50'`` and the ResNet-50 with a dilated block 5
(``--resnet-block5-dilation 2``) with random BatchNorm statistics, optimized, ``.to(bfloat16)``, channels_last, input 2 x 3 x 97 x 65
(real kernels, MI355X).

1. switch on: a recorder on ``fused._launch`` counts 3 / 4 / 4 launches of ``opa_gemm2_bias_act_bf16`` and forward hooks on every
   ``downsample[0]`` never fire; switch off: none of the symbol, and the hooks fire 3 / 4 / 4 times;
2. with ``PAIR_BF16``, ``CONV3_BF16`` and ``STEM7_BF16`` on no ``nn.Conv2d`` of resnet18's ``base_net`` is called at all, and the trunk
   output of two forwards is equal bit for bit; the same for resnet50 with ``OPA_CONV1X1=gemm``;
3. the error bar.  ``e_on`` / ``e_off``: rms error of all head fields, route on / off, against the float32 forward of the same
   weights upcast, relative to the rms of that forward; only this switch differs between on and off.  The yardstick is ``e_off``; the
   margin is ``e_off``'s own seed-to-seed spread, max / min over the four seeds run.  Asserted: ``e_on <= spread * e_off`` on every
   seed, with the spread of THAT run -- once with ``CONV3_BF16`` off (a Bottleneck's conv2 leaves its bias + ReLU to the kernel's
   operand prologue) and once with it on.  The rows are printed as ``PAIRBF16ROUTE`` lines; one run is kept as
   profiles/gemm2_bf16/route_errors.log."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, headmeta, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_gemm2_bias_act_bf16'
SEEDS = (0, 1, 2, 3)
NETS = {'resnet18': 3, 'resnet50': 4, 'resnet50-block5-dilation2': 4}          # downsampling convolutions


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the switches restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    for name in ('PAIR_BF16', 'CONV3_BF16', 'STEM7_BF16'):
        monkeypatch.setattr(fused, name, getattr(fused, name))
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
    fused.PAIR_BF16 = on
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out


def _rms_error(got, ref):
    num = sum(float(((g.double() - r) ** 2).sum()) for g, r in zip(got, ref))
    den = sum(float((r ** 2).sum()) for r in ref)
    return (num / den) ** 0.5


def _hooked(modules, fired):
    return [m.register_forward_hook(lambda mod, args, out: fired.append(mod)) for m in modules]


@pytest.mark.parametrize('name', sorted(NETS))
def test_one_launch_per_downsampling_convolution_and_none_with_the_switch_off(launches, name):
    net, x, ref = _case(name, 0)
    downs = [m.downsample[0] for m in net.modules() if getattr(m, 'downsample', None) is not None]
    assert len(downs) == NETS[name] and all(isinstance(d, nn.Conv2d) and d.kernel_size == (1, 1) for d in downs)
    if name == 'resnet50-block5-dilation2':
        assert downs[-1].stride == (1, 1) and downs[-2].stride == (2, 2)
    fired = []
    handles = _hooked(downs, fired)
    try:
        del launches[:]                                                # (the float32 reference's, where this call computed it)
        out = _forward(net, x, True)
        assert launches.count(SYMBOL) == len(downs) and not fired, (launches.count(SYMBOL), len(fired))
        assert len(out) == len(ref) and all(f.shape == r.shape and f.isfinite().all() for f, r in zip(out, ref))
        del launches[:]
        off = _forward(net, x, False)
        assert SYMBOL not in launches and len(fired) == len(downs) and set(fired) == set(downs)
        assert all(f.shape == g.shape for f, g in zip(out, off))
    finally:
        for h in handles:
            h.remove()


@pytest.mark.parametrize('name', ['resnet18', 'resnet50'])
def test_no_convolution_of_the_trunk_is_torchs_and_the_trunk_repeats_bit_for_bit(launches, monkeypatch, name):
    net, x, _ = _case(name, 0)
    if name == 'resnet50':                                             # every 1x1 convolution to the GEMM, whatever a timing would say
        monkeypatch.setenv('OPA_CONV1X1', 'gemm')
        monkeypatch.setattr(fused, '_CHOICE', {})                      # (and whatever an earlier forward of these shapes entered)
    fused.CONV3_BF16, fused.STEM7_BF16 = True, True
    trunk = net.base_net
    convs = [m for m in trunk.modules() if isinstance(m, nn.Conv2d)]
    assert len(convs) == {'resnet18': 20, 'resnet50': 53}[name]
    fired = []
    handles = _hooked(convs, fired)
    try:
        first = _forward(trunk, x, True)
        again = _forward(trunk, x, True)
        assert not fired, [type(m).__name__ for m in fired][:5]
        assert first.dtype == BF16 and first.isfinite().all()
        assert torch.equal(first.contiguous().view(torch.int16), again.contiguous().view(torch.int16))
        _forward(trunk, x, False)                                      # (the hooks do fire: the downsampling convolutions)
        assert len(fired) == NETS[name]
    finally:
        for h in handles:
            h.remove()


@pytest.mark.parametrize('conv3_bf16', [False, True], ids=['pro', 'plain'])
@pytest.mark.parametrize('name', sorted(NETS))
def test_the_error_is_within_torchs_own_spread(launches, name, conv3_bf16):
    fused.CONV3_BF16 = conv3_bf16
    rows = []
    for seed in SEEDS:
        net, x, ref = _case(name, seed)
        e_on, e_off = _rms_error(_forward(net, x, True), ref), _rms_error(_forward(net, x, False), ref)
        print('PAIRBF16ROUTE %s | CONV3_BF16 %d | seed %d | e_off (torch downsampling convolution) %.4e | e_on (bf16 two-source GEMM) %.4e | '
              'e_on / e_off %.3f' % (name, conv3_bf16, seed, e_off, e_on, e_on / e_off))
        rows.append((seed, e_on, e_off))
    spread = max(r[2] for r in rows) / min(r[2] for r in rows)
    print('PAIRBF16ROUTE %s | CONV3_BF16 %d | spread of e_off over seeds %s: %.3f' % (name, conv3_bf16, SEEDS, spread))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > spread * r[2]]
    assert not bad, (bad, spread)
