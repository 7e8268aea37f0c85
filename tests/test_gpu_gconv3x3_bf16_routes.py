"""A ResNeXt cast to bfloat16 with its grouped 3x3 convolutions on the bf16 implicit GEMM (``fused.GCONV_BF16``,
csrc/gconv3x3_bf16.hip): ``network.factory('resnext50')`` and the ResNeXt-50 with a dilated block 5 (``--resnet-block5-dilation 2``)
with random BatchNorm statistics, optimized, ``.to(bfloat16)``, channels_last, input 2 x 3 x 33 x 25 (real kernels, MI355X).

1. switch on: a recorder on ``fused.gconv3x3_bias_act_bf16`` counts one call per block (16) and forward hooks on every 3x3
   ``nn.Conv2d`` never fire; the dilated blocks take the route too; switch off: no call, the hooks fire 16 times, and the launches are
   those of the route table without the row (the parent commit's);
2. with ``CONV3_BF16``, ``STEM7_BF16`` and ``PAIR_BF16`` on as well no ``nn.Conv2d`` of the trunk is called at all, two forwards give
   equal bits, and the pair kernel receives ``a_bias=None`` (nothing is owed to its operand prologue);
3. the head fields: the rms error against the float32 forward of the same weights upcast, relative to the rms of that forward, with
   the route on is <= 1.05 x that with the route off (torch's grouped bfloat16 convolution) -- the project's relative bar.  Both are
   printed as ``GCONVBF16ROUTE`` lines; one run is kept as profiles/gconv_bf16/route_errors.log."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, headmeta, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_gconv3x3_act_bf16'
NETS = ('resnext50', 'resnext50-block5-dilation2')
SWITCHES = ('GCONV_BF16', 'PAIR_BF16', 'CONV3_BF16', 'STEM7_BF16')


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the switches restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    for name in SWITCHES:
        monkeypatch.setattr(fused, name, getattr(fused, name))
    return symbols


def _build(name, seed):
    if name == 'resnext50':
        return network.factory(name, seed=seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        base = network.Resnet('resnext50', block5_dilation=2)
        net = network.Shell(base, [network.CompositeField4(m, base.out_features) for m in headmeta.cocokp_metas()])
    finally:
        torch.random.set_rng_state(state)
    return net.eval()


@functools.lru_cache(maxsize=None)
def _case(name, seed=0):
    """-> (the optimized bfloat16 network, x, the head fields of its float32 copy on x upcast), computed once and left unchanged."""
    net = _build(name, seed).cuda()
    torch.manual_seed(100 + seed)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    network.optimize_for_inference_(net)
    net = net.to(BF16).to(memory_format=CL).requires_grad_(False)
    x = torch.randn((2, 3, 33, 25), device='cuda').to(BF16).contiguous(memory_format=CL)
    table = fused.choices()                                            # (the float32 forward may enter its decisions: put the table back)
    try:
        with torch.no_grad():
            ref = tuple(f.double() for f in copy.deepcopy(net).float()(x.float()))
    finally:
        fused.set_choices(table, replace=True)
    assert all(f.isfinite().all() for f in ref)
    return net, x, ref


def _forward(net, x, on):
    fused.GCONV_BF16 = on
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


def _grouped(net):
    return [m for m in net.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3)]


@pytest.fixture
def calls(monkeypatch):
    """Recorders on the two launchers -> {'gconv': [conv, ...], 'pair': [a_bias, ...]}"""
    seen = {'gconv': [], 'pair': []}
    gconv, pair = fused.gconv3x3_bias_act_bf16, fused.conv1x1_pair_bias_act_bf16

    def traced_gconv(conv, *args, **kw):
        seen['gconv'].append(conv)
        return gconv(conv, *args, **kw)

    def traced_pair(conv, dconv, h, x, bias, relu=True, a_bias=None):
        seen['pair'].append(a_bias)
        return pair(conv, dconv, h, x, bias, relu, a_bias)
    monkeypatch.setattr(fused, 'gconv3x3_bias_act_bf16', traced_gconv)
    monkeypatch.setattr(fused, 'conv1x1_pair_bias_act_bf16', traced_pair)
    return seen


@pytest.mark.parametrize('name', NETS)
def test_one_call_per_block_and_the_parents_launches_with_the_switch_off(launches, calls, monkeypatch, name):
    net, x, ref = _case(name)
    convs = _grouped(net)
    assert len(convs) == 16 and all(m.groups == 32 and m.in_channels == m.out_channels for m in convs)
    assert sorted({m.in_channels // m.groups for m in convs}) == [4, 8, 16, 32]
    if name == 'resnext50-block5-dilation2':
        assert [m.dilation for m in convs[-3:]] == [(2, 2)] * 3 and all(m.stride == (1, 1) for m in convs[-3:])
    fired = []
    handles = _hooked(convs, fired)
    try:
        del launches[:]                                                # (the float32 reference's, where this call computed it)
        out = _forward(net, x, True)
        assert calls['gconv'] == convs and launches.count(SYMBOL) == 16 and not fired, (len(calls['gconv']), len(fired))
        assert 'opa_gemm_pro_bias_act_bf16' not in launches             # conv2's bias + ReLU are the kernel's: nothing owed
        assert len(out) == len(ref) and all(f.shape == r.shape and f.isfinite().all() for f, r in zip(out, ref))
        _forward(net, x, False)                                        # (a shape seen for the first time is timed: let it be)
        del launches[:], calls['gconv'][:], fired[:]
        off = _forward(net, x, False)
        off_launches = list(launches)
        assert SYMBOL not in launches and not calls['gconv'] and fired == convs
        assert all(f.shape == g.shape for f, g in zip(out, off))
        # the parent commit's route table: the same launches (not the same bits: torch's bfloat16 convolutions do not repeat them)
        monkeypatch.setattr(network, '_CONV3_ROUTES', tuple(r for r in network._CONV3_ROUTES if r[0] != 'gconv-bf16'))
        assert len(network._CONV3_ROUTES) == 5
        del launches[:], fired[:]
        parent = _forward(net, x, False)
        assert launches == off_launches and fired == convs
        assert all(f.shape == g.shape and g.isfinite().all() for f, g in zip(off, parent))
    finally:
        for h in handles:
            h.remove()


def test_no_convolution_of_the_trunk_is_torchs_and_the_trunk_repeats_bit_for_bit(launches, calls, monkeypatch):
    net, x, _ = _case('resnext50')
    monkeypatch.setenv('OPA_CONV1X1', 'gemm')                          # every 1x1 convolution to the GEMM, whatever a timing would say
    monkeypatch.setattr(fused, '_CHOICE', {})                          # (and whatever an earlier forward of these shapes entered)
    fused.CONV3_BF16, fused.STEM7_BF16, fused.PAIR_BF16 = True, True, True
    trunk = net.base_net
    convs = [m for m in trunk.modules() if isinstance(m, nn.Conv2d)]
    assert len(convs) == 53
    fired = []
    handles = _hooked(convs, fired)
    try:
        first = _forward(trunk, x, True)
        again = _forward(trunk, x, True)
        assert not fired, [(type(m).__name__, m.kernel_size, m.groups) for m in fired][:5]
        assert first.dtype == BF16 and first.isfinite().all()
        assert torch.equal(first.contiguous().view(torch.int16), again.contiguous().view(torch.int16))
        assert len(calls['gconv']) == 32 and len(calls['pair']) == 8 and all(a is None for a in calls['pair'])
        del calls['pair'][:]
        _forward(trunk, x, False)                                      # (the hooks do fire: the grouped convolutions, whose epilogue is owed)
        assert [m for m in fired if m.groups == 32] == [m for m in convs if m.groups == 32] and len(fired) >= 16
        assert all(a is not None for a in calls['pair'])
    finally:
        for h in handles:
            h.remove()


@pytest.mark.parametrize('others', [False, True], ids=['alone', 'with-the-other-bf16-routes'])
@pytest.mark.parametrize('name', NETS)
def test_the_head_fields_are_no_further_from_float32_than_with_torchs_grouped_convolution(launches, name, others):
    net, x, ref = _case(name)
    fused.CONV3_BF16 = fused.STEM7_BF16 = fused.PAIR_BF16 = others
    e_on, e_off = _rms_error(_forward(net, x, True), ref), _rms_error(_forward(net, x, False), ref)
    print('GCONVBF16ROUTE %s | other bf16 routes %d | e_off (torch grouped bfloat16) %.4e | e_on (bf16 grouped implicit GEMM) %.4e | '
          'e_on / e_off %.3f' % (name, others, e_off, e_on, e_on / e_off))
    assert e_off > 0 and e_on <= 1.05 * e_off, (e_on, e_off)
