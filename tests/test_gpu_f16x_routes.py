"""A ResNeXt-50 and a ResNet-18 cast to float16 with NO ``nn.Conv2d`` left in the forward: the grouped 3x3 convolutions behind
``fused.GCONV_F16`` (csrc/gconv3x3_bf16.hip on v_mfma_f32_32x32x16_f16) and the 7x7 stem behind ``fused.STEM7_F16``
(csrc/stem7x7_bf16.hip), next to ``fused.F16`` and ``fused.HEAD16``.  The method is ``test_gpu_f16_routes.py``'s: ``network.factory``
with random BatchNorm statistics, optimized, ``.half()``, channels_last, input 2 x 3 x 97 x 65, seeds 0 - 3, ``OPA_CONV1X1=gemm``, a
recorder on ``fused._launch`` and forward hooks on every ``nn.Conv2d`` (real kernels, MI355X).

1. every switch on: 16 ``opa_gconv3x3_act_f16`` and one ``opa_stem7x7_act_f16`` (resnet18: the stem, also from a cropped NCHW view
   with the bits of the dense input's result), no ``opa_gemm_pro_bias_act_f16`` (nothing is owed), no ``_bf16`` symbol, no
   ``nn.Conv2d`` called, and the whole forward -- trunk and heads -- twice with equal bits;
2. the two new switches off, everything else on: the stem and the 16 grouped convolutions are the convolutions called, none of the
   new symbols is launched; every bfloat16 switch on and the new ones off: the same; the new switches on: a bfloat16 network
   launches what it launched without them;
3. the error bar.  ``e_on`` / ``e_off``: rms error of all head fields against the float32 forward of the same weights upcast,
   relative to the rms of that forward, with every switch on / with only the two new switches off.  The yardstick is ``e_off``
   -- torch's own float16 stem and grouped convolutions --, the margin its own seed-to-seed spread, max / min over the four seeds
   of THAT run: ``e_on <= spread * e_off`` on every seed.  The rows are printed as ``F16XROUTE`` lines; one run is kept as
   profiles/f16x/route_errors.log."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F16, BF16 = torch.float16, torch.bfloat16
SEEDS = (0, 1, 2, 3)
NETS = ('resnext50', 'resnet18')
NEW = ('GCONV_F16', 'STEM7_F16')
NEW_SYMBOLS = ('opa_gconv3x3_act_f16', 'opa_stem7x7_act_f16')
OLD = ('F16', 'HEAD16')
BF16_SWITCHES = ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16', 'GCONV_BF16')
ALL = NEW + OLD + BF16_SWITCHES


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the plain 1x1 choice pinned to the
    GEMM, nothing timed; the switches restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    monkeypatch.setenv('OPA_CONV1X1', 'gemm')
    monkeypatch.setattr(fused, '_CHOICE', {})
    for name in ALL:
        monkeypatch.setattr(fused, name, False)
    return symbols


def _reference(net, x):
    table = fused.choices()                                            # (the float32 forward may enter its decisions: put the table back)
    try:
        with torch.no_grad():
            ref = tuple(f.double() for f in copy.deepcopy(net).float()(x.float()))
    finally:
        fused.set_choices(table, replace=True)
    assert all(f.isfinite().all() for f in ref)
    return ref


@functools.lru_cache(maxsize=None)
def _case(name, seed):
    """-> {dtype: (the optimized network cast to it, x, the head fields of its float32 copy on x upcast)} for float16 and bfloat16
    (bfloat16: no reference), the same weights before the cast; computed once and left unchanged."""
    net = network.factory(name, seed=seed).cuda()
    torch.manual_seed(100 + seed)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    network.optimize_for_inference_(net)
    x32 = torch.randn((2, 3, 97, 65), device='cuda')
    out = {}
    for dt in (F16, BF16):
        cast = copy.deepcopy(net).to(dt).to(memory_format=CL).requires_grad_(False)
        x = x32.to(dt).contiguous(memory_format=CL)
        out[dt] = (cast, x, _reference(cast, x) if dt == F16 else None)
    return out


def _forward(net, x, *on):
    for name in ALL:
        setattr(fused, name, name in on)
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out


def _bits(fields):
    return [f.contiguous().view(torch.int32 if f.dtype == torch.float32 else torch.int16) for f in fields]


def _hooked(net, called):
    convs = {m: n for n, m in net.named_modules() if isinstance(m, nn.Conv2d)}
    return convs, [m.register_forward_hook(lambda mod, args, out: called.append(convs[mod])) for m in convs]


@pytest.mark.parametrize('name', NETS)
def test_a_half_network_calls_no_convolution_and_repeats_bit_for_bit(launches, name):
    net, x, ref = _case(name, 0)[F16]
    called = []
    convs, hooks = _hooked(net, called)
    grouped = sorted(n for m, n in convs.items() if m.groups > 1)
    assert len(grouped) == (16 if name == 'resnext50' else 0)
    try:
        del launches[:]                                                # (the float32 reference's, where this call computed it)
        out = _forward(net, x, *(NEW + OLD))
        on = list(launches)
        assert on.count('opa_gconv3x3_act_f16') == len(grouped) and on.count('opa_stem7x7_act_f16') == 1 and on[0] == 'opa_stem7x7_act_f16'
        assert 'opa_gemm_pro_bias_act_f16' not in on and 'opa_bias_act' not in on          # nothing is owed, no epilogue pass
        assert not [s for s in on if s.endswith('_bf16')]
        assert on.count('opa_head_conv_fields_f16') == len(net.head_nets)
        assert called == [], called                                    # no nn.Conv2d, trunk or heads
        assert len(out) == len(ref) and all(f.shape == r.shape and f.isfinite().all() for f, r in zip(out, ref))
        again = _forward(net, x, *(NEW + OLD))
        assert all(torch.equal(a, b) for a, b in zip(_bits(out), _bits(again)))             # the whole forward, bit for bit

        # the new switches off, everything else on -- the bfloat16 switches too: what a float16 network ran before
        del launches[:], called[:]
        off = _forward(net, x, *(OLD + BF16_SWITCHES))
        assert not [s for s in launches if s in NEW_SYMBOLS or s.endswith('_bf16')]
        assert sorted(called) == sorted(['base_net.input_block.0'] + grouped)                 # the stem and the grouped convolutions
        assert launches.count('opa_gemm_pro_bias_act_f16') == (12 if name == 'resnext50' else 0)
        assert launches[0] == 'opa_bias_act' and launches.count('opa_bias_act') == 1        # the stem's epilogue pass
        assert all(f.shape == g.shape and g.isfinite().all() for f, g in zip(out, off))
        del launches[:], called[:]
        _forward(net, x, *BF16_SWITCHES)                               # every bfloat16 switch on alone: no kernel of this project's trunk
        assert not [s for s in launches if s.endswith('_f16') or s.endswith('_bf16')]
        assert len(called) == len(convs)
    finally:
        for h in hooks:
            h.remove()


def test_the_stem_reads_a_cropped_nchw_view_with_the_dense_inputs_bits(launches):
    net, x, _ = _case('resnet18', 0)[F16]
    trunk = net.base_net
    big = torch.full((2, 3, 97 + 5, 65 + 4), float('nan'), dtype=F16, device='cuda')        # NCHW, NaN around the image
    view = big[:, :, 2:2 + 97, 1:1 + 65]
    view.copy_(x)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=CL)
    del launches[:]
    dense = _forward(trunk, x, *(NEW + OLD))
    cropped = _forward(trunk, view, *(NEW + OLD))
    assert launches.count('opa_stem7x7_act_f16') == 2 and dense.isfinite().all()
    assert torch.equal(_bits([dense])[0], _bits([cropped])[0])


@pytest.mark.parametrize('name', NETS)
def test_a_bfloat16_network_launches_what_it_launched(launches, name):
    net, x, _ = _case(name, 0)[BF16]
    called = []
    convs, hooks = _hooked(net, called)
    try:
        for switches in ((), BF16_SWITCHES + ('HEAD16',)):
            del launches[:], called[:]
            before = _forward(net, x, *switches)
            want = (list(launches), list(called))
            del launches[:], called[:]
            after = _forward(net, x, *(switches + NEW))
            assert (list(launches), list(called)) == want and not [s for s in launches if s.endswith('_f16')]
            if switches:                                               # (its own kernels repeat; torch's convolutions need not)
                assert all(torch.equal(a, b) for a, b in zip(_bits(before), _bits(after)))
                assert called == [] and launches.count('opa_gconv3x3_act_bf16') == (16 if name == 'resnext50' else 0)
    finally:
        for h in hooks:
            h.remove()


@pytest.mark.parametrize('name', NETS)
def test_the_error_is_within_torchs_own_spread(launches, name):
    rows = []
    for seed in SEEDS:
        net, x, ref = _case(name, seed)[F16]
        off = _forward(net, x, *OLD)
        assert all(f.isfinite().all() for f in off)                    # the yardstick itself stays inside float16's range
        e_off, e_on = _rms_error(off, ref), _rms_error(_forward(net, x, *(NEW + OLD)), ref)
        print('F16XROUTE %s | seed %d | e_off (torch float16 stem and grouped 3x3) %.4e | e_on (float16 kernels) %.4e | e_on / e_off %.3f'
              % (name, seed, e_off, e_on, e_on / e_off))
        rows.append((seed, e_on, e_off))
    spread = max(r[2] for r in rows) / min(r[2] for r in rows)
    print('F16XROUTE %s | spread of e_off over seeds %s: %.3f' % (name, SEEDS, spread))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > spread * r[2]]
    assert not bad, (bad, spread)


def _rms_error(got, ref):
    num = sum(float(((g.double() - r) ** 2).sum()) for g, r in zip(got, ref))
    den = sum(float((r ** 2).sum()) for r in ref)
    return (num / den) ** 0.5
