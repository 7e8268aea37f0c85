"""ResNets cast to float16 on the project's kernels (``fused.F16``: csrc/gemm_epilogue.hip, csrc/conv3x3_bf16.hip and
csrc/gemm2_bf16.hip instantiated for float16 on v_mfma_f32_32x32x16_f16), with the method of ``test_gpu_conv3x3_bf16_routes.py``:
``network.factory('resnet18')``, ``'resnet50'`` and the ResNet-50 with a dilated block 5 (``--resnet-block5-dilation 2``) with random
BatchNorm statistics, optimized, ``.half()``, channels_last, input 2 x 3 x 97 x 65, seeds 0 - 3, ``OPA_CONV1X1=gemm`` (real kernels,
MI355X).

Range: on the CPU in float32, for exactly these networks and seeds, the largest convolution output is 17.5 (resnet18) and 1150
(resnet50), a factor 57 below float16's 65504; the test asserts that the float16 torch trunk's fields are finite before it uses them
as the yardstick.

1. switch on: a recorder on ``fused._launch`` and forward hooks on the modules count one ``opa_conv3x3_act_f16`` per dense 3x3
   ``nn.Conv2d``, one ``opa_gemm2_bias_act_f16`` per downsampling convolution, ``opa_gemm_bias_act_f16`` for the remaining 1x1
   convolutions of the blocks, no ``opa_gemm_pro_bias_act_f16`` (conv2's bias + ReLU are the 3x3 kernel's), and the stem as the only
   ``nn.Conv2d`` called in the trunk; switch off: none of the ``_f16`` symbols;
2. the outputs are finite and have the float32 network's shapes; two forwards of the trunk with the switch on are bit-equal, like
   the bfloat16 twins' trunks (the heads' 1x1 convolutions stay torch's, and those do not repeat of their own: measured on resnet18,
   where the stem and the blocks repeat and the heads on ONE trunk output do not -- ``test_gpu_unit_bf16_routes.py`` says the same of
   a bfloat16 head that stays with MIOpen);
3. the error bar.  ``e_on`` / ``e_off``: rms error of all head fields, route on / off, against the float32 forward of the same
   weights upcast, relative to the rms of that forward.  The yardstick is ``e_off``, torch's own float16 trunk; the margin is
   ``e_off``'s own seed-to-seed spread, max / min over the four seeds of THAT run.  Asserted: ``e_on <= spread * e_off`` on every
   seed.  The same test prints ``e_bf16``, the bfloat16 cast of the same network with ``CONV3_BF16``, ``PAIR_BF16`` and ``STEM7_BF16``
   on, against ITS float32 upcast; ``e_on / e_bf16`` is printed, not asserted (from the mantissa widths one expects about 1/8).  The
   rows are printed as ``F16ROUTE`` lines; one run is kept as profiles/f16/route_errors.log."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, headmeta, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F16, BF16 = torch.float16, torch.bfloat16
SEEDS = (0, 1, 2, 3)
NETS = ('resnet18', 'resnet50', 'resnet50-block5-dilation2')
F16_SYMBOLS = ('opa_gemm_bias_act_f16', 'opa_gemm_pro_bias_act_f16', 'opa_conv3x3_act_f16', 'opa_gemm2_bias_act_f16')
BF16_SWITCHES = ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16')


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
    for name in ('F16',) + BF16_SWITCHES:
        monkeypatch.setattr(fused, name, False)
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
    """-> {dtype: (the optimized network cast to it, x, the head fields of its float32 copy on x upcast)} for float16 and bfloat16,
    the same weights before the cast; computed once and left unchanged."""
    net = _build(name, seed).cuda()
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
        out[dt] = (cast, x, _reference(cast, x))
    return out


def _forward(net, x, **switches):
    for name in ('F16',) + BF16_SWITCHES:
        setattr(fused, name, bool(switches.get(name, False)))
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out


def _rms_error(got, ref):
    num = sum(float(((g.double() - r) ** 2).sum()) for g, r in zip(got, ref))
    den = sum(float((r ** 2).sum()) for r in ref)
    return (num / den) ** 0.5


@pytest.mark.parametrize('name', NETS)
def test_the_trunk_runs_on_the_float16_kernels_and_not_with_the_switch_off(launches, name):
    net, x, ref = _case(name, 0)[F16]
    trunk = net.base_net
    convs = {m: n for n, m in trunk.named_modules() if isinstance(m, nn.Conv2d)}
    dense3 = [m for m in convs if m.kernel_size == (3, 3) and m.groups == 1]
    down = [m for m, n in convs.items() if n.endswith('downsample.0')]
    assert len(dense3) == 16 and len(down) == (3 if name == 'resnet18' else 4)
    called = []
    hooks = [m.register_forward_hook(lambda mod, args, out: called.append(convs[mod])) for m in convs]
    try:
        del launches[:]                                                # (the float32 reference's, where this call computed it)
        out = _forward(net, x, F16=True)
        on = list(launches)
        assert on.count('opa_conv3x3_act_f16') == len(dense3) and on.count('opa_gemm2_bias_act_f16') == len(down)
        pairs = 0 if name == 'resnet18' else len(down)                 # a Bottleneck's conv3 goes into the pair's launch
        assert on.count('opa_gemm_bias_act_f16') == len(convs) - 1 - len(dense3) - len(down) - pairs
        assert 'opa_gemm_pro_bias_act_f16' not in on and not [s for s in on if s.endswith('_bf16')]
        assert called == ['input_block.0'], called
        assert len(out) == len(ref) and all(f.shape == r.shape and f.isfinite().all() for f, r in zip(out, ref))
        first, again = _forward(trunk, x, F16=True), _forward(trunk, x, F16=True)
        assert first.dtype == F16 and first.isfinite().all()
        assert torch.equal(first.contiguous().view(torch.int16), again.contiguous().view(torch.int16))
        del launches[:], called[:]
        off = _forward(net, x, **{s: True for s in BF16_SWITCHES})      # ... whatever the bfloat16 switches say
        assert not [s for s in launches if s in F16_SYMBOLS or s.endswith('_bf16')]
        assert sorted(called) == sorted(convs.values())
        assert all(f.shape == g.shape and g.isfinite().all() for f, g in zip(out, off))
    finally:
        for h in hooks:
            h.remove()


@pytest.mark.parametrize('name', NETS)
def test_the_error_is_within_torchs_own_spread(launches, name):
    rows = []
    for seed in SEEDS:
        case = _case(name, seed)
        net, x, ref = case[F16]
        off = _forward(net, x)
        assert all(f.isfinite().all() for f in off)                    # the yardstick itself stays inside float16's range
        e_off, e_on = _rms_error(off, ref), _rms_error(_forward(net, x, F16=True), ref)
        bnet, bx, bref = case[BF16]
        e_bf16 = _rms_error(_forward(bnet, bx, **{s: True for s in BF16_SWITCHES}), bref)
        print('F16ROUTE %s | seed %d | e_off (torch float16 trunk) %.4e | e_on (float16 kernels) %.4e | e_on / e_off %.3f | '
              'e_bf16 (bfloat16 kernels) %.4e | e_on / e_bf16 %.3f' % (name, seed, e_off, e_on, e_on / e_off, e_bf16, e_on / e_bf16))
        rows.append((seed, e_on, e_off))
    spread = max(r[2] for r in rows) / min(r[2] for r in rows)
    print('F16ROUTE %s | spread of e_off over seeds %s: %.3f' % (name, SEEDS, spread))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > spread * r[2]]
    assert not bad, (bad, spread)
