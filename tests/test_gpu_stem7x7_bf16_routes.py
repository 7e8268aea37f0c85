"""ResNets cast to bfloat16 with their 7x7 stem on the bf16 implicit GEMM (``fused.STEM7_BF16``, csrc/stem7x7_bf16.hip):
``network.factory('resnet18')`` and ``'resnet50'`` with random BatchNorm statistics, optimized, ``.to(bfloat16)``, channels_last,
input 2 x 3 x 97 x 65 (real kernels, MI355X).

1. resnet18 with ``fused.CONV3_BF16`` also on: a recorder on ``fused._launch`` counts exactly one ``opa_stem7x7_act_bf16`` and no
   ``opa_bias_act`` at all (the stem's epilogue pass was the last one left); ``STEM7_BF16`` off: none of the symbol;
2. the outputs are finite and of the same shapes with the route on;
3. the error bar, ``CONV3_BF16`` at its default so that the stem alone differs.  ``e_on`` / ``e_off``: rms error of all head fields,
   route on / off, against the float32 forward of the same weights upcast, relative to the rms of that forward.  The yardstick is
   ``e_off``, torch's own bfloat16 stem; the margin is ``e_off``'s own seed-to-seed spread, max / min over the four seeds run -- what
   the yardstick itself moves by when nothing but the random weights and input change.  Asserted: ``e_on <= spread * e_off`` on every
   seed, with the spread of THAT run.  The rows are printed as ``STEM7BF16ROUTE`` lines; one run is kept as
   profiles/stem7_bf16/route_errors.log;
4. a trunk forward (``CONV3_BF16`` on) from a non-contiguous input -- a crop of a larger NCHW bfloat16 tensor -- has the bits of the
   forward from the same crop made channels-last, and repeats bit for bit: the kernel reads the image where it lies.  The trunk, not
   the heads: their convolutions are torch's, and two runs of those on one input differ in their bits."""
import copy
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_stem7x7_act_bf16'
SEEDS = (0, 1, 2, 3)
NETS = ('resnet18', 'resnet50')


@pytest.fixture
def launches(monkeypatch):
    """A recorder on ``fused._launch`` (the launch still runs) -> the list of launched symbols; the switches restored afterwards."""
    symbols = []
    launch = fused._launch

    def recording(symbol, *args):
        symbols.append(symbol)
        return launch(symbol, *args)
    monkeypatch.setattr(fused, '_launch', recording)
    monkeypatch.setattr(fused, 'STEM7_BF16', fused.STEM7_BF16)
    monkeypatch.setattr(fused, 'CONV3_BF16', fused.CONV3_BF16)
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
    fused.STEM7_BF16 = on
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out


def _rms_error(got, ref):
    num = sum(float(((g.double() - r) ** 2).sum()) for g, r in zip(got, ref))
    den = sum(float((r ** 2).sum()) for r in ref)
    return (num / den) ** 0.5


@pytest.mark.parametrize('name', NETS)
def test_one_launch_for_the_stem_and_none_with_the_switch_off(launches, name):
    net, x, ref = _case(name, 0)
    fused.CONV3_BF16 = True
    del launches[:]                                                    # (the float32 reference's, where this call computed it)
    out = _forward(net, x, True)
    assert launches.count(SYMBOL) == 1, launches[:3]
    if name == 'resnet18':                                             # every epilogue pass is a kernel's own now
        assert launches.count('opa_bias_act') == 0
    assert len(out) == len(ref) and all(f.shape == r.shape and f.isfinite().all() for f, r in zip(out, ref))
    del launches[:]
    off = _forward(net, x, False)
    assert SYMBOL not in launches
    if name == 'resnet18':
        assert launches.count('opa_bias_act') == 1                     # the stem's
    assert all(f.shape == g.shape for f, g in zip(out, off))


@pytest.mark.parametrize('name', NETS)
def test_the_error_is_within_torchs_own_spread(launches, name):
    rows = []
    for seed in SEEDS:
        net, x, ref = _case(name, seed)
        e_on, e_off = _rms_error(_forward(net, x, True), ref), _rms_error(_forward(net, x, False), ref)
        print('STEM7BF16ROUTE %s | seed %d | e_off (torch bfloat16 stem) %.4e | e_on (bf16 7x7 implicit GEMM) %.4e | e_on / e_off %.3f'
              % (name, seed, e_off, e_on, e_on / e_off))
        rows.append((seed, e_on, e_off))
    spread = max(r[2] for r in rows) / min(r[2] for r in rows)
    print('STEM7BF16ROUTE %s | spread of e_off over seeds %s: %.3f' % (name, SEEDS, spread))
    assert all(e_off > 0 for _, _, e_off in rows)
    bad = [r for r in rows if r[1] > spread * r[2]]
    assert not bad, (bad, spread)


def test_a_cropped_nchw_input_gives_the_bits_of_the_same_crop_made_channels_last(launches):
    net, x, _ = _case('resnet18', 0)
    torch.manual_seed(7)
    big = torch.randn((2, 3, 97 + 6, 65 + 5), device='cuda').to(BF16)                    # NCHW
    crop = big[:, :, 4:4 + 97, 3:3 + 65]
    assert not crop.is_contiguous() and not crop.is_contiguous(memory_format=CL)
    fused.CONV3_BF16 = True                      # every convolution behind the stem in the project's kernels too: the trunk repeats bit for bit
    trunk = net.base_net                         # (the heads' convolutions are torch's, whose bits differ between two runs on ONE input)
    del launches[:]
    from_view = _forward(trunk, crop, True)
    assert launches.count(SYMBOL) == 1
    from_dense = _forward(trunk, crop.contiguous(memory_format=CL), True)
    again = _forward(trunk, crop, True)
    assert from_view.dtype == BF16 and from_view.isfinite().all() and tuple(from_view.shape) == tuple(from_dense.shape)
    assert torch.equal(from_view.contiguous().view(torch.int16), from_dense.contiguous().view(torch.int16))
    assert torch.equal(from_view.contiguous().view(torch.int16), again.contiguous().view(torch.int16))
