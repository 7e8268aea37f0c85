"""SqueezeNet on the project's kernels (real kernels, MI355X): the ceil-mode max-pool (``opa_maxpool3x3_ceil_bias_act``), the Fire
expand kernel (``csrc/fire.hip``), the Fire route built from it and the unit-mode GEMM (``network._Fire._forward_unit``), and the
whole network.

The error criterion is the one of ``test_gpu_unit_routes.py`` and ``test_gpu_mobilenetv3.py``: ``ref64`` the unfused module or op in
``double()``; ``e0`` the error against ``ref64`` of the SAME unfused float32 torch module or op (the median of nine calls), not of the
code under test; ``err = max |got - ref64| / max |ref64|`` and the same as an rms; required ``err <= 2 * e0`` (two independent errors
of size ``e0``).  Every case prints an ``SQZ`` line (``pytest -s``); the lines of a run are kept in
``profiles/squeezenet/route_errors.log``.  The route is off by default (``fused.FIRE``); the ``rec`` fixture switches it on.  The
kernel is tested with six and with nine terms; the route runs with ``fused.FIRE_TERMS`` (nine: see there) while ``X3_TERMS`` is at
its default of six, which the heads' convolutions of the whole network use."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openpifpaf_amd import fused, network

import trunk_common as tc

pytestmark = pytest.mark.gpu

CL = torch.channels_last
_LAUNCHERS = {'conv1x1_unit_x3': 'unit', 'fire_expand_bias_relu': 'fire_expand', 'maxpool3x3_bias_act_': 'pool', 'bias_act_': 'bias_act',
              'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3', 'head_conv_x3': 'head_x3', 'head_epilogue': 'head_epilogue'}
# in, squeeze, expand 1x1, expand 3x3: the eight Fire modules of squeezenet1_1
FIRES = [cfg for cfg in network.SqueezeNet.CONFIGS['squeezenet'] if cfg is not None]
PAIRS = [(16, 64), (32, 128), (48, 192), (64, 256)]
# (1, 1): every tap but the centre in the padding; (9, 7): smaller than one 8 x 16 pixel tile of the kernel (two tile rows, the second
# ragged); (17, 35): three tile rows and three tile columns with a ragged last tile each way (17 = 2 * 8 + 1, 35 = 2 * 16 + 3)
SIZES = [(1, 1), (9, 7), (17, 35)]


_report = functools.partial(tc.report, 'SQZ')


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder; nothing may be timed; the route switched on, the other switches at their defaults and the choice table
    empty, all restored after."""
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_UNIT', 'FIRE'))


# ---- 1. the pool in ceil mode ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('relu', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_pool_ceil_mode(dtype, relu):
    """``torch.equal`` to torch's ceil-mode pool; an even size has a last window that holds one row / column alone; two images, so
    that an index error across images shows."""
    for H, W in [(1, 1), (2, 2), (7, 8), (8, 7), (8, 8), (16, 17)]:
        for C in (8, 64, 128):
            x = torch.randn((2, C, H, W), generator=tc.gen(100 * H + W + C)).to(dtype).cuda().contiguous(memory_format=CL)
            assert fused.maxpool3x3_supported(x)
            want = F.max_pool2d(F.relu(x) if relu else x, 3, 2, 1, ceil_mode=True)
            x0 = x.clone()
            got = fused.maxpool3x3_bias_act_(x, relu=relu, ceil_mode=True)
            what = '%s %dx%d C %d' % (dtype, H, W, C)
            assert tuple(got.shape) == tuple(want.shape) == (2, C) + fused.maxpool3x3_out_hw(H, W, True), what
            assert got.is_contiguous(memory_format=CL) and torch.equal(x, x0), what
            assert torch.equal(got, want), what
            # floor mode is what it was: the same entry point as before, torch's floor-mode sizes
            assert torch.equal(fused.maxpool3x3_bias_act_(x, relu=relu), F.max_pool2d(F.relu(x) if relu else x, 3, 2, 1)), what


# ---- 2. the Fire expand kernel -----------------------------------------------------------------------------------------------

def _expands(s, e, seed):
    fire = tc.randomize_(network._Fire(2 * e, s, e, e), seed).cuda()
    return fire.expand1x1, fire.expand3x3


def _expand_torch(e1, e3, h):
    return torch.cat([F.relu(e1(h)), F.relu(e3(h))], 1)


@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('s,e', PAIRS)
def test_fire_expand(s, e, size, terms):
    e1, e3 = _expands(s, e, s + e)
    h = F.relu(torch.randn((2, s) + size, generator=tc.gen(s + size[0]))).cuda().contiguous(memory_format=CL)     # (a squeezed tensor is >= 0)
    with torch.no_grad():
        ref64 = _expand_torch(copy.deepcopy(e1).double(), copy.deepcopy(e3).double(), h.double())
        assert fused.fire_expand_supported(e1, e3, h)
        h0 = h.clone()
        got = fused.fire_expand_bias_relu(e1, e3, h, terms=terms)
        assert torch.equal(h, h0) and got.is_contiguous(memory_format=CL) and got.shape == ref64.shape and got.isfinite().all()
        assert torch.equal(got, fused.fire_expand_bias_relu(e1, e3, h, terms=terms))
        if terms == fused.FIRE_TERMS:
            assert torch.equal(got, fused.fire_expand_bias_relu(e1, e3, h)), 'the route\'s term count is FIRE_TERMS'
        ok = True
        what = 's %d e %d %dx%d terms %d' % (s, e, size[0], size[1], terms)
        # both halves alone as well as whole: a wrong half cannot hide behind the other's scale
        for part, sl in (('whole', slice(None)), ('1x1', slice(0, e)), ('3x3', slice(e, 2 * e))):
            e0 = tc.e0(lambda: _expand_torch(e1, e3, h)[:, sl], ref64[:, sl])
            ok &= _report('fire expand %s %s' % (what, part), tc.errors(got[:, sl], ref64[:, sl]), e0)
    assert ok


@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('pixel', [(0, 4, 3), (1, 0, 0), (1, 8, 6)], ids=['interior', 'corner00', 'corner86'])
def test_fire_expand_non_finite(pixel, value, terms):
    """A NaN or +Inf in one element of ``h``: NaN in every 1x1 channel at its pixel and in every 3x3 channel at the pixels whose window
    holds it (of its image only); every other output bit for bit the clean run's."""
    s, e, H, W = 16, 64, 9, 7
    e1, e3 = _expands(s, e, 5)
    h = F.relu(torch.randn((2, s, H, W), generator=tc.gen(6))).cuda().contiguous(memory_format=CL)
    b, y, x = pixel
    with torch.no_grad():
        clean = fused.fire_expand_bias_relu(e1, e3, h, terms=terms)
        h[b, 5, y, x] = value
        got = fused.fire_expand_bias_relu(e1, e3, h, terms=terms)
    want = torch.zeros(clean.shape, dtype=torch.bool, device='cuda')
    want[b, :e, y, x] = True
    want[b, e:, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    assert clean.isfinite().all()
    assert torch.equal(got.isnan(), want), 'NaN in %d outputs, expected in %d' % (int(got.isnan().sum()), int(want.sum()))
    assert torch.equal(got[~want], clean[~want])


# ---- 3. the block route ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(cfg, seed):
    """-> (the unfused Fire on the CPU, x, ref64, e0)."""
    module = tc.randomize_(network._Fire(*cfg), seed)
    x = F.relu(torch.randn((2, cfg[0], 9, 7), generator=tc.gen(1000 + seed))).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(module).double().cuda()(x.double())
        plain = copy.deepcopy(module).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0


@pytest.mark.parametrize('cfg', FIRES, ids=lambda c: '-'.join(map(str, c)))
def test_block_route(rec, cfg):
    module, x, ref64, e0 = _reference(cfg, 0)
    opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
    x0 = x.clone()
    with torch.no_grad():
        first = opt(x)
        rec.trace.clear()
        got = opt(x)
        trace = list(rec.trace)
    assert trace == ['unit', 'fire_expand'], trace
    assert torch.equal(x, x0) and torch.equal(first, got)
    assert fused.choices() == {}, 'the route made a choice-table entry'
    assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape and got.isfinite().all()
    assert _report('block %s | %s' % ('-'.join(map(str, cfg)), ' '.join(trace)), tc.errors(got, ref64), e0)
    # switched off: torch's forward, convolution for convolution
    fused.FIRE = False
    with torch.no_grad():
        rec.trace.clear()
        off = opt(x)
    assert rec.trace == ['miopen:squeeze', 'miopen:expand1x1', 'miopen:expand3x3'], rec.trace
    assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max())


def test_block_route_declines(rec):
    """bfloat16, NCHW, autocast and a tensor that autograd follows take the torch forward."""
    module, x, _, _ = _reference(FIRES[3], 0)
    opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
    with torch.no_grad():
        assert opt._route_supported(x)
        assert not opt._route_supported(x.contiguous()) and not opt._route_supported(x.bfloat16())
        with torch.autocast('cuda', dtype=torch.bfloat16):
            assert not opt._route_supported(x)
            rec.trace.clear()
            opt(x)
        assert rec.trace and all(t.startswith('miopen:') for t in rec.trace), rec.trace
    xg = x.clone(memory_format=torch.preserve_format).requires_grad_()
    assert not opt._route_supported(xg)
    rec.trace.clear()
    opt(xg).sum().backward()
    assert all(t.startswith('miopen:') for t in rec.trace) and xg.grad is not None


def test_forward_after_load_state_dict(rec):
    cfg = FIRES[5]
    _, x, _, _ = _reference(cfg, 0)
    module1, _, _, _ = _reference(cfg, 1)
    opt = tc.optimized(tc.randomize_(network._Fire(*cfg), 0)).cuda().to(memory_format=CL)
    other = tc.optimized(module1).cuda().to(memory_format=CL)
    with torch.no_grad():
        before = opt(x)
        opt.load_state_dict(other.state_dict(), strict=True)
        rec.trace.clear()
        after = opt(x)
        assert rec.trace == ['unit', 'fire_expand'], rec.trace
        ref64 = copy.deepcopy(module1).double().cuda()(x.double())
        plain = copy.deepcopy(module1).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
        assert not torch.equal(before, after)
        assert torch.equal(after, other(x)), 'stale operand: max |delta| %.3g' % (after - other(x)).abs().max().item()
    assert _report('block %s after load_state_dict' % '-'.join(map(str, cfg)), tc.errors(after, ref64), e0)


# ---- 4. the whole network ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(2, 3, 65, 49), (1, 3, 64, 50)], ids=['odd', 'even'])
def test_whole_network(rec, shape):
    """cocokp heads: the optimized channels-last model with the route on against the double model, both head outputs.  The heads'
    1x1 convolutions are pinned to the split-operand kernel (512 input channels: ``head_conv_x3``), so nothing is timed.  The even
    input makes every pool's input even: 32 x 25 -> 17 x 13 -> 9 x 7 -> 5 x 4."""
    net = tc.randomize_(network.factory('squeezenet'), 7)
    x = torch.randn(shape, generator=tc.gen(8)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(net).double().cuda()(x.double())
        plain = copy.deepcopy(net).cuda().to(memory_format=CL)
        fused.FORCE_PICK = 'conv'                                      # e0: torch's own convolutions, the heads' too
        e0s = [tc.e0(lambda: plain(x)[i], r) for i, r in enumerate(ref64)]
        fused.FORCE_PICK = 'x3'
        opt = rec.watch(network.optimize_for_inference_(copy.deepcopy(net)).cuda().to(memory_format=CL))
        rec.trace.clear()
        got = opt(x)
        trace = list(rec.trace)
        again = opt(x)
    assert trace.count('fire_expand') == 8 and trace.count('unit') == 8 and trace.count('pool') == 3, trace
    assert [t for t in trace if t.startswith('miopen:')] == ['miopen:base_net.backbone.0'], 'only the stem is torch\'s'
    ok = True
    for i, (g, a, r) in enumerate(zip(got, again, ref64)):
        assert g.shape == r.shape and torch.equal(g, a) and g.isfinite().all()
        ok &= _report('squeezenet %s head %d' % ('x'.join(map(str, shape)), i), tc.errors(g, r), e0s[i])
    assert ok


# ---- 5. Predictor ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('on_device', [False, True], ids=['host-preprocess', 'device-preprocess'])
def test_predictor_smoke(on_device):
    from openpifpaf_amd.predictor import Predictor
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (64, 40, 3), dtype=np.uint8)]
    saved = Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess
    Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = 65, 2, on_device
    try:
        pred = Predictor('squeezenet')
        assert isinstance(pred.model_cpu.base_net, network.SqueezeNet)
        out = [p for p, _, _ in pred.numpy_images(frames)]
    finally:
        Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = saved
    assert len(out) == 2 and all(isinstance(p, list) for p in out)
