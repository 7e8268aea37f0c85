"""Group norm + activation on the project's kernels (real kernels, MI355X): ``opa_groupnorm_actp`` (``csrc/groupnorm.hip``), its launcher
``fused.group_norm_act`` and the group-norm route of ``network.ShuffleNetV2K(layer_norm='group')`` behind ``fused.GN``.

The moments kernel cuts the pixels of an image into chunks of P = 512 (``kGnChunkPixels``, ``OPA_GN_CHUNK_PIXELS``), so the pixel counts
are 1, 2, 15 (3 x 5), 512 (one chunk exactly), 529 (23 x 23: one chunk and a tail of 17) and 1041 (3 x 347: two chunks and a tail of
17), at batch 1 and 2.  The (channels, groups) pairs: (8, 4) and (24, 4), (32, 4) -- the stems --, (174, 29) and (348, 29) -- k16, 2 mod 4
and 0 mod 4 --, (256, 32), and (2048, 32) on the three small pixel counts (eight workgroups of channel pairs).  ``x`` is dense, or
the upper channel half of a tensor of 2C channels (for C = 174 on an 8-byte and no 16-byte boundary); the output goes into a
sentinel-guarded buffer, or in place.

Criteria.  KNOWN ANSWERS: per (image, group) half of the elements are ``m + d`` and half ``m - d`` (``m`` an integer), with
``d^2 + eps`` a power of four, ``gamma`` multiples of 0.25 and ``beta`` of 0.125: every sum in any order, the mean ``m``, the variance
``d^2``, ``rstd``, ``a``, ``s`` and ``y`` are exactly representable, so the result is the analytic ``(x - m) rstd gamma + beta``,
``torch.equal``.  ACTIVATIONS: the activation is the kernel's last float32 operation, so the output is torch's float32 activation of
the ``act = 0`` output of the same call, value for value.  RANDOM DATA: ``err <= 2 * e0`` as a maximum and as an rms (``tc.report``,
the project's standing k = 2), ``e0`` the error of torch's own float32 ``group_norm`` against the float64 one (median of nine), never
of the code under test; the ``GN`` lines of a run (``pytest -s``) are kept in ``profiles/shufflenetv2k_norms/route_errors.log``.
ROUTES: the same ``2 * e0`` against the double model for both head outputs, ``e0`` of the plain torch model."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import _lib, fused, headmeta, network

import trunk_common as tc

pytestmark = pytest.mark.gpu

CL = torch.channels_last
P = 512
SENTINEL = 12345.5
GUARD = 256
HW = [(1, 1), (1, 2), (3, 5), (16, 32), (23, 23), (3, 347)]
SMALL = HW[:3]
PAIRS = [(8, 4), (24, 4), (32, 4), (174, 29), (348, 29), (256, 32), (2048, 32)]
EXACT = [(1.0, 3.0), (1.5, 1.75), (2.0, 12.0)]                 # (d, eps): d^2 + eps = 4, 4, 16
ACTS = [(1, 0.0), (2, 0.0), (3, 0.01), (3, 0.25), (4, 6.0), (4, 1.5)]
OPA_ERR_WORKSPACE = 4
_LAUNCHERS = {'stem_conv3x3_bias_act': 'stem', 'conv1x1_unit_x3': 'unit', 'dwconv_bias_act': 'dwconv', 'channel_interleave': 'interleave',
              'group_norm_act': 'gn', 'bias_act_': 'bias_act', 'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3',
              'head_conv_x3': 'head_x3', 'head_epilogue': 'head_epilogue'}

_report = functools.partial(tc.report, 'GN')


def test_the_shapes_are_the_chunks_edges():
    assert fused.GN_CHUNK_PIXELS == P
    assert [h * w for h, w in HW] == [1, 2, 15, P, P + 17, 2 * P + 17]


def _hw_of(pair):
    return SMALL if pair[0] == 2048 else HW


def _operand(x, kind):
    """``x`` ``[B, C, H, W]`` on the host -> (the tensor the kernel reads, the tensor that owns its memory): dense channels-last, or
    the upper channel half of a channels-last tensor of 2C channels whose lower half holds 99."""
    if kind == 'dense':
        t = x.cuda().contiguous(memory_format=CL)
        return t, t
    B, C, H, W = x.shape
    big = torch.full((B, 2 * C, H, W), 99.0, device='cuda').contiguous(memory_format=CL)
    view = big[:, C:]
    view.copy_(x)
    assert view.data_ptr() == big.data_ptr() + 4 * C and view.stride(1) == 1
    return view, big


def _raw(x, gamma, beta, groups, eps, act=0, param=0.0, in_place=False, workspace_short=0):
    """``opa_groupnorm_actp``, raw.  Out of place: into an output inside a larger sentinel-filled buffer -- no sentinel left inside,
    every sentinel in front and behind intact --, returned as ``[B, C, H, W]`` (a channels-last view); in place: ``x`` itself.
    ``workspace_short``: that many bytes less than the workspace needs are declared -> the status."""
    B, C, H, W = x.shape
    n = B * H * W * C
    xs = C if x.storage_offset() == 0 else 2 * C                 # (``_operand``: dense, or the upper half of 2C channels)
    assert fused._pixel_stride(x) in (xs, None if B * H * W > 1 else C)
    lib, vp = _lib.lib(), ctypes.c_void_p
    nbytes = lib.opa_groupnorm_workspace_bytes(B, H * W, C)
    assert nbytes == B * ((H * W + P - 1) // P) * C * 16 + B * C * 8
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device='cuda')
    if in_place:
        buf, out, os_ = None, x, xs
    else:
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device='cuda')
        out, os_ = buf[GUARD:GUARD + n], C
    status = lib.opa_groupnorm_actp(vp(x.data_ptr()), xs, None if gamma is None else vp(gamma.data_ptr()),
                                    None if beta is None else vp(beta.data_ptr()), vp(out.data_ptr()), os_, B, H * W, C, groups, float(eps),
                                    act, float(param), vp(ws.data_ptr()), nbytes - workspace_short, None)
    torch.cuda.synchronize()
    if workspace_short:
        assert bool((buf == SENTINEL).all()) and bool((ws == 0).all()), 'a refused call launched something'
        return status
    assert status == 0, lib.opa_last_error().decode()
    if in_place:
        return x
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), 'the kernel wrote outside its output'
    assert not bool((out == SENTINEL).any()), 'an output element was not written'
    return out.view(B, H, W, C).permute(0, 3, 1, 2)


# ---- 1. known answers, bit for bit ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _known(batch, pair, hw, which):
    """-> (x, gamma, beta on the host, eps, the analytic answer with and without the affine terms, rounded to float32 (exact))"""
    C, G = pair
    cg, (H, W) = C // G, hw
    d, eps = EXACT[which]
    g = tc.gen(100000 * which + 1000 * batch + C + 7 * H * W)
    n = cg * H * W
    assert n % 2 == 0
    m = torch.randint(-8, 9, (batch, G, 1), generator=g).double()
    signs = torch.cat((torch.ones(n // 2), -torch.ones(n // 2))).double()
    signs = torch.stack([signs[torch.randperm(n, generator=g)] for _ in range(batch * G)]).reshape(batch, G, n)
    x64 = (m + d * signs).reshape(batch, G, cg, H, W).reshape(batch, C, H, W)
    gamma = torch.randint(-8, 9, (C,), generator=g).double() * 0.25
    beta = torch.randint(-32, 33, (C,), generator=g).double() * 0.125
    rstd = 1.0 / (d * d + eps) ** 0.5
    assert rstd in (0.5, 0.25)
    plain64 = (x64 - m.reshape(batch, G, 1, 1, 1).expand(batch, G, cg, H, W).reshape(batch, C, H, W)) * rstd
    want64 = plain64 * gamma.reshape(1, C, 1, 1) + beta.reshape(1, C, 1, 1)
    x, want, plain = x64.float(), want64.float(), plain64.float()
    assert torch.equal(x.double(), x64) and torch.equal(want.double(), want64) and torch.equal(plain.double(), plain64)
    return x, gamma.float(), beta.float(), eps, want, plain


@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: 'C%d-G%d' % p)
def test_known_answers(pair):
    """Every pixel count at batch 1 and 2, dense and sliced, out of place and in place: the analytic answer, bit for bit; out of place
    the input -- and the other half of a sliced operand's tensor, always -- unchanged."""
    case = 0
    for hw in _hw_of(pair):
        for batch in (1, 2):
            which = case % len(EXACT)
            case += 1
            x, gamma, beta, eps, want, plain = _known(batch, pair, hw, which)
            gd, bd = gamma.cuda(), beta.cuda()
            for kind in ('dense', 'slice'):
                view, owner = _operand(x, kind)
                if kind == 'slice' and pair[0] == 174:
                    assert view.data_ptr() % 16 == 8, 'the slice of 174 channels begins on an 8-byte and no 16-byte boundary'
                before = owner.clone()
                got = _raw(view, gd, bd, pair[1], eps)
                assert torch.equal(owner, before), 'the kernel wrote into its input'
                assert got.shape == want.shape and torch.equal(got.cpu(), want), (hw, batch, kind, float((got.cpu() - want).abs().max()))
                got = _raw(view, gd, bd, pair[1], eps, in_place=True)
                assert got is view and torch.equal(view.cpu(), want), (hw, batch, kind, 'in place')
                if kind == 'slice':
                    assert bool((owner[:, :pair[0]] == 99.0).all()), 'the kernel wrote into the frame of its operand'
            # without affine terms; with one of the two
            dense = _operand(x, 'dense')[0]
            assert torch.equal(_raw(dense, None, None, pair[1], eps).cpu(), plain), (hw, batch)
            assert torch.equal(_raw(dense, gd, None, pair[1], eps).cpu(), want - beta.reshape(1, -1, 1, 1))
            assert torch.equal(_raw(dense, None, bd, pair[1], eps).cpu(), plain + beta.reshape(1, -1, 1, 1))


# ---- 2. activations ---------------------------------------------------------------------------------------------------------------------

def _torch_act(y, act, param):
    """torch's float32 activation of ``y`` on the host (hardswish as ``y * clamp(y + 3, 0, 6) / 6``)."""
    y = y.cpu()
    if act == 1:
        return torch.relu(y)
    if act == 2:
        return y * torch.clamp(y + 3.0, 0.0, 6.0) / 6.0
    if act == 3:
        return F.leaky_relu(y, param)
    return torch.clamp(y, 0.0, param)


def _random(batch, pair, hw, seed, offset=0.0):
    g = tc.gen(seed)
    x = torch.randn((batch, pair[0]) + hw, generator=g) * 3.0 + offset
    gamma = torch.rand(pair[0], generator=g) + 0.5
    beta = torch.randn(pair[0], generator=g) * 0.5
    return x, gamma, beta


@pytest.mark.parametrize('act,param', ACTS)
def test_activations(act, param):
    """gamma of size 4, so that the outputs (a few units wide) pass -3, 0, 1.5, 3 and 6."""
    for pair, hw in (((24, 4), (23, 23)), ((174, 29), (3, 5)), ((256, 32), (16, 32))):
        x, gamma, beta = _random(2, pair, hw, 7)
        gamma = gamma * 4.0
        for kind in ('dense', 'slice'):
            view, _ = _operand(x, kind)
            y = _raw(view, gamma.cuda(), beta.cuda(), pair[1], 1e-5)
            got = _raw(view, gamma.cuda(), beta.cuda(), pair[1], 1e-5, act, param)
            yc = y.cpu()
            assert yc.isfinite().all() and bool((yc < -3).any()) and bool(((yc > -3) & (yc < 0)).any()) and bool((yc > 6).any()) and bool(((yc > 0) & (yc < 1.5)).any())
            assert torch.equal(got.cpu(), _torch_act(y, act, param)) and not torch.equal(got, y)
            got = _raw(view, gamma.cuda(), beta.cuda(), pair[1], 1e-5, act, param, in_place=True)
            assert torch.equal(got.cpu(), _torch_act(y, act, param))


# ---- 3. random data against float64 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('offset', [0.0, 30.0, 1000.0])
def test_random_data_against_float64(offset):
    ok = True
    for pair, hw in (((24, 4), (3, 347)), ((32, 4), (23, 23)), ((174, 29), (23, 23)), ((348, 29), (16, 32)), ((256, 32), (3, 347)),
                     ((2048, 32), (3, 5)), ((8, 4), (1, 2))):
        for seed in (0, 1, 2):
            x, gamma, beta = _random(2, pair, hw, 10 * seed + 1, offset)
            x, gamma, beta = x.cuda().contiguous(memory_format=CL), gamma.cuda(), beta.cuda()
            ref64 = F.group_norm(x.double(), pair[1], gamma.double(), beta.double(), 1e-5)
            e0 = tc.e0(lambda: F.group_norm(x, pair[1], gamma, beta, 1e-5), ref64)
            got = _raw(x, gamma, beta, pair[1], 1e-5)
            assert e0[0] > 0 and ref64.isfinite().all()
            ok &= _report('kernel C %d G %d %s offset %g seed %d' % (pair + ('x'.join(map(str, hw)), offset, seed)), tc.errors(got, ref64), e0)
    assert ok


# ---- 4. repeatability, the workspace ----------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits():
    for pair, hw in (((24, 4), (3, 347)), ((174, 29), (23, 23)), ((2048, 32), (3, 5))):
        x, gamma, beta = _random(2, pair, hw, 3, 30.0)
        view, _ = _operand(x, 'slice')
        a = _raw(view, gamma.cuda(), beta.cuda(), pair[1], 1e-5, 1)
        b = _raw(view, gamma.cuda(), beta.cuda(), pair[1], 1e-5, 1)
        assert torch.equal(a, b)


def test_a_workspace_one_byte_short_is_refused_and_nothing_runs():
    x, gamma, beta = _random(2, (24, 4), (23, 23), 4)
    view, _ = _operand(x, 'dense')
    assert _raw(view, gamma.cuda(), beta.cuda(), 4, 1e-5, workspace_short=1) == OPA_ERR_WORKSPACE
    assert b'workspace is too small' in _lib.lib().opa_last_error()


# ---- 5. the launcher --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pair', [(24, 4), (174, 29), (256, 32)], ids=lambda p: 'C%d-G%d' % p)
def test_launcher_returns_the_raw_calls_bits(pair):
    x, gamma, beta = _random(2, pair, (23, 23), 5)
    norm = nn.GroupNorm(pair[1], pair[0]).cuda().requires_grad_(False)
    with torch.no_grad():
        norm.weight.copy_(gamma); norm.bias.copy_(beta)
    bare = nn.GroupNorm(pair[1], pair[0], affine=False).cuda()
    for kind in ('dense', 'slice'):
        view, _ = _operand(x, kind)
        assert fused.group_norm_supported(norm, view) and fused.group_norm_supported(bare, view)
        for act, param in [(0, 0.0), (1, 0.0), (3, 0.01)]:
            want = _raw(view, norm.weight, norm.bias, pair[1], norm.eps, act, param)
            got = fused.group_norm_act(norm, view, act=act, act_param=param)
            assert got.is_contiguous(memory_format=CL) and got.dtype == torch.float32 and torch.equal(got, want)
            clone = view.clone(memory_format=torch.preserve_format) if kind == 'dense' else _operand(x, 'slice')[0]
            assert fused.group_norm_act(norm, clone, act=act, act_param=param, out=clone) is clone and torch.equal(clone, want)
        assert torch.equal(fused.group_norm_act(bare, view), _raw(view, None, None, pair[1], bare.eps))
    # the workspace is kept per device and stream, and grows
    key = (str(view.device), torch.cuda.current_stream().cuda_stream)
    kept = fused._GN_WORKSPACE[key]
    fused.group_norm_act(norm, view)
    assert fused._GN_WORKSPACE[key] is kept
    big = torch.zeros((2, pair[0], 64, 64), device='cuda').contiguous(memory_format=CL)
    fused.group_norm_act(norm, big)
    assert fused._GN_WORKSPACE[key].numel() > kept.numel()


# ---- 6. the routes ------------------------------------------------------------------------------------------------------------------------

TINY = ([1, 1, 1], [24, 232, 64, 256, 24])


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder; nothing may be timed; ``GN`` and ``STEM`` on, every ``pick`` forced to the project's kernel; the switches and the
    choice table restored after."""
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_UNIT', 'STEM', 'GN'), force_pick='x3')


def _watch(rec, module):
    """``rec.watch`` (``miopen:<name>`` per torch convolution) and ``torchnorm:<name>`` per norm module that runs."""
    for name, m in module.named_modules():
        if isinstance(m, (nn.GroupNorm, nn.InstanceNorm2d, nn.BatchNorm2d)):
            m.register_forward_hook(lambda mod, args, out, name=name: rec.trace.append('torchnorm:' + name))
    return rec.watch(module)


def _net(kind, seed, **options):
    if kind == 'tiny':
        base = network.ShuffleNetV2K('tiny', config=TINY, **options)
    else:
        base = network.ShuffleNetV2K(kind, **options)
    net = network.Shell(base, [network.CompositeField4(m, base.out_features) for m in headmeta.cocokp_metas()]).eval()
    tc.randomize_(net, seed)
    g = tc.gen(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.GroupNorm, nn.InstanceNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
            if isinstance(m, nn.InstanceNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
    return net


def _plain_e0(net, x, ref64):
    plain = copy.deepcopy(net).cuda().to(memory_format=CL)
    saved, fused.FORCE_PICK = fused.FORCE_PICK, 'conv'                 # e0: torch's own convolutions, the heads' too
    try:
        return [tc.e0(lambda: plain(x)[i], r) for i, r in enumerate(ref64)]
    finally:
        fused.FORCE_PICK = saved


def _forward(opt, x, rec):
    rec.trace.clear()
    out = opt(x)
    return out, list(rec.trace)


@pytest.mark.parametrize('name,options,shape', [('tiny', {}, (2, 3, 33, 25)), ('tiny', dict(leaky_relu=True), (1, 3, 49, 33)),
                                                ('shufflenetv2k16', {}, (2, 3, 97, 65))], ids=['tiny', 'tiny-leaky', 'k16'])
def test_route(rec, name, options, shape):
    """cocokp heads on a small input, channels-last.  ``GN`` (and ``STEM``) on: the trace holds no torch convolution and no torch norm
    in the stem, the units and ``conv5`` and one norm launch per ``GroupNorm``; both head outputs within 2 e0 of the double model; the
    forward repeats bit for bit.  ``GN`` off: the same criterion, no norm launch, every norm torch's."""
    net = _net(name, 7, layer_norm='group', **options)
    norms = sum(isinstance(m, nn.GroupNorm) for m in net.modules())
    x = torch.randn(shape, generator=tc.gen(8)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(net).double().cuda()(x.double())
        e0s = _plain_e0(net, x, ref64)
        opt = _watch(rec, network.optimize_for_inference_(copy.deepcopy(net)).cuda().to(memory_format=CL))
        assert sum(isinstance(m, nn.GroupNorm) for m in opt.modules()) == norms
        x0 = x.clone()
        got, trace = _forward(opt, x, rec)
        again, trace2 = _forward(opt, x, rec)
        assert torch.equal(x, x0), 'the forward wrote into its input'
        assert trace2 == trace and trace[:2] == ['stem', 'gn'], trace
        assert not [t for t in trace if t.startswith(('miopen:base_net', 'torchnorm:'))], trace
        assert trace.count('gn') == norms, (trace.count('gn'), norms)
        ok = True
        for i, (g, a, r) in enumerate(zip(got, again, ref64)):
            assert g.isfinite().all() and g.shape == r.shape
            assert torch.equal(g, a), 'head %d is not repeatable bit for bit' % i
            ok &= _report('%s%s GN on head %d | %d launches' % (name, '-leaky' if options else '', i, len(trace)), tc.errors(g, r), e0s[i])
        assert fused.choices() == {}, 'the route made a choice-table entry'
        fused.GN = False
        off, trace_off = _forward(opt, x, rec)
        fused.GN = True
        assert 'gn' not in trace_off and len([t for t in trace_off if t.startswith('torchnorm:')]) == norms, trace_off
        for i, (o, r) in enumerate(zip(off, ref64)):
            ok &= _report('%s%s GN off head %d | %d launches' % (name, '-leaky' if options else '', i, len(trace_off)), tc.errors(o, r), e0s[i])
    assert ok


def test_instance_norm_network_takes_the_batch_norm_networks_routes(rec):
    """Optimized, the instance-norm network IS a folded batch-norm network: the same trace, launch for launch."""
    x = torch.randn((2, 3, 33, 25), generator=tc.gen(8)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        inst = _net('tiny', 7, layer_norm='instance')
        ref64 = copy.deepcopy(inst).double().cuda()(x.double())
        e0s = _plain_e0(inst, x, ref64)
        opt = _watch(rec, network.optimize_for_inference_(copy.deepcopy(inst)).cuda().to(memory_format=CL))
        got, trace = _forward(opt, x, rec)
        batch = _watch(rec, network.optimize_for_inference_(_net('tiny', 7)).cuda().to(memory_format=CL))
        _, trace_bn = _forward(batch, x, rec)
        assert trace == trace_bn and trace[0] == 'stem' and 'gn' not in trace and not [t for t in trace if t.startswith('torchnorm:')], (trace, trace_bn)
        ok = True
        for i, (g, r) in enumerate(zip(got, ref64)):
            ok &= _report('tiny instance head %d | %d launches' % (i, len(trace)), tc.errors(g, r), e0s[i])
    assert ok
