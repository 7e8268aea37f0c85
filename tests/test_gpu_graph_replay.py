"""Whole networks captured into ONE HIP graph and replayed, on every trunk route (real kernels, MI355X).  What can go wrong under
capture is not in the kernels but in the host state around them: a launch that leaves the capture stream, a value read on the host at
capture time, an operand derived inside the capture and kept (``fused.derived``), a kept tensor whose address the graph baked and an
eager call then frees (``fused._gn_workspace``, a derived operand replaced after ``load_state_dict``).

One harness (``_Harness``): a recorder on ``fused._launch`` (symbol and arguments, the launch still runs) and forward hooks on every
``nn.Conv2d`` in ONE trace (``trunk_common.recorder`` / ``Recorder.watch``), ``OPA_CONV1X1=gemm``, ``FORCE_PICK = 'x3'``, an empty choice
table, timing raises; every switch that ships off is off unless the case names it, the split-operand switches (``X3_*``,
``winograd.X3``) are on.  Everything runs on a side stream that has waited for the current one, and every capture is one linear
capture on that stream (torch's default ``capture_error_mode='global'``: a host synchronisation or a raw allocation inside raises).

The cases -- network, dtype, switches (``CASES``); input 2 x 3 x 97 x 65, the tiny ShuffleNetV2K 2 x 3 x 33 x 41, channels-last:

====================  ========  ===========================================================  =========================
case                  dtype     switches                                                     an ``nn.Conv2d`` still runs
====================  ========  ===========================================================  =========================
resnet50-f32          float32   (defaults)                                                   no
resnet18-f32          float32   (defaults)                                                   yes
resnext50-f32         float32   GCONV                                                        no
resnet50-bf16         bfloat16  CONV3_BF16 PAIR_BF16 STEM7_BF16 HEAD16                       no
resnext50-bf16        bfloat16  CONV3_BF16 PAIR_BF16 STEM7_BF16 HEAD16 GCONV_BF16            no
resnet18-f16          float16   F16 GCONV_F16 STEM7_F16 HEAD16                               no
resnext50-f16         float16   F16 GCONV_F16 STEM7_F16 HEAD16                               no
shufflenetv2k16-f32   float32   X3_UNIT STEM                                                 no
shufflenetv2k16-bf16  bfloat16  UNIT_BF16 HEAD16                                             yes
shufflenetv2k16-f16   float16   UNIT_F16 HEAD16                                              yes
tiny-group            float32   GN STEM   (``ShuffleNetV2K(config=TINY, layer_norm='group')``)  no
tiny-instance         float32   GN STEM   (``layer_norm='instance'``)                          no
mobilenetv2           float32   MBV2 STEM                                                    no
mobilenetv3small      float32   MBV3 STEM                                                    no
squeezenet            float32   FIRE STEM                                                    no
====================  ========  ===========================================================  =========================

(``EXACT`` is the "no" rows; the hooks of every run are held against it, and the log names the convolutions that remain.)

EQUALS.  Where the hooks show that no ``nn.Conv2d`` ran, every kernel is this project's and repeats: equality is ``torch.equal`` on
the bits of every head field.  Where a torch convolution remains MIOpen may choose another algorithm under capture; there the rms
error of all head fields against the float64 forward of the same (cast) weights is compared: the replay's error is at most the eager
forward's error times the seed-to-seed spread (max / min over ``SEEDS``) of the eager error -- the project's margin rule
(``test_gpu_f16x_routes.py``), printed as ``GRAPHREPLAY`` lines; one run is kept as ``profiles/graph_replay/route_errors.log``.

THE CHECKS.  (a) warm-up on the capture stream, capture on a static input, replay: the capture's trace (symbols and convolutions,
in order) is the eager forward's, the replay equals the eager output.  (b) refill ``x.copy_(x2)``, replay: equals an eager forward
on ``x2`` made afterwards; once more: the same bits (EQUALS holds here too: on resnet18-f32 two replays of ONE graph differ in their
bits, as a replay and the eager forward do -- MIOpen's float32 kernels there do not repeat); ``x`` is still ``x2``.  (c) the FIRST forward of a fresh copy inside a capture,
then an eager forward BEFORE any replay: it equals the eager forward of a copy whose operands were derived eagerly (never a second
run of the capture path), no operand was kept by the capture, and the replay equals it -- one case per ``derived`` family
(``FAMILIES``).  (d) after (a), ``load_state_dict`` of another seed's weights / ``mul_(1.25)`` on every parameter, an eager forward,
a replay: the replay follows the parameters as a torch module's would (``FAMILIES`` and the GroupNorm network).  (e) the GroupNorm
workspace: no launch of the capture was handed the kept workspace, the table is untouched, and after an eager call outgrew and freed
it the replay leaves that memory alone.  (f) one whole step as the benchmark captures it: resnet18 + ``native.CifCaf.call_batch``,
fields refilled in place; the decode equals the eager decode bit for bit and the oracle's (``oracle.port.decode``) as
``test_gpu_host_api.py`` compares with it."""
import copy
import functools
import gc

import numpy as np
import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, headmeta, native, network, synth, winograd

import trunk_common as tc

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SEEDS = (0, 1, 2, 3)
TINY = ([1, 1, 1], [24, 232, 64, 256, 24])
SHIP_OFF = ('GCONV', 'MBV3', 'FIRE', 'MBV2', 'UNIT_LEAKY', 'STEM', 'GN', 'UNIT_BF16', 'CONV3_BF16', 'STEM7_BF16', 'PAIR_BF16', 'GCONV_BF16',
            'F16', 'HEAD16', 'UNIT_F16', 'GCONV_F16', 'STEM7_F16')
SHIP_ON = ('X3_PAIR', 'X3_CONV3', 'X3_HEAD', 'X3_STEM', 'X3_UNIT')
_BF16_RESNET = ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16', 'HEAD16')
_F16_RESNET = ('F16', 'GCONV_F16', 'STEM7_F16', 'HEAD16')
# case -> (network, dtype, switches, input height and width)
CASES = {
    'resnet50-f32': ('resnet50', F32, (), (97, 65)),
    'resnet18-f32': ('resnet18', F32, (), (97, 65)),
    'resnext50-f32': ('resnext50', F32, ('GCONV',), (97, 65)),
    'resnet50-bf16': ('resnet50', BF16, _BF16_RESNET, (97, 65)),
    'resnext50-bf16': ('resnext50', BF16, _BF16_RESNET + ('GCONV_BF16',), (97, 65)),
    'resnet18-f16': ('resnet18', F16, _F16_RESNET, (97, 65)),
    'resnext50-f16': ('resnext50', F16, _F16_RESNET, (97, 65)),
    'shufflenetv2k16-f32': ('shufflenetv2k16', F32, ('X3_UNIT', 'STEM'), (97, 65)),
    'shufflenetv2k16-bf16': ('shufflenetv2k16', BF16, ('UNIT_BF16', 'HEAD16'), (97, 65)),
    'shufflenetv2k16-f16': ('shufflenetv2k16', F16, ('UNIT_F16', 'HEAD16'), (97, 65)),
    'tiny-group': ('tiny:group', F32, ('GN', 'STEM'), (33, 41)),
    'tiny-instance': ('tiny:instance', F32, ('GN', 'STEM'), (33, 41)),
    'mobilenetv2': ('mobilenetv2', F32, ('MBV2', 'STEM'), (97, 65)),
    'mobilenetv3small': ('mobilenetv3small', F32, ('MBV3', 'STEM'), (97, 65)),
    'squeezenet': ('squeezenet', F32, ('FIRE', 'STEM'), (97, 65)),
}
# the cases in whose forward no ``nn.Conv2d`` runs: bit equality
EXACT = frozenset(CASES) - {'resnet18-f32', 'shufflenetv2k16-bf16', 'shufflenetv2k16-f16'}
# one case per family of ``fused.derived`` operands: split weights, 16-bit repacked weights (two), unit mode, Fire, head16
FAMILIES = ('resnet50-f32', 'resnet50-bf16', 'resnext50-f16', 'shufflenetv2k16-f32', 'squeezenet', 'resnet18-f16')
GN_WORKSPACE_ARG = 13                    # opa_groupnorm_actp: ..., act_param, workspace, its bytes
SENTINEL = 12345.5


# ---- networks and inputs: built once, left unchanged ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net(case, seed):
    """The unoptimized network of ``case`` on the GPU, float32, its norms' statistics and affine terms drawn at random."""
    name = CASES[case][0]
    if name.startswith('tiny:'):
        base = network.ShuffleNetV2K('tiny', config=TINY, layer_norm=name[5:])
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
        return net.cuda()
    net = network.factory(name, seed=seed).cuda()
    state = torch.random.get_rng_state()
    torch.manual_seed(100 + seed)
    try:
        for m in net.modules():                                        # (as test_gpu_f16x_routes.py)
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    finally:
        torch.random.set_rng_state(state)
    return net


def _fresh(case, seed=0):
    """A new optimized copy cast to the case's dtype, channels-last: no derived operand yet."""
    opt = network.optimize_for_inference_(copy.deepcopy(_net(case, seed)))
    return opt.to(CASES[case][1]).to(memory_format=CL).requires_grad_(False)


@functools.lru_cache(maxsize=None)
def _input(case, seed):
    h, w = CASES[case][3]
    x = torch.randn((2, 3, h, w), generator=tc.gen(1000 + seed)).cuda()
    return x.to(CASES[case][1]).contiguous(memory_format=CL)


def _bits(fields):
    return [f.contiguous().view(torch.int32 if f.dtype == torch.float32 else torch.int16) for f in fields]


def _same_bits(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(_bits(a), _bits(b)))


def _rms_error(got, ref):
    num = sum(float(((g.double() - r) ** 2).sum()) for g, r in zip(got, ref))
    den = sum(float((r ** 2).sum()) for r in ref)
    return (num / den) ** 0.5


def _derived_attrs(module):
    return sorted('%s.%s' % (n, a) for n, m in module.named_modules() for a in vars(m) if a.startswith('_opa'))


# ---- the harness ------------------------------------------------------------------------------------------------------------------

class _Harness:
    """``rec.trace``: launched symbols and ``miopen:<name>`` of every ``nn.Conv2d`` called, in order; ``launches``: (symbol, arguments);
    ``stream``: the capture stream, current while the test runs."""

    def __init__(self, monkeypatch):
        self.monkeypatch = monkeypatch
        self.rec = tc.recorder(monkeypatch, {}, force_pick='x3')
        self.launches = []
        launch = fused._launch

        def recording(symbol, *args):
            self.rec.trace.append(symbol)
            self.launches.append((symbol, args))
            return launch(symbol, *args)
        monkeypatch.setattr(fused, '_launch', recording)
        monkeypatch.setenv('OPA_CONV1X1', 'gemm')
        monkeypatch.setattr(winograd, 'X3', True)
        monkeypatch.setattr(winograd, '_mode', 'auto')
        monkeypatch.setattr(fused, '_GN_WORKSPACE', {})
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())
        self._spread = {}

    def switches(self, case):
        for name in SHIP_OFF + SHIP_ON:
            self.monkeypatch.setattr(fused, name, name in SHIP_ON or name in CASES[case][2])

    def fresh(self, case, seed=0):
        return self.rec.watch(_fresh(case, seed))

    def clear(self):
        del self.rec.trace[:], self.launches[:]

    def eager(self, opt, x):
        """-> (the head fields, cloned; the trace)"""
        self.clear()
        with torch.no_grad():
            out = tuple(f.clone() for f in opt(x))
        return out, list(self.rec.trace)

    def capture(self, opt, x):
        """One linear capture of ``opt(x)`` on the side stream -> (graph, the static head fields, the trace of the capture)"""
        self.clear()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            with torch.no_grad():
                out = opt(x)
        assert self.rec.timed == 0
        return graph, out, list(self.rec.trace)

    def replay(self, graph, out):
        graph.replay()
        self.stream.synchronize()
        return tuple(f.clone() for f in out)

    def reference(self, opt, x):
        """The head fields of the same (cast) weights upcast to float64 on ``x`` upcast."""
        table = fused.choices()
        try:
            with torch.no_grad():
                ref = tuple(f.double() for f in copy.deepcopy(opt).double()(x.double()))
        finally:
            fused.set_choices(table, replace=True)
        assert all(f.isfinite().all() for f in ref)
        return ref

    def spread(self, case):
        """max / min over ``SEEDS`` of the eager forward's rms error against the float64 forward."""
        if case not in self._spread:
            errs = []
            for seed in SEEDS:
                opt, x = _fresh(case, seed), _input(case, seed)
                with torch.no_grad():
                    errs.append(_rms_error(opt(x), self.reference(opt, x)))
            assert min(errs) > 0, errs
            print('GRAPHREPLAY %s | eager rms error over seeds %s: %s | spread %.3f'
                  % (case, SEEDS, ' '.join('%.4e' % e for e in errs), max(errs) / min(errs)))
            self._spread[case] = max(errs) / min(errs)
        return self._spread[case]

    def equals(self, case, what, got, want, trace, opt, x):
        """``got`` (a replay, or the forward under test) equals ``want`` (the eager forward): the bits where no ``nn.Conv2d`` is on the
        route, else the margin rule against the float64 forward of ``opt`` on ``x``."""
        assert len(got) == len(want) and all(g.shape == w.shape for g, w in zip(got, want))
        if not [t for t in trace if t.startswith('miopen:')]:
            assert _same_bits(got, want), '%s %s: the bits differ' % (case, what)
            return
        ref = self.reference(opt, x)
        e_got, e_want, spread = _rms_error(got, ref), _rms_error(want, ref), self.spread(case)
        print('GRAPHREPLAY %s | %s | e_eager %.4e | e_got %.4e | e_got / e_eager %.3f | spread %.3f | bits %s'
              % (case, what, e_want, e_got, e_got / e_want, spread, 'equal' if _same_bits(got, want) else 'differ'))
        assert e_got <= spread * e_want, (case, what, e_got, e_want, spread)


@pytest.fixture
def h(monkeypatch):
    harness = _Harness(monkeypatch)
    with torch.cuda.stream(harness.stream):
        yield harness
        harness.stream.synchronize()
    gc.collect()


def _finite(fields):
    return all(f.isfinite().all() for f in fields)


# ---- (a) warm-up, capture, replay; (b) refill ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', list(CASES))
def test_replay_equals_eager_and_follows_the_refilled_input(h, case):
    h.switches(case)
    opt = h.fresh(case)
    x, x1, x2 = _input(case, 0).clone(memory_format=torch.preserve_format), _input(case, 0), _input(case, 1)
    eager, trace = h.eager(opt, x)                                     # the warm-up, on the capture stream
    assert _finite(eager) and [t for t in trace if t.startswith('opa_')]
    graph, out, captured = h.capture(opt, x)
    assert captured == trace, (captured, trace)                        # every launch and every nn.Conv2d, in order
    h.equals(case, 'a: replay on the captured input', h.replay(graph, out), eager, trace, opt, x1)
    x.copy_(x2)                                                        # (b) refill the static input
    got2 = h.replay(graph, out)
    eager2, trace2 = h.eager(opt, x2)                                  # ... an eager forward made afterwards
    assert trace2 == trace and _finite(eager2) and not _same_bits(eager2, eager)
    h.equals(case, 'b: replay on the refilled input', got2, eager2, trace, opt, x2)
    # once more: the same bits -- where a torch convolution remains, what EQUALS says (MIOpen's kernels need not repeat, replayed or not)
    h.equals(case, 'b: a second replay', h.replay(graph, out), got2, trace, opt, x2)
    assert _same_bits([x], [x2]), 'the forward wrote into its input'
    convs = [t[7:] for t in trace if t.startswith('miopen:')]
    if convs:
        print('GRAPHREPLAY %s | %d of %d trace entries are nn.Conv2d calls: %s' % (case, len(convs), len(trace), ' '.join(convs)))
    assert (not convs) == (case in EXACT), convs


# ---- (c) the first call under capture, an eager call before any replay ----------------------------------------------------------------

@pytest.mark.parametrize('case', FAMILIES)
def test_first_call_under_capture_then_eager_before_any_replay(h, case):
    h.switches(case)
    x = _input(case, 0)
    warm = h.fresh(case)
    want, trace = h.eager(warm, x)                                     # operands derived eagerly: the reference forward
    assert _finite(want) and _derived_attrs(warm)
    cold = h.fresh(case)
    assert _derived_attrs(cold) == []
    graph, out, captured = h.capture(cold, x)                          # its FIRST forward
    assert captured == trace, (captured, trace)
    assert _derived_attrs(cold) == [], _derived_attrs(cold)            # nothing made inside the capture is kept
    got, trace_c = h.eager(cold, x)                                    # before any replay: on operands of its own
    assert trace_c == trace and _derived_attrs(cold) == _derived_attrs(warm)
    h.equals(case, 'c: eager after a first call under capture', got, want, trace, warm, x)
    h.equals(case, 'c: the first replay', h.replay(graph, out), got, trace, warm, x)


# ---- (d) parameters changed in place after the capture --------------------------------------------------------------------------------

def _event(opt, other, name):
    with torch.no_grad():
        if name == 'load_state_dict':
            opt.load_state_dict(other.state_dict(), strict=True)       # copy_: the pointers stay, the versions rise
        else:
            for p in opt.parameters():
                p.mul_(1.25)


@pytest.mark.parametrize('event', ['load_state_dict', 'in_place'])
@pytest.mark.parametrize('case', FAMILIES + ('tiny-group',))
def test_replay_follows_parameters_changed_in_place(h, case, event):
    h.switches(case)
    opt, x = h.fresh(case), _input(case, 0)
    before, trace = h.eager(opt, x)
    graph, out, captured = h.capture(opt, x)
    assert captured == trace
    h.equals(case, 'd: replay before the event', h.replay(graph, out), before, trace, opt, x)
    operands = {n: t.data_ptr() for n, t in _operands(opt)}
    _event(opt, _fresh(case, 1), event)
    eager, trace_e = h.eager(opt, x)                                   # brings the kept operands up to date, in place
    assert trace_e == trace and not _same_bits(eager, before)
    assert {n: t.data_ptr() for n, t in _operands(opt)} == operands    # the addresses the graph holds
    h.equals(case, 'd: replay after %s' % event, h.replay(graph, out), eager, trace, opt, x)


def _operands(module):
    """[(name, tensor)] of every derived operand kept on ``module``'s submodules."""
    out = []
    for n, m in module.named_modules():
        for a, v in vars(m).items():
            if a.startswith('_opa'):
                kept = v[1] if isinstance(v[1], (tuple, list)) else (v[1],)
                out += [('%s.%s[%d]' % (n, a, i), t) for i, t in enumerate(kept) if isinstance(t, torch.Tensor)]
    return out


# ---- (e) the GroupNorm workspace --------------------------------------------------------------------------------------------------------

def test_a_capture_neither_takes_nor_replaces_the_kept_groupnorm_workspace(h):
    case = 'tiny-group'
    h.switches(case)
    opt, x = h.fresh(case), _input(case, 0)
    h.eager(opt, x)                                                    # warm-up: an eager workspace large enough for every norm
    key = (str(x.device), h.stream.cuda_stream)
    kept = fused._GN_WORKSPACE[key]
    lo, numel = kept.data_ptr(), kept.numel()
    graph, out, captured = h.capture(opt, x)
    norms = [args for symbol, args in h.launches if symbol == 'opa_groupnorm_actp']
    assert norms and len(norms) == sum(isinstance(m, nn.GroupNorm) for m in opt.modules())
    for args in norms:                                                 # no launch of the capture was handed the kept workspace
        ws, nbytes = args[GN_WORKSPACE_ARG], args[GN_WORKSPACE_ARG + 1]
        assert nbytes > 0 and (ws + nbytes <= lo or ws >= lo + 8 * numel), (ws, nbytes, lo, numel)
    assert fused._GN_WORKSPACE[key] is kept and list(fused._GN_WORKSPACE) == [key]
    # only now: an eager call on that stream outgrows the kept workspace, which is freed ...
    norm = nn.GroupNorm(32, 256).cuda().requires_grad_(False)
    fused.group_norm_act(norm, torch.zeros((2, 256, 64, 64), device='cuda').contiguous(memory_format=CL))
    assert fused._GN_WORKSPACE[key] is not kept and fused._GN_WORKSPACE[key].numel() > numel
    del kept
    # ... and its memory is someone else's
    others = [torch.full((numel,), SENTINEL, dtype=torch.float64, device='cuda') for _ in range(4)]
    got = h.replay(graph, out)
    assert all(bool((t == SENTINEL).all()) for t in others), 'the replay wrote into memory that was not the graph\'s'
    eager, trace = h.eager(opt, x)
    assert trace == captured
    h.equals(case, 'e: replay after the workspace was outgrown', got, eager, trace, opt, x)


# ---- (f) one whole step: the network and the decode in one graph ---------------------------------------------------------------------------

def test_one_whole_step_in_one_graph(h, coco_skeleton0):
    from oracle import port
    case = 'resnet18-f32'
    h.switches(case)
    opt = h.fresh(case)
    x, x2 = _input(case, 0).clone(memory_format=torch.preserve_format), _input(case, 1)
    fields = [synth.synth_fields(seed, 1, height=41, width=41) for seed in (500, 501)]       # one person each
    cif_s, caf_s = (torch.from_numpy(f[None]).cuda() for f in fields[0])
    dec, eager_dec = (native.CifCaf(17, torch.from_numpy(coco_skeleton0)) for _ in range(2))
    with torch.no_grad():                                              # the warm-up, as bench.py's
        opt(x)
    dec.call_batch(cif_s, 8, caf_s, 8)
    h.stream.synchronize()
    h.clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=h.stream):
        with torch.no_grad():
            out = opt(x)
        g_out, g_ids, g_counts = dec.call_batch(cif_s, 8, caf_s, 8)
    trace = list(h.rec.trace)
    for cif, caf in (fields[1], fields[0], fields[1]):
        cif_s.copy_(torch.from_numpy(cif[None]))                       # refilled in place
        caf_s.copy_(torch.from_numpy(caf[None]))
        x.copy_(x2)
        graph.replay()
        h.stream.synchronize()
        w_out, w_ids, w_counts = eager_dec.call_batch(torch.from_numpy(cif[None]).cuda(), 8, torch.from_numpy(caf[None]).cuda(), 8)
        n = int(g_counts[0])
        native.check_counts(g_counts.cpu())
        assert n >= 1 and torch.equal(g_counts, w_counts)
        assert torch.equal(g_out[0, :n], w_out[0, :n]) and torch.equal(g_ids[0, :n], w_ids[0, :n])     # the eager decode, bit for bit
        want, _ = port.decode(cif, 8, caf, 8, coco_skeleton0)                                          # the oracle's, as test_gpu_host_api.py
        assert len(want) == n
        for row, w in zip(g_out[0, :n].cpu().numpy(), want):
            assert np.allclose(row, w, atol=1e-4)
    eager2, trace2 = h.eager(opt, x2)
    assert trace2 == trace
    h.equals(case, 'f: the network of the whole step', tuple(f.clone() for f in out), eager2, trace, opt, x2)
