"""The dispatch logic of ``_Bottleneck.forward`` / ``fused.pick`` / ``fused.conv_bias_act`` on the CPU, the kernels stood in by
their PyTorch restatements: whichever way the tail's decision is made -- forced to the pair product, forced to two launches, or
TIMED on the first call (``fused._time_ms`` calls each candidate seven times) -- the block must compute the float64 block's
output at float32 rounding level.  conv2 leaves its bias + ReLU to the next operand here (``a_bias = fb2``, as on the GPU when
MIOpen runs conv2 raw), and the two-launch side applies them IN PLACE: a timing that lets those calls accumulate hands the winner
``relu(...relu(out + b)... + b)`` (0.94 of the output's largest value before ``pick`` saved and restored the operand)."""
import copy

import pytest
import torch

from openpifpaf_amd import fused

import trunk_common as tc


def _pair_supported(conv, dconv, h, x, bias, a_bias=None):
    return (conv.kernel_size == (1, 1) and dconv.kernel_size == (1, 1) and h.dtype == torch.float32 and x.dtype == torch.float32
            and conv.out_channels == dconv.out_channels and conv.bias is None and dconv.bias is None)


def _pair(conv, dconv, h, x, bias, relu=True, a_bias=None):
    """``fused.conv1x1_pair_bias_act_x3`` in PyTorch: reads ``h``, writes nothing but its result."""
    if a_bias is not None:
        h = torch.relu(h + a_bias.view(1, -1, 1, 1))
    out = conv(h) + dconv(x) + bias.view(1, -1, 1, 1)
    return torch.relu(out) if relu else out


@pytest.fixture
def model(monkeypatch):
    """-> ``arm(times)``: the stand-ins installed, the choice table emptied (and put back afterwards), ``_time_ms`` answering with
    ``times`` in turn after calling its candidate seven times like the real one (1 + 2 x 3)."""
    calls = []

    def arm(times=()):
        answers = iter(times)

        def time_ms(fn, reps=3):
            for _ in range(1 + 2 * reps):
                fn()
            calls.append(fn)
            return next(answers)
        monkeypatch.setattr(fused, '_time_ms', time_ms)
        monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
        monkeypatch.setattr(fused, 'pair_supported', _pair_supported)
        monkeypatch.setattr(fused, 'conv1x1_pair_bias_act_x3', _pair)
        monkeypatch.setattr(fused, 'FORCE_PICK', None)
        monkeypatch.delenv('OPA_CONV1X1', raising=False)
        return calls
    saved = fused.choices()
    fused.set_choices({}, replace=True)
    yield arm
    fused.set_choices(saved, replace=True)


def _block_and_reference(seed):
    block = tc.bottleneck(64, 32, 2, True, seed)
    x = torch.randn((3, 64, 11, 9), generator=torch.Generator().manual_seed(100 + seed)).relu()
    with torch.no_grad():
        ref64 = copy.deepcopy(block).double()(x.double())
        e0 = tc.errors(block(x), ref64)
    return tc.optimized(block), x, ref64, e0


def _check(opt, x, ref64, e0):
    x0 = x.clone()
    with torch.no_grad():
        first = opt(x)
        second = opt(x)
    assert torch.equal(x, x0)                                     # the residual path aliases the input: it is read only
    err = tc.errors(first, ref64)
    print('e0 max %.3g rms %.3g   err max %.3g rms %.3g' % (e0 + err))
    assert err[0] <= 4 * e0[0] and err[1] <= 4 * e0[1], (err, e0)
    assert torch.equal(first, second)                             # the first call computes what every later call computes


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('side', ['x3', 'conv'])
def test_forced_tail_of_a_strided_bottleneck_with_deferred_bias(model, monkeypatch, side, seed):
    calls = model()
    monkeypatch.setattr(fused, 'FORCE_PICK', side)
    opt, x, ref64, e0 = _block_and_reference(seed)
    assert opt.fb2.abs().max() > 0.1
    _check(opt, x, ref64, e0)
    assert not calls and not any(k[0].endswith('/pair') for k in fused.choices())


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('winner', ['x3', 'conv'])
def test_timed_first_call_of_the_tail_computes_what_the_forced_routes_compute(model, winner, seed):
    calls = model((1.0, 2.0) if winner == 'x3' else (2.0, 1.0))
    opt, x, ref64, e0 = _block_and_reference(seed)
    _check(opt, x, ref64, e0)
    assert len(calls) == 2                                        # both sides were timed, once, on the first call
    pair_keys = [k for k in fused.choices() if k[0] == 'torch.float32/pair']
    assert len(pair_keys) == 1 and pair_keys[0][-1] is True       # (the deferred-bias entry) ...
    assert fused.choices()[pair_keys[0]] == winner                # ... and the side the clock named


# ---- the decision itself: ``fused._decide`` on plain values, and what ``pick`` / ``conv_bias_act`` add to it ---------------------

KEY = ('torch.float32/test', 7, 8, 9, False, False)


def _never():
    raise AssertionError('timed')


def test_a_table_entry_times_nothing(model):
    calls = model()
    fused.set_choices({KEY: 'b'})
    assert fused._decide(KEY, 'a', _never) == 'b' and fused._decide(KEY, 'a', _never, may_time=False) == 'b'
    assert not calls and fused.choices() == {KEY: 'b'}


@pytest.mark.parametrize('why', ['may_time', 'capture', 'multi_rank'])
def test_where_nothing_may_be_timed_the_default_is_taken_and_remembered(model, monkeypatch, why):
    calls = model()
    if why == 'capture':
        monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    if why == 'multi_rank':
        monkeypatch.setattr(fused, '_in_multi_rank_job', lambda: True)
    assert fused._decide(KEY, 'a', _never, may_time=why != 'may_time') == 'a'
    assert not calls and fused.choices() == {KEY: 'a'}
    monkeypatch.undo()                                            # eager, one rank, timing allowed: the remembered default stays
    assert fused._decide(KEY, 'b', _never) == 'a'


@pytest.mark.parametrize('times,winner', [((3.0, 1.0, 2.0), 'b'), ((1.0, 2.0, 3.0), 'a'), ((3.0, 2.0, 1.0), 'c'),
                                          ((2.0, 1.0, 1.0), 'b'), ((1.0, 1.0, 1.0), 'a')])
def test_a_timed_decision_times_every_candidate_once_and_takes_the_fastest_or_the_first_of_a_tie(model, times, winner):
    calls = model(times)
    ran = {'a': 0, 'b': 0, 'c': 0}
    thunks = {n: (lambda n=n: ran.__setitem__(n, ran[n] + 1)) for n in ran}
    asked = []

    def timed():
        asked.append(1)
        return {n: fused._time_ms(thunks[n]) for n in ('a', 'b', 'c')}
    assert fused._decide(KEY, 'c', timed) == winner
    assert calls == [thunks['a'], thunks['b'], thunks['c']] and ran == {'a': 7, 'b': 7, 'c': 7}
    assert fused.choices() == {KEY: winner}
    assert fused._decide(KEY, 'c', timed) == winner and len(asked) == 1 and len(calls) == 3          # remembered: not timed again


@pytest.mark.parametrize('side', ['x3', 'conv'])
def test_force_pick_ignores_the_table_and_leaves_it_untouched(model, monkeypatch, side):
    calls = model()
    key = ('torch.float32/test', 7, 8, 9, True, False)
    other = 'conv' if side == 'x3' else 'x3'
    monkeypatch.setattr(fused, 'FORCE_PICK', side)
    for table in ({}, {key: other}):
        fused.set_choices(table, replace=True)
        assert fused.pick('test', 7, 8, 9, True, False, lambda: 'x3', lambda: 'conv') == side
        assert fused.pick('test', 20000, 8, 9, True, False, lambda: 'x3', lambda: 'conv', timing=False) == side
        assert fused.choices() == table and not calls


def test_pick_decides_by_size_where_it_may_not_time_and_a_tie_goes_to_x3(model):
    calls = model((1.0, 1.0))
    assert fused.pick('test', 16384, 8, 9, False, False, lambda: 'x3', lambda: 'conv', timing=False) == 'x3'
    assert fused.pick('test', 16383, 8, 9, False, False, lambda: 'x3', lambda: 'conv', timing=False) == 'conv'
    assert not calls
    assert fused.pick('test', 5, 8, 9, False, False, lambda: 'x3', lambda: 'conv') == 'x3' and len(calls) == 2
    assert fused.choices() == {('torch.float32/test', 16384, 8, 9, False, False): 'x3', ('torch.float32/test', 16383, 8, 9, False, False): 'conv',
                               ('torch.float32/test', 5, 8, 9, False, False): 'x3'}


@pytest.fixture
def gemm_model(model, monkeypatch):
    """``conv_bias_act`` on the CPU: its GEMM launchers stood in by PyTorch restatements that say who ran, its operands declared
    supported.  -> ``arm(times)`` -> (the names that ran, the ``_time_ms`` calls, conv, x, bias, a_bias, the expected output)."""
    def arm(times=()):
        calls, ran = model(times), []

        def gemm(x, w2d, bias, residual=None, relu=True, a_bias=None, name='gemm'):
            ran.append(name)
            if a_bias is not None:
                x = torch.relu(x + a_bias.view(1, -1, 1, 1))
            out = torch.nn.functional.conv2d(x, w2d[:, :, None, None]) + bias.view(1, -1, 1, 1)
            out = out if residual is None else out + residual
            return torch.relu(out) if relu else out

        def gemm3(x, w3, bias, residual=None, relu=True, a_bias=None, terms=9):
            return gemm(x, w3.float().sum(0), bias, residual, relu, a_bias, name='gemm3')
        monkeypatch.setattr(fused, 'conv1x1_supported', lambda *a: True)
        monkeypatch.setattr(fused, 'conv1x1_bias_act', gemm)
        monkeypatch.setattr(fused, 'conv1x1_bias_act_x3', gemm3)
        monkeypatch.setattr(fused, 'X3_TERMS', 6)
        g = torch.Generator().manual_seed(5)
        conv = torch.nn.Conv2d(64, 64, 1, bias=False).requires_grad_(False)
        x, bias, a_bias = torch.randn((2, 64, 3, 5), generator=g), torch.randn(64, generator=g), torch.randn(64, generator=g)
        return ran, calls, conv, x, bias, a_bias
    return arm


GEMM_KEY = ('torch.float32', 30, 64, 64, False, False)


@pytest.mark.parametrize('pinned', ['gemm', 'conv'])
def test_opa_conv1x1_is_read_at_the_call_and_remembered(gemm_model, monkeypatch, pinned):
    ran, calls, conv, x, bias, _ = gemm_model()
    want = torch.relu(conv(x) + bias.view(1, -1, 1, 1))
    monkeypatch.setenv('OPA_CONV1X1', pinned)
    assert torch.allclose(fused.conv_bias_act(conv, x, bias), want, atol=1e-5)
    assert fused.choices() == {GEMM_KEY: pinned} and ran == (['gemm'] if pinned == 'gemm' else []) and not calls
    monkeypatch.setenv('OPA_CONV1X1', 'conv' if pinned == 'gemm' else 'gemm')          # a table entry wins over the variable
    fused.conv_bias_act(conv, x, bias)
    monkeypatch.delenv('OPA_CONV1X1')
    fused.conv_bias_act(conv, x, bias)
    assert fused.choices() == {GEMM_KEY: pinned} and ran == (['gemm'] * 3 if pinned == 'gemm' else []) and not calls


@pytest.mark.parametrize('why', ['capture', 'multi_rank'])
def test_conv_bias_act_takes_the_gemm_where_it_may_not_time(gemm_model, monkeypatch, why):
    ran, calls, conv, x, bias, _ = gemm_model()
    monkeypatch.setattr(*((torch.cuda, 'is_current_stream_capturing') if why == 'capture' else (fused, '_in_multi_rank_job')), lambda: True)
    fused.conv_bias_act(conv, x, bias)
    assert fused.choices() == {GEMM_KEY: 'gemm'} and ran == ['gemm'] and not calls


@pytest.mark.parametrize('deferred,winner', [(False, 'gemm'), (False, 'gemm3'), (False, 'conv'),
                                             (True, 'gemm'), (True, 'gemm3'), (True, 'pass+gemm'), (True, 'conv')])
def test_conv_bias_act_times_its_candidates_in_order_on_a_scratch_copy(gemm_model, deferred, winner):
    names = ['gemm', 'gemm3', 'pass+gemm', 'conv'] if deferred else ['gemm', 'gemm3', 'conv']
    ran, calls, conv, x, bias, a_bias = gemm_model([1.0 if n == winner else 2.0 for n in names])
    h = torch.relu(x + a_bias.view(1, -1, 1, 1)) if deferred else x
    want, x0 = torch.relu(conv(h) + bias.view(1, -1, 1, 1)), x.clone()
    got = fused.conv_bias_act(conv, x, bias, a_bias=a_bias if deferred else None)
    assert torch.allclose(got, want, atol=1e-5)                   # (seven timed calls of an in-place epilogue did not reach the operand)
    assert torch.equal(x, h if deferred and winner in ('pass+gemm', 'conv') else x0)       # (those two apply the epilogue in place, once)
    assert len(calls) == len(names)                               # every candidate timed once ...
    # ... in this order, seven calls each ('pass+gemm' is the epilogue pass and the 'gemm' launcher; 'conv' has no stand-in), then the winner
    timed = ['gemm'] * 7 + ['gemm3'] * 7 + (['gemm'] * 7 if deferred else [])
    assert ran == timed + {'gemm': ['gemm'], 'gemm3': ['gemm3'], 'pass+gemm': ['gemm'], 'conv': []}[winner]
    assert fused.choices() == {GEMM_KEY[:5] + (deferred,): winner}


def test_a_remembered_gemm3_that_is_switched_off_runs_the_gemm_and_keeps_the_entry(gemm_model, monkeypatch):
    ran, calls, conv, x, bias, _ = gemm_model()
    fused.set_choices({GEMM_KEY: 'gemm3'})
    fused.conv_bias_act(conv, x, bias)
    monkeypatch.setattr(fused, 'X3_TERMS', 0)
    fused.conv_bias_act(conv, x, bias)
    assert ran == ['gemm3', 'gemm'] and fused.choices() == {GEMM_KEY: 'gemm3'} and not calls
