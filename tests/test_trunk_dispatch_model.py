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
