"""The 128-channel workgroups of the split-operand Winograd kernel (csrc/winograd.hip, ``winograd_f23_w8x3w_kernel``: variant 5,
32 tiles x 128 output channels) against the 64-channel ones (variant 4 held narrow with ``OPA_WINO_X3_BN=64``).  Every output
element sums the same products in the same order in both, so the two results are equal BIT FOR BIT (NaNs compared as bit
patterns) -- and, beside that, within the bound of ``test_gpu_winograd_x3.py`` of a float64 convolution.  Shapes: the smallest
that reach each path of the kernel (named in ``SHAPES``).

The reference here is the other kernel, which shares the filter operand and the transforms' text with this one.  The checks that
are independent of it live elsewhere: tests/test_gpu_winograd_regimes.py runs variant 5 at ``winograd_common.WIDE_REGIMES`` (every
regime of its own launch; the dense integer case bit for bit against the float64 convolution, guard bands, invariances, the
componentwise error bound), and tests/test_gpu_x3_edges.py at ``x3_common.WINO_WIDE`` (power-of-two taps and scalings, the wide
dynamic range, non-finite pixels, filters and biases against torch's float32 convolution).  This file keeps what only it can
say: that the two kernels agree in every bit, and that the launcher's rule and its override choose between equal kernels."""
import pytest
import torch

from test_gpu_winograd_x3 import _errors, _inputs

pytestmark = pytest.mark.gpu

# test_gpu_winograd_x3.py's bound on the largest error over the output's largest magnitude (a literal in its assertions, so
# there is no name to import; its helpers are imported above)
MAX_ERROR = 2e-5

SHAPES = [(1, 16, 128, 8, 8),        # one chunk, 16 tiles: under one tile block
          (1, 32, 128, 8, 16),       # exactly 32 tiles; two chunks: both shifts' prefetch paths
          (1, 48, 256, 5, 3),        # odd extents, clipped right and bottom tiles; two channel blocks; three chunks
          (2, 64, 128, 7, 9),        # 40 tiles: a partial second block, an image boundary inside a tile block
          (3, 64, 256, 21, 21),      # 363 tiles: many blocks, both workgroup orders
          (2, 128, 384, 6, 6)]       # an odd number of 128-channel blocks


def _bits(y):
    return y.contiguous(memory_format=torch.channels_last).view(torch.int32)


def _pair(monkeypatch, x, w, b, relu, order, out=None):
    """-> (variant 5, variant 4 held to the 64-channel kernel) on the same operands"""
    from openpifpaf_amd import winograd
    u3 = winograd.split_filter(w)
    O = w.shape[0]
    monkeypatch.delenv('OPA_WINO_X3_BN', raising=False)
    wide = winograd.conv3x3_x3(x, u3, O, bias=b, relu=relu, variant=5, order=order, out=out)
    monkeypatch.setenv('OPA_WINO_X3_BN', '64')
    narrow = winograd.conv3x3_x3(x, u3, O, bias=b, relu=relu, variant=4, order=order)
    monkeypatch.delenv('OPA_WINO_X3_BN')
    return wide, narrow


@pytest.mark.parametrize('bias,relu', [(False, False), (True, True)])
@pytest.mark.parametrize('shape', SHAPES)
def test_wide_equals_narrow_bit_for_bit(monkeypatch, shape, bias, relu):
    x, w, b = _inputs(*shape, bias, seed=7)
    for order in (0, 1):
        wide, narrow = _pair(monkeypatch, x, w, b, relu, order)
        assert torch.equal(_bits(wide), _bits(narrow)), (shape, order)
        max_err, _ = _errors(wide, x, w, b, relu)
        print('X3WIDE %s order %d bias %d relu %d: max error %.3g' % (shape, order, bias, relu, max_err))
        assert max_err < MAX_ERROR, (shape, order, max_err)


def test_the_rule_and_the_override_choose_between_equal_kernels(monkeypatch):
    """Variant 4 as the network calls it (the rule), and forced wide: the bits of the 64-channel kernel either way."""
    from openpifpaf_amd import winograd
    x, w, b = _inputs(3, 64, 256, 21, 21, True, seed=9)
    u3 = winograd.split_filter(w)
    _, narrow = _pair(monkeypatch, x, w, b, True, 0)
    assert torch.equal(_bits(winograd.conv3x3_x3(x, u3, 256, bias=b, relu=True)), _bits(narrow))
    monkeypatch.setenv('OPA_WINO_X3_BN', '128')
    assert torch.equal(_bits(winograd.conv3x3_x3(x, u3, 256, bias=b, relu=True)), _bits(narrow))
    x64, w64, _ = _inputs(1, 16, 64, 8, 8, False, seed=9)          # (the override never overrides divisibility)
    assert winograd.conv3x3_x3(x64, winograd.split_filter(w64), 64).isfinite().all()


def test_wide_writes_into_out(monkeypatch):
    x, w, b = _inputs(2, 64, 128, 7, 9, True, seed=11)
    out = torch.full((2, 128, 7, 9), float('nan'), device='cuda').contiguous(memory_format=torch.channels_last)
    wide, narrow = _pair(monkeypatch, x, w, b, False, 0, out=out)
    assert wide.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(out), _bits(narrow))


@pytest.mark.parametrize('value', [float('nan'), float('inf')])
def test_a_non_finite_pixel_makes_the_same_outputs_nan(monkeypatch, value):
    x, w, _ = _inputs(2, 64, 128, 7, 9, False, seed=13)
    x[1, 5, 3, 4] = value
    x[0, 63, 0, 0] = value                                         # (a corner tile: beside the zero padding)
    wide, narrow = _pair(monkeypatch, x, w, None, False, 0)
    assert torch.equal(wide.isnan(), narrow.isnan()) and bool(wide.isnan().any()) and not bool(wide.isnan().all())
    assert torch.equal(_bits(wide), _bits(narrow))


@pytest.mark.parametrize('c_out', [64, 192])
def test_wide_is_refused_where_c_out_is_no_multiple_of_128(c_out):
    from openpifpaf_amd import winograd
    x, w, _ = _inputs(1, 32, c_out, 8, 8, False, seed=5)
    u3 = winograd.split_filter(w)
    out = torch.zeros((1, c_out, 8, 8), device='cuda').contiguous(memory_format=torch.channels_last)
    with pytest.raises(Exception):
        winograd.conv3x3_x3(x, u3, c_out, variant=5, out=out)
    torch.cuda.synchronize()
    assert not bool(out.any())                                     # (refused, not launched)
    assert not winograd.supported(x, w, 5)
    assert winograd.conv3x3_x3(x, u3, c_out).isfinite().all()      # (and the library still works)


def test_wide_launch_in_a_hip_graph_follows_the_refilled_input(monkeypatch):
    from openpifpaf_amd import winograd
    x1, w, b = _inputs(2, 64, 128, 7, 9, True, seed=17)
    x2 = _inputs(2, 64, 128, 7, 9, True, seed=19)[0]
    u3 = winograd.split_filter(w)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    x = x1.clone(memory_format=torch.preserve_format)
    with torch.cuda.stream(stream):
        winograd.conv3x3_x3(x, u3, 128, bias=b, relu=True, variant=5)          # warm-up on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = winograd.conv3x3_x3(x, u3, 128, bias=b, relu=True, variant=5)
    for refill in (x1, x2, x2):
        x.copy_(refill)
        torch.cuda.synchronize()
        graph.replay()
        stream.synchronize()
        torch.cuda.synchronize()
        got = out.clone(memory_format=torch.preserve_format)
        eager = winograd.conv3x3_x3(refill, u3, 128, bias=b, relu=True, variant=5)
        assert torch.equal(_bits(got), _bits(eager))
