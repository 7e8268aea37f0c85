"""The block-tail GEMMs (``out = relu(A W^T + bias + residual)``; csrc/gemm_f32x3.hip and csrc/gemm_f32.hip) request the residual
in the last K-steps and at the epilogue's entry instead of inside the store loop.  Only loads moved: the arithmetic and its
order are ``((acc + low) + bias) + residual``, then ``fmaxf``, as before -- so the launch with a residual must equal, BIT FOR
BIT, the same launch without one followed by the same float32 addition and ReLU.  No tolerance applies."""
import functools

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

M_MAX = 161 * 3
KERNELS = ['x3-6', 'x3-9', 'f32']          # split-operand kernel with six and nine terms; the float32-MFMA kernel


@functools.lru_cache(maxsize=None)
def _operands(K, N):
    """Seeded once per (K, N) and shared by every M (rows [:M]); never written."""
    from openpifpaf_amd import fused
    g = torch.Generator(device='cuda').manual_seed(1000 * K + N)
    a = torch.randn(M_MAX, K, device='cuda', generator=g).clamp_(min=0)          # post-ReLU activations
    w = torch.randn(N, K, device='cuda', generator=g) * (2.0 / K) ** 0.5
    bias = torch.randn(N, device='cuda', generator=g) * 0.1
    res = torch.randn(M_MAX, N, device='cuda', generator=g)
    return a, w, fused.split_weight(w), bias, res


def _gemm(kernel, a, w, w3, bias, res, relu, out=None):
    """One launch through the C entry point the network uses: ``a`` [M, K], ``res`` / ``out`` [M, N] with contiguous rows."""
    from openpifpaf_amd import fused
    from openpifpaf_amd.native import _ptr
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device='cuda')
    assert a.is_contiguous() and out.is_contiguous() and (res is None or res.is_contiguous())
    if kernel == 'f32':
        fused._launch('opa_gemm_bias_act_f32', _ptr(a), None, _ptr(w), _ptr(bias), _ptr(res), _ptr(out), M, N, K, int(relu))
    else:
        fused._launch('opa_gemm_bias_act_f32x3', _ptr(a), None, _ptr(w3), _ptr(bias), _ptr(res), _ptr(out), M, N, K, int(relu),
                      int(kernel[-1]))
    return out


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('N', [64, 128, 256])            # the 64-wide tile, one 128-wide tile, two N-tiles
@pytest.mark.parametrize('K', [64, 128, 256])            # two K-steps (the peeled ones are the whole loop), one or three regular pairs in front
def test_residual_path_is_bit_identical_to_plain_plus_residual(K, N, kernel):
    a_all, w, w3, bias, res_all = _operands(K, N)
    for M in (1, 31, 128, 129, M_MAX):                   # one row; a tile that ends inside the first 32-row block; an exact tile; one row in a second tile; four tiles
        a, res = a_all[:M], res_all[:M]
        plain = _gemm(kernel, a, w, w3, bias, None, False)
        tail = _gemm(kernel, a, w, w3, bias, res, True)
        assert torch.isfinite(tail).all()
        assert torch.equal(tail, torch.relu(plain + res)), (kernel, M, N, K)
        no_relu = _gemm(kernel, a, w, w3, bias, res, False)
        assert torch.equal(no_relu, plain + res), (kernel, M, N, K)


@pytest.mark.parametrize('kernel', KERNELS)
def test_rows_past_m_are_neither_read_nor_written(kernel):
    """Residual and output are the first M rows of tensors whose other rows are NaN: a residual row past M that reached a stored
    element would show as NaN, a store past M as a number."""
    M, N, K = 129, 128, 64
    a_all, w, w3, bias, res_all = _operands(K, N)
    a = a_all[:M]
    res_big = torch.full((M + 128, N), float('nan'), device='cuda')
    res_big[:M] = res_all[:M]
    out_big = torch.full((M + 128, N), float('nan'), device='cuda')
    plain = _gemm(kernel, a, w, w3, bias, None, False)
    _gemm(kernel, a, w, w3, bias, res_big[:M], True, out=out_big[:M])
    assert torch.isfinite(out_big[:M]).all()
    assert torch.equal(out_big[:M], torch.relu(plain + res_all[:M]))
    assert torch.isnan(out_big[M:]).all()
    assert torch.isnan(res_big[M:]).all()


@pytest.mark.parametrize('choice', ['gemm3', 'gemm'])
def test_same_result_through_the_networks_entry(choice):
    """``fused.conv_bias_act(conv3, out, fb3, identity)`` on one layer-2-shaped block (128 -> 512, 9 x 9, batch 2), on the split-operand
    kernel and on the float32-MFMA kernel."""
    from openpifpaf_amd import fused
    torch.manual_seed(7)
    conv3 = torch.nn.Conv2d(128, 512, 1, bias=False).cuda()
    h = torch.randn(2, 128, 9, 9, device='cuda').clamp_(min=0).contiguous(memory_format=torch.channels_last)
    fb3 = torch.randn(512, device='cuda') * 0.1
    identity = torch.randn(2, 512, 9, 9, device='cuda').contiguous(memory_format=torch.channels_last)
    saved = fused.choices()
    try:
        fused.set_choices({(str(h.dtype), 2 * 9 * 9, 128, 512, with_res, False): choice for with_res in (False, True)})
        plain = fused.conv_bias_act(conv3, h, fb3, None, relu=False)
        tail = fused.conv_bias_act(conv3, h, fb3, identity)
    finally:
        fused.set_choices(saved, replace=True)
    assert tail.shape == identity.shape and tail.is_contiguous(memory_format=torch.channels_last)
    assert torch.isfinite(tail).all()
    assert torch.equal(tail, torch.relu(plain + identity))
