"""The 16-bit head in one kernel (``fused.head_conv_fields16``: ``opa_head_conv_fields_bf16`` / ``opa_head_conv_fields_f16``,
csrc/head16.hip) on a real MI355X: the head's 1x1 convolution on the 16-bit MFMA and ``CompositeField4``'s epilogue on its float32 sums.

Shapes ``(B, hc, wc, F, C, us)`` with K input channels -- the five geometries of the store plan's checker (``head16_common.GEOMETRIES``:
a partial row tile; three row tiles whose 32-row blocks cross image rows and images; no upsampling; one pixel with three of its four
sub-pixels cropped; M = 128 exactly with 20 live columns in the last N-tile), K = 64 (one K-step) or 192 (three, the register prefetch
live), the component counts of Cif (5), Caf (8) and CifDet (6: no scales, offset mask 0b01) -- and one wide row ``(1, 1, 300)`` that
``head_epilogue_supported`` declines (its LDS row buffer) and this route takes.  Both 16-bit types.  Every case runs in well under a
second; the float64 references are computed once per case and left unchanged.

1. known answers, bit for bit: operands on a grid on which every product and every partial sum is exact in float32 in any order;
2. random operands against float64 within the bound of float32 accumulation carried through the field function;
3. why the route exists: its rms error against float64 is at most 1/16 of torch's 16-bit convolution + ``head_epilogue``;
4. guard words around the output stay, no word inside keeps the sentinel;
5. a NaN and a +Inf in one activation element reach exactly that pixel's output positions;
6. two launches give equal bits."""
import functools

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network
from openpifpaf_amd.native import _ptr, _stream

import head16_common as hc

pytestmark = pytest.mark.gpu

CL = torch.channels_last
DTYPES = {'bfloat16': torch.bfloat16, 'float16': torch.float16}
KS = (64, 192, 192, 64, 192)                                           # per geometry
SHAPES = {'%dx%dx%d-f%dc%du%d-k%d' % (g + (k,)): g + (k,) for g, k in zip(hc.GEOMETRIES, KS)}
SHAPES['wide-1x1x300-f2c5u2-k64'] = (1, 1, 300, 2, 5, 2, 64)
NARROW = [s for s in SHAPES if not s.startswith('wide')]
U = 2.0 ** -24                                                         # float32's unit roundoff


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    monkeypatch.setattr(fused, 'HEAD16', True)


def _meta(shape):
    B, hcells, wcells, F, C, us, K = SHAPES[shape]
    return hc.meta(hc.KIND_OF_COMPONENTS[C], F, us)


def _classes(meta):
    """component -> 'pass' | 'sigmoid' | 'vector' | 'softplus'"""
    out = ['pass'] + ['sigmoid'] * meta.n_confidences + ['vector'] * (2 * meta.n_vectors) + ['softplus'] * meta.n_scales
    assert len(out) == hc.n_components(meta)
    return out


def shuffle_crop(t, meta):
    """``[B, hc, wc, N]`` -> ``[B, F, C, H, W]``: the pixel shuffle and the crop of reference network/heads.py:330-343 (low_cut 0 for us 1, 2)"""
    B, hcells, wcells, N = t.shape
    us, C = meta.upsample_stride, hc.n_components(meta)
    F = N // (C * us * us)
    t = t.reshape(B, hcells, wcells, F * C, us, us).permute(0, 3, 1, 4, 2, 5).reshape(B, F * C, hcells * us, wcells * us)
    return t[:, :, :hcells * us - (us - 1), :wcells * us - (us - 1)].reshape(B, F, C, hcells * us - (us - 1), wcells * us - (us - 1)).contiguous()


def fields64(pre64, meta):
    """The field function in float64 on ``[B, hc, wc, N]`` pre-activation values -> ``[B, F, C, H, W]``"""
    out = shuffle_crop(pre64, meta)
    H, W = out.shape[3:]
    ii = torch.arange(W, device=out.device, dtype=out.dtype)
    jj = torch.arange(H, device=out.device, dtype=out.dtype).unsqueeze(1)
    vector = 0
    for c, kind in enumerate(_classes(meta)):
        if kind == 'sigmoid':
            out[:, :, c] = torch.sigmoid(out[:, :, c])
        elif kind == 'vector':
            if meta.vector_offsets[vector // 2]:
                out[:, :, c] += jj if vector % 2 else ii
            vector += 1
        elif kind == 'softplus':
            out[:, :, c] = nn.functional.softplus(out[:, :, c], beta=1, threshold=20)
    return out


def _head(shape, dtype, x, w, b):
    """-> (the head's convolution with these parameters, x as the dense channels-last 16-bit tensor the trunk hands over, the meta)"""
    B, hcells, wcells, F, C, us, K = SHAPES[shape]
    conv = nn.Conv2d(K, F * C * us * us, 1).to('cuda', dtype).requires_grad_(False)
    with torch.no_grad():
        conv.weight.copy_(w.reshape(conv.weight.shape))
        conv.bias.copy_(b)
    xt = x.to(dtype).reshape(B, hcells, wcells, K).permute(0, 3, 1, 2)
    assert xt.is_contiguous(memory_format=CL) or xt.numel() == K
    return conv, xt, _meta(shape)


def _run(conv, x, meta):
    assert fused.head_conv_fields16_supported(conv, x, meta)
    out = fused.head_conv_fields16(conv, x, meta)
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. known answers, bit for bit -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_case(shape):
    """x and w multiples of 1/8 in [-1, 1], the bias a multiple of 1/64 in [-1, 1] (exact in both 16-bit types) -- the bias of the first
    scale plane's columns 24, so that softplus takes its > 20 branch: every product is a multiple of 1/64 and every sum of them at most
    K <= 192 in size, exact in float32 in any order.  -> (x, w, b, the exact pre-activation [B, hc, wc, N] as float32)"""
    B, hcells, wcells, F, C, us, K = SHAPES[shape]
    meta = _meta(shape)
    g = torch.Generator().manual_seed(len(shape) + K)
    M, N = B * hcells * wcells, F * C * us * us
    x = torch.randint(-8, 9, (M, K), generator=g).double() / 8
    w = torch.randint(-8, 9, (N, K), generator=g).double() / 8
    b = torch.randint(-64, 65, (N,), generator=g).double() / 64
    if meta.n_scales:
        first_scale = 1 + meta.n_confidences + 2 * meta.n_vectors
        b.view(F, C, us * us)[:, first_scale] = 24.0
    pre = x @ w.t() + b
    assert torch.equal(pre.float().double(), pre) and torch.equal((pre * 64).round(), pre * 64)
    return x.cuda(), w.cuda(), b.cuda(), pre.float().reshape(B, hcells, wcells, N).cuda()


class _Fixed(nn.Module):
    """Stands for a head's convolution in ``CompositeField4``: answers with the pre-activation tensor it was given."""

    def __init__(self, value, in_channels):
        super().__init__()
        self.value, self.in_channels = value, in_channels

    def forward(self, x):
        return self.value


def _ulps(a, b):
    """the distance of two float32 tensors of one sign pattern in units in the last place"""
    return (_bits(a).long() - _bits(b).long()).abs()


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_known_answers_bit_for_bit(shape, dtype):
    x, w, b, pre32 = _exact_case(shape)
    conv, xt, meta = _head(shape, DTYPES[dtype], x, w, b)
    assert torch.equal(xt.double().permute(0, 2, 3, 1).reshape(x.shape), x) and torch.equal(conv.bias.double(), b)    # the grid is exact in 16 bits
    got = _run(conv, xt, meta)
    pre_cl = pre32.permute(0, 3, 1, 2)                                                      # [B, N, hc, wc], channels-last in memory
    classes = _classes(meta)
    if fused.head_epilogue_supported(pre_cl, meta):
        want = fused.head_epilogue(pre_cl, meta)                                            # one field function on equal float32 values
        torch.cuda.synchronize()
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    else:                                                                                   # the wide row: CompositeField4's torch branch
        assert shape.startswith('wide')
        field = network.CompositeField4(meta, SHAPES[shape][6]).cuda().eval()
        field.fused_epilogue, field.conv = False, _Fixed(pre_cl, SHAPES[shape][6])
        with torch.no_grad():
            want = field(torch.zeros(xt.shape))                                             # (what the stand-in is asked is not read)
        assert got.shape == want.shape
        for c, kind in enumerate(classes):
            if kind in ('pass', 'vector'):
                assert torch.equal(_bits(got[:, :, c]), _bits(want[:, :, c])), (c, kind)
            else:                                                                           # expf / log1pf against torch's
                assert int(_ulps(got[:, :, c], want[:, :, c]).max()) <= 2, (c, kind)
    if 'softplus' in classes:                                                               # the > 20 branch is taken: the value itself
        c = classes.index('softplus')
        plane = shuffle_crop(pre32, meta)[:, :, c]
        assert bool((plane > 20.0).any()) and torch.equal(got[:, :, c][plane > 20.0], plane[plane > 20.0])


# ---- 2., 3. random operands against float64 ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_case(shape, dtype):
    """N(0, 1) activations, N(0, 1/K) weights, N(0, 1) biases, rounded to the 16-bit type -> (x, w, b as float64, the float64 fields,
    the bound of the fields' error)"""
    B, hcells, wcells, F, C, us, K = SHAPES[shape]
    meta = _meta(shape)
    g = torch.Generator().manual_seed(1000 + len(shape) + K)
    M, N = B * hcells * wcells, F * C * us * us
    dt = DTYPES[dtype]
    x = torch.randn((M, K), generator=g).to(dt).double().cuda()
    w = (torch.randn((N, K), generator=g) / K ** 0.5).to(dt).double().cuda()
    b = torch.randn((N,), generator=g).to(dt).double().cuda()
    pre = (x @ w.t() + b).reshape(B, hcells, wcells, N)
    ref = fields64(pre, meta)
    # any order of float32 accumulation of the K exact products, + the bias: (K + 2) u (sum |a| |w| + |b|), componentwise
    pre_bound = ((K + 2) * U * (x.abs() @ w.abs().t() + b.abs())).reshape(B, hcells, wcells, N)
    lipschitz = torch.tensor([0.25 if kind == 'sigmoid' else 1.0 for kind in _classes(meta)], dtype=torch.float64, device='cuda')
    bound = shuffle_crop(pre_bound, meta) * lipschitz.view(1, 1, -1, 1, 1) + 2.0 ** -22 * ref.abs()     # ... + the function's own rounding
    return x, w, b, ref, bound


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_random_operands_stay_within_the_bound_of_float32_accumulation(shape, dtype):
    x, w, b, ref, bound = _random_case(shape, dtype)
    got = _run(*_head(shape, DTYPES[dtype], x, w, b))
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print('HEAD16 bound | %s | %s | largest error / bound %.4f' % (shape, dtype, worst))
    assert got.shape == ref.shape and bool(got.isfinite().all()) and worst <= 1.0


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_the_error_is_a_sixteenth_of_the_two_kernel_routes(dtype):
    """Per component class, over the shapes ``head_epilogue`` can run: the rms error against float64 of the one kernel is at most 1/16
    of the rms error of torch's 16-bit convolution (its output rounded to 8 or 11 significand bits) + ``head_epilogue``."""
    new, old = {}, {}
    for shape in NARROW:
        x, w, b, ref, _ = _random_case(shape, dtype)
        conv, xt, meta = _head(shape, DTYPES[dtype], x, w, b)
        got = _run(conv, xt, meta)
        with torch.no_grad():
            y = conv(xt).contiguous(memory_format=CL)
        assert y.dtype == DTYPES[dtype] and fused.head_epilogue_supported(y, meta)
        two = fused.head_epilogue(y, meta)
        torch.cuda.synchronize()
        for c, kind in enumerate(_classes(meta)):
            if kind == 'pass':
                continue
            for sums, fields in ((new, got), (old, two)):
                e = (fields[:, :, c].double() - ref[:, :, c])
                n, s = sums.get(kind, (0, 0.0))
                sums[kind] = (n + e.numel(), s + float((e ** 2).sum()))
    assert sorted(new) == ['sigmoid', 'softplus', 'vector']
    for kind in sorted(new):
        rms_new, rms_old = (new[kind][1] / new[kind][0]) ** 0.5, (old[kind][1] / old[kind][0]) ** 0.5
        print('HEAD16 ratio | %s | %s | rms error one kernel %.3e | conv + epilogue %.3e | ratio %.5f' % (dtype, kind, rms_new, rms_old, rms_new / rms_old))
        assert rms_old > 0 and rms_new <= rms_old / 16, (kind, rms_new, rms_old)


# ---- 4. guard words ---------------------------------------------------------------------------------------------------------------------

SENTINEL = 0x7FC0BEEF                                                   # a NaN with a payload no computation produces
GUARD = 37                                                              # words in front: the output begins on a 4-byte boundary alone


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_guard_words_around_the_output_stay(shape, dtype):
    B, hcells, wcells, F, C, us, K = SHAPES[shape]
    x, w, b, ref, bound = _random_case(shape, dtype)
    conv, xt, meta = _head(shape, DTYPES[dtype], x, w, b)
    wp, bp = fused.head16_operands_of(conv)
    n = ref.numel()
    buffer = torch.full((GUARD + n + 64,), SENTINEL, dtype=torch.int32, device='cuda')
    out = buffer[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 4
    symbol = getattr(_lib.lib(), 'opa_head_conv_fields_' + ('bf16' if dtype == 'bfloat16' else 'f16'))
    status = symbol(_ptr(xt), _ptr(wp), _ptr(bp), _ptr(out), B, hcells, wcells, K, F, C, us, meta.n_confidences, meta.n_vectors, hc.offset_mask(meta),
                    meta.n_scales, _stream())
    torch.cuda.synchronize()
    assert status == 0, _lib.lib().opa_last_error()
    assert bool((buffer[:GUARD] == SENTINEL).all()) and bool((buffer[GUARD + n:] == SENTINEL).all())
    assert not bool((out == SENTINEL).any())
    assert torch.equal(out, _bits(_run(conv, xt, meta)).reshape(-1))                    # what the launcher's own output holds


# ---- 5. non-finite values -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('value', ['nan', 'inf'])
@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_a_non_finite_activation_reaches_its_pixel_alone(shape, dtype, value):
    """One element of one pixel NaN, or +Inf: exactly that pixel's uncropped sub-pixel positions of EVERY plane change, and to nothing
    finite in the pre-activation -- NaN for NaN; for +Inf the field function of +Inf, -Inf (the weight's sign) or NaN (a zero weight,
    the grid has some), which for a confidence or a scale can be the finite 0 or 1: the fields must equal, bit for bit (any NaN for a
    NaN), ``head_epilogue`` / the field function applied to that pre-activation.  The zero weight rows behind N multiply the NaN too:
    nothing of them may be stored, which the untouched neighbours and guard test show."""
    B, hcells, wcells, F, C, us, K = SHAPES[shape]
    x, w, b, pre32 = _exact_case(shape)
    conv, xt, meta = _head(shape, DTYPES[dtype], x, w, b)
    clean = _run(conv, xt, meta)
    M = x.shape[0]
    m, k = (M * 2) // 3, K - 3                                                              # a pixel inside the last row tile, a late K chunk
    bad = x.clone()
    bad[m, k] = float(value)
    got = _run(*_head(shape, DTYPES[dtype], bad, w, b))
    hit = torch.zeros((M, 1), dtype=torch.float64, device='cuda')
    hit[m] = 1.0
    H, W = clean.shape[3:]
    touched = shuffle_crop(hit.expand(M, F * C * us * us).reshape(B, hcells, wcells, -1), meta) > 0      # that pixel's positions, every plane
    assert int(touched.sum()) == F * C * len([1 for dy in range(us) for dx in range(us)
                                              if (m // wcells % hcells) * us + dy < H and (m % wcells) * us + dx < W])
    assert torch.equal(_bits(got)[~touched], _bits(clean)[~touched])                        # nowhere else, bit for bit
    if value == 'nan':
        assert bool(got[touched].isnan().all())
        return
    pre = (bad @ w.t() + b).float().reshape(B, hcells, wcells, -1)                          # float64 sums of exact terms: +-Inf, or NaN from Inf * 0
    assert not bool(shuffle_crop(pre.double(), meta)[touched].isfinite().any())
    pre_cl = pre.permute(0, 3, 1, 2)
    if fused.head_epilogue_supported(pre_cl, meta):
        want = fused.head_epilogue(pre_cl, meta)
        torch.cuda.synchronize()
    else:
        want = fields64(pre.double(), meta).float()                                          # (0, 1, +-Inf, NaN: exact in any precision)
    same = (_bits(got) == _bits(want)) | (got.isnan() & want.isnan())
    assert bool(same[touched].all())
    classes = _classes(meta)
    for c in [c for c, kind in enumerate(classes) if kind in ('pass', 'vector')]:
        assert not bool(got[:, :, c][touched[:, :, c]].isfinite().any()), c


# ---- 6. repeatability ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_two_launches_give_equal_bits(shape, dtype):
    x, w, b, _, _ = _random_case(shape, dtype)
    conv, xt, meta = _head(shape, DTYPES[dtype], x, w, b)
    first, again = _run(conv, xt, meta), _run(conv, xt, meta)
    assert first.data_ptr() != again.data_ptr() and torch.equal(_bits(first), _bits(again))
