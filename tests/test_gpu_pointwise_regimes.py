"""Every launch regime of the four small producer-side kernels against a plain reference: ``bias_act_kernel`` (bit-equal to the
same float32 operations on the CPU), ``dwconv_kernel`` (float64 convolution, derived bound, each channel on its own scale),
``channel_interleave_kernel`` (bit-equal through an integer view) and ``head_epilogue_kernel`` (layout and offsets bit-equal,
sigmoid / softplus against float64).  The case lists and the regime each case takes live in ``pointwise_common``;
test_pointwise_cases.py asserts on the CPU that they reach every regime."""
import ctypes

import pytest

torch = pytest.importorskip('torch')

import pointwise_common as pc  # noqa: E402

pytestmark = pytest.mark.gpu


def _ids(case):
    return '-'.join(str(v) for v in case)


def _vp(ptr):
    return ctypes.c_void_p(ptr)


def _padded(n, dtype, fill=pc.SENTINEL):
    """-> (buffer of PAD + n + PAD elements holding ``fill``, the view of the n in the middle): 16-byte aligned."""
    buf = torch.full((2 * pc.PAD + n,), fill, dtype=dtype, device='cuda')
    assert buf.data_ptr() % 256 == 0
    return buf, buf[pc.PAD:pc.PAD + n]


# ---- bias_act ---------------------------------------------------------------------------------------------------------------
def _bias_run(rows, C, dtype, with_res, relu, seed=0):
    from openpifpaf_amd import fused
    dt = pc.DTYPES[dtype]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C), generator=g).to(dt)
    bias = (torch.randn((C,), generator=g) * 2).to(dt)
    res = torch.randn((rows, C), generator=g).to(dt) if with_res else None
    buf, view = _padded(rows * C, dt)
    xg = view.view(rows, C)
    xg.copy_(x)
    assert xg.data_ptr() % 16 == 0
    rg = res.cuda() if with_res else None
    got = fused.bias_act_(xg, bias.cuda(), rg, relu)
    assert got.data_ptr() == xg.data_ptr()
    assert (buf[:pc.PAD] == pc.SENTINEL).all() and (buf[-pc.PAD:] == pc.SENTINEL).all()
    if with_res:
        assert torch.equal(rg.cpu(), res)
    return got.cpu(), pc.bias_act_reference(x, bias, res, relu)


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('with_res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('case', pc.BIAS_CASES, ids=_ids)
def test_bias_act_bit_equal_in_every_regime(case, with_res, relu):
    got, want = _bias_run(*case, with_res, relu)
    assert torch.equal(pc.bits(got), pc.bits(want)), float((got.float() - want.float()).abs().max())


@pytest.mark.parametrize('case', pc.BIAS_CAPPED_CASES, ids=_ids)
def test_bias_act_capped_grid_with_a_ragged_last_iteration(case):
    rows, C, dtype, with_res, relu = case
    vec_per_row, blocks, col_step, outer, tail = pc.bias_act_regime(rows, C, dtype)
    assert blocks == 4096 and col_step != 0 and outer >= 3 and tail != 0
    got, want = _bias_run(rows, C, dtype, with_res, relu)
    assert torch.equal(pc.bits(got), pc.bits(want))


def test_bias_act_4d_channels_last():
    from openpifpaf_amd import fused
    g = torch.Generator().manual_seed(1)
    x = torch.randn((3, 24, 17, 19), generator=g).contiguous(memory_format=torch.channels_last)
    b, r = torch.randn((24,), generator=g), torch.randn((3, 24, 17, 19), generator=g).contiguous(memory_format=torch.channels_last)
    got = fused.bias_act_(x.cuda(), b.cuda(), r.cuda(), True).cpu()
    assert torch.equal(got, ((x + b.view(1, -1, 1, 1)) + r).clamp_min(0))


@pytest.mark.slow
def test_bias_act_above_two_to_the_31_elements():
    from openpifpaf_amd import fused
    rows, C, dtype = pc.BIAS_HUGE_CASE
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip('needs 24 GB of free device memory')
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.empty((rows, C), dtype=torch.bfloat16, device='cuda')
    r = torch.empty((rows, C), dtype=torch.bfloat16, device='cuda')
    chunk = 1 << 20
    for i in range(0, rows, chunk):
        x[i:i + chunk] = torch.randn((min(chunk, rows - i), C), generator=g, device='cuda').to(torch.bfloat16)
        r[i:i + chunk] = torch.randn((min(chunk, rows - i), C), generator=g, device='cuda').to(torch.bfloat16)
    bias = torch.randn((C,), generator=g, device='cuda').to(torch.bfloat16)
    x0 = x.clone()
    fused.bias_act_(x, bias, r, True)
    # chunk by chunk; the last chunks on the CPU (the operations the kernel is held to), all of them in float32 on the device
    for i in range(0, rows, chunk):
        want = ((x0[i:i + chunk].float() + bias.float()) + r[i:i + chunk].float()).clamp_min(0).to(torch.bfloat16)
        assert torch.equal(x[i:i + chunk], want), i
    for i in (0, (rows // chunk) * chunk):
        want = pc.bias_act_reference(x0[i:i + chunk].cpu(), bias.cpu(), r[i:i + chunk].cpu(), True)
        assert torch.equal(x[i:i + chunk].cpu(), want), i


def _columns(dtype, xs, bs):
    """Known answers as columns: x[r, c] = xs[c], bias[c] = bs[c], padded with zeros to whole vectors."""
    per_vec = 16 // pc.ELEM_BYTES[dtype]
    C = (len(xs) + per_vec - 1) // per_vec * per_vec
    x = torch.zeros((3, C), dtype=torch.float64)
    b = torch.zeros((C,), dtype=torch.float64)
    x[:, :len(xs)] = torch.tensor(xs, dtype=torch.float64)
    b[:len(bs)] = torch.tensor(bs, dtype=torch.float64)
    return x.to(pc.DTYPES[dtype]), b.to(pc.DTYPES[dtype])


KNOWN = {
    # ties to even, overflow of the rounding to inf, the largest finite value kept
    'bfloat16': ([1.0, 1.0078125, 2.0 ** 127 * (2 - 2.0 ** -7), 2.0 ** 127 * (2 - 2.0 ** -7)], [2.0 ** -8, 2.0 ** -8, 2.0 ** 119, 2.0 ** 118],
                 [1.0, 1.015625, float('inf'), 2.0 ** 127 * (2 - 2.0 ** -7)]),
    # ties, overflow, subnormal results
    'float16': ([1.0, 1.0 + 2.0 ** -10, 65504.0, 65504.0, 2.0 ** -24, 2.0 ** -14], [2.0 ** -11, 2.0 ** -11, 16.0, 8.0, 2.0 ** -24, -2.0 ** -24],
                [1.0, 1.0 + 2.0 ** -9, float('inf'), 65504.0, 2.0 ** -23, 2.0 ** -14 - 2.0 ** -24]),
    # subnormal inputs and results are kept
    'float32': ([2.0 ** -149, 2.0 ** -126, 2.0 ** -140, 1.0], [2.0 ** -149, -2.0 ** -149, 0.0, 2.0 ** -24],
                [2.0 ** -148, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -140, 1.0]),
}


@pytest.mark.parametrize('dtype', sorted(KNOWN))
def test_bias_act_known_answers(dtype):
    from openpifpaf_amd import fused
    xs, bs, want = KNOWN[dtype]
    x, b = _columns(dtype, xs, bs)
    for relu in (False, True):
        got = fused.bias_act_(x.cuda(), b.cuda(), None, relu).cpu()
        assert got[:, :len(want)].double().tolist() == [want] * 3, (dtype, relu)
        assert torch.equal(pc.bits(got), pc.bits(pc.bias_act_reference(x, b, None, relu)))


@pytest.mark.parametrize('dtype', ['float32', 'float16', 'bfloat16'])
def test_bias_act_special_values(dtype):
    """Without ReLU NaN and +-inf come out where the float32 sum has them and nowhere else.  With ReLU the kernel's fmaxf(v, 0)
    gives 0 for NaN where torch gives NaN: either is accepted, no other value; -inf gives 0, +inf stays."""
    from openpifpaf_amd import fused
    dt = pc.DTYPES[dtype]
    g = torch.Generator().manual_seed(3)
    rows, C = 301, 24
    x = torch.randn((rows, C), generator=g)
    r = torch.randn((rows, C), generator=g)
    special = torch.tensor([float('nan'), float('inf'), float('-inf')])
    where = torch.rand((rows, C), generator=g) < 0.05
    x[where] = special[torch.randint(3, (int(where.sum()),), generator=g)]
    where = torch.rand((rows, C), generator=g) < 0.02
    r[where] = special[torch.randint(3, (int(where.sum()),), generator=g)]
    x, r = x.to(dt), r.to(dt)
    b = torch.randn((C,), generator=g).to(dt)
    pre = (x.float() + b.float()) + r.float()
    assert pre.isnan().any() and (pre == float('inf')).any() and (pre == float('-inf')).any()
    for relu in (False, True):
        got = fused.bias_act_(x.clone().cuda(), b.cuda(), r.cuda(), relu).cpu()
        want = pc.bias_act_reference(x, b, r, relu)
        nan = pre.isnan()
        assert torch.equal(pc.bits(got)[~nan], pc.bits(want)[~nan])
        if relu:
            assert bool((got[nan].isnan() | (got[nan] == 0)).all())
            assert bool((got[pre == float('-inf')] == 0).all()) and bool((got[pre == float('inf')] == float('inf')).all())
        else:
            assert bool(got[nan].isnan().all())


def test_bias_act_fallbacks_and_refusals():
    """What the kernel cannot run takes the torch path in Python and still equals the reference (float32: the same operations);
    the C entry point returns an error and writes nothing."""
    from openpifpaf_amd import _lib, fused
    g = torch.Generator().manual_seed(4)
    lib = _lib.lib()

    def raw(x, b, r, rows, C):
        rc = lib.opa_bias_act(_vp(x), _vp(b), _vp(r) if r else None, rows, C, 0, 1, None)
        torch.cuda.synchronize()
        return rc
    rows = 50
    # C % 4 != 0
    x, b = torch.randn((rows, 6), generator=g), torch.randn((6,), generator=g)
    assert torch.equal(fused.bias_act_(x.cuda(), b.cuda(), None, True).cpu(), pc.bias_act_reference(x, b, None, True))
    # a misaligned x (storage offset), a misaligned bias
    x, b, r = torch.randn((rows, 8), generator=g), torch.randn((8,), generator=g), torch.randn((rows, 8), generator=g)
    buf = torch.zeros((rows * 8 + 1,), device='cuda')
    xg = buf[1:].view(rows, 8)
    xg.copy_(x)
    assert xg.data_ptr() % 16 == 4
    assert torch.equal(fused.bias_act_(xg, b.cuda(), r.cuda(), True).cpu(), pc.bias_act_reference(x, b, r, True))
    bb = torch.zeros((9,), device='cuda')
    bg = bb[1:]
    bg.copy_(b)
    assert torch.equal(fused.bias_act_(x.cuda(), bg, r.cuda(), False).cpu(), pc.bias_act_reference(x, b, r, False))
    # a residual that is not channels-last
    x4 = torch.randn((2, 8, 5, 7), generator=g).contiguous(memory_format=torch.channels_last)
    r4 = torch.randn((2, 8, 5, 7), generator=g)
    got = fused.bias_act_(x4.cuda(), b.cuda(), r4.cuda(), True).cpu()
    assert torch.equal(got, ((x4 + b.view(1, -1, 1, 1)) + r4).clamp_min(0))
    # the C entry point
    buf, view = _padded(rows * 8, torch.float32)
    bias, res = b.cuda(), r.cuda()
    p = view.data_ptr()
    assert raw(p, bias.data_ptr(), None, rows, 6) == 1
    assert raw(p + 4, bias.data_ptr(), None, rows - 1, 8) == 1
    assert raw(p, bias.data_ptr() + 4, None, rows, 8) == 1
    assert raw(p, bias.data_ptr(), res.data_ptr() + 4, rows - 1, 8) == 1
    assert raw(p, None, None, rows, 8) == 1
    assert (buf == pc.SENTINEL).all()
    assert raw(p, bias.data_ptr(), None, 0, 8) == 0 and (buf == pc.SENTINEL).all()


# ---- depthwise convolution ---------------------------------------------------------------------------------------------------
def _dw_launcher_v(x_ptr, xs, w_ptr, b_ptr, o_ptr, os_, C, es):
    def ok(v):
        a = v * es
        return C % v == 0 and xs % v == 0 and os_ % v == 0 and x_ptr % a == 0 and o_ptr % a == 0 and w_ptr % a == 0 and \
            (not b_ptr or b_ptr % a == 0)
    return 4 if ok(4) else 2 if ok(2) else 1


def _dw_run(case, x, w, b, relu, check_regime=True):
    """The C entry point on the case's layout: the input inside a NaN-filled pixel grid, the output inside a sentinel buffer.
    -> the output [B, C, Ho, Wo] on the CPU (everything outside it was checked to hold the sentinel)."""
    from openpifpaf_amd import _lib
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias = case
    dt, es = pc.DTYPES[dtype], pc.ELEM_BYTES[dtype]
    Ho, Wo = pc.dw_out_size(H, k, s), pc.dw_out_size(W, k, s)
    xbuf = torch.full((B * H * W * xs + 2 * pc.PAD,), float('nan'), dtype=dt, device='cuda')
    xv = xbuf.as_strided((B, C, H, W), (H * W * xs, 1, W * xs, xs), pc.PAD + x_off)
    xv.copy_(x)
    obuf = torch.full((B * Ho * Wo * os_ + 2 * pc.PAD,), pc.SENTINEL, dtype=dt, device='cuda')
    ov = obuf.as_strided((B, C, Ho, Wo), (Ho * Wo * os_, 1, Wo * os_, os_), pc.PAD + o_off)
    wg, bg = w.cuda(), (b.cuda() if b is not None else None)
    assert xbuf.data_ptr() % 256 == 0 and obuf.data_ptr() % 256 == 0 and (pc.PAD * es) % 16 == 0
    assert xv.data_ptr() % 16 == (x_off * es) % 16 and ov.data_ptr() % 16 == (o_off * es) % 16
    if check_regime:
        assert _dw_launcher_v(xv.data_ptr(), xs, wg.data_ptr(), bg.data_ptr() if bg is not None else 0, ov.data_ptr(), os_, C, es) == \
            pc.dwconv_regime(case)[0]
    rc = _lib.lib().opa_dwconv_bias_act(_vp(xv.data_ptr()), xs, _vp(wg.data_ptr()), _vp(bg.data_ptr()) if bg is not None else None,
                                        _vp(ov.data_ptr()), os_, B, H, W, C, k, s, 0 if dtype == 'float32' else 2, int(relu), None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().opa_last_error()
    got = ov.cpu()
    ov.fill_(pc.SENTINEL)
    assert (obuf == pc.SENTINEL).all(), 'written outside the output pixels'
    return got, xv


@pytest.mark.parametrize('case', pc.DW_CASES, ids=_ids)
def test_dwconv_against_float64_in_every_regime(case):
    from openpifpaf_amd import fused
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias = case
    x, w, b = pc.dw_inputs(case)
    for relu in (False, True):
        got, xv = _dw_run(case, x, w, b, relu)
        ref, bound = pc.dw_reference(x, w, b, k, s, relu)
        assert got.shape == ref.shape and bool(got.isfinite().all())
        ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
        assert ratio <= 1.0, (relu, ratio)
        # the same bits from a dense copy of the operand, and through the Python entry point where it can express the layout
        dense_case = pc._dw(dtype, k, s, B, H, W, C, bias=has_bias)
        dense, _ = _dw_run(dense_case, x, w, b, relu, check_regime=False)
        assert torch.equal(pc.bits(got), pc.bits(dense))
        if os_ == C and o_off == 0 and fused._pixel_stride(xv) is not None:
            assert fused.dwconv_supported(xv, k, s) and fused._pixel_stride(xv) == xs
            py = fused.dwconv_bias_act(xv, w.cuda(), b.cuda() if b is not None else None, k, s, relu)
            assert py.is_contiguous(memory_format=torch.channels_last) and torch.equal(pc.bits(py.cpu()), pc.bits(got))


@pytest.mark.parametrize('C', [8, 5])
@pytest.mark.parametrize('k,s', pc.DW_KS)
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_dwconv_impulses_give_the_flipped_taps_bit_for_bit(dtype, k, s, C):
    """A single 1.0 at each corner and the centre of each image of a batch of 3, in the first and last channel, tap weights
    1..k*k: the output is the flipped tap pattern clipped at the borders, exact in either dtype; nothing crosses between images."""
    B, H, W = 3, 9, 11
    case = pc._dw(dtype, k, s, B, H, W, C, bias=False)
    x = torch.zeros((B, C, H, W))
    for c in (0, C - 1):
        for y, xx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
            x[:, c, y, xx] = 1.0
    x[1] *= 2.0                                                   # the middle image differs from its neighbours
    w = torch.arange(1.0, k * k + 1).view(k * k, 1).repeat(1, C)
    x, w = x.to(pc.DTYPES[dtype]), w.to(pc.DTYPES[dtype])
    got, _ = _dw_run(case, x, w, None, False)
    ref, _ = pc.dw_reference(x, w, None, k, s, False)
    assert torch.equal(got.double(), ref)
    assert float(ref.max()) >= k * k and bool((got[:, 1:C - 1] == 0).all())
    # spelled out for the top-left impulse: out[y, x] = w[P - y*s, P - x*s]
    P = k // 2
    for y in range((P // s) + 1):
        for xx in range((P // s) + 1):
            assert float(got[0, 0, y, xx]) == (P - y * s) * k + (P - xx * s) + 1


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('k,s,C', [(5, 1, 8), (3, 2, 5), (5, 2, 6), (3, 1, 5)])
def test_dwconv_special_values(dtype, k, s, C):
    """A NaN pixel reaches its k x k neighbourhood in its own channel and nothing else; +-inf likewise.  Under ReLU an affected
    element is NaN or 0 (fmaxf), -inf gives 0, +inf stays.  NaNs of several payloads in bfloat16 stay NaN through the rounding."""
    B, H, W = 2, 9, 10
    case = pc._dw(dtype, k, s, B, H, W, C)
    x, w, b = pc.dw_inputs(case, seed=5)
    x, b = (x.float() / pc.dw_channel_scales(C).view(1, C, 1, 1).float()).to(x.dtype), None if b is None else torch.ones_like(b)
    w = w.abs() + 0.25                                            # positive taps: an inf keeps its sign, no inf - inf besides the planted pair
    x[0, 0, 4, 4] = float('nan')
    x[1, C - 1, 0, 0] = float('inf')
    x[1, 1, 8, 9] = float('-inf')
    x[0, 2, 2, 2], x[0, 2, 2, 3] = float('inf'), float('-inf')    # inf - inf where both are in the window
    if dtype == 'bfloat16':
        payloads = torch.tensor([0x7fc0, 0x7fff, 0x7f81, -63], dtype=torch.int16).view(torch.bfloat16)     # -63 = 0xffc1
        x[1, 3, 3, 1:5] = payloads
    ref, bound = pc.dw_reference(x, w, b, k, s, False)
    assert ref.isnan().any() and (ref == float('inf')).any() and (ref == float('-inf')).any()
    got, _ = _dw_run(case, x, w, b, False)
    assert torch.equal(got.isnan(), ref.isnan())
    assert torch.equal(got == float('inf'), ref == float('inf')) and torch.equal(got == float('-inf'), ref == float('-inf'))
    fin = ref.isfinite()
    assert bool(((got.double() - ref).abs()[fin] <= bound[fin]).all())
    relu, _ = _dw_run(case, x, w, b, True)
    nan = ref.isnan()
    assert bool((relu[nan].isnan() | (relu[nan] == 0)).all())
    assert bool((relu[ref == float('-inf')] == 0).all()) and bool((relu[ref == float('inf')] == float('inf')).all())
    assert torch.equal(relu[fin], got.clamp_min(0)[fin])


def test_dwconv_grid_limit():
    """B * Ho = 65535 runs; 65536 is refused on the host with OPA_ERR_INVALID_ARGUMENT, nothing is launched or written."""
    from openpifpaf_amd import _lib, fused
    case = pc.DW_GRID_OK
    x, w, b = pc.dw_inputs(case)
    got, xv = _dw_run(case, x, w, b, False)
    ref, bound = pc.dw_reference(x, w, b, 3, 1, False)
    assert bool(((got.double() - ref).abs() <= bound).all())
    assert fused.dwconv_supported(xv, 3, 1)
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias = pc.DW_GRID_REFUSED
    xg = torch.zeros((B, C, H, W), device='cuda')
    assert not fused.dwconv_supported(xg, k, s)
    out = torch.full((H + 8,), pc.SENTINEL, device='cuda')
    wg = torch.ones((9, 1), device='cuda')
    rc = _lib.lib().opa_dwconv_bias_act(_vp(xg.data_ptr()), 1, _vp(wg.data_ptr()), None, _vp(out.data_ptr()), 1, B, H, W, C, k, s, 0, 0, None)
    torch.cuda.synchronize()
    assert rc == 1 and (out == pc.SENTINEL).all()
    assert torch.cuda.current_stream().query() and float(torch.ones(1, device='cuda').sum()) == 1.0      # no sticky launch error


# ---- channel interleave ------------------------------------------------------------------------------------------------------
_INT = {'float32': torch.int32, 'float16': torch.int16, 'bfloat16': torch.int16}
_CODE = {'float32': 0, 'float16': 1, 'bfloat16': 2}
_SPECIAL_BITS = {
    'float32': [0x7fc00000, 0x7fc00001, 0x7f800001, -1, -0x80000000, 0x7f800000, -0x00800000, 1, -0x7fffffff, 0x007fffff],
    'float16': [0x7e00, 0x7e01, 0x7c01, -1, -0x8000, 0x7c00, -0x0400, 1, -0x7fff, 0x03ff],
    'bfloat16': [0x7fc0, 0x7fc1, 0x7f81, -1, -0x8000, 0x7f80, -0x0080, 1, -0x7fff, 0x007f],
}


@pytest.mark.parametrize('case', pc.INTERLEAVE_CASES, ids=_ids)
def test_channel_interleave_bit_equal_in_every_regime(case):
    """Random bit patterns (NaNs of every payload, subnormals) plus -0.0, +-inf and chosen NaNs, compared as integers."""
    from openpifpaf_amd import _lib
    dtype, rows, half, pa, a_off, pb, b_off, o_off = case
    it, es = _INT[dtype], pc.ELEM_BYTES[dtype]
    g = torch.Generator().manual_seed(6)
    lim = 2 ** 31 if es == 4 else 2 ** 15
    abuf = torch.randint(-lim, lim, (rows * pa + 2 * pc.PAD,), generator=g, dtype=torch.int64).to(it)
    bbuf = torch.randint(-lim, lim, (rows * pb + 2 * pc.PAD,), generator=g, dtype=torch.int64).to(it)
    sp = torch.tensor(_SPECIAL_BITS[dtype], dtype=torch.int64).to(it)
    a = abuf.as_strided((rows, half), (pa, 1), pc.PAD + a_off)
    b = bbuf.as_strided((rows, half), (pb, 1), pc.PAD + b_off)
    a[:, 0] = sp[torch.arange(rows) % len(sp)]
    b[:, half - 1] = sp[(torch.arange(rows) + 3) % len(sp)]
    want = torch.stack((a, b), dim=2).reshape(rows, 2 * half)
    ag, bg = abuf.cuda(), bbuf.cuda()
    sentinel = 0x5a5a
    obuf = torch.full((rows * 2 * half + 2 * pc.PAD,), sentinel, dtype=it, device='cuda')
    ptr = lambda t, off: t.data_ptr() + (pc.PAD + off) * es                                 # noqa: E731
    pa_, pb_, po_ = ptr(ag, a_off), ptr(bg, b_off), ptr(obuf, o_off)
    assert ag.data_ptr() % 256 == 0 and bg.data_ptr() % 256 == 0 and obuf.data_ptr() % 256 == 0

    def ok(v):
        al = v * es
        return half % v == 0 and pa % v == 0 and pb % v == 0 and pa_ % al == 0 and pb_ % al == 0 and po_ % (2 * al) == 0
    assert (4 if ok(4) else 2 if ok(2) else 1) == pc.interleave_regime(case)
    rc = _lib.lib().opa_channel_interleave(_vp(pa_), pa, _vp(pb_), pb, _vp(po_), rows, half, _CODE[dtype], None)
    torch.cuda.synchronize()
    assert rc == 0
    out = obuf.cpu()
    lo = pc.PAD + o_off
    assert torch.equal(out[lo:lo + rows * 2 * half].view(rows, 2 * half), want)
    assert (out[:lo] == sentinel).all() and (out[lo + rows * 2 * half:] == sentinel).all()


@pytest.mark.parametrize('dtype', ['float32', 'float16', 'bfloat16'])
def test_channel_interleave_python_entry_and_fallbacks(dtype):
    from openpifpaf_amd import fused, network
    dt = pc.DTYPES[dtype]
    g = torch.Generator().manual_seed(7)
    wide = torch.randn((2, 2 * 174, 5, 7), generator=g).to(dt).contiguous(memory_format=torch.channels_last).cuda()
    other = torch.randn((2, 174, 5, 7), generator=g).to(dt).contiguous(memory_format=torch.channels_last).cuda()
    for a, b in ((wide[:, :174], other), (other, wide[:, 174:]), (wide[:, 174:], wide[:, :174])):
        want = network._channel_shuffle(torch.cat((a, b), dim=1), 2)
        got = fused.channel_interleave(a, b)
        assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(pc.bits(got.cpu()), pc.bits(want.cpu()))
    # the torch path.  Another dtype:
    b2 = other.to(torch.float32 if dt != torch.float32 else torch.float16)
    assert torch.equal(fused.channel_interleave(other, b2), network._channel_shuffle(torch.cat((other, b2), dim=1), 2))
    # another shape: a narrower b, same B, H, W (the guard that keeps the kernel from reading `half` channels out of it)
    narrow = torch.randn((2, 172, 5, 7), generator=g).to(dt).contiguous(memory_format=torch.channels_last).cuda()
    for a, b in ((other, narrow), (narrow, other), (wide[:, :174], narrow)):
        assert a.shape != b.shape and fused._pixel_stride(a) and fused._pixel_stride(b)
        got = fused.channel_interleave(a, b)
        assert got.shape == (2, 346, 5, 7)
        assert torch.equal(pc.bits(got.cpu()), pc.bits(network._channel_shuffle(torch.cat((a, b), dim=1), 2).cpu()))
    # another layout: an operand that is not channels-innermost
    nchw = other.contiguous()
    assert fused._pixel_stride(nchw) is None
    assert torch.equal(fused.channel_interleave(nchw, other), network._channel_shuffle(torch.cat((nchw, other), dim=1), 2))


# ---- head epilogue -----------------------------------------------------------------------------------------------------------
def _head_check(case, special=False):
    from openpifpaf_amd import fused
    name, us, dtype, B, Hc, Wc = case
    meta = pc.head_meta(name, us)
    x = pc.head_input(case, special=special)
    xg = x.cuda()
    assert xg.is_contiguous(memory_format=torch.channels_last) and fused.head_epilogue_supported(xg, meta)
    got = fused.head_epilogue(xg, meta).cpu()
    lay = pc.head_layout(x, meta)
    exact, ref64, kind = pc.head_reference(lay, meta)
    assert got.shape == lay.shape and got.dtype == torch.float32
    lay_g = lay.cuda()
    report = {}
    for c in range(lay.shape[2]):
        g_, l_, e_, r_ = got[:, :, c], lay[:, :, c], exact[:, :, c], ref64[:, :, c]
        if special:
            assert torch.equal(g_.isnan(), r_.isnan()), c
            assert torch.equal(g_ == float('inf'), r_ == float('inf')) and torch.equal(g_ == float('-inf'), r_ == float('-inf')), c
            if kind[c] == 0:                                                    # a NaN in the LDS tile does not disturb its neighbours
                fin = e_.isfinite()
                assert torch.equal(pc.bits(g_)[fin], pc.bits(e_)[fin]), c
            continue
        if kind[c] == 0:
            assert torch.equal(pc.bits(g_), pc.bits(e_)), c                     # layout, and float32 v + float(index)
            continue
        if kind[c] == 2:
            above = l_ > 20.0
            assert torch.equal(pc.bits(g_)[above], pc.bits(l_)[above]), c       # softplus above its threshold: the input itself
        aten = (torch.sigmoid(lay_g[:, :, c]) if kind[c] == 1 else torch.nn.functional.softplus(lay_g[:, :, c])).cpu()
        ulp = pc.ulp32(r_)
        normal = r_ >= pc.FLT_MIN
        a_err = (aten.double() - r_).abs()
        a_max = float((a_err / ulp)[normal].max())
        err = (g_.double() - r_).abs()
        k_max = float((err / ulp)[normal].max())
        key = 'sigmoid' if kind[c] == 1 else 'softplus'
        report[key] = (max(a_max, report.get(key, (0, 0))[0]), max(k_max, report.get(key, (0, 0))[1]))
        # element by element: no more than ATen float32's own error on the same input in this run plus 2 ulp; below FLT_MIN the
        # kernel may return 0 where ATen returns a subnormal
        assert bool((err <= torch.maximum(a_err + 2 * ulp, torch.full_like(ulp, pc.FLT_MIN))).all()), (c, a_max, k_max)
    return report


@pytest.mark.parametrize('case', pc.HEAD_CASES, ids=_ids)
def test_head_epilogue_in_every_regime(case):
    report = _head_check(case)
    for key, (a_max, k_max) in sorted(report.items()):
        print('head_errors: %-28s %-8s max ulp vs float64: ATen %.3f  kernel %.3f' % (_ids(case), key, a_max, k_max))


@pytest.mark.parametrize('case', [('caf', 2, 'float32', 2, 9, 13), ('cif', 1, 'bfloat16', 2, 9, 13), ('cifdet', 2, 'float16', 2, 9, 13),
                                  ('cifdet', 1, 'float32', 1, 9, 13)], ids=_ids)
def test_head_epilogue_special_values(case):
    """NaN and +-inf in exactly the reference's positions: sigmoid(+-inf) = 1 / 0, softplus(+inf) = +inf, softplus(-inf) = 0."""
    _head_check(case, special=True)


@pytest.mark.parametrize('name,us,wc', pc.HEAD_OVER_LIMIT)
def test_head_one_column_above_the_lds_limit_takes_the_torch_path(name, us, wc):
    from openpifpaf_amd import fused, network
    meta = pc.head_meta(name, us)
    torch.manual_seed(8)
    head = network.CompositeField4(meta, 8).cuda().eval().to(memory_format=torch.channels_last)
    feat = torch.randn(1, 8, 2, wc, device='cuda').contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        conv = head.conv(feat)
        assert not fused.head_epilogue_supported(conv, meta)
        at_limit = conv[:, :, :, :wc - 1].contiguous(memory_format=torch.channels_last)
        assert fused.head_epilogue_supported(at_limit, meta)
        head.fused_epilogue = False
        want = head(feat)
        head.fused_epilogue = True
        got = head(feat)
    assert torch.equal(got, want) and bool(got.isfinite().all())
