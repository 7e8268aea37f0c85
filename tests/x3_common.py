"""Shared by the split-operand kernels' edge tests (test_x3_cases.py on the CPU, test_gpu_x3_edges.py on the GPU): the kernels'
arithmetic restated in torch on the CPU (three bfloat16 pieces per operand, six or nine piece products), the float64 reference,
the componentwise error measure, the class a non-finite result must fall in, and the input builders -- everything from a seeded
``torch.Generator``, everything float32 on the CPU.  An operand here is always the GEMM's own: ``a`` ``[M, K]`` (for the implicit
modes the im2col of the image, built by ``im2col_3x3`` / ``im2col_stem``), ``w`` ``[N, K]``."""
import torch

SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))              # the piece products the six-term kernels keep: i + j <= 2
NINE = tuple((i, j) for i in range(3) for j in range(3))
EXTRA = {9: 0.0, 6: 2.0 ** -23}                                     # the three dropped products: (2^-24 + 2^-24 + 2^-32) |a||w|
FINITE, NAN, PINF, NINF = 0, 1, 2, 3


def _top(x):
    return (x.view(torch.int32) & -65536).view(torch.float32)


def split3(t):
    """float32 -> ``[3, ...]`` float32: the pieces as ``split4`` (csrc/split_bf16.hpp) and ``fused.split_weight`` cut them (the low
    16 bits cleared by an integer mask, the remainder by a float32 subtraction, twice)."""
    t = t.detach().to(torch.float32).contiguous()
    p1 = _top(t)
    r = t - p1
    p2 = _top(r)
    return torch.stack((p1, p2, r - p2))


def model(a, w, terms, mutate=None):
    """``[M, K] x [N, K]`` -> float64 ``[M, N]``: the six or nine piece products summed in float64 -- what the kernels compute apart
    from the rounding of their float32 accumulation.  ``mutate(pa, pw)`` may damage the pieces first (the mutants of test_x3_cases)."""
    pa, pw = split3(a).double(), split3(w).double()
    if mutate is not None:
        pa, pw = mutate(pa, pw)
    out = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float64)
    for i, j in (SIX if terms == 6 else NINE):
        out += pa[i] @ pw[j].t()
    return out


def model_f32(a, w, terms):
    """``model`` with the kernels' float32 accumulators (csrc/gemm_f32x3.hip): per 16 columns of K -- one MFMA -- the leading
    products a1 w1 go to one float32 accumulator, the corrections to a second one, smallest first, and the two are joined at the
    end.  An MFMA is taken as a k-ordered chain of float32 ``fma`` (one rounding per exact product), which is what the float32
    MFMA of gfx950 is known to compute; how the bf16 pipe rounds among its 16 products is not documented, and a wider internal
    sum could only be more exact.  -> float32 ``[M, N]``."""
    pa, pw = split3(a).double(), split3(w).double()
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32)
    low = torch.zeros_like(acc)
    order = [(i, s - i) for s in (4, 3, 2, 1) for i in range(3) if 0 <= s - i <= 2 and (terms == 9 or s <= 2)]

    def chain(c, x, y, sl):
        for k in range(sl.start, min(sl.stop, x.shape[1])):
            c = (c.double() + x[:, k:k + 1] * y[:, k].unsqueeze(0)).float()
        return c
    for k0 in range(0, a.shape[1], 16):
        sl = slice(k0, k0 + 16)
        acc = chain(acc, pa[0], pw[0], sl)
        for i, j in order:
            low = chain(low, pa[i], pw[j], sl)
    return acc + low


def operand(a, a_bias=None):
    """The operand behind the prologue ``max(a + a_bias, 0)``, float64 (``a`` itself without ``a_bias``)."""
    a = a.double()
    return a if a_bias is None else (a + a_bias.double()).clamp_min(0)


def operand32(a, a_bias=None):
    """The same in float32 as the kernel forms it (one rounding of the sum)."""
    return a if a_bias is None else (a + a_bias).clamp_min(0)


def ref64(a, w, bias=None, res=None, a_bias=None, relu=False):
    """The plain float64 product with bias, residual, prologue and activation."""
    out = operand(a, a_bias) @ w.double().t()
    if bias is not None:
        out = out + bias.double()
    if res is not None:
        out = out + res.double()
    return out.clamp_min(0) if relu else out


def ref32(a, w, bias=None, res=None, a_bias=None, relu=False):
    """torch's own float32 result on the CPU (the classes of ``nonfinite_class`` are taken from it)."""
    out = operand32(a, a_bias) @ w.t()
    if bias is not None:
        out = out + bias
    if res is not None:
        out = out + res
    return torch.relu(out) if relu else out


def scale_of(a, w, bias=None, res=None, a_bias=None):
    """``S[m, n] = sum_k |a_mk| |w_nk| + |bias_n| + |res_mn|`` in float64: what a componentwise-stable product is accurate to."""
    s = operand(a, a_bias).abs() @ w.double().abs().t()
    if bias is not None:
        s = s + bias.double().abs()
    if res is not None:
        s = s + res.double().abs()
    return s


def err_c(got, ref, S):
    """``max |got - ref| / S``; an element with ``S == 0`` has to match exactly (inf if it does not)."""
    d = (got.double() - ref).abs()
    zero = S == 0
    if bool((d[zero] != 0).any()):
        return float('inf')
    return float((d / S.masked_fill(zero, 1.0)).masked_fill(zero, 0.0).max())


def nonfinite_class(r32):
    """Per element of the float32 reference: FINITE, NAN, PINF or NINF."""
    c = torch.zeros(r32.shape, dtype=torch.int64)
    c[r32.isnan()] = NAN
    c[r32 == float('inf')] = PINF
    c[r32 == float('-inf')] = NINF
    return c


def nonfinite_violations(got, clean, cls, relu, zeroed=None):
    """Elements of ``got`` that break the split-operand path's contract, as a dict of counts (all zero: the contract holds).
    ``clean``: the same launch with every planted value replaced by a finite one; ``cls``: ``nonfinite_class`` of the float32
    reference (taken before the activation); ``zeroed``: a mask of the elements whose non-finite operand the prologue's ``fmaxf``
    may have turned into 0 -- there the clean bits are a legal answer too.
      * FINITE: finite and the clean run's bits (nothing leaks inside a tile);
      * NAN: NaN -- with ReLU, NaN or +0 (``fmaxf(NaN, 0)`` is 0);
      * PINF / NINF: that infinity or NaN (an infinite OPERAND leaves the split as (Inf, NaN, NaN)) -- with ReLU, NaN, 0 or +Inf."""
    same = got.view(torch.int32) == clean.view(torch.int32)
    nan, zero, pinf, ninf = got.isnan(), got == 0, got == float('inf'), got == float('-inf')
    if zeroed is None:
        zeroed = torch.zeros_like(same)
    bad = {}
    fin = cls == FINITE
    bad['finite position differs from the clean run'] = int((fin & ~(same & got.isfinite())).sum())
    if relu:
        ok = nan | zero | pinf
        bad['non-finite position holds another value (ReLU)'] = int((~fin & ~ok & ~(zeroed & same)).sum())
    else:
        bad['NaN position is not NaN'] = int(((cls == NAN) & ~nan & ~(zeroed & same)).sum())
        bad['+Inf position is neither +Inf nor NaN'] = int(((cls == PINF) & ~(pinf | nan) & ~(zeroed & same)).sum())
        bad['-Inf position is neither -Inf nor NaN'] = int(((cls == NINF) & ~(ninf | nan) & ~(zeroed & same)).sum())
    return bad


# ---- input builders -------------------------------------------------------------------------------------------------------------------

def gen(seed):
    return torch.Generator().manual_seed(seed)


def full_significand(shape, g, emin=-60, emax=60):
    """float32 with all 24 significand bits in use (the lowest one set: no piece can be left out), exponents uniform in
    ``[emin, emax]``, either sign."""
    mant = torch.randint(0, 2 ** 23, shape, generator=g, dtype=torch.int64) | 1
    exp = torch.randint(emin + 127, emax + 128, shape, generator=g, dtype=torch.int64)
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64)
    bits = (sign << 31) | (exp << 23) | mant
    return (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)


def selection_columns(n, k, offset, g):
    """``col[n]``: the K column output channel n selects -- ``offset + a permutation of [0, n)``, wrapped into ``[0, k)``."""
    return (offset + torch.randperm(n, generator=g)) % k


def selection_weight(cols, k):
    """``[N, K]``: row n is 1.0 at ``cols[n]`` and 0 elsewhere."""
    w = torch.zeros((len(cols), k))
    w[torch.arange(len(cols)), cols] = 1.0
    return w


def selection_offsets(n, k):
    """Offsets with which ``selection_columns`` reaches every column of K."""
    return list(range(0, k, n))


def one_hot(m, k):
    """``[M, K]``: row m is 1.0 at column ``m mod K``."""
    a = torch.zeros((m, k))
    a[torch.arange(m), torch.arange(m) % k] = 1.0
    return a


def wide_rows(m, k, g, row_range=40.0, elem_range=12.0):
    """``[M, K]``: N(0, 1) times ``2^U(-row_range, row_range)`` per row times ``2^U(-elem_range, elem_range)`` per element."""
    rows = (torch.rand((m, 1), generator=g, dtype=torch.float64) * 2 - 1) * row_range
    elem = (torch.rand((m, k), generator=g, dtype=torch.float64) * 2 - 1) * elem_range
    return (torch.randn((m, k), generator=g, dtype=torch.float64) * torch.exp2(rows + elem)).float()


def wide_weight(n, k, g, elem_range=6.0):
    elem = (torch.rand((n, k), generator=g, dtype=torch.float64) * 2 - 1) * elem_range
    return (torch.randn((n, k), generator=g, dtype=torch.float64) * torch.exp2(elem) * (2.0 / k) ** 0.5).float()


def integers(shape, g, bits):
    """Integers of ``bits`` bits (sign apart) as float32: ``|v| < 2^bits``."""
    return torch.randint(-(2 ** bits) + 1, 2 ** bits, shape, generator=g).float()


def sparse_integer_weight(n, k, g, bits=9, nnz=32):
    """``[N, K]`` integer weights, ``nnz`` non-zero columns per row at random places: with 9-bit activations a row's
    ``sum_k |a||w|`` stays below ``32 x 511^2 < 2^23`` whatever K is."""
    w = torch.zeros((n, k))
    for r in range(n):
        cols = torch.randperm(k, generator=g)[:min(nnz, k)]
        v = integers((len(cols),), g, bits)
        w[r, cols] = torch.where(v == 0, torch.ones_like(v), v)
    return w


def small_row_exponent(m):
    """The exponent of row m of ``subnormal_piece_rows`` where ``m % 4 == 1``: -105 down to -126, one after the other."""
    return -105 - (torch.arange(m) // 4) % 22


def subnormal_piece_rows(m, k, g):
    """``[M, K]`` N(0, 1)-sized operand whose rows ``m % 4 == 1`` have ``|a|`` in ``[2^-126, 2^-104)`` -- full significands, ONE exponent
    per row (``small_row_exponent``): normal float32 numbers whose low pieces are subnormal bfloat16 numbers -- and whose rows
    ``m % 16 == 3`` are subnormal float32 themselves."""
    a = torch.randn((m, k), generator=g)
    mant = full_significand((m, k), g, 0, 0)
    small = mant * torch.exp2(small_row_exponent(m).double()).float().unsqueeze(1)
    sub = (torch.randint(1, 2 ** 23, (m, k), generator=g, dtype=torch.int32)
           | (torch.randint(0, 2, (m, k), generator=g, dtype=torch.int32) << 31)).view(torch.float32)
    rows = torch.arange(m)
    a[rows % 4 == 1] = small[rows % 4 == 1]
    a[rows % 16 == 3] = sub[rows % 16 == 3]
    return a


def representable_small_rows(m):
    """Rows of ``subnormal_piece_rows`` with ``|a|`` in ``[2^-110, 2^-104)``: all three pieces ARE bfloat16 numbers (no bit lies below
    2^-133) and part of the third ones are subnormal -- the rows that tell a pipe that keeps subnormal inputs from one that
    flushes them (one element can lose up to 2^-16 of its size; what the measure shows is in ``KEPT_BELOW``)."""
    rows = torch.arange(m)
    return (rows % 4 == 1) & (small_row_exponent(m) >= -110)


def flush_cost(a, w, a_bias=None):
    """``2^-125 sum_k (|a_mk| + |w_nk|)``: an upper bound of what flushing every subnormal piece to zero costs an element."""
    return 2.0 ** -125 * (operand(a, a_bias).abs().sum(1, keepdim=True) + w.double().abs().sum(1).unsqueeze(0))


def plant(t, places):
    """A copy of ``t`` with ``value`` at every ``(index tuple, value)`` of ``places``."""
    t = t.clone()
    for idx, value in places:
        t[idx] = value
    return t


# ---- the implicit modes' operands -------------------------------------------------------------------------------------------------------

def im2col_3x3(x, stride):
    """``[B, C, H, W]`` -> ``[B ho wo, 9 C]``, column ``(3 ky + kx) C + c`` = pixel ``(stride oy - 1 + ky, stride ox - 1 + kx)``,
    +0.0 in the padding: the operand of ``opa_conv3x3_f32x3`` (weights as ``fused.split_weight_3x3`` orders them)."""
    return _im2col(x, 3, stride, 1)


def im2col_stem(x):
    """``[B, 3, H, W]`` -> ``[B ho wo, 147]`` for the 7x7 stride-2 padding-3 stem, column ``(7 ky + kx) 3 + c``."""
    return _im2col(x, 7, 2, 3)


def _im2col(x, ksize, stride, pad):
    B, C, H, W = x.shape
    ho, wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    xp = torch.zeros((B, C, H + 2 * pad, W + 2 * pad), dtype=x.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    cols = xp.unfold(2, ksize, stride).unfold(3, ksize, stride)             # [B, C, ho, wo, ky, kx]
    assert cols.shape[2:4] == (ho, wo)
    return cols.permute(0, 2, 3, 4, 5, 1).reshape(B * ho * wo, ksize * ksize * C).contiguous()


def weight_rows(weight4d):
    """``[N, C, kh, kw]`` -> ``[N, (ky, kx, c)]``: the weight in ``_im2col``'s column order."""
    return weight4d.permute(0, 2, 3, 1).reshape(weight4d.shape[0], -1).contiguous()


def weight_4d(w2d, c, ksize):
    """The inverse of ``weight_rows``."""
    return w2d.reshape(w2d.shape[0], ksize, ksize, c).permute(0, 3, 1, 2).contiguous()


def rows_of(t):
    """``[B, C, H, W]`` -> ``[B H W, C]`` (values, contiguous)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def image_of(rows, b, h, w):
    """``[B H W, C]`` -> ``[B, C, H, W]`` (values, standard layout)."""
    return rows.reshape(b, h, w, rows.shape[1]).permute(0, 3, 1, 2).contiguous()


# ---- Winograd F(2x2, 3x3), variant 4 -----------------------------------------------------------------------------------------------------

def tap_filter(c_out, c_in, g, pmax=2):
    """``[O, C, 3, 3]``: output channel o reads ONE input channel ``chan[o]`` through ONE tap ``(r[o], s[o])`` with weight
    ``2^p[o]``, p in ``[0, pmax]``: ``G g G^T`` is then powers of two (one bfloat16 piece).  -> (filter, chan, r, s, p)."""
    chan = torch.randint(0, c_in, (c_out,), generator=g)
    tap = torch.arange(c_out) % 9                           # every tap
    r, s = tap // 3, tap % 3
    p = torch.randint(0, pmax + 1, (c_out,), generator=g)
    f = torch.zeros((c_out, c_in, 3, 3))
    f[torch.arange(c_out), chan, r, s] = torch.exp2(p.float())
    return f, chan, r, s, p


def tap_expected(x, chan, r, s, p):
    """``out[b, o, y, x] = 2^p x[b, chan[o], y + r - 1, x + s - 1]``, zero in the padding (float64, exact)."""
    B, C, H, W = x.shape
    xp = torch.zeros((B, C, H + 2, W + 2), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x.double()
    out = torch.zeros((B, len(chan), H, W), dtype=torch.float64)
    for o in range(len(chan)):
        out[:, o] = xp[:, chan[o], r[o]:r[o] + H, s[o]:s[o] + W] * 2.0 ** int(p[o])
    return out


def winograd_intermediates(x, weight):
    """Every intermediate of F(2x2, 3x3) on ``x`` with this filter, in float64: (V = B^T d B, U = G g G^T, the products U V per
    input channel summed over channels M, the output tiles Y = A^T M A) -- for the bit budget of the Winograd known-answer case."""
    x = x.double()
    B, C, H, W = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros((B, C, 2 * th + 2, 2 * tw + 2), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    bt = torch.tensor(((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1)), dtype=torch.float64)
    at = torch.tensor(((1, 1, 1, 0), (0, 1, -1, -1)), dtype=torch.float64)
    gm = torch.tensor(((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0)), dtype=torch.float64)
    u = torch.einsum('ar,oirs,bs->aboi', gm, weight.double(), gm)
    tiles = xp.unfold(2, 4, 2).unfold(3, 4, 2)
    half = torch.einsum('ai,bcyxij->bcyxaj', bt, tiles)                    # the transform's first pass (rows)
    v = torch.einsum('bcyxaj,dj->adbcyx', half, bt)
    m_abs = torch.einsum('adoc,adbcyx->adboyx', u.abs(), v.abs())           # bounds every partial sum over channels
    m = torch.einsum('adoc,adbcyx->adboyx', u, v)
    y_abs = torch.einsum('pa,adboyx,qd->boypxq', at.abs(), m_abs, at.abs())
    return half, v, u, m_abs, m, y_abs


# ---- the cases both suites run: (mode, ...) ------------------------------------------------------------------------------------------------
# M = 2 x 13 x 11 = 286: two full 128-row tiles and a tail; N = 64 takes the 64-wide tile, 128 the 128-wide one (six terms), 192 the
# 64-wide one three times; K = 64 is the shortest loop the kernel runs (two K-steps), 192 takes it three times round
BHW = (2, 13, 11)
PLAIN = [('plain', k, n) for k in (64, 192) for n in (64, 128, 192)]
PAIR = [('pair', 32, 96, 64, 2), ('pair', 64, 64, 128, 1)]                  # (k1, k2, n, stride), input 3 x 9 x 7
CONV3 = [('conv3', 1), ('conv3', 2), ('conv3', 3)]                         # C 64, N 64, input 3 x 9 x 7
STEM = [('stem',)]                                                         # 2 x 3 x 37 x 52, N 64
UNIT = [('unit', 72, 40), ('unit', 174, 128), ('unit', 64, 34)]
WINO = [(2, 32, 64, 7, 9), (1, 16, 64, 1, 1)]                              # (B, C, O, H, W): variant 4 on its 64-channel kernel
WINO_WIDE = [(2, 32, 128, 7, 9), (1, 16, 128, 1, 1)]                       # the same for variant 5's 128-channel workgroups
GEMM_SPECS = PLAIN + PAIR + CONV3 + STEM + UNIT
SCALINGS = [(40, 0), (-40, 17), (0, -30), (60, -60)]                       # (s, t): A by 2^s, W by 2^t


def spec_id(spec):
    return '-'.join(str(v) for v in spec)


def dims(spec):
    """-> (K, N) of the GEMM the case amounts to."""
    mode = spec[0]
    if mode in ('plain', 'unit'):
        return spec[1], spec[2]
    if mode == 'pair':
        return spec[1] + spec[2], spec[3]
    if mode == 'conv3':
        return 9 * 64, 64
    return 147, 64


def activation_shapes(spec):
    """Shapes of the case's activation tensors ([x], or [h, x] for the pair)."""
    mode = spec[0]
    if mode in ('plain', 'unit'):
        return [(BHW[0], spec[1]) + BHW[1:]]
    if mode == 'pair':
        _, k1, k2, _, s = spec
        return [(3, k1, (9 - 1) // s + 1, (7 - 1) // s + 1), (3, k2, 9, 7)]
    return [(3, 64, 9, 7)] if mode == 'conv3' else [(2, 3, 37, 52)]


def operand_of(spec, nat):
    """The GEMM operand ``[M, K]`` the case's activation tensors amount to."""
    mode = spec[0]
    if mode in ('plain', 'unit'):
        return rows_of(nat[0])
    if mode == 'pair':
        s = spec[4]
        return torch.cat((rows_of(nat[0]), rows_of(nat[1][:, :, ::s, ::s])), dim=1)
    return im2col_3x3(nat[0], spec[1]) if mode == 'conv3' else im2col_stem(nat[0])


def activations(spec, fill):
    """The case's activation tensors (standard layout, values from ``fill(shape)``; the pair's second one is drawn first) and the
    GEMM operand they amount to -> (list of tensors, a)."""
    nat = [fill(shape) for shape in reversed(activation_shapes(spec))][::-1]
    return nat, operand_of(spec, nat)


def out_shape(spec):
    """(B, ho, wo) of the case's output."""
    mode = spec[0]
    if mode in ('plain', 'unit'):
        return BHW
    if mode in ('pair', 'conv3'):
        s = spec[4] if mode == 'pair' else spec[1]
        return 3, (9 - 1) // s + 1, (7 - 1) // s + 1
    return 2, 19, 26


def has_prologue(spec):
    return spec[0] in ('plain', 'pair')


def has_residual(spec):
    return spec[0] in ('plain', 'unit')


def prologue_bias(spec, ab_first):
    """The prologue vector over ALL K columns: the pair mode applies ``a_bias`` to its first activation and zeros to the second."""
    if spec[0] == 'pair':
        return torch.cat((ab_first, torch.zeros(spec[2])))
    return ab_first


def integer_problem(spec, seed, with_res, with_pro):
    """Integer operands inside the exact regime -> (tensors, a, w, bias, res, a_bias): 9-bit activations and weights (two pieces
    each), at most 32 weights per row non-zero, bias, residual and a_bias below 2^20 / 2^20 / 2^8."""
    g = gen(seed)
    K, N = dims(spec)
    pro = with_pro and has_prologue(spec)
    # (the pair's second activation is not negative where a prologue runs: it meets max(x + 0, 0))
    nat, a = activations(spec, lambda shape: integers(shape, g, 9).abs() if pro else integers(shape, g, 9))
    w = sparse_integer_weight(N, K, g)
    bias = integers((N,), g, 20)
    res = integers((a.shape[0], N), g, 20) if with_res and has_residual(spec) else None
    k_first = spec[1] if spec[0] == 'pair' else K
    a_bias = integers((k_first,), g, 8) if pro else None
    return nat, a, w, bias, res, a_bias


def randn_problem(spec, seed, with_res, with_pro):
    """Unit-scale operands (the scaling cases) -> (tensors, a, w, bias, res, a_bias)."""
    g = gen(seed)
    K, N = dims(spec)
    pro = with_pro and has_prologue(spec)
    nat, a = activations(spec, lambda shape: torch.randn(shape, generator=g).abs() if pro else torch.randn(shape, generator=g))
    w = torch.randn((N, K), generator=g) * (2.0 / K) ** 0.5
    bias = torch.randn((N,), generator=g)
    res = torch.randn((a.shape[0], N), generator=g) if with_res and has_residual(spec) else None
    k_first = spec[1] if spec[0] == 'pair' else K
    a_bias = torch.randn((k_first,), generator=g) * 0.3 if pro else None
    return nat, a, w, bias, res, a_bias


def lowest_bit(t):
    """The exponent e of the lowest set significand bit 2^e of every non-zero element (float64 tensor; zeros give +inf)."""
    t = t.double()
    mant, exp = torch.frexp(t)                                             # t = mant 2^exp, 0.5 <= |mant| < 1
    m = (mant.abs() * 2.0 ** 53).to(torch.int64)
    low = m & -m                                                           # the lowest set bit of the 53-bit significand
    e = exp.double() - 53 + torch.log2(low.double().clamp_min(1))
    return torch.where(t == 0, torch.full_like(e, float('inf')), e)


def winograd_integer_case(shape, seed):
    B, C, O, H, W = shape
    g = gen(seed)
    x = integers((B, C, H, W), g, 15)
    f, chan, r, s, p = tap_filter(O, C, g)
    return x, f, tap_expected(x, chan, r, s, p)


def winograd_randn_case(shape, seed):
    B, C, O, H, W = shape
    g = gen(seed)
    x = torch.randn((B, C, H, W), generator=g)
    f = torch.randn((O, C, 3, 3), generator=g) * (2.0 / (9 * C)) ** 0.5
    return x, f, torch.randn((O,), generator=g)


def wide_problem(spec, seed):
    """Rows of A scaled by 2^U(-40, 40), elements by 2^U(-12, 12), weights by 2^U(-6, 6); for the implicit modes the IMAGE's pixels
    take the row scale (a window then spans several scales, which the componentwise measure allows for)."""
    g = gen(seed)
    K, N = dims(spec)

    def fill(shape):
        b, c, h, w = shape
        return image_of(wide_rows(b * h * w, c, g), b, h, w)
    nat, a = activations(spec, fill)
    w = wide_weight(N, K, g)
    S0 = scale_of(a, w)
    bias = (torch.randn((N,), generator=g).double() * S0.median(0).values).float()     # of the column's own size
    return nat, a, w, bias


# ---- Winograd: the measure, the wide case and the model of variant 4 ----------------------------------------------------------------------------

_BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))
_AT = ((1, 1, 1, 0), (0, 1, -1, -1))
_GM = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def _tiles(x, dtype):
    B, C, H, W = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros((B, C, 2 * th + 2, 2 * tw + 2), dtype=dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x.to(dtype)
    return xp.unfold(2, 4, 2).unfold(3, 4, 2)                              # [B, C, th, tw, 4, 4]


def _untile(yt, H, W):
    B, O, th, _, tw, _ = yt.shape
    return yt.reshape(B, O, 2 * th, 2 * tw)[:, :, :H, :W].contiguous()


def winograd_scale(x, f):
    """What F(2x2, 3x3) is accurate to, per output: ``|A^T| (sum_c (|G||g||G^T|) o (|B^T||d||B|)) |A|`` -- the algorithm's own
    ``sum |a||w|``: every term its transforms form, taken by magnitude, in float64.  It is never below the convolution's
    ``sum_k |x||w|`` over the 3x3 window and all channels (the products the output keeps are among the terms), and it exceeds it
    where the transforms add what the output transform takes away again: other taps, and the tile's pixels outside the window.
    -> [B, O, H, W]."""
    bt, at, gm = (torch.tensor(m, dtype=torch.float64).abs() for m in (_BT, _AT, _GM))
    u = torch.einsum('ar,oirs,bs->aboi', gm, f.double().abs(), gm)
    v = torch.einsum('ai,bcyxij,dj->adbcyx', bt, _tiles(x.abs(), torch.float64), bt)
    m = torch.einsum('adoc,adbcyx->adboyx', u, v)
    return _untile(torch.einsum('pa,adboyx,qd->boypxq', at, m, at), x.shape[2], x.shape[3])


def winograd_model_f32(x, f, mutate=None):
    """Variant 4 of csrc/winograd.hip restated: U = G g G^T in float64 rounded to float32 once, V = B^T d B in float32, both cut
    into three pieces, the six kept products of 16 channels at a time added to ONE float32 accumulator (the leading product,
    then a1 u3, a2 u2, a3 u1, a1 u2, a2 u1; each MFMA a k-ordered chain of float32 fma), the output transform in float32.
    ``mutate(pv, pu)`` may damage the pieces.  -> float32 [B, O, H, W]."""
    bt, at = torch.tensor(_BT, dtype=torch.float32), torch.tensor(_AT, dtype=torch.float32)
    gm = torch.tensor(_GM, dtype=torch.float64)
    u = torch.einsum('ar,oirs,bs->aboi', gm, f.double(), gm).float()       # [4, 4, O, C]
    t = _tiles(x, torch.float32)
    v = torch.einsum('bcyxaj,dj->adbcyx', torch.einsum('ai,bcyxij->bcyxaj', bt, t), bt)        # [4, 4, B, C, th, tw]
    pv, pu = split3(v).double(), split3(u).double()
    if mutate is not None:
        pv, pu = mutate(pv, pu)
    B, C = x.shape[:2]
    acc = torch.zeros((4, 4, B, f.shape[0]) + tuple(v.shape[4:]), dtype=torch.float32)
    for c0 in range(0, C, 16):
        for i, j in ((0, 0), (0, 2), (1, 1), (2, 0), (0, 1), (1, 0)):
            for c in range(c0, min(c0 + 16, C)):
                acc = (acc.double() + pu[j][:, :, None, :, c, None, None] * pv[i][:, :, :, None, c]).float()
    return _untile(torch.einsum('pa,adboyx,qd->boypxq', at, acc, at), x.shape[2], x.shape[3])


def wino_wide_case(shape, seed):
    """N(0, 1) x 2^U(-3, 3) per element, x a per-row scale that moves by at most 2^+-1 from one image row to the next (a 3x3 window
    then stays inside 2^+-4), x 2^U(-40, 40) per image; filter elements x 2^U(-6, 6)."""
    B, C, O, H, W = shape
    g = gen(seed)
    elem = (torch.rand((B, C, H, W), generator=g, dtype=torch.float64) * 2 - 1) * 3
    step = torch.rand((B, 1, H, 1), generator=g, dtype=torch.float64) * 2 - 1
    image = (torch.rand((B, 1, 1, 1), generator=g, dtype=torch.float64) * 2 - 1) * 40
    x = (torch.randn((B, C, H, W), generator=g, dtype=torch.float64) * torch.exp2(elem + step.cumsum(2) + image)).float()
    return x, weight_4d(wide_weight(O, 9 * C, g), C, 3)


# ---- subnormal pieces: the case and the elements that tell a pipe that keeps them from one that flushes them -----------------------------------

SUBNORMAL_SPECS = [('plain', 192, 64), ('plain', 64, 128), ('pair', 32, 96, 64, 2), ('conv3', 1), ('unit', 174, 128)]
# err_c of the telling elements: kept, they are as exact as any other (float32 rounding, below 2^-23); flushed, test_x3_cases.py
# measures 1.0e-06 and more on every telling case.  The threshold lies between the two and is asserted there from both sides.
KEPT_BELOW = 2.0 ** -21


def subnormal_problem(spec, small, seed=31):
    """small = 'a': ``subnormal_piece_rows`` as the activation against weights of order 1; 'w': the same rows as the weight against
    activations of order 1.  -> (tensors, a, w, tell) with ``tell`` [M, N] the elements whose small operand row lies in
    [2^-110, 2^-104) -- None for the implicit modes, whose windows mix pixels of every kind."""
    g = gen(seed)
    K, N = dims(spec)

    def fill(shape):
        b, c, h, w = shape
        rows = subnormal_piece_rows(b * h * w, c, g) if small == 'a' else torch.randn((b * h * w, c), generator=g)
        return image_of(rows, b, h, w)
    nat, a = activations(spec, fill)
    w = subnormal_piece_rows(N, K, g) if small == 'w' else torch.randn((N, K), generator=g)
    order1 = (w.abs() > 2.0 ** -100).all(1)
    w[order1] *= (2.0 / K) ** 0.5
    tell = None
    if spec[0] in ('plain', 'unit'):
        ra = representable_small_rows(a.shape[0]).unsqueeze(1) if small == 'a' else torch.ones((a.shape[0], 1), dtype=torch.bool)
        rw = representable_small_rows(N).unsqueeze(0) if small == 'w' else torch.ones((1, N), dtype=torch.bool)
        tell = ra & rw
    return nat, a, w, tell


def flush_subnormal_pieces(pa, pw):
    """A ``model`` mutant: every piece below 2^-126, a subnormal bfloat16 number, is read as zero."""
    tiny = 2.0 ** -126
    return torch.where(pa.abs() < tiny, torch.zeros_like(pa), pa), torch.where(pw.abs() < tiny, torch.zeros_like(pw), pw)
