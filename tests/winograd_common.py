"""Shared by the Winograd regime tests (test_winograd_cases.py on the CPU, test_gpu_winograd_regimes.py on the GPU): a model of
the launch of every variant of csrc/winograd.hip (``wino_geometry``: read off ``launch_wino*`` and the kernels' first lines), the
shapes that together reach every regime of that launch (``WINO_REGIMES``; ``WIDE_REGIMES`` for variant 5), the dense integer case whose convolution every
variant must return bit for bit, the kernels' walk over tile blocks restated in float64 with the mutants the CPU test applies to
it (``tile_walk``), and the float32 restatement the accuracy bar is taken from (``model_f32``).  Everything from a seeded
``torch.Generator``, everything on the CPU."""
import functools

import torch

import x3_common as xc

VARIANTS = (0, 1, 2, 3, 4, 5)                          # 4: held to its 64-channel kernel by the GPU tests; 5: the 128-channel one
KC = {0: 16, 1: 8, 2: 16, 3: 16, 4: 16, 5: 16}         # input channels per K-chunk
BN = {0: 64, 1: 32, 2: 64, 3: 64, 4: 64, 5: 128}       # output channels per workgroup
TB = {0: 64, 1: 64, 2: 64, 3: 64, 4: 64, 5: 32}        # tiles per workgroup: the tile block
WAVE_TILES = {0: 16, 1: 16, 2: 8, 3: 8, 4: 8, 5: 4}    # consecutive tiles one wave stages (tile_l = tid >> 2 / tid >> 3 / tid >> 4)
ONE, BELOW8, MIXED, MULTIPLE8 = 'nwg = 1', 'nwg < 8', 'nwg = 8q + r', 'nwg = 8q'

# (B, C_in, C_out, H, W).  The table of which shape reaches which class for which variant is in test_winograd_cases.py, and
# ``test_every_class_is_reached`` there derives it from ``wino_geometry``.
WALK = (1, 32, 512, 96, 97)                            # variant 3: 37 tile blocks, G = 32 on 256 compute units
WINO_REGIMES = [
    (1, 16, 64, 1, 1),            # one tile, one workgroup, one chunk; H = W = 1
    (2, 32, 64, 7, 9),            # x3_common.WINO[0]: two chunks, 40 tiles; the shape of the non-finite tests
    (3, 48, 192, 9, 11),          # 90 tiles in 2 blocks x 3 channel blocks: nwg = 6; three chunks; H, W odd
    (5, 48, 192, 16, 13),         # 280 tiles in 5 blocks x 3: nwg = 15 = 8 + 7; images straddle the blocks; H even
    (2, 32, 64, 8, 7),            # T = 32: the second output half is empty
    (3, 16, 64, 2, 21),           # T = 33: the second output half holds one tile; H = 2
    (4, 32, 64, 8, 7),            # T = 64: T % 64 = 0
    (2, 16, 128, 5, 1),           # W = 1 under H > 1
    (2, 32, 64, 1, 6),            # H = 1 under W > 1, W even
    (17, 16, 64, 3, 3),           # 4 tiles per image: a block holds 16 images, the 17th is a block of its own
    (1, 16, 64, 6, 80),           # tiles 48..63 lie inside the image: waves without a border tile (8 and 16 tiles per wave)
    (1, 512, 64, 5, 5),           # 32 chunks (variant 1: 64)
    (1, 256, 128, 6, 6),          # 16 chunks, two channel blocks (variant 1: 32 chunks, four)
    WALK,                         # nwg = 296 = 8 x 37 (variant 1: 592, variant 3: 256 with walks of 1 and 2 blocks)
    # variant 1 only (C_in % 16 != 0, or the channel-block count of its 32-wide blocks):
    (1, 8, 32, 2, 3),             # one chunk of 8
    (3, 24, 64, 9, 11),           # three chunks of 8; 2 blocks x 2 channel blocks: nwg = 4
    (1, 128, 64, 3, 4),           # 16 chunks of 8, two channel blocks
]
NONFINITE_SHAPE = (2, 32, 64, 7, 9)
# Variant 5 (``winograd_f23_w8x3w_kernel``: 32 tiles x 128 channels per workgroup, grid ceil(T / 32) x C_out / 128) has a list of its
# own: C_out a multiple of 128, and the tile counts that matter taken modulo 32.
WIDE_REGIMES = [
    (1, 16, 128, 1, 1),           # one tile, one workgroup, one chunk; H = W = 1; T % 32 = 1
    (2, 32, 128, 8, 7),           # T = 32: one full tile block
    (3, 16, 128, 2, 21),          # T = 33: the second block holds one tile; H = 2; three images in block 0
    (1, 16, 128, 2, 62),          # T = 31: the block's last tile is a clamped duplicate; W even
    (2, 32, 128, 7, 9),           # x3_common.WINO_WIDE[0]: two chunks, 40 tiles in 2 blocks; the shape of the non-finite tests
    (2, 32, 256, 7, 9),           # 2 tile blocks x 2 channel blocks: nwg = 4
    (3, 48, 384, 9, 11),          # 90 tiles in 3 blocks x 3 channel blocks: nwg = 9 = 8 + 1; three chunks; H, W odd
    (5, 48, 384, 16, 13),         # 280 tiles in 9 blocks x 3: nwg = 27 = 24 + 3; images straddle the blocks; H even
    (1, 512, 128, 5, 5),          # 32 chunks
    (1, 256, 256, 6, 6),          # 16 chunks, two channel blocks
    WALK,                         # 74 blocks x 4: nwg = 296 = 8 x 37 (where variant 4's rule takes this kernel)
    (2, 16, 128, 5, 1),           # W = 1 under H > 1
    (2, 32, 128, 1, 6),           # H = 1 under W > 1
    (9, 16, 128, 3, 3),           # 4 tiles per image: a block holds 8 images, the 9th starts the next
    (1, 16, 128, 6, 80),          # tiles 44..47 (and more) lie inside the image: waves of 4 tiles without a border tile
]


def supports(variant, shape):
    return shape[1] % KC[variant] == 0 and shape[2] % BN[variant] == 0


def shapes_of(variant):
    return [s for s in (WIDE_REGIMES if variant == 5 else WINO_REGIMES) if supports(variant, s)]


def logical_of(block, nwg):
    """The kernels' XCD-aware remap of ``blockIdx.x`` (hardware round-robins workgroups over 8 XCDs): the logical workgroup."""
    xcd, in_xcd, q8, r8 = block & 7, block >> 3, nwg >> 3, nwg & 7
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + in_xcd


def _tile_is_inside(t, H, W, TH, TW):
    tx, ty = t % TW, (t // TW) % TH
    return ty >= 1 and 2 * ty + 2 <= H - 1 and tx >= 1 and 2 * tx + 2 <= W - 1


def wino_geometry(shape, variant, order=0, cus=256):
    """The launch of ``shape`` = (B, C_in, C_out, H, W) by ``variant`` on a part with ``cus`` compute units -> dict:
      T, n_tb, n_nb, nwg, xcd (ONE / BELOW8 / MIXED / MULTIPLE8), t_mod (T % the tile block: 64, variant 5: 32), nchunks,
      interior_wave: some wave of some block stages no border tile (clamped duplicates past T included, as the kernel sees them),
      images_per_block: the most images one tile block holds tiles of,
      blocks: ``blocks[blockIdx.x]`` = (channel block, [tile blocks this workgroup computes, in order]),
      variant 3 only: G, longest_walk, shortest_walk."""
    B, cin, cout, H, W = shape
    assert supports(variant, shape), (variant, shape)
    TH, TW = (H + 1) // 2, (W + 1) // 2
    T = B * TH * TW
    tbs = TB[variant]
    n_tb, n_nb = (T + tbs - 1) // tbs, cout // BN[variant]
    geo = {'T': T, 'TH': TH, 'TW': TW, 'n_tb': n_tb, 'n_nb': n_nb, 't_mod': T % tbs, 'nchunks': cin // KC[variant]}
    if variant == 3:
        G = min(max(cus // n_nb, 1), n_tb)
        nwg = G * n_nb
        walks = [list(range(tb, n_tb, G)) for tb in range(G)]
        geo.update(G=G, longest_walk=max(len(w) for w in walks), shortest_walk=min(len(w) for w in walks))
    else:
        nwg = n_tb * n_nb
    blocks = []
    for block in range(nwg):
        logical = logical_of(block, nwg)
        if variant == 3:
            blocks.append((logical % n_nb, walks[logical // n_nb]))
        elif order:                                    # nb_major: n_tb = nwg / n_nb
            blocks.append((logical // n_tb, [logical % n_tb]))
        else:
            blocks.append((logical % n_nb, [logical // n_nb]))
    per = WAVE_TILES[variant]
    interior = any(all(_tile_is_inside(min(tb * tbs + w * per + i, T - 1), H, W, TH, TW) for i in range(per))
                   for tb in range(n_tb) for w in range(tbs // per))
    images = max(len({t // (TH * TW) for t in range(tb * tbs, min(tb * tbs + tbs, T))}) for tb in range(n_tb))
    geo.update(nwg=nwg, xcd=ONE if nwg == 1 else BELOW8 if nwg < 8 else MULTIPLE8 if nwg % 8 == 0 else MIXED,
               interior_wave=interior, images_per_block=images, blocks=blocks)
    return geo


# The classes the shapes must reach together, per variant: name -> predicate on (shape, geometry).
CLASSES = {
    'nwg = 1': lambda s, g: g['xcd'] == ONE,
    'nwg < 8, 2+ tile blocks x 2+ channel blocks': lambda s, g: g['xcd'] == BELOW8 and g['n_nb'] >= 2 and g['nwg'] // g['n_nb'] >= 2,
    'nwg = 8q + r': lambda s, g: g['xcd'] == MIXED,
    'nwg = 8q': lambda s, g: g['xcd'] == MULTIPLE8,
    'T % 64 = 1': lambda s, g: g['t_mod'] == 1,
    'T % 64 = 32': lambda s, g: g['t_mod'] == 32,
    'T % 64 = 33': lambda s, g: g['t_mod'] == 33,
    'T % 64 = 0': lambda s, g: g['t_mod'] == 0,
    'H odd': lambda s, g: s[3] % 2 == 1 and s[3] > 1,
    'H even': lambda s, g: s[3] % 2 == 0 and s[3] > 2,
    'W odd': lambda s, g: s[4] % 2 == 1 and s[4] > 1,
    'W even': lambda s, g: s[4] % 2 == 0,
    'H = 1': lambda s, g: s[3] == 1,
    'W = 1': lambda s, g: s[4] == 1,
    'H = 2': lambda s, g: s[3] == 2,
    '3 x 3 images, 17+ of them': lambda s, g: s[3:] == (3, 3) and s[0] >= 17 and g['images_per_block'] == 16,
    '3+ images in a block': lambda s, g: g['images_per_block'] >= 3,
    'a wave without a border tile': lambda s, g: g['interior_wave'],
    '1 chunk': lambda s, g: g['nchunks'] == 1,
    '2 chunks': lambda s, g: g['nchunks'] == 2,
    '3 chunks': lambda s, g: g['nchunks'] == 3,
    '32 chunks': lambda s, g: g['nchunks'] == 32,
    '16 chunks x 2+ channel blocks': lambda s, g: g['nchunks'] == 16 and g['n_nb'] >= 2,
}
# variant 5: the tile counts modulo its 32-tile block (a block of 1 tile, of 31 with one clamped duplicate, a full one), eight images
# of 4 tiles to a block, and an odd count of 128-channel blocks (the split filter is laid out in 64-channel blocks 2 nb, 2 nb + 1)
_NARROW_ONLY = ('T % 64 = 1', 'T % 64 = 32', 'T % 64 = 33', 'T % 64 = 0', '3 x 3 images, 17+ of them')
WIDE_CLASSES = {name: holds for name, holds in CLASSES.items() if name not in _NARROW_ONLY}
WIDE_CLASSES.update({
    'T % 32 = 1': lambda s, g: g['t_mod'] == 1,
    'T % 32 = 31': lambda s, g: g['t_mod'] == 31,
    'T % 32 = 0': lambda s, g: g['t_mod'] == 0,
    '3 x 3 images, 9+ of them': lambda s, g: s[3:] == (3, 3) and s[0] >= 9 and g['images_per_block'] == 8,
    'an odd number of channel blocks': lambda s, g: g['n_nb'] >= 3 and g['n_nb'] % 2 == 1,
})


def classes_of(variant):
    return WIDE_CLASSES if variant == 5 else CLASSES
# variant 3 on 256 compute units: a second block is walked, the last (partial) block as a second block, and some workgroup walks one
WALK_CLASS = 'variant 3 walks a second block'


def walks_a_second_block(shape, geo):
    last = geo['n_tb'] - 1
    return (geo.get('longest_walk', 0) >= 2 and geo['shortest_walk'] == 1 and geo['t_mod'] != 0
            and any(len(walk) >= 2 and walk[-1] == last for _, walk in geo['blocks']))


def reached(variant, cus=256):
    """class name -> the shapes of ``shapes_of(variant)`` that reach it under ``variant``."""
    out = {name: [] for name in classes_of(variant)}
    if variant == 3:
        out[WALK_CLASS] = []
    for shape in shapes_of(variant):
        geo = wino_geometry(shape, variant, 0, cus)
        for name, holds in classes_of(variant).items():
            if holds(shape, geo):
                out[name].append(shape)
        if variant == 3 and walks_a_second_block(shape, geo):
            out[WALK_CLASS].append(shape)
    return out


# ---- the dense integer case ---------------------------------------------------------------------------------------------------------------

# Bits of x per shape: the largest b <= 12 for which every partial sum of the case, in any order, is a float32 number -- i.e.
# ``winograd_intermediates`` keeps y_abs (which bounds m_abs) below 2^24 quarter-units (U = G g G^T has a lowest bit of 1/4).
# test_winograd_cases.py asserts the budget and, where b < 12, that b + 1 would break it.  12 bits is where the search stops:
# V = B^T d B then has 14 bits, two bfloat16 pieces, which is what variant 4 has to get right.
MAX_BITS = 12
BITS = {
    (1, 16, 64, 1, 1): 12,
    (2, 32, 64, 7, 9): 12,
    (3, 48, 192, 9, 11): 12,
    (5, 48, 192, 16, 13): 12,
    (2, 32, 64, 8, 7): 12,
    (3, 16, 64, 2, 21): 12,
    (4, 32, 64, 8, 7): 12,
    (2, 16, 128, 5, 1): 12,
    (2, 32, 64, 1, 6): 12,
    (17, 16, 64, 3, 3): 12,
    (1, 16, 64, 6, 80): 12,
    (1, 512, 64, 5, 5): 9,
    (1, 256, 128, 6, 6): 10,
    WALK: 12,
    (1, 8, 32, 2, 3): 12,
    (3, 24, 64, 9, 11): 12,
    (1, 128, 64, 3, 4): 10,
    # WIDE_REGIMES ((2, 16, 128, 5, 1) and WALK are above)
    (1, 16, 128, 1, 1): 12,
    (2, 32, 128, 8, 7): 12,
    (3, 16, 128, 2, 21): 12,
    (1, 16, 128, 2, 62): 12,
    (2, 32, 128, 7, 9): 12,
    (2, 32, 256, 7, 9): 12,
    (3, 48, 384, 9, 11): 12,
    (5, 48, 384, 16, 13): 12,
    (1, 512, 128, 5, 5): 9,
    (1, 256, 256, 6, 6): 10,
    (2, 32, 128, 1, 6): 12,
    (9, 16, 128, 3, 3): 12,
    (1, 16, 128, 6, 80): 12,
}
BUDGET = 2.0 ** 22                                      # 2^24 quarter-units
BIAS_BITS = 20                                          # |y| < 2^22 and |bias| < 2^20: the sum stays an exact float32


def dense_integer_operands(shape, seed, bits):
    B, C, O, H, W = shape
    g = xc.gen(seed)
    x = xc.integers((B, C, H, W), g, bits)
    f = torch.randint(-4, 5, (O, C, 3, 3), generator=g).float()
    bias = xc.integers((O,), g, BIAS_BITS)
    return x, f, bias


@functools.lru_cache(maxsize=None)
def winograd_dense_integer_case(shape, seed=21):
    """x: integers of ``BITS[shape]`` bits; a DENSE filter of integers in [-4, 4] -- every output depends on every tap of every
    input channel of every chunk; an integer bias.  -> (x, f, bias, want): ``want`` the float64 convolution WITHOUT the bias, which
    is exact (integers far below 2^53).  Shared, read-only."""
    x, f, bias = dense_integer_operands(shape, seed, BITS[shape])
    want = torch.nn.functional.conv2d(x.double(), f.double(), padding=1)
    return x, f, bias, want


def budget_used(x, f):
    """The largest sum of magnitudes any order of the case's additions can meet, as a fraction of 2^24 quarter-units."""
    _, _, _, m_abs, _, y_abs = xc.winograd_intermediates(x, f)
    return max(float(m_abs.max()), float(y_abs.max())) / BUDGET


@functools.lru_cache(maxsize=None)
def winograd_randn_case(shape, seed=22):
    """N(0, 1) inputs, He-scaled filter, N(0, 1) bias -> (x, f, bias, ref64 with the bias, S = winograd_scale + |bias|)."""
    x, f, bias = xc.winograd_randn_case(shape, seed)
    ref = torch.nn.functional.conv2d(x.double(), f.double(), bias.double(), padding=1)
    return x, f, bias, ref, xc.winograd_scale(x, f) + bias.double().abs()[None, :, None, None]


# ---- the kernels' walk over tile blocks, in float64 -----------------------------------------------------------------------------------

MUTANTS = ('last chunk skipped', 'chunks 0 and 1 swapped on V only', 'tile index clamped to T - 2',
           'second output half of the last block not written', 'tile of image n read from image n - 1',
           'padding select dropped for one border pixel', 'block tb + G of the walk skipped',
           "chunk c's filter used with chunk c + 1's pixels for one position",
           'an out-of-range offset lands in range for one border pixel')
# Variant 5 has no padding select: the pixel's offset is out of its buffer descriptor's range, and MUTANTS[8] takes MUTANTS[5]'s
# place.  Its 'second output half' (MUTANTS[3]) is the second 64 CHANNELS of the block, over all 32 tiles.  MUTANTS[7] is its
# filter rotation losing one reload (fragment (pl ^ 1, j) of the next chunk): every variant's walk can express it.
ROTATION_POSITION = (1, 1)                              # the position (xi, nu) whose filter stays a chunk behind: wave 2's second
                                                        # (d1 + d2 along both axes: not zero by the padding even where H = W = 1)


def mutant_applies(mutant, shape, geo, variant=2):
    """Whether the mutated code path is executed at all at this shape (where it is not, the mutant is the kernel itself)."""
    if mutant == MUTANTS[5]:
        return variant != 5
    if mutant == MUTANTS[8]:
        return variant == 5
    if mutant == MUTANTS[3] and variant == 5:
        return True                                     # the second channel half of a block is always written
    if mutant in (MUTANTS[1], MUTANTS[7]):
        return geo['nchunks'] >= 2
    if mutant == MUTANTS[2]:
        return geo['T'] >= 2
    if mutant == MUTANTS[3]:
        return geo['t_mod'] == 0 or geo['t_mod'] > 32
    if mutant == MUTANTS[4]:
        return shape[0] >= 2
    if mutant == MUTANTS[6]:
        return geo.get('longest_walk', 0) >= 2
    return True


ROW_OUT, COL_OUT = 0x80000000, 0x40000000              # variant 5's byte offsets of a row / a column in the padding


def _pixels_by_select(n, r, c, H, W):
    """Variants 0-4: offsets clamped into the image, and a select that replaces what lies in the padding by zero.
    -> (valid [tiles, 4, 4], pixel index [tiles, 4, 4])."""
    valid = ((r >= 0) & (r < H))[:, :, None] & ((c >= 0) & (c < W))[:, None, :]
    return valid, ((n[:, None] * H + r.clamp(0, H - 1)) * W)[:, :, None] + c.clamp(0, W - 1)[:, None, :]


def _pixels_by_range_check(n, r, c, H, W, C, images):
    """Variant 5: a row or a column in the padding gets a byte offset that, with any partner, lies past the ``images * H * W * C * 4``
    bytes of the buffer descriptor (the kernel computes ``images`` as T / (TH * TW)); a load past the range returns zero and reads
    nothing.  The 32-bit sum of the two offsets, as the kernel forms it.  -> (valid, pixel index; 0 where nothing is read)."""
    rowoff = torch.where((r >= 0) & (r < H), (n[:, None] * H + r) * W * C * 4, torch.tensor(ROW_OUT))
    coloff = torch.where((c >= 0) & (c < W), c * C * 4, torch.tensor(COL_OUT))
    off = (rowoff[:, :, None] + coloff[:, None, :]) & 0xFFFFFFFF
    valid = off + C * 4 <= images * H * W * C * 4
    return valid, torch.where(valid, off // (C * 4), torch.zeros((), dtype=off.dtype))


def tile_walk(x, f, variant=2, order=0, cus=256, mutant=None):
    """What the kernels do, workgroup by workgroup, in float64: every ``blockIdx.x`` of the launch takes its channel block and its
    tile blocks from ``wino_geometry``; a block's 64 tiles (variant 5: 32) are clamped to T - 1; each tile's 4x4 pixels are read at
    offsets clamped into the image and replaced by zero where they lie in the padding (variant 5: at offsets that are out of the
    descriptor's range in the padding, where nothing is read and the load is zero); V = B^T d B; the products with U = G g G^T
    are added chunk by chunk; the output transform runs in two halves of 32 tiles (variant 5: of 64 channels, over all 32 tiles)
    and writes the tiles below T, the pixels inside the image.  Unwritten outputs stay NaN.  ``mutant``: one of ``MUTANTS``.
    -> float64 [B, C_out, H, W]."""
    B, C, H, W = x.shape
    O = f.shape[0]
    geo = wino_geometry((B, C, O, H, W), variant, order, cus)
    T, TH, TW, kc, bn, tbs = geo['T'], geo['TH'], geo['TW'], KC[variant], BN[variant], TB[variant]
    wide = variant == 5
    bt, at, gm = (torch.tensor(m, dtype=torch.float64) for m in (xc._BT, xc._AT, xc._GM))
    u = torch.einsum('ar,oirs,bs->aboi', gm, f.double(), gm)                 # [4, 4, O, C]
    rows = x.double().permute(0, 2, 3, 1).reshape(B * H * W, C)              # NHWC pixel rows
    y = torch.full((B, H, W, O), float('nan'), dtype=torch.float64)
    i4 = torch.arange(4)
    pa, pb = ROTATION_POSITION
    for nb, walk in geo['blocks']:
        for step, tb in enumerate(walk):
            if mutant == MUTANTS[6] and step == 1:
                continue
            t = (tb * tbs + torch.arange(tbs)).clamp_max(T - 2 if mutant == MUTANTS[2] else T - 1)
            tx, ty, n = t % TW, (t // TW) % TH, t // (TW * TH)
            if mutant == MUTANTS[4]:
                n = torch.where(n > 0, n - 1, n)
            r, c = 2 * ty[:, None] - 1 + i4, 2 * tx[:, None] - 1 + i4       # [tiles, 4]
            valid, pix = _pixels_by_range_check(n, r, c, H, W, C, T // (TH * TW)) if wide else _pixels_by_select(n, r, c, H, W)
            if mutant in (MUTANTS[5], MUTANTS[8]) and tb == 0:               # tile 0's pixel (-1, -1): the clamped pixel is read
                valid[0, 0, 0], pix[0, 0, 0] = True, n[0] * H * W
            d = torch.where(valid[..., None], rows[pix], torch.zeros((), dtype=torch.float64))      # [tiles, 4, 4, C]
            v = torch.einsum('ai,tijc,bj->abtc', bt, d, bt)
            m = torch.zeros((4, 4, tbs, bn), dtype=torch.float64)
            ub = u[:, :, nb * bn:(nb + 1) * bn]
            for chunk in range(geo['nchunks']):
                if mutant == MUTANTS[0] and chunk == geo['nchunks'] - 1:
                    continue
                vc = 1 - chunk if mutant == MUTANTS[1] and chunk < 2 else chunk
                term = torch.einsum('abtc,aboc->abto', v[..., vc * kc:(vc + 1) * kc], ub[..., chunk * kc:(chunk + 1) * kc])
                if mutant == MUTANTS[7] and chunk == 1:                      # chunk 0's filter is still in the registers
                    term[pa, pb] = v[pa, pb, :, kc:2 * kc] @ ub[pa, pb, :, :kc].t()
                m += term
            yt = torch.einsum('pa,abto,qb->tpqo', at, m, at)                 # [tiles, 2, 2, bn]
            for half in (0, 1):
                if mutant == MUTANTS[3] and half == 1 and tb == geo['n_tb'] - 1:
                    continue
                # the 32 tiles and the channels of this half: variant 5 halves its 128 channels, the others their 64 tiles
                tl = torch.arange(32) + (0 if wide else half * 32)
                ch = torch.arange(64) + half * 64 if wide else torch.arange(bn)
                tt = tb * tbs + tl
                ox, oy, on = tt % TW, (tt // TW) % TH, tt // (TW * TH)
                oh, ow = 2 * oy[:, None, None] + i4[:2, None], 2 * ox[:, None, None] + i4[None, :2]      # [32, 2, 1], [32, 1, 2]
                keep = (tt < T)[:, None, None] & (oh < H) & (ow < W)
                oh, ow, on = (a.expand(32, 2, 2)[keep] for a in (oh, ow, on[:, None, None]))
                y[on[:, None], oh[:, None], ow[:, None], (nb * bn + ch)[None, :]] = yt[tl][:, :, :, ch][keep]
    return y.permute(0, 3, 1, 2)


# ---- the float32 restatement the rms bar is taken from ----------------------------------------------------------------------------------

def sampled_channels(shape):
    """The output channels the restatement is computed for (the kernel's rms is taken over the same ones): all of them up to 192,
    every eighth of more -- one of every 64-channel block of WALK, whose chain over 512 channels would take the CPU half a minute."""
    O = shape[2]
    return torch.arange(O) if O <= 192 else torch.arange(0, O, 8)


def _bt_pass(t, dim):
    t0, t1, t2, t3 = t.unbind(dim)
    return torch.stack((t0 - t2, t1 + t2, t2 - t1, t1 - t3), dim)


def _at_pass(t, dim):
    m0, m1, m2, m3 = t.unbind(dim)
    return torch.stack(((m0 + m1) + m2, (m1 - m2) - m3), dim)


def model_plain_f32(x, f):
    """Variants 0-3 restated in float32: U = G g G^T in float64 rounded once, V = B^T d B in two float32 passes, the channels
    added in k order (a chain of float32 fma: what the float32 MFMA of gfx950 computes), the output transform as (m0 + m1) + m2 and
    (m1 - m2) - m3 along either axis.  -> float32 [B, O, H, W] (without bias)."""
    gm = torch.tensor(xc._GM, dtype=torch.float64)
    u = torch.einsum('ar,oirs,bs->aboi', gm, f.double(), gm).float().double()                  # [4, 4, O, C]
    t = xc._tiles(x, torch.float32)                                                            # [B, C, th, tw, 4, 4]
    v = _bt_pass(_bt_pass(t, 4), 5).permute(4, 5, 0, 1, 2, 3).double()                         # [4, 4, B, C, th, tw]
    acc = torch.zeros((4, 4, x.shape[0], f.shape[0]) + tuple(v.shape[4:]), dtype=torch.float32)
    for c in range(x.shape[1]):
        acc = (acc.double() + u[:, :, None, :, c, None, None] * v[:, :, :, None, c]).float()
    yt = _at_pass(_at_pass(acc, 0), 1).permute(2, 3, 4, 0, 5, 1)                               # [B, O, th, 2, tw, 2]
    return xc._untile(yt.contiguous(), x.shape[2], x.shape[3])


@functools.lru_cache(maxsize=None)
def model_f32(shape, x3):
    """The restatement of the randn case at ``shape`` on ``sampled_channels``, with the bias: ``model_plain_f32`` for variants 0-3,
    ``x3_common.winograd_model_f32`` for variants 4 and 5 (``x3``: the two agree bit for bit).  Deterministic, computed once."""
    x, f, bias, _, _ = winograd_randn_case(shape)
    ch = sampled_channels(shape)
    out = xc.winograd_model_f32(x, f[ch]) if x3 else model_plain_f32(x, f[ch])
    return out + bias[ch][None, :, None, None]


def max_rms(got, ref, S):
    """(``x3_common.err_c``, the rms of the same ratio) of ``got`` against ``ref`` in the componentwise measure."""
    ratio = (got.double() - ref).abs() / S
    return xc.err_c(got, ref, S), float(ratio.pow(2).mean().sqrt())
