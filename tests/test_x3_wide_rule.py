"""The 128 x 256 tile of csrc/gemm_f32x3.hip, as far as it can be checked without a GPU: the launcher's rule restated (which
launches take the wide tile, what ``OPA_X3_TILE`` does to it), the dynamic LDS it asks for against the 160 KB of a gfx950 compute
unit, and the staging maps -- every element of the 128 x 32 activation tile and of the 3 x 256 x 32 weight planes is fetched by
exactly one thread and lands in an LDS slot of its own inside its plane.  The constants are read from the source, so that the
restatement cannot drift from it."""
import itertools
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'openpifpaf_amd', 'csrc', 'gemm_f32x3.hip')
BM, BK = 128, 32                                 # rows of a tile, floats of a K-step
LDS_PER_CU = 160 * 1024
PLAIN, PAIR, TAPS, UNIT = range(4)


@pytest.fixture(scope='module')
def consts():
    with open(SRC) as f:
        text = f.read()

    def value(name):
        m = re.search(r'\b%s = (\d+)\b' % name, text)
        assert m, name + ' is not a plain constant of csrc/gemm_f32x3.hip any more'
        return int(m.group(1))
    return {name: value(name) for name in ('kX3WideBN', 'kX3WideThreads', 'kX3WideCUs', 'kX3WideMinKRes', 'kX3BM')}


def wide_pays(c, blocks, res, k):
    """``x3_wide_pays``: ceil(W / CUs) whole rounds at 15/16 of the 128-wide tile's time per round, against W / CUs rounds and a
    quarter; at least two rounds; a residual only behind kX3WideMinKRes columns of K."""
    cus = c['kX3WideCUs']
    if res and k < c['kX3WideMinKRes']:
        return False
    rounds = (blocks + cus - 1) // cus
    return blocks >= 2 * cus and rounds * cus * 15 <= (blocks + cus // 4) * 16


def takes_wide_tile(c, mode, terms, m, n, k=1024, res=False, env=None):
    """``launch_x3``'s rule: an instantiation exists (not UNIT, six terms, N a multiple of the tile width) AND the switch asks for
    the wide tile or, the switch unset (or anything but 128 / 256), ``x3_wide_pays`` for the launch."""
    if mode == UNIT or terms != 6 or n % c['kX3WideBN'] != 0:
        return False
    forced = int(env) if env not in (None, '') else 0
    blocks = (m + c['kX3BM'] - 1) // c['kX3BM'] * (n // c['kX3WideBN'])
    return forced == c['kX3WideBN'] or (forced != 128 and wide_pays(c, blocks, res, k))


def test_constants(consts):
    assert consts['kX3WideBN'] == 256 and consts['kX3WideThreads'] == 512 and consts['kX3BM'] == BM
    assert consts['kX3WideCUs'] == 256 and consts['kX3WideMinKRes'] % 64 == 0


def test_rule_on_the_launches_of_a_resnet50_step(consts):
    """641 px, batch 32: the wide tile's workgroups per launch and what the rule makes of them (profiles/x3_wide/README.md)."""
    m3, m4 = 32 * 81 * 81, 32 * 41 * 41
    for m, n, k, res, want in ((m3, 256, 1024, False, True),               # reduce, layer 3: 1641 workgroups, 6.4 rounds
                               (m4, 512, 2048, False, False),              # reduce, layer 4: 842, 3.3 rounds -- four whole ones
                               (m3, 512, 1024, False, True), (32 * 161 * 161, 256, 512, False, True),
                               (32 * 161 * 161, 512, 128, True, False), (m3, 1024, 256, True, False), (m4, 2048, 512, True, False),
                               (32 * 321 * 321, 256, 128, False, True), (m4, 2048, 1536, False, True)):
        assert takes_wide_tile(consts, PLAIN, 6, m, n, k, res) == want, (m, n, k, res)


def test_rule(consts):
    cus = consts['kX3WideCUs']
    for mode in (PLAIN, PAIR, TAPS):
        # whole rounds from two on; one row block more starts a round that is nearly empty
        for rounds in (2, 3, 8):
            assert takes_wide_tile(consts, mode, 6, BM * cus * rounds, 256)
            assert not takes_wide_tile(consts, mode, 6, BM * (cus * rounds + 1), 256)
        assert not takes_wide_tile(consts, mode, 6, BM * cus, 256) and not takes_wide_tile(consts, mode, 6, 1, 256)
        assert takes_wide_tile(consts, mode, 6, BM * cus, 512)                 # two N-tiles per row block count
        assert all(takes_wide_tile(consts, mode, 6, BM * w, 256) for w in range(16 * cus, 18 * cus))     # many rounds: any remainder
        assert not takes_wide_tile(consts, mode, 9, BM * cus * 8, 256)
        for n in (64, 128, 320, 384, 640):                                     # the heads and the narrow layers
            assert not any(takes_wide_tile(consts, mode, 6, BM * cus * 8, n, env=env) for env in (None, '128', '256'))
    # a residual: only behind a K loop of kX3WideMinKRes columns
    kr = consts['kX3WideMinKRes']
    assert takes_wide_tile(consts, PLAIN, 6, BM * cus * 8, 256, kr, True) and not takes_wide_tile(consts, PLAIN, 6, BM * cus * 8, 256, kr - 64, True)
    assert takes_wide_tile(consts, PLAIN, 6, BM * cus * 8, 256, 64, False)
    # the switch overrides x3_wide_pays in both directions and nothing else
    assert takes_wide_tile(consts, PLAIN, 6, 1, 256, 64, True, '256') and not takes_wide_tile(consts, PLAIN, 6, BM * cus * 8, 256, env='128')
    assert not takes_wide_tile(consts, PLAIN, 9, BM * cus * 8, 256, env='256') and not takes_wide_tile(consts, UNIT, 6, BM * cus * 8, 256, env='256')
    assert takes_wide_tile(consts, PLAIN, 6, BM * cus * 8, 256, env='') and takes_wide_tile(consts, PLAIN, 6, BM * cus * 8, 256, env='64')


def test_lds_fits_a_compute_unit(consts):
    bn, waves = consts['kX3WideBN'], consts['kX3WideThreads'] // 64
    stage = 3 * (BM + bn) * BK * 2                            # three bf16 planes of both operands
    total = 2 * stage + bn * 4                                # two stages, the tile's bias behind them
    assert stage == 73728 and total == 148480 and total <= LDS_PER_CU
    assert waves * 32 * 64 * 4 <= stage, 'the epilogue patches (32 x 64 floats per wave) reach into stage 1'
    # ... and one workgroup per compute unit is all that fits: the kernel's loop is built for that
    assert 2 * total > LDS_PER_CU


def x3_lds(row, k):
    """bf16 offset of element k of row ``row`` in a plane: rows of 32, their 16-byte chunks XOR-swizzled by (row / 4) % 4."""
    return row * BK + ((((k >> 3) ^ (row >> 2)) & 3) << 3) + (k & 7)


def test_staging_maps_cover_the_tiles_once(consts):
    threads, bn = consts['kX3WideThreads'], consts['kX3WideBN']
    # the activation: 16-byte vectors of four floats, 8 per row, 64 rows per pass, two passes; split into 8-byte plane stores
    seen, slots = set(), set()
    for tid, p in itertools.product(range(threads), range(BM * BK // 4 // threads)):
        row, col = p * (threads // 8) + tid // 8, (tid % 8) * 4
        assert 0 <= row < BM
        slot = x3_lds(tid // 8, col) + p * (threads // 8) * BK               # (the kernel adds the pass as a constant: period 16 rows)
        assert slot == x3_lds(row, col) and slot % 4 == 0 and slot + 4 <= BM * BK
        for e in range(4):
            assert (row, col + e) not in seen
            seen.add((row, col + e))
            slots.add(slot + e)
    assert len(seen) == BM * BK and len(slots) == BM * BK
    # the weight: vector t of a thread is plane t / 2, row (t % 2) * 128 + tid / 4, eight bf16 from column (tid % 4) * 8
    seen, slots = set(), set()
    per_thread = 3 * bn * BK // 8 // threads
    assert per_thread == 6
    for tid, t in itertools.product(range(threads), range(per_thread)):
        plane, row, col = t // 2, (t % 2) * 128 + tid // 4, (tid % 4) * 8
        assert 0 <= row < bn
        slot = plane * bn * BK + (t % 2) * 128 * BK + x3_lds(tid // 4, col)
        assert slot == plane * bn * BK + x3_lds(row, col) and slot % 8 == 0
        for e in range(8):
            assert (plane, row, col + e) not in seen
            seen.add((plane, row, col + e))
            slots.add(slot + e)
    assert len(seen) == 3 * bn * BK and len(slots) == 3 * bn * BK and max(slots) < 3 * bn * BK


def test_fragment_reads_of_a_wave_spread_over_the_banks():
    """The swizzle's purpose, for the rows a wave reads: the 16-byte fragments of 16 consecutive rows at one K offset fall on 16
    different 16-byte groups of the 256-byte bank line."""
    for first, kof in itertools.product(range(0, 256, 16), (0, 8, 16, 24)):
        groups = {(x3_lds(first + r, kof) * 2 // 16) % 16 for r in range(16)}
        assert len(groups) == 16
