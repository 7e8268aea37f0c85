"""Variant 4 of the Winograd kernel (csrc/winograd.hip: F(2x2, 3x3) on the bf16 MFMA pipe with exactly split operands), host
side: the three filter planes, their layout as the kernel's lanes read them, the K permutation that lets one float32 chunk be
one bf16 K-step, and the filter cache that follows the weight.  No GPU."""
import numpy as np
import torch

from openpifpaf_amd import network, winograd


def _weight(cout, cin, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5


def _planes(u3, cout, cin):
    """[block][chunk][pos][j][piece][lane][8] -> float32 numpy"""
    return u3.float().numpy().reshape(cout // 64, cin // 16, 16, 2, 3, 64, 8)


def test_the_three_planes_sum_exactly_to_the_float32_filter():
    cout, cin = 128, 32
    w = _weight(cout, cin, 1)
    u3 = winograd.split_filter(w)
    assert u3.dtype == torch.bfloat16 and u3.numel() == 3 * 16 * cin * cout
    p = _planes(u3, cout, cin)
    total = (p[:, :, :, :, 0].astype(np.float64) + p[:, :, :, :, 1] + p[:, :, :, :, 2])   # exact: 24 significant bits
    # back to variant 2's order [block][chunk][pos][j][kq][lane][e]
    total = total.reshape(cout // 64, cin // 16, 16, 2, 64, 2, 4).transpose(0, 1, 2, 3, 5, 4, 6).reshape(-1)
    u = winograd.transform_filter(w, 2).numpy().astype(np.float64)
    assert np.array_equal(total, u)
    # each piece carries at most 8 significant bits and the pieces do not overlap: the leading one is the truncation of U
    lead = p[:, :, :, :, 0].reshape(-1).astype(np.float32)
    full = total.reshape(cout // 64, cin // 16, 16, 2, 2, 64, 4).transpose(0, 1, 2, 3, 5, 4, 6).reshape(-1).astype(np.float32)
    assert np.array_equal(lead.view(np.uint32), full.view(np.uint32) & np.uint32(0xFFFF0000))


def test_plane_layout_is_what_the_lanes_read():
    """Lane l of the wave that owns position p loads 16-byte vector ((((block * chunks + chunk) * 16 + p) * 2 + j) * 3 + q) * 64
    + l of the planes and uses its element e as B[k' = 8 (l // 32) + e][c = l % 32] of piece q: that must be piece q of
    U[p][k = chunk * 16 + 2 e + l // 32][c = 32 (2 block + j) + l % 32]."""
    cout, cin = 128, 48
    w = _weight(cout, cin, 2)
    u3 = winograd.split_filter(w).float().numpy().reshape(-1, 8)
    G = np.array(winograd._G)
    U = np.einsum('ar,oirs,bs->aboi', G, w.double().numpy(), G).reshape(16, cout, cin).astype(np.float32)
    chunks = cin // 16
    rng = np.random.default_rng(0)
    for _ in range(400):
        block, chunk, p, j, lane, e = (rng.integers(cout // 64), rng.integers(chunks), rng.integers(16), rng.integers(2),
                                       rng.integers(64), rng.integers(8))
        k = chunk * 16 + 2 * e + lane // 32
        c = 32 * (2 * block + j) + lane % 32
        pieces = [u3[((((block * chunks + chunk) * 16 + p) * 2 + j) * 3 + q) * 64 + lane, e] for q in range(3)]
        assert np.float64(pieces[0]) + pieces[1] + pieces[2] == np.float64(U[p, c, k])
        u1 = np.array([U[p, c, k]], dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
        assert np.float32(pieces[0]) == u1.view(np.float32)[0]


def test_k_permutation_pairs_the_real_k():
    """The bf16 MFMA pairs A element e of lane (r, h) with B element e of lane (c, h) as virtual k' = 8 h + e.  When both
    operands put real k = 2 e + h there (what the LDS reads and split_filter do), the product is A @ B over the real k."""
    rng = np.random.default_rng(1)
    A = rng.standard_normal((32, 16))               # [tile, real k]
    B = rng.standard_normal((16, 32))               # [real k, channel]
    afrag = np.zeros((64, 8))
    bfrag = np.zeros((64, 8))
    for lane in range(64):
        r, h = lane % 32, lane // 32
        for e in range(8):
            afrag[lane, e] = A[r, 2 * e + h]
            bfrag[lane, e] = B[2 * e + h, r]
    # the instruction: D[r][c] = sum over k' of A'[r][k'] B'[k'][c], A'[r][8 h + e] = afrag[h * 32 + r][e], likewise B'
    Av = np.zeros((32, 16))
    Bv = np.zeros((16, 32))
    for lane in range(64):
        r, h = lane % 32, lane // 32
        Av[r, 8 * h:8 * h + 8] = afrag[lane]
        Bv[8 * h:8 * h + 8, r] = bfrag[lane]
    assert np.allclose(Av @ Bv, A @ B, rtol=0, atol=1e-12)
    assert not np.allclose(Av, A)                   # (it is a permutation, not the identity)


def test_split_filter_follows_the_weight_after_load_state_dict():
    """The optimized network's split planes are derived from conv.weight through a cache keyed on (pointer, version, device):
    loading another state into an optimized network must not leave the old filter in use."""
    net = network.optimize_for_inference_(network.factory('resnet50'))
    other = network.optimize_for_inference_(network.factory('resnet50', seed=1))
    block = next(m for m in net.modules() if isinstance(m, network._Bottleneck) and hasattr(m, 'wino_u'))
    before = winograd.split_filter_of(block.conv2).clone()
    assert winograd.split_filter_of(block.conv2) is winograd.split_filter_of(block.conv2)      # cached
    net.load_state_dict(other.state_dict())
    after = winograd.split_filter_of(block.conv2)
    assert not torch.equal(before, after)
    assert torch.equal(after, winograd.split_filter(block.conv2.weight))
    with torch.no_grad():
        block.conv2.weight.mul_(2.0)                # in place: the version counter moves
    assert torch.equal(winograd.split_filter_of(block.conv2), winograd.split_filter(block.conv2.weight))


def test_variant_table_and_switch():
    assert winograd.VARIANTS[winograd.X3_VARIANT] == winograd.VARIANTS[winograd.DEFAULT_VARIANT]
    assert isinstance(winograd.X3, bool)
