"""The split-operand GEMM's two tiles against each other on the launches of a resnet50 step at 641 px / batch 32 whose N is a
multiple of 256: the 1x1 reduces, the block tails (with a residual), the four pairs and the two strided 3x3 convolutions.

``OPA_X3_TILE`` (read by ``launch_x3`` on every launch) switches between the 128-wide tile -- the only one before the wide tile
existed: the same machine code -- and the 128 x 256 tile inside one process, so the two alternate on the same operands: ROUNDS
rounds, each a window of REPS launches per tile between two events.  Printed per shape: workgroups of the wide tile, the lowest
and the median window of either tile, and whether the wide tile's median lies below the 128-wide tile's LOWEST window (the
condition under which a shape may stay in the launcher's rule).  Both outputs are compared bit for bit.

    python tools/gpu/gemm_x3_tile_ab.py              # B=32; SHAPES=reduce,tail ... selects by prefix; ROUNDS, REPS
    python tools/gpu/gemm_x3_tile_ab.py --sweep      # where the launcher's rule turns: the workgroup count, and K behind a residual
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from openpifpaf_amd import fused  # noqa: E402

B = int(os.environ.get('B', '32'))
ROUNDS, REPS = int(os.environ.get('ROUNDS', '7')), int(os.environ.get('REPS', '10'))
CL = torch.channels_last
# (name, mode, output side, K (pair: (k1, k2); taps: C), N, residual | stride)
SHAPES = [
    ('reduce L3 1024->256', 'plain', 81, 1024, 256, False),
    ('reduce L4 2048->512', 'plain', 41, 2048, 512, False),
    ('reduce first L3 512->256', 'plain', 161, 512, 256, False),
    ('reduce first L4 1024->512', 'plain', 81, 1024, 512, False),
    ('tail L2 128->512', 'plain', 161, 128, 512, True),
    ('tail L3 256->1024', 'plain', 81, 256, 1024, True),
    ('tail L4 512->2048', 'plain', 41, 512, 2048, True),
    ('pair L1 64+64->256', 'pair', 321, (64, 64), 256, 1),
    ('pair L2 128+256->512', 'pair', 161, (128, 256), 512, 2),
    ('pair L3 256+512->1024', 'pair', 81, (256, 512), 1024, 2),
    ('pair L4 512+1024->2048', 'pair', 41, (512, 1024), 2048, 2),
    ('conv3 s2 256->256', 'taps', 81, 256, 256, 2),
    ('conv3 s2 512->512', 'taps', 41, 512, 512, 2),
]
# the rule's two edges: the reduce shapes of layers 3 and 4 at 2 ... 8 wide workgroups per compute unit (256 of them; one image of
# 1 x M pixels) -- whole rounds and rounds that have only begun --, and the layer-3 tail with a residual over K
SWEEP = [('reduce K %d N %d, %d WGs' % (k, n, wgs), 'plain', (1, wgs * 128 * 256 // n), k, n, False)
         for k, n in ((1024, 256), (2048, 512)) for wgs in (512, 600, 768, 842, 1030, 1300, 1536, 2048)]
SWEEP += [('tail K %d N 1024' % k, 'plain', 81, k, 1024, True) for k in (128, 256, 384, 512, 768, 1024)]
SWEEP += [('no residual K %d N 1024' % k, 'plain', 81, k, 1024, False) for k in (128, 256)]
if '--sweep' in sys.argv[1:]:
    SHAPES = SWEEP
if os.environ.get('SHAPES'):
    SHAPES = [sh for sh in SHAPES if any(sh[0].startswith(f) for f in os.environ['SHAPES'].split(','))]


def dims(side):
    """an output side: B square images; (h, w): one image"""
    return (B, side, side) if isinstance(side, int) else (1,) + tuple(side)


def act(channels, side):
    b, h, w = dims(side)
    return torch.randn((b, channels, h, w), device='cuda').clamp_(min=0).contiguous(memory_format=CL)   # (post-ReLU activations)


def conv(n, c, k, stride=1, padding=0):
    return torch.nn.Conv2d(c, n, k, stride, padding, bias=False).cuda().requires_grad_(False)


def launcher(mode, side, k, n, extra):
    bias = torch.randn(n, device='cuda') * 0.1
    if mode == 'plain':
        x, w3 = act(k, side), fused.split_weight(torch.randn((n, k), device='cuda') * (2.0 / k) ** 0.5)
        r = act(n, side) if extra else None
        return lambda: fused.conv1x1_bias_act_x3(x, w3, bias, r, True, None, 6), 2.0 * k
    if mode == 'pair':
        k1, k2 = k
        c3, cd = conv(n, k1, 1), conv(n, k2, 1, extra)
        h, x = act(k1, side), act(k2, (side - 1) * extra + 1)
        assert fused.pair_supported(c3, cd, h, x, bias)
        return lambda: fused.conv1x1_pair_bias_act_x3(c3, cd, h, x, bias, True), 2.0 * (k1 + k2)
    c = conv(n, k, 3, extra, 1)
    x = act(k, (side - 1) * extra + 1)
    assert fused.conv3x3_x3_supported(c, x, bias)
    return lambda: fused.conv3x3_bias_act_x3(c, x, bias, True), 2.0 * 9 * k


def window_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    assert fused.X3_TERMS == 6
    torch.manual_seed(0)
    print('# B %d, %d rounds of %d launches per tile, alternating; ms per launch' % (B, ROUNDS, REPS), flush=True)
    with torch.no_grad():
        for name, mode, side, k, n, extra in SHAPES:
            fn, flops_per_mn = launcher(mode, side, k, n, extra)
            b, h, w = dims(side)
            m = b * h * w
            outs, times = {}, {128: [], 256: []}
            for tile in (128, 256):
                os.environ['OPA_X3_TILE'] = str(tile)
                outs[tile] = fn()
                fn()
            torch.cuda.synchronize()
            same = torch.equal(outs[128].view(torch.int32), outs[256].view(torch.int32))
            outs.clear()
            for _ in range(ROUNDS):
                for tile in (128, 256):
                    os.environ['OPA_X3_TILE'] = str(tile)
                    times[tile].append(window_ms(fn))
            lo = {t: min(v) for t, v in times.items()}
            med = {t: statistics.median(v) for t, v in times.items()}
            hi128 = max(times[128])
            verdict = 'FASTER' if med[256] < lo[128] else ('slower' if med[256] > hi128 else 'inside the 128 tile\'s spread')
            print('%-28s M %8d N %4d wide WGs %6d | 128: min %.4f med %.4f max %.4f | 256: min %.4f med %.4f max %.4f | med/med %+5.1f %% %5.1f TF %s | bits %s'
                  % (name, m, n, (m + 127) // 128 * (n // 256), lo[128], med[128], hi128, lo[256], med[256], max(times[256]),
                     (med[256] / med[128] - 1) * 100, flops_per_mn * m * n / med[256] * 1e-9, verdict, 'equal' if same else 'DIFFER'), flush=True)
    os.environ.pop('OPA_X3_TILE', None)


if __name__ == '__main__':
    main()
