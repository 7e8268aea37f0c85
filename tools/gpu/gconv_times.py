"""The grouped 3x3 convolutions of resnext50 (32x4d) and resnext101 (32x8d) at 641 px on one MI355X, float32 channels-last: the route
without the stencil kernel -- side A, ``fused.bias_act_(conv(x), bias)``: torch's grouped convolution (MIOpen) + the epilogue pass --
against ``fused.gconv3x3_bias_act`` (side B, ``csrc/gconv.hip``), alternating in one process.  Every shape is warmed up on both sides
(code objects, MIOpen's search); a window is at least ``--window-ms`` of device time between two events; ``--rounds`` windows per
side give the median and the spread (max - min).  Per shape: both times, the bytes (input read once + output written + the weight
operand) and FLOPs (2 * 9 * cg per output) computed from the shape, and the kernel's share of the larger of its two bounds
(6.29 TB/s measured copy rate, 157 TFLOP/s float32: ``MI355X_MICROARCH.md``).  A markdown table on stdout, then the verdict per
(group width, stride) class at batch 32: the kernel wins a class if it beats side A on every shape of the class by more than side
A's own spread.

    python tools/gpu/gconv_times.py                      # the layers, batch 32 and batch 1
    python tools/gpu/gconv_times.py --network            # a whole optimized resnext50 forward, batch 32, switch on against off
"""
import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from openpifpaf_amd import fused, headmeta, network  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
F32_FLOP_PER_S = 157e12

# (H, C, cg, stride): the grouped layers at 641 px, block2 ... block5
LAYERS = {
    'resnext50': [(321, 128, 4, 1), (321, 256, 8, 2), (161, 256, 8, 1), (161, 512, 16, 2), (81, 512, 16, 1), (81, 1024, 32, 2),
                  (41, 1024, 32, 1)],
    'resnext101': [(321, 256, 8, 1), (321, 512, 16, 2), (161, 512, 16, 1), (161, 1024, 32, 2), (81, 1024, 32, 1), (81, 2048, 64, 2),
                   (41, 2048, 64, 1)],
}


def shape_work(batch, H, C, cg, s):
    """(bytes, flops) the operation needs, from the shape alone."""
    Ho = (H - 1) // s + 1
    return 4 * (batch * H * H * C + batch * Ho * Ho * C + 9 * cg * C), 2 * 9 * cg * batch * Ho * Ho * C


def window_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(sides, rounds, min_window_ms):
    """``sides``: {name: fn}.  Warm-up of each, then ``rounds`` windows of each in turn -> {name: [ms per call]}."""
    reps = {}
    for name, fn in sides.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(3, min(400, int(min_window_ms / max(window_ms(fn, 3), 1e-3)) + 1))
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(window_ms(fn, reps[name]))
    return times


def med(v):
    return sorted(v)[len(v) // 2]


def layers(args):
    shapes = []
    for name in args.models:
        for shape in LAYERS[name]:
            if shape not in shapes:
                shapes.append(shape)
    print('| batch | H -> Ho | C | cg | stride | A: conv + bias_act ms (spread) | B: kernel ms (spread) | A / B | MB | GFLOP | bound | kernel share of bound |')
    print('|---|---|---|---|---|---|---|---|---|---|---|---|')
    verdict = {}
    for batch in args.batches:
        for H, C, cg, s in shapes:
            conv = nn.Conv2d(C, C, 3, s, 1, groups=C // cg, bias=False).cuda().to(memory_format=torch.channels_last).requires_grad_(False)
            bias = torch.randn(C, device='cuda')
            x = torch.randn(batch, C, H, H, device='cuda').contiguous(memory_format=torch.channels_last)
            assert fused.gconv3x3_supported(conv, x, bias)
            with torch.no_grad():
                a, b = fused.bias_act_(conv(x), bias), fused.gconv3x3_bias_act(conv, x, bias)
                delta = float((a - b).abs().max()) / float(a.abs().max())
                assert delta < 1e-4, delta
                del a, b
                t = alternate({'A': lambda: fused.bias_act_(conv(x), bias), 'B': lambda: fused.gconv3x3_bias_act(conv, x, bias)},
                              args.rounds, args.window_ms)
            nbytes, flops = shape_work(batch, H, C, cg, s)
            t_mem, t_alu = 1e3 * nbytes / HBM_BYTES_PER_S, 1e3 * flops / F32_FLOP_PER_S
            ma, mb = med(t['A']), med(t['B'])
            spread_a, spread_b = max(t['A']) - min(t['A']), max(t['B']) - min(t['B'])
            print('| %d | %d -> %d | %d | %d | %d | %.3f (%.3f) | %.3f (%.3f) | %.2f | %.1f | %.2f | %s | %.0f %% |' % (
                batch, H, (H - 1) // s + 1, C, cg, s, ma, spread_a, mb, spread_b, ma / mb, nbytes / 1e6, flops / 1e9,
                'HBM' if t_mem >= t_alu else 'float32 VALU', 100 * max(t_mem, t_alu) / mb), flush=True)
            if batch == 32:
                verdict.setdefault((cg, s), []).append(ma - mb > spread_a)
            del conv, x
            torch.cuda.empty_cache()
    print()
    for (cg, s), wins in sorted(verdict.items()):
        print('class cg %d stride %d at batch 32: the kernel %s' % (cg, s, 'wins' if all(wins) else 'does NOT win'))


def whole_network(args):
    net = network.factory('resnext50', list(headmeta.cocokp_metas()))
    network.optimize_for_inference_(net)
    net = net.cuda().to(memory_format=torch.channels_last)
    x = torch.randn(args.batches[0], 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
    outs = {}

    def forward(on):
        fused.GCONV = on
        outs[on] = net(x)
    with torch.no_grad():
        t = alternate({'off': lambda: forward(False), 'on': lambda: forward(True)}, args.rounds, args.window_ms)
    delta = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(outs[True], outs[False]))
    for name in ('off', 'on'):
        print('resnext50 forward, %d px, batch %d, float32, fused.GCONV %s: median %.2f ms (min %.2f, max %.2f) = %.1f images/s'
              % (args.size, args.batches[0], name, med(t[name]), min(t[name]), max(t[name]), 1e3 * args.batches[0] / med(t[name])))
    print('largest difference of a field between the two, relative to the largest field value: %.2e' % delta)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--network', action='store_true', help='time a whole optimized resnext50 forward, switch on against off')
    ap.add_argument('--models', nargs='+', default=list(LAYERS), choices=list(LAYERS))
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=200.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    assert args.rounds >= 5, 'at least five windows per side'
    fused.GCONV = True
    return whole_network(args) if args.network else layers(args)


if __name__ == '__main__':
    main()
