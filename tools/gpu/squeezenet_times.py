"""Forward time of the SqueezeNet trunk (with the cocokp heads) at 641 px, batch 32 and batch 1, float32 channels-last on one
MI355X: the Fire / pool route on the project's kernels (``OPA_FIRE=1``) against the same optimized model's plain torch / MIOpen
forward (the default until this has been run; what a PyTorch-ROCm user gets), alternating in one process.  Device events around
``--steps`` forwards after ``--warmup`` of each; ``--rounds`` rounds give the spread.  Then every Fire shape of the trunk alone, route
on against route off in the same manner, with the bytes the module has to move (input read once + output written) per second.
One JSON line per measurement; a run's output is kept in ``profiles/squeezenet/times.log``.

    python tools/gpu/squeezenet_times.py                        # the trunk at both batches, then the eight Fire shapes at each
    python tools/gpu/squeezenet_times.py --batches 32 --no-fires
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu/squeezenet_times.py --batches 32 --routes on --rounds 1 --steps 1 --no-fires
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from openpifpaf_amd import fused, headmeta, network  # noqa: E402


def alternate(fn, routes, steps, warmup, rounds):
    """``fn()`` timed with the route on and off alternately -> ({route: [ms per call, one per round]}, {route: last output})."""
    times, outs = {route: [] for route in routes}, {}
    with torch.no_grad():
        for route in routes:                            # warm up every shape of both routes (code objects, MIOpen's search)
            fused.FIRE = route == 'on'
            for _ in range(warmup):
                outs[route] = fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for route in routes:
                fused.FIRE = route == 'on'
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(steps):
                    fn()
                end.record()
                end.synchronize()
                times[route].append(start.elapsed_time(end) / steps)
    return times, outs


def median(values):
    return sorted(values)[len(values) // 2]


def fire_shapes(size):
    """(backbone index, (in, squeeze, e1, e3), rows = columns of its input) for every Fire of the trunk at ``size`` px."""
    hw, shapes = size, []
    for i, m in enumerate(network.SqueezeNet().backbone):
        if isinstance(m, torch.nn.Conv2d):
            hw = (hw - 1) // 2 + 1
        elif isinstance(m, torch.nn.MaxPool2d):
            hw = fused.maxpool3x3_out_hw(hw, hw, True)[0]
        elif isinstance(m, network._Fire):
            shapes.append((i, (m.squeeze.in_channels, m.squeeze.out_channels, m.expand1x1.out_channels, m.expand3x3.out_channels), hw))
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--routes', nargs='+', default=['on', 'off'], choices=['on', 'off'])
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-fires', action='store_true', help='the whole trunk only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    net = network.optimize_for_inference_(network.factory('squeezenet', list(headmeta.cocokp_metas())))
    net = net.cuda().to(memory_format=torch.channels_last)
    for batch in args.batches:
        x = torch.randn(batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
        times, outs = alternate(lambda: net(x), args.routes, args.steps, args.warmup, args.rounds)
        delta = None
        if len(outs) == 2:                                  # the two routes compute the same fields (reordered float32 sums)
            delta = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(outs['on'], outs['off']))
        for route in args.routes:
            ms = median(times[route])
            print(json.dumps({'model': 'squeezenet', 'route': route, 'batch': batch, 'size': args.size, 'steps': args.steps,
                              'ms_per_batch_median': ms, 'ms_per_batch_all': times[route], 'images_per_s': 1e3 * batch / ms,
                              'max_rel_delta_on_vs_off': delta}), flush=True)
    if args.no_fires:
        return
    for batch in args.batches:
        for index, cfg, hw in fire_shapes(args.size):
            fire = net.base_net.backbone[index]
            x = torch.relu(torch.randn(batch, cfg[0], hw, hw, device='cuda')).contiguous(memory_format=torch.channels_last)
            # (a single Fire is tens of microseconds: ten times the steps, so that a window is not all launch latency)
            times, outs = alternate(lambda: fire(x), args.routes, 10 * args.steps, args.warmup, args.rounds)
            delta = float((outs['on'] - outs['off']).abs().max()) / float(outs['off'].abs().max()) if len(outs) == 2 else None
            moved = 4 * batch * hw * hw * (cfg[0] + cfg[2] + cfg[3])
            for route in args.routes:
                ms = median(times[route])
                print(json.dumps({'fire': 'backbone.%d' % index, 'config': cfg, 'input': [batch, cfg[0], hw, hw], 'route': route,
                                  'ms_median': ms, 'ms_all': times[route], 'TB_per_s_in_plus_out': moved / ms / 1e9,
                                  'max_rel_delta_on_vs_off': delta}), flush=True)


if __name__ == '__main__':
    main()
