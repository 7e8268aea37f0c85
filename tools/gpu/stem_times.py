"""Times of the RGB stem route (``fused.STEM``, ``csrc/stem.hip``) at 641 px, batch 32 and batch 1, float32 channels-last on one MI355X.

1. The KERNEL against what ships for the same layer -- ``act(conv(x))`` of the folded torch modules (MIOpen's convolution, then torch's
   in-place activation) -- for each of the five stems: 16 channels / stride 1 / hardswish (MobileNetV3), 24 / 2 / ReLU (shufflenetv2k16,
   ShuffleNetV2), 32 / 2 / ReLU6 (MobileNetV2; shufflenetv2k20 .. 44 have the same convolution with a ReLU), 42 / 2 / ReLU
   (shufflenetv2kx5), 64 / 2 / ReLU (SqueezeNet).  Per case the algorithmic bytes -- the input once plus the output once --, the
   bytes/s that makes of the kernel's time, and that rate's share of the 6.29 TB/s float4 copy rate measured on this GPU
   (``MI355X_MICROARCH.md``: HBM3E, 8.0 TB/s by specification): a share of the measured copy rate, not of the specification's peak.
   At batch 1 input and output (at most 6.6 MB) stay in the caches; the rate is given all the same and is not an HBM rate.
   ``faster``: the kernel's slowest round is faster than torch's fastest round -- the difference exceeds the spread of this run's
   own rounds.
2. The WHOLE TRUNK with heads, ``STEM`` on against off, the family's own switch on: mobilenetv2 (``MBV2``), shufflenetv2k16,
   mobilenetv3large (``MBV3``), squeezenet (``FIRE``).

Device events around ``--steps`` calls after ``--warmup`` of each side; both sides alternate in one process, ``--rounds`` rounds give
the spread.  One JSON line per case.

    python tools/gpu/stem_times.py                               # everything
    python tools/gpu/stem_times.py --parts kernel --batches 32
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from openpifpaf_amd import fused, headmeta, network  # noqa: E402

COPY_RATE = 6.29e12        # bytes/s, float4 copy measured on an MI355X (MI355X_MICROARCH.md)
# stem -> (output channels, stride, the network's non-linearity)
STEMS = {'mobilenetv3': (16, 1, lambda: nn.Hardswish(inplace=True)), 'shufflenetv2k16': (24, 2, lambda: nn.ReLU(inplace=True)),
         'mobilenetv2': (32, 2, lambda: nn.ReLU6(inplace=True)), 'shufflenetv2kx5': (42, 2, lambda: nn.ReLU(inplace=True)),
         'squeezenet': (64, 2, lambda: nn.ReLU(inplace=True))}
# model -> the family's own switch (None: its units are decided by the choice table and by size)
TRUNKS = {'mobilenetv2': 'MBV2', 'shufflenetv2k16': None, 'mobilenetv3large': 'MBV3', 'squeezenet': 'FIRE'}


def _rounds(sides, steps, warmup, rounds):
    """``sides``: {name: callable}.  -> {name: [ms per call, one per round]}, the sides alternating inside every round."""
    times = {name: [] for name in sides}
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in sides.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(steps):
                fn()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) / steps)
    return times


def _median(v):
    return sorted(v)[len(v) // 2]


def kernel_cases(args):
    for name, (channels, stride, make_act) in STEMS.items():
        torch.manual_seed(0)
        conv = nn.Conv2d(3, channels, 3, stride, 1).cuda().to(memory_format=torch.channels_last).requires_grad_(False)
        nonlin = make_act()
        act, param = network._stem_act(nonlin)
        for batch in args.batches:
            x = torch.randn(batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
            assert fused.stem_conv3x3_supported(conv, x)
            with torch.no_grad():
                times = _rounds({'kernel': lambda: fused.stem_conv3x3_bias_act(conv, x, act=act, act_param=param),
                                 'torch': lambda: nonlin(conv(x))}, args.kernel_steps, args.warmup, args.rounds)
                ours, theirs = fused.stem_conv3x3_bias_act(conv, x, act=act, act_param=param), nonlin(conv(x))
            delta = float((ours - theirs).abs().max()) / float(theirs.abs().max())
            ho, wo = fused.stem_conv_out_hw(args.size, args.size, stride)
            nbytes = 4 * batch * (3 * args.size * args.size + channels * ho * wo)
            rate = nbytes / (_median(times['kernel']) * 1e-3)
            print(json.dumps({'part': 'kernel', 'stem': name, 'channels': channels, 'stride': stride, 'act': act, 'batch': batch, 'size': args.size,
                              'steps': args.kernel_steps, 'kernel_ms_median': _median(times['kernel']), 'kernel_ms_all': times['kernel'],
                              'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'],
                              'faster': max(times['kernel']) < min(times['torch']),
                              'algorithmic_bytes': nbytes, 'kernel_bytes_per_s': rate, 'share_of_measured_copy_rate': rate / COPY_RATE,
                              'max_rel_delta_kernel_vs_torch': delta}), flush=True)
            del x, ours, theirs


def trunk_cases(args):
    for name, switch in TRUNKS.items():
        if name not in args.models:
            continue
        torch.manual_seed(0)
        net = network.optimize_for_inference_(network.factory(name, list(headmeta.cocokp_metas()))).cuda().to(memory_format=torch.channels_last)
        if switch:
            setattr(fused, switch, True)
        for batch in args.batches:
            x = torch.randn(batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
            outs = {}

            def side(on):
                def run():
                    fused.STEM = on
                    outs[on] = net(x)
                return run
            with torch.no_grad():
                times = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
            fused.STEM = False
            delta = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(outs[True], outs[False]))
            print(json.dumps({'part': 'trunk', 'model': name, 'switch': switch, 'batch': batch, 'size': args.size, 'steps': args.steps,
                              'stem_on_ms_median': _median(times['on']), 'stem_on_ms_all': times['on'],
                              'stem_off_ms_median': _median(times['off']), 'stem_off_ms_all': times['off'],
                              'max_rel_delta_on_vs_off': delta}), flush=True)
            del x, outs
        if switch:
            setattr(fused, switch, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['kernel', 'trunk'], choices=['kernel', 'trunk'])
    ap.add_argument('--models', nargs='+', default=list(TRUNKS), choices=list(TRUNKS))
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=5, help='forwards per round of a whole trunk')
    ap.add_argument('--kernel-steps', type=int, default=50, help='calls per round of the stem alone')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    if 'kernel' in args.parts:
        kernel_cases(args)
    if 'trunk' in args.parts:
        trunk_cases(args)


if __name__ == '__main__':
    main()
