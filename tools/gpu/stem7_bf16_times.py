"""Times of the bf16 7x7 stem route of a ResNet cast to bfloat16 (``fused.STEM7_BF16``, ``csrc/stem7x7_bf16.hip``) at 641 px, batch 32
and batch 1, channels-last on one MI355X.

1. The KERNEL against what runs without the switch for the same layer -- torch's bfloat16 ``nn.Conv2d`` followed by
   ``fused.bias_act_`` (the folded bias and the ReLU) -- for the stem of resnet18 / resnet50 (3 -> 64 channels, stride 2), and the
   POOLED variant (``--resnet-pool0-stride 2``): the kernel + the pool kernel without a bias against ``nn.Conv2d`` + the pool kernel
   with the bias.  ``faster``: the kernel's slowest round is faster than torch's fastest round; ``slower``: the reverse.
   ``bytes_moved``: the image read once + the output written once (+ the pool's read and write), and ``ms_at_copy_rate``: those bytes
   over the 6.29 TB/s measured copy rate -- what the layer would take if it moved its bytes and did nothing else.
2. The WHOLE NETWORK, trunk + heads, of resnet50 and resnet18 in bfloat16 with ``CONV3_BF16`` on: the stem route on against off.

The comparison is always against the route off in the same run.  Device events around a window of calls after ``--warmup`` of each
side; the sides alternate in one process, ``--rounds`` rounds give the spread, medians are reported.  Every (part, network, batch) runs
in a child process of its own under a ``timeout`` of its own, and the first that fails ends the run; one JSON line per case, appended
to ``profiles/stem7_bf16/times.log``.

    python tools/gpu/stem7_bf16_times.py                               # everything
    python tools/gpu/stem7_bf16_times.py --parts kernel --batches 32
"""
import argparse
import copy
import json
import os
import subprocess
import sys

import torch
from torch import nn

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
from openpifpaf_amd import fused, network  # noqa: E402

LOG = os.path.join(ROOT, 'profiles', 'stem7_bf16', 'times.log')
MODELS = ('resnet50', 'resnet18')
COPY_TBS = 6.29
CL = torch.channels_last
BF16 = torch.bfloat16


def _window(fn, steps):
    """-> ms per call of ``steps`` calls between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def _rounds(sides, steps, warmup, rounds, window_ms=0.0):
    """``sides``: {name: callable}.  -> ({name: [ms per call, one per round]}, calls per window), the sides alternating inside every
    round.  ``window_ms``: a window is at least this long on the fastest side (at most 20 000 calls)."""
    times = {name: [] for name in sides}
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    if window_ms > 0:
        fastest = min(_window(fn, steps) for fn in sides.values())
        steps = min(max(steps, int(window_ms / max(fastest, 1e-6)) + 1), 20000)
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(_window(fn, steps))
    return times, steps


def _median(v):
    return sorted(v)[len(v) // 2]


def kernel_case(args, batch, pooled):
    n, s = 64, 2
    torch.manual_seed(0)
    conv = nn.Conv2d(3, n, 7, s, 3, bias=False).cuda().to(BF16).requires_grad_(False)
    bias = (torch.randn(n, device='cuda') * 0.5).to(BF16)
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(BF16).contiguous(memory_format=CL)
    ho = (args.size - 1) // s + 1
    fused.STEM7_BF16 = True
    assert fused.stem7x7_bf16_supported(conv, x, bias)
    if pooled:
        assert fused.maxpool3x3_supported(torch.empty(batch, n, ho, ho, device='cuda', dtype=BF16).contiguous(memory_format=CL), bias)
        sides = {'kernel': lambda: fused.maxpool3x3_bias_act_(fused.stem7x7_bias_act_bf16(conv, x, bias, relu=True), None, relu=False),
                 'torch': lambda: fused.maxpool3x3_bias_act_(conv(x), bias, relu=True)}
    else:
        sides = {'kernel': lambda: fused.stem7x7_bias_act_bf16(conv, x, bias, relu=True),
                 'torch': lambda: fused.bias_act_(conv(x), bias, None, True)}
    with torch.no_grad():
        times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['torch']().float()
        delta = float((sides['kernel']().float() - theirs).abs().max()) / float(theirs.abs().max())
    m = batch * ho * ho
    po = (ho - 1) // 2 + 1
    moved = 2 * (x.numel() + m * n) + (2 * (m * n + batch * po * po * n) if pooled else 0)
    return {'part': 'kernel', 'pooled': pooled, 'c_out': n, 'stride': s, 'batch': batch, 'm': m, 'size': args.size, 'steps': steps,
            'kernel_ms_median': _median(times['kernel']), 'kernel_ms_all': times['kernel'],
            'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'],
            'faster': max(times['kernel']) < min(times['torch']), 'slower': min(times['kernel']) > max(times['torch']),
            'bytes_moved': moved, 'ms_at_copy_rate': moved / (COPY_TBS * 1e12) * 1e3, 'max_rel_delta_kernel_vs_torch': delta}


def trunk_case(args, name, batch):
    net = network.optimize_for_inference_(network.factory(name)).cuda().to(BF16).to(memory_format=CL).requires_grad_(False)
    net32 = copy.deepcopy(net).float()
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(BF16).contiguous(memory_format=CL)
    outs = {}
    fused.CONV3_BF16 = True                                            # on both sides

    def side(on):
        def run():
            fused.STEM7_BF16 = on
            outs[on] = net(x)
        return run
    with torch.no_grad():
        times, _ = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
        fused.STEM7_BF16 = fused.CONV3_BF16 = False
        ref = net32(x.float())

    def rms(which):
        num = sum(float(((a.double() - b.double()) ** 2).sum()) for a, b in zip(outs[which], ref))
        return (num / sum(float((b.double() ** 2).sum()) for b in ref)) ** 0.5
    return {'part': 'trunk', 'model': name, 'batch': batch, 'size': args.size, 'steps': args.steps, 'conv3_bf16': True,
            'stem7_route_on_ms_median': _median(times['on']), 'stem7_route_on_ms_all': times['on'],
            'stem7_route_off_ms_median': _median(times['off']), 'stem7_route_off_ms_all': times['off'],
            'faster': max(times['on']) < min(times['off']), 'slower': min(times['on']) > max(times['off']),
            'rms_error_vs_float32_on': rms(True), 'rms_error_vs_float32_off': rms(False)}


def groups(args):
    """-> [group id]: 'kernel/stem/<batch>' and 'trunk/<network>/<batch>', each a child process"""
    out = ['kernel/stem/%d' % b for b in args.batches] if 'kernel' in args.parts else []
    return out + ['trunk/%s/%d' % (name, b) for name in args.models for b in args.batches if 'trunk' in args.parts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['kernel', 'trunk'], choices=['kernel', 'trunk'])
    ap.add_argument('--models', nargs='+', default=list(MODELS), choices=list(MODELS))
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=5, help='forwards per round of a whole network')
    ap.add_argument('--kernel-steps', type=int, default=20, help='calls per round of the layer alone, at least')
    ap.add_argument('--kernel-window-ms', type=float, default=10.0, help='... and as many as make the faster side\'s window this long')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--group-timeout', type=int, default=240, help='seconds a child process may take')
    ap.add_argument('--log', default=LOG)
    ap.add_argument('--group', help='(a child process:) run this one group and print its lines')
    args = ap.parse_args()
    if args.group:
        assert torch.cuda.is_available(), 'needs a GPU'
        part, name, batch = args.group.split('/')
        if part == 'kernel':
            for pooled in (False, True):
                print(json.dumps(kernel_case(args, int(batch), pooled)), flush=True)
        else:
            print(json.dumps(trunk_case(args, name, int(batch))), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    passed = [a for a in sys.argv[1:]]
    with open(args.log, 'a') as log:
        for group in groups(args):
            cmd = ['timeout', '-k', '10', str(args.group_timeout), sys.executable, os.path.abspath(__file__)] + passed + ['--group', group]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            for line in (ln for ln in proc.stdout.split('\n') if ln.startswith('{')):
                print(line, flush=True)
                log.write(line + '\n')
            log.flush()
            if proc.returncode != 0:                     # a fault, an abort, a time limit: nothing more is started on this GPU
                print('%s: exit status %d\n%s' % (group, proc.returncode, proc.stderr[-2000:]), file=sys.stderr, flush=True)
                return proc.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
