"""Times of the bf16 unit-mode GEMM route of a ShuffleNetV2K cast to bfloat16 (``fused.UNIT_BF16``, ``csrc/gemm_unit_bf16.hip``) at 641 px,
batch 32 and batch 1, channels-last on one MI355X.

1. The KERNEL against what runs without the switch for the same layer -- torch's bfloat16 ``nn.Conv2d`` (with the folded bias)
   followed by its in-place ReLU -- for every distinct 1x1 layer of shufflenetv2k16 and shufflenetv2k30: per stage the two
   convolutions in front of the shuffle of a first unit (on the stage's dense input, before and behind the stride), the first
   convolution of a later unit (its operand the upper channel half of the unit's input: a slice), the last one (stored into the
   shuffled position next to the pass-through half, the partner), then ``conv5`` and, for k16, the two heads (K = 1392; k30's heads
   have K = 2048 and keep their route).  For a layer with a partner torch's side is also given with the interleave pass the kernel
   saves (``fused.channel_interleave``).  ``faster``: the kernel's slowest round is faster than torch's fastest round; ``slower``: the
   reverse.
2. The WHOLE NETWORK, trunk + heads, of shufflenetv2k16 and shufflenetv2k30 in bfloat16: the route on against off; the float32
   network on its own routes (the split-operand unit mode where the shipped table takes it) for context.
3. REPEATABILITY (``--parts repeat``; not a time): the networks of ``tests/test_gpu_unit_bf16_routes.py`` (random BatchNorm statistics,
   optimized, bfloat16, input 2 x 3 x 97 x 65, seeds 0 and 1), route on and off: how many DIFFERENT results (bit patterns) 20 calls
   give, per part and with its input held fixed -- the input block, the stages + ``conv5`` from one input-block output, each head from
   one trunk output, the whole forward.  One JSON line per (network, seed, route), appended to ``profiles/unit_bf16/repeatability.log``.

Device events around a window of calls after ``--warmup`` of each side; the sides alternate in one process, ``--rounds`` rounds give
the spread, medians are reported.  A window of the kernel part is ``--kernel-steps`` calls or as many as fill ``--kernel-window-ms``
on the faster side, whichever is more (``steps`` of the line): at batch 1 a call is 0.01 - 0.04 ms, and twenty of them would time the
clock.  The times are device events AROUND the calls, launch overhead included, on one unchanged input -- at batch 1 the operands
stay in the caches for both sides.  Every (part, network, batch) runs in a child process of its own under a ``timeout`` of its own,
and the first that fails ends the run; one JSON line per layer or network, appended to ``profiles/unit_bf16/times.log``.

    python tools/gpu/unit_bf16_times.py                               # everything
    python tools/gpu/unit_bf16_times.py --parts kernel --batches 32
    python tools/gpu/unit_bf16_times.py --parts repeat
"""
import argparse
import json
import os
import subprocess
import sys

import torch
from torch import nn

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
from openpifpaf_amd import fused, network  # noqa: E402

LOG = os.path.join(ROOT, 'profiles', 'unit_bf16', 'times.log')
REPEAT_LOG = os.path.join(ROOT, 'profiles', 'unit_bf16', 'repeatability.log')
# network -> (stem width, the three branch widths, conv5's width)
WIDTHS = {'shufflenetv2k16': (24, 174, 348, 696, 1392), 'shufflenetv2k30': (32, 256, 512, 1024, 2048)}
HEADS = (('cif', 17 * 5 * 4), ('caf', 19 * 9 * 4))
CL = torch.channels_last
BF16 = torch.bfloat16


def layers(name, size):
    """-> [(label, K, N, side, operand, third)]: operand 'dense' | 'slice', third None | 'partner'; each distinct layer once."""
    c0, b2, b3, b4, c5 = WIDTHS[name]
    s1 = (size - 1) // 2 + 1
    sides = [s1]
    for _ in range(3):
        sides.append((sides[-1] - 1) // 2 + 1)
    out, cin = [], c0
    for stage, (b, sa, sb) in enumerate(zip((b2, b3, b4), sides[:3], sides[1:]), start=2):
        out += [('stage%d first unit, branch1' % stage, cin, b, sb, 'dense', None),
                ('stage%d first unit, branch2 first' % stage, cin, b, sa, 'dense', None),
                ('stage%d unit, first' % stage, b, b, sb, 'slice', None),
                ('stage%d unit, last' % stage, b, b, sb, 'dense', 'partner')]
        cin = 2 * b
    out.append(('conv5', cin, c5, sides[3], 'dense', None))
    if c5 % 64 != 0:
        out += [('head %s' % h, c5, n, sides[3], 'dense', 'head') for h, n in HEADS]
    return out


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
    round.  ``window_ms``: a window is at least this long on the fastest side (one trial window of ``steps`` calls per side says how
    many calls that takes; at most 20 000)."""
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


def kernel_case(args, name, index, batch):
    label, k, n, side, operand, third = layers(name, args.size)[index]
    torch.manual_seed(0)
    conv = nn.Conv2d(k, n, 1).cuda().to(BF16).requires_grad_(False)
    relu = third != 'head'
    nonlin = nn.ReLU(inplace=True) if relu else nn.Identity()

    def activation(channels):
        return torch.randn(batch, channels, side, side, device='cuda').relu_().to(BF16).contiguous(memory_format=CL)
    x = activation(2 * k)[:, k:] if operand == 'slice' else activation(k)
    partner = activation(2 * n)[:, :n] if third == 'partner' else None
    fused.UNIT_BF16 = True
    assert fused.unit_conv_bf16_supported(conv, x, partner)
    sides = {'kernel': lambda: fused.conv1x1_unit_bf16(conv, x, relu=relu, partner=partner), 'torch': lambda: nonlin(conv(x))}
    if partner is not None:
        sides['torch+interleave'] = lambda: fused.channel_interleave(partner, nonlin(conv(x)))
    with torch.no_grad():
        times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['torch+interleave' if partner is not None else 'torch']().float()
        delta = float((sides['kernel']().float() - theirs).abs().max()) / float(theirs.abs().max())
    m = batch * side * side
    line = {'part': 'kernel', 'network': name, 'layer': label, 'k': k, 'n': n, 'side': side, 'batch': batch, 'm': m, 'operand': operand,
            'third': third, 'size': args.size, 'steps': steps, 'kernel_ms_median': _median(times['kernel']),
            'kernel_ms_all': times['kernel'], 'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'],
            'faster': max(times['kernel']) < min(times['torch']), 'slower': min(times['kernel']) > max(times['torch']),
            'kernel_call_tflops': 2.0 * m * k * n / (_median(times['kernel']) * 1e-3) / 1e12,       # (of the call, launch overhead included)
            'max_rel_delta_kernel_vs_torch': delta}
    if partner is not None:
        line.update(torch_plus_interleave_ms_median=_median(times['torch+interleave']), torch_plus_interleave_ms_all=times['torch+interleave'])
    return line


def trunk_case(args, name, batch):
    net32 = network.optimize_for_inference_(network.factory(name)).cuda().to(memory_format=CL).requires_grad_(False)
    import copy
    net = copy.deepcopy(net32).to(BF16)
    x32 = torch.randn(batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=CL)
    x = x32.to(BF16)
    outs = {}

    def side(on):
        def run():
            fused.UNIT_BF16 = on
            outs[on] = net(x)
        return run

    def float32():
        fused.UNIT_BF16 = False
        outs['float32'] = net32(x32)
    with torch.no_grad():
        times, _ = _rounds({'on': side(True), 'off': side(False), 'float32': float32}, args.steps, args.warmup, args.rounds)
    fused.UNIT_BF16 = False

    def rms(which):
        num = sum(float(((a.double() - b.double()) ** 2).sum()) for a, b in zip(outs[which], outs['float32']))
        return (num / sum(float((b.double() ** 2).sum()) for b in outs['float32'])) ** 0.5
    return {'part': 'trunk', 'model': name, 'batch': batch, 'size': args.size, 'steps': args.steps,
            'bf16_route_on_ms_median': _median(times['on']), 'bf16_route_on_ms_all': times['on'],
            'bf16_route_off_ms_median': _median(times['off']), 'bf16_route_off_ms_all': times['off'],
            'float32_ms_median': _median(times['float32']), 'float32_ms_all': times['float32'],
            'faster': max(times['on']) < min(times['off']), 'slower': min(times['on']) > max(times['off']),
            'rms_error_vs_float32_on': rms(True), 'rms_error_vs_float32_off': rms(False)}


def _distinct(fn, calls):
    """-> how many different results (bit patterns of every tensor) ``calls`` calls of ``fn`` give."""
    seen = set()
    for _ in range(calls):
        out = fn()
        out = out if isinstance(out, (tuple, list)) else (out,)
        torch.cuda.synchronize()
        seen.add(tuple(t.contiguous().view(torch.uint8).cpu().numpy().tobytes() for t in out))
    return len(seen)


def repeat_case(args, name, seed):
    """The network and input of ``tests/test_gpu_unit_bf16_routes._case``.  -> one line per route (on, off)"""
    net = network.factory(name, seed=seed).cuda()
    torch.manual_seed(100 + seed)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = network.optimize_for_inference_(net).to(BF16).to(memory_format=CL).requires_grad_(False)
    x = torch.randn((2, 3, 97, 65), device='cuda').to(BF16).contiguous(memory_format=CL)
    base, lines = net.base_net, []
    with torch.no_grad():
        for on in (True, False):
            fused.UNIT_BF16 = on
            h = base._input_block_forward(x)

            def trunk(h=h):
                return network._conv5_forward(base, base.stage4(base.stage3(base.stage2(h))))
            f = trunk()
            lines.append({'part': 'repeat', 'model': name, 'seed': seed, 'route': 'on' if on else 'off', 'calls': args.repeat_calls,
                          'input': [2, 3, 97, 65], 'heads_on_the_kernel': [bool(on and hn.conv.in_channels % 64 != 0) for hn in net.head_nets],
                          'distinct_input_block': _distinct(lambda: base._input_block_forward(x), args.repeat_calls),
                          'distinct_trunk_from_one_input_block_output': _distinct(trunk, args.repeat_calls),
                          'distinct_heads_from_one_trunk_output': [_distinct(lambda hn=hn: hn(f), args.repeat_calls) for hn in net.head_nets],
                          'distinct_whole_forward': _distinct(lambda: net(x), args.repeat_calls)})
    fused.UNIT_BF16 = False
    return lines


def groups(args):
    """-> [group id]: 'kernel/<network>/<batch>', 'trunk/<network>/<batch>' and 'repeat/<network>/<seed>', each a child process"""
    out = ['%s/%s/%d' % (part, name, b) for part in ('kernel', 'trunk') if part in args.parts for name in args.models for b in args.batches]
    if 'repeat' in args.parts:
        out += ['repeat/%s/%d' % (name, seed) for name in args.models for seed in (0, 1)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['kernel', 'trunk', 'repeat'], choices=['kernel', 'trunk', 'repeat'])
    ap.add_argument('--models', nargs='+', default=list(WIDTHS), choices=list(WIDTHS))
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=5, help='forwards per round of a whole network')
    ap.add_argument('--kernel-steps', type=int, default=20, help='calls per round of one layer alone, at least')
    ap.add_argument('--kernel-window-ms', type=float, default=10.0, help='... and as many as make the faster side\'s window this long')
    ap.add_argument('--repeat-calls', type=int, default=20, help='calls per part of the repeatability count')
    ap.add_argument('--repeat-log', default=REPEAT_LOG)
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
            for index in range(len(layers(name, args.size))):
                print(json.dumps(kernel_case(args, name, index, int(batch))), flush=True)
        elif part == 'trunk':
            print(json.dumps(trunk_case(args, name, int(batch))), flush=True)
        else:
            for line in repeat_case(args, name, int(batch)):
                print(json.dumps(line), flush=True)
        return 0
    for path in (args.log, args.repeat_log):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    passed = [a for a in sys.argv[1:]]
    with open(args.log, 'a') as times_log, open(args.repeat_log, 'a') as repeat_log:
        for group in groups(args):
            log = repeat_log if group.startswith('repeat/') else times_log
            cmd = ['timeout', '-k', '10', str(args.group_timeout), sys.executable, os.path.abspath(__file__)] + passed + ['--group', group]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in proc.stdout.split('\n') if ln.startswith('{')]
            for line in lines:
                print(line, flush=True)
                log.write(line + '\n')
            log.flush()
            if proc.returncode != 0:                     # a fault, an abort, a time limit: nothing more is started on this GPU
                print('%s: exit status %d\n%s' % (group, proc.returncode, proc.stderr[-2000:]), file=sys.stderr, flush=True)
                return proc.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
