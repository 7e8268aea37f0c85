"""The ShuffleNetV2K options at 641 px on one MI355X, float32 channels-last, each against torch's own route, alternating in one process
like ``resnet_variant_times.py`` (warm-up of both sides, windows of at least ``--window-ms`` of device time between two events,
``--rounds`` windows per side: median and spread):

* ``layer``:  one depthwise convolution per (kernel width, dilation) the stencil accepts, on the stride-8 map of a dilated stage 4
  (696 channels, 81 x 81; stride 2: 348 channels, 81 -> 41) -- side A torch's grouped convolution with the folded bias (MIOpen),
  side B ``fused.dwconv_bias_act``.  A ``VERDICT`` line per combination: where B is slower than A, ``fused.DW_DECLINED`` must name it.
* ``net-<variant>``:  the whole trunk + cocokp heads -- side A the same network's torch forward, NOT optimised (batch norms
  unfolded, every convolution torch's), side B ``optimize_for_inference_`` with every decision the shipped defaults make (nothing
  forced, nothing timed: the units decide by the table, else by size).  Variants: shufflenetv2k16 by default (for scale), with
  ``stage4_dilation=2``, ``kernel_width`` 3 and 7, ``conv5_as_stage``; shufflenetv2k30 with ``stage4_dilation=2``.

Every (step, batch) runs in a process of its own under a time limit of its own; the first that fails or runs out of time ends the
run.  Everything printed is also written to ``profiles/shufflenetv2k_options/times.log``.

    python tools/gpu/shufflenetv2k_option_times.py                              # every step, batch 32 and batch 1
    python tools/gpu/shufflenetv2k_option_times.py --step layer --batch 32      # one step, in this process
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, 'profiles', 'shufflenetv2k_options', 'times.log')
NETS = {
    'net-k16-default': ('shufflenetv2k16', {}),
    'net-k16-dilation2': ('shufflenetv2k16', dict(stage4_dilation=2)),
    'net-k30-dilation2': ('shufflenetv2k30', dict(stage4_dilation=2)),
    'net-k16-kernel3': ('shufflenetv2k16', dict(kernel_width=3)),
    'net-k16-kernel7': ('shufflenetv2k16', dict(kernel_width=7)),
    'net-k16-conv5-stage': ('shufflenetv2k16', dict(conv5_as_stage=True)),
}
STEPS = dict({'layer': 240}, **{name: 240 for name in NETS})                    # step -> seconds it may take


def window_ms(fn, reps):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(sides, rounds, min_window_ms):
    """``sides``: {name: fn}.  Warm-up of each, then ``rounds`` windows of each in turn -> {name: [ms per call]}."""
    import torch
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


def line(what, t, a='A', b='B'):
    ma, mb = med(t[a]), med(t[b])
    print('%s | A %.3f ms (spread %.3f) | B %.3f ms (spread %.3f) | A / B %.2f' % (
        what, ma, max(t[a]) - min(t[a]), mb, max(t[b]) - min(t[b]), ma / mb), flush=True)
    return ma, mb


def step_layer(args):
    import torch
    from torch import nn
    from openpifpaf_amd import fused
    size = (args.size - 1) // 8 + 1
    combos = [(k, 1, d) for d in (2, 4, 1) for k in (3, 5, 7)] + [(7, 2, 1), (5, 2, 1)]
    declined = fused.DW_DECLINED
    fused.DW_DECLINED = frozenset()                                             # measure every combination, the declined ones too
    for k, s, d in combos:
        C = 696 if s == 1 else 348
        conv = nn.Conv2d(C, C, k, s, k // 2 * d, d, groups=C).cuda().to(memory_format=torch.channels_last).requires_grad_(False)
        h = torch.randn(args.batch, C, size, size, device='cuda').contiguous(memory_format=torch.channels_last)
        taps = fused.depthwise_taps(conv.weight)
        assert fused.dwconv_supported(h, k, s, d)
        with torch.no_grad():
            a, b = conv(h), fused.dwconv_bias_act(h, taps, conv.bias, k, s, dilation=d)
            delta = float((a - b).abs().max()) / float(a.abs().max())
            assert a.shape == b.shape and delta < 1e-5, delta
            del a, b
            t = alternate({'A': lambda: conv(h), 'B': lambda: fused.dwconv_bias_act(h, taps, conv.bias, k, s, dilation=d)},
                          args.rounds, args.window_ms)
        ho = (size - 1) // s + 1
        ma, mb = line('layer k %d stride %d dilation %d, %d channels, %d x %d, batch %d: A torch conv, B stencil' % (k, s, d, C, size, size, args.batch), t)
        nbytes = 4.0 * args.batch * C * (size * size + ho * ho)
        print('    %.0f MB read + written once: B %.2f TB/s' % (nbytes / 1e6, nbytes / mb / 1e9))
        print('    VERDICT k %d dilation %d stride %d batch %d: the stencil is %s torch\'s convolution (%.2f x)%s' % (
            k, d, s, args.batch, 'at least as fast as' if mb <= ma else 'SLOWER than', ma / mb,
            '; declined by fused.DW_DECLINED' if (k, d) in declined else ''), flush=True)
        del h, conv
        torch.cuda.empty_cache()


def step_net(args):
    import copy
    import torch
    from openpifpaf_amd import headmeta, network
    name, options = NETS[args.step]
    torch.manual_seed(1)
    base = network.ShuffleNetV2K(name, **options)
    net = network.Shell(base, [network.CompositeField4(m, base.out_features) for m in headmeta.cocokp_metas()]).eval()
    plain = copy.deepcopy(net).cuda().to(memory_format=torch.channels_last)
    opt = network.optimize_for_inference_(net).cuda().to(memory_format=torch.channels_last)
    x = torch.randn(args.batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        a, b = plain(x), opt(x)
        delta = max(float((u - v).abs().max()) / float(u.abs().max()) for u, v in zip(a, b))
        del a, b
        t = alternate({'A': lambda: plain(x), 'B': lambda: opt(x)}, args.rounds, args.window_ms)
    what = ' '.join('%s=%s' % kv for kv in options.items()) or 'default'
    line('%s %s, stride %d, %d px, batch %d: A torch forward, B HIP route' % (name, what, base.stride, args.size, args.batch), t)
    print('    largest difference between the two outputs, relative to the largest value: %.2e' % delta, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', choices=list(STEPS), help='run this one step in this process (default: every step, a process each)')
    ap.add_argument('--steps', nargs='+', choices=list(STEPS), default=list(STEPS))
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--append', action='store_true', help='add to the log instead of starting it')
    args = ap.parse_args()
    assert args.rounds >= 5, 'at least five windows per side'
    if args.step:
        import torch
        assert torch.cuda.is_available(), 'needs a GPU'
        return (step_layer if args.step == 'layer' else step_net)(args)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, 'a' if args.append else 'w') as log:
        for step in args.steps:
            for batch in args.batches:
                cmd = ['timeout', '-k', '10', str(STEPS[step]), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(batch),
                       '--size', str(args.size), '--rounds', str(args.rounds), '--window-ms', str(args.window_ms)]
                proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                for out in proc.stdout:                                         # (line by line: a long step is seen to be alive)
                    sys.stdout.write(out)
                    sys.stdout.flush()
                    log.write(out)
                    log.flush()
                status = proc.wait()
                if status != 0:                                                 # a fault, an abort or the time limit: nothing more runs
                    msg = 'step %s batch %d ended with status %d: stopping\n' % (step, batch, status)
                    sys.stdout.write(msg)
                    log.write(msg)
                    return status
    return 0


if __name__ == '__main__':
    sys.exit(main())
