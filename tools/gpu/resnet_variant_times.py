"""The kernels behind the ResNet options at 641 px on one MI355X, float32 channels-last (the pool in bfloat16 too), each against the
route without it, alternating in one process like ``gconv_times.py`` (warm-up of both sides, windows of at least ``--window-ms`` of
device time between two events, ``--rounds`` windows per side: median and spread):

* ``conv``:  the dilated 3x3 of block 5 (512 -> 512, d = 2, on the 81 x 81 map of ``block5_dilation=2``) -- side A
  ``fused.bias_act_(conv(h), bias)``: torch's convolution (MIOpen) + the epilogue pass, side B ``fused.conv3x3_dilated_bias_act_x3``;
* ``pool``:  the input max-pool on the stem's output (64 channels, 321 x 321) -- side A ``F.max_pool2d(fused.bias_act_(x, bias), 3, 2, 1)``,
  side B ``fused.maxpool3x3_bias_act_(x, bias, relu=True)``; and behind a stem that applied its own epilogue, ``F.max_pool2d(x, 3, 2, 1)``
  against ``fused.maxpool3x3_bias_act_(x)``;
* ``trunk-dilated`` / ``trunk-pool``:  the whole optimized resnet50 trunk with ``block5_dilation=2`` / ``pool0_stride=2``, the kernel's
  route against the other, and the route ``fused.pick`` takes by itself for the block-5 shape.

Every (step, batch) runs in a process of its own under a time limit of its own; the first that fails or runs out of time ends the
run.  Everything printed is also written to ``profiles/resnet_variants/times.log``.

    python tools/gpu/resnet_variant_times.py                       # every step, batch 32 and batch 1
    python tools/gpu/resnet_variant_times.py --step pool --batch 32   # one step, in this process
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, 'profiles', 'resnet_variants', 'times.log')
STEPS = {'conv': 180, 'pool': 180, 'trunk-dilated': 360, 'trunk-pool': 300}      # step -> seconds it may take


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


def step_conv(args):
    import torch
    from torch import nn
    from openpifpaf_amd import fused
    size = (args.size - 1) // 8 + 1                                             # the stride-8 map block 5 works on
    conv = nn.Conv2d(512, 512, 3, 1, 2, 2, bias=False).cuda().to(memory_format=torch.channels_last).requires_grad_(False)
    bias = torch.randn(512, device='cuda')
    h = torch.randn(args.batch, 512, size, size, device='cuda').relu().contiguous(memory_format=torch.channels_last)
    assert fused.conv3x3_dilated_x3_supported(conv, h, bias)
    with torch.no_grad():
        a, b = fused.bias_act_(conv(h), bias), fused.conv3x3_dilated_bias_act_x3(conv, h, bias)
        delta = float((a - b).abs().max()) / float(a.abs().max())
        assert delta < 1e-4, delta
        del a, b
        t = alternate({'A': lambda: fused.bias_act_(conv(h), bias), 'B': lambda: fused.conv3x3_dilated_bias_act_x3(conv, h, bias)},
                      args.rounds, args.window_ms)
    flops = 2.0 * 9 * 512 * 512 * args.batch * size * size
    ma, mb = line('conv 512 -> 512, d 2, %d x %d, batch %d, terms %d: A conv + bias_act, B kernel' % (size, size, args.batch, fused.X3_TERMS), t)
    print('    %.1f GFLOP of the direct form: A %.1f, B %.1f TFLOP/s' % (flops / 1e9, flops / ma / 1e9, flops / mb / 1e9))


def step_pool(args):
    import torch
    import torch.nn.functional as F
    from openpifpaf_amd import fused
    size = (args.size - 1) // 2 + 1
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(args.batch, 64, size, size, device='cuda').to(dtype).contiguous(memory_format=torch.channels_last)
        bias = (torch.randn(64, device='cuda') * 0.01).to(dtype)
        assert fused.maxpool3x3_supported(x, bias)
        with torch.no_grad():
            assert torch.equal(fused.maxpool3x3_bias_act_(x, bias, relu=True), F.max_pool2d(F.relu(x + bias.view(1, -1, 1, 1)), 3, 2, 1))
            assert torch.equal(fused.maxpool3x3_bias_act_(x), F.max_pool2d(x, 3, 2, 1))
            what = 'pool 64 ch, %d x %d, batch %d, %s' % (size, size, args.batch, str(dtype).replace('torch.', ''))
            # (side A's pass works in place: the values drift by the bias per call, the time does not depend on them)
            t = alternate({'A': lambda: F.max_pool2d(fused.bias_act_(x, bias), 3, 2, 1),
                           'B': lambda: fused.maxpool3x3_bias_act_(x, bias, relu=True)}, args.rounds, args.window_ms)
            ma, mb = line(what + ', raw stem: A bias_act + max_pool2d, B kernel', t)
            nbytes = x.numel() * x.element_size() * 1.25
            print('    %.0f MB read + written once: B %.2f TB/s' % (nbytes / 1e6, nbytes / mb / 1e9))
            if args.batch == 32:
                print('    VERDICT %s raw stem batch 32: the kernel is %s torch\'s two passes' % (
                    str(dtype).replace('torch.', ''), 'at least as fast as' if mb <= ma else 'SLOWER than'))
            t = alternate({'A': lambda: F.max_pool2d(x, 3, 2, 1), 'B': lambda: fused.maxpool3x3_bias_act_(x)}, args.rounds, args.window_ms)
            ma, mb = line(what + ', epilogue done: A max_pool2d, B kernel', t)
            if args.batch == 32:
                print('    VERDICT %s epilogue done batch 32: the kernel is %s torch\'s pool' % (
                    str(dtype).replace('torch.', ''), 'at least as fast as' if mb <= ma else 'SLOWER than'))
        del x
        torch.cuda.empty_cache()


def _trunk(**options):
    import torch
    from openpifpaf_amd import network
    base = network.Resnet('resnet50', **options).eval()
    network.optimize_for_inference_(base)
    return base.cuda().to(memory_format=torch.channels_last)


def step_trunk_dilated(args):
    import torch
    from openpifpaf_amd import fused
    base = _trunk(block5_dilation=2)
    x = torch.randn(args.batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
    size = (args.size - 1) // 8 + 1
    key = ('torch.float32/conv3d2', args.batch * size * size, 9 * 512, 512, False, False)
    outs = {}

    def forward(choice):
        fused.set_choices({key: choice})
        outs[choice] = base(x)
    with torch.no_grad():
        base(x)                                                                 # every other choice is made here, once
        torch.cuda.synchronize()
        own = fused.choices().get(key)
        print('trunk block5_dilation=2, batch %d: pick(%r) by itself -> %s' % (args.batch, key, own), flush=True)
        t = alternate({'A': lambda: forward('conv'), 'B': lambda: forward('x3')}, args.rounds, args.window_ms)
    delta = float((outs['conv'] - outs['x3']).abs().max()) / float(outs['conv'].abs().max())
    line('resnet50 trunk block5_dilation=2, %d px, batch %d: A block 5 conv + bias_act, B kernel' % (args.size, args.batch), t)
    print('    largest difference between the two outputs, relative to the largest value: %.2e' % delta)


def step_trunk_pool(args):
    import torch
    from openpifpaf_amd import fused
    base = _trunk(pool0_stride=2)
    x = torch.randn(args.batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
    real = fused.maxpool3x3_supported
    outs, blocks = {}, {}

    def kernel(on):
        fused.maxpool3x3_supported = real if on else (lambda *a, **k: False)

    def forward(on):
        kernel(on)
        outs[on] = base(x)
    try:
        with torch.no_grad():
            base(x)                                                             # every choice is made here, once (the pool kernel on)
            torch.cuda.synchronize()
            t = alternate({'A': lambda: forward(False), 'B': lambda: forward(True)}, args.rounds, args.window_ms)
            # the pool's own part: the input block on either route; and the kernel's route twice -- what lies behind the pool may go
            # through MIOpen convolutions that add partial sums with atomics, so two calls of ONE route can differ there
            for on in (False, True):
                kernel(on)
                blocks[on] = base._input_block_fused(x)
            again = base(x)
    finally:
        fused.maxpool3x3_supported = real
    line('resnet50 trunk pool0_stride=2, %d px, batch %d: A F.max_pool2d, B kernel' % (args.size, args.batch), t)
    print('    stem choice %s; the input block (stem + pool) of the two routes equal bit for bit: %s'
          % ([v for k, v in fused.choices().items() if k[0].endswith('/stempool')], torch.equal(blocks[True], blocks[False])))
    print('    trunk outputs of the two routes equal bit for bit: %s; of two calls of route B: %s'
          % (torch.equal(outs[True], outs[False]), torch.equal(outs[True], again)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', choices=list(STEPS), help='run this one step in this process (default: every step, a process each)')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=200.0)
    args = ap.parse_args()
    assert args.rounds >= 5, 'at least five windows per side'
    if args.step:
        import torch
        assert torch.cuda.is_available(), 'needs a GPU'
        return {'conv': step_conv, 'pool': step_pool, 'trunk-dilated': step_trunk_dilated, 'trunk-pool': step_trunk_pool}[args.step](args)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, 'w') as log:
        for step, limit in STEPS.items():
            for batch in args.batches:
                cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(batch),
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
