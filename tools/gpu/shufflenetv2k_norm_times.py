"""Times of the group-norm route of ``ShuffleNetV2K(layer_norm='group')`` (``fused.GN``, ``csrc/groupnorm.hip``) at 641 px, batch 32 and
batch 1, float32 channels-last on one MI355X.

1. The KERNELS (three launches: moments, coefficients, apply) against what runs without the switch for the same layer -- torch's
   ``nn.GroupNorm`` followed by its in-place ReLU on the same channels-last tensor -- for every (channels, groups, pixels) layer of
   shufflenetv2k16 and of shufflenetv2k20 / 30 / 44.  Per case the algorithmic bytes -- 12 per element: two reads and one write --, the
   bytes/s that makes of the kernels' time, and that rate's share of the 6.29 TB/s float4 copy rate measured on this GPU
   (``MI355X_MICROARCH.md``): a share of the measured copy rate, not of the specification's peak.  At batch 1 the small layers stay in
   the caches; the rate is given all the same and is not an HBM rate.  ``faster``: the kernels' slowest round is faster than torch's
   fastest round.  With ``--launches`` the three launches are also timed one by one (the library's profile marks).
2. The WHOLE NETWORK, trunk + heads, of group-norm shufflenetv2k16 and shufflenetv2k30: ``GN`` and ``STEM`` on against both off.

Device events around ``--steps`` calls after ``--warmup`` of each side; both sides alternate in one process, ``--rounds`` rounds give
the spread.  Every case runs in a child process of its own under a ``timeout`` of its own, and the first case that fails ends the run;
one JSON line per case, appended to ``profiles/shufflenetv2k_norms/times.log``.

    python tools/gpu/shufflenetv2k_norm_times.py                               # everything
    python tools/gpu/shufflenetv2k_norm_times.py --parts kernel --batches 32
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
from openpifpaf_amd import fused, headmeta, network  # noqa: E402

COPY_RATE = 6.29e12        # bytes/s, float4 copy measured on an MI355X (MI355X_MICROARCH.md)
LOG = os.path.join(ROOT, 'profiles', 'shufflenetv2k_norms', 'times.log')
# network -> its five widths; the layers are (width, side of the feature map as a divisor of the input's): the stem's norm, and per
# stage the norms of the first unit in front of and behind its stride, at the branch width and (branch1's first norm) at the input's
WIDTHS = {'shufflenetv2k16': (24, 174, 348, 696, 1392), 'shufflenetv2k30': (32, 256, 512, 1024, 2048)}
TRUNKS = ('shufflenetv2k16', 'shufflenetv2k30')


def layers(name, size):
    """-> [(channels, groups, side)] of the network's group norms at a ``size`` x ``size`` input, each once."""
    c0, c2, c3, c4, c5 = WIDTHS[name]
    s1 = (size - 1) // 2 + 1
    s2, s3, s4 = (s1 - 1) // 2 + 1, ((s1 - 1) // 2) // 2 + 1, (((s1 - 1) // 2) // 2) // 2 + 1
    out = [(c0, s1), (c0, s2), (c2, s1), (c2, s2), (c3, s2), (c3, s3), (c4, s3), (c4, s4), (c5, s4)]
    return [(c, (32 if c % 32 == 0 else 29) if c > 100 else 4, s) for c, s in out]


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


def _launches(norm, x, out, reps=20):
    """-> {kernel: median ms} of the three launches, from the library's own profile marks."""
    from openpifpaf_amd import _lib
    per = {}
    for _ in range(reps):
        _lib.profile_begin(torch.cuda.current_stream().cuda_stream)
        fused.group_norm_act(norm, x, act=fused.ACT_RELU, out=out)
        for name, ms in _lib.profile_end():
            per.setdefault(name, []).append(ms)
    return {name: _median(v) for name, v in per.items()}


def kernel_case(args, name, index, batch):
    channels, groups, side = layers(name, args.size)[index]
    torch.manual_seed(0)
    norm = nn.GroupNorm(groups, channels).cuda().requires_grad_(False)
    nonlin = nn.ReLU(inplace=True)
    x = (torch.randn(batch, channels, side, side, device='cuda') * 3.0 + 1.0).contiguous(memory_format=torch.channels_last)
    out = torch.empty_like(x)
    assert fused.group_norm_supported(norm, x)
    with torch.no_grad():
        times = _rounds({'kernel': lambda: fused.group_norm_act(norm, x, act=fused.ACT_RELU, out=out), 'torch': lambda: nonlin(norm(x))},
                        args.kernel_steps, args.warmup, args.rounds)
        theirs = nonlin(norm(x))
        delta = float((fused.group_norm_act(norm, x, act=fused.ACT_RELU, out=out) - theirs).abs().max()) / float(theirs.abs().max())
        launches = _launches(norm, x, out) if args.launches else None
    nbytes = 12 * x.numel()
    rate = nbytes / (_median(times['kernel']) * 1e-3)
    return {'part': 'kernel', 'network': name, 'channels': channels, 'groups': groups, 'side': side, 'batch': batch, 'size': args.size,
            'steps': args.kernel_steps, 'kernel_ms_median': _median(times['kernel']), 'kernel_ms_all': times['kernel'],
            'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'], 'faster': max(times['kernel']) < min(times['torch']),
            'slower': min(times['kernel']) > max(times['torch']), 'algorithmic_bytes': nbytes, 'kernel_bytes_per_s': rate,
            'share_of_measured_copy_rate': rate / COPY_RATE, 'max_rel_delta_kernel_vs_torch': delta, 'launch_ms': launches}


def trunk_case(args, name, batch):
    torch.manual_seed(0)
    base = network.ShuffleNetV2K(name, layer_norm='group')
    net = network.Shell(base, [network.CompositeField4(m, base.out_features) for m in headmeta.cocokp_metas()]).eval()
    net = network.optimize_for_inference_(net).cuda().to(memory_format=torch.channels_last)
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
    outs = {}

    def side(on):
        def run():
            fused.GN = fused.STEM = on
            outs[on] = net(x)
        return run
    with torch.no_grad():
        times = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
    fused.GN = fused.STEM = False
    delta = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(outs[True], outs[False]))
    return {'part': 'trunk', 'model': name, 'layer_norm': 'group', 'batch': batch, 'size': args.size, 'steps': args.steps,
            'gn_on_ms_median': _median(times['on']), 'gn_on_ms_all': times['on'], 'gn_off_ms_median': _median(times['off']),
            'gn_off_ms_all': times['off'], 'faster': max(times['on']) < min(times['off']), 'max_rel_delta_on_vs_off': delta}


def cases(args):
    """-> [case id]: 'kernel/<network>/<layer index>/<batch>' and 'trunk/<network>/<batch>'"""
    out = []
    if 'kernel' in args.parts:
        out += ['kernel/%s/%d/%d' % (name, i, b) for name in args.models for i in range(len(layers(name, args.size))) for b in args.batches]
    if 'trunk' in args.parts:
        out += ['trunk/%s/%d' % (name, b) for name in args.models for b in args.batches]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['kernel', 'trunk'], choices=['kernel', 'trunk'])
    ap.add_argument('--models', nargs='+', default=list(TRUNKS), choices=list(TRUNKS))
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=5, help='forwards per round of a whole network')
    ap.add_argument('--kernel-steps', type=int, default=20, help='calls per round of one norm alone')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', action='store_true', help='time the three launches one by one as well')
    ap.add_argument('--case-timeout', type=int, default=120, help='seconds a case may take')
    ap.add_argument('--log', default=LOG)
    ap.add_argument('--case', help='(a child process:) run this one case and print its line')
    args = ap.parse_args()
    if args.case:
        assert torch.cuda.is_available(), 'needs a GPU'
        part, name, *rest = args.case.split('/')
        line = kernel_case(args, name, int(rest[0]), int(rest[1])) if part == 'kernel' else trunk_case(args, name, int(rest[0]))
        print(json.dumps(line), flush=True)
        return 0
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    passed = [a for a in sys.argv[1:]]
    with open(args.log, 'a') as log:
        for case in cases(args):
            cmd = ['timeout', '-k', '10', str(args.case_timeout), sys.executable, os.path.abspath(__file__)] + passed + ['--case', case]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:                     # a fault, an abort, a time limit: nothing more is started on this GPU
                print('%s: exit status %d\n%s' % (case, proc.returncode, proc.stderr[-2000:]), file=sys.stderr, flush=True)
                return proc.returncode
            line = proc.stdout.strip().split('\n')[-1]
            print(line, flush=True)
            log.write(line + '\n')
            log.flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
