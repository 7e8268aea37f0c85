"""Variant 4 of the Winograd kernel (csrc/winograd.hip: F(2x2, 3x3) on the bf16 MFMA pipe with exactly split operands) beside
variant 2 (float32 MFMA): error against a float64 convolution (max and rms over the output's largest magnitude) on a small
batch, then time per launch on the ResNet-50 shapes at 641 px / batch 32.
    python tools/gpu/winograd_x3_probe.py [--batch 32] [--reps 20] [--diag] [--bn 64|128] [--rounds 7]
--bn: instead of all that, variant 4 on its 64-channel and on its 128-channel workgroups (OPA_WINO_X3_BN, which the launcher
reads on every launch), alternated in this process: --rounds rounds of --reps launches each, min / median / max of the rounds'
ms per launch, the given width named first (the one a counter pass wants first); bits compared.
--diag: also variant 4's timing experiments (wrong results) from a library built with -DOPA_WINO_DIAG
(lib/libopenpifpaf_amd_winodiag.so, built here if it is not there): 21 no split, 22 the leading products only,
23 no pixel fetches / transforms."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--diag', action='store_true')
ap.add_argument('--bn', type=int, choices=(64, 128))
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--order', type=int, default=0, choices=(0, 1), help='--bn: the workgroup order (1: channel block major)')
ap.add_argument('--channels', type=int, nargs='*', default=[64, 128, 256, 512])
args = ap.parse_args()
if args.diag:
    from openpifpaf_amd import build  # noqa: E402
    diag_lib = os.path.join(os.path.dirname(build.OUT), 'libopenpifpaf_amd_winodiag.so')
    os.environ['OPA_LIB_PATH'] = diag_lib if os.path.exists(diag_lib) else build.build_diagnostic('OPA_WINO_DIAG=1', 'winodiag', source='winograd.hip')

import torch  # noqa: E402
from openpifpaf_amd import winograd  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from winograd_probe import time_ms  # noqa: E402


def errors(y, ref):
    d = y.double() - ref
    s = ref.abs().max().item()
    return d.abs().max().item() / s, d.pow(2).mean().sqrt().item() / s


SHAPES = [(C, H) for (C, H) in ((64, 321), (128, 161), (256, 81), (512, 41)) if C in args.channels]


def bn_ab(C, H):
    """One shape on both workgroup widths, alternated round by round."""
    w = torch.randn((C, C, 3, 3), device='cuda') * (2.0 / (9 * C)) ** 0.5
    u3 = winograd.split_filter(w)
    x = torch.randn((args.batch, C, H, H), device='cuda').contiguous(memory_format=torch.channels_last)
    widths = [bn for bn in (args.bn, 192 - args.bn) if C % bn == 0]
    outs = {bn: torch.empty_like(x) for bn in widths}
    times = {bn: [] for bn in widths}
    for _ in range(args.rounds):
        for bn in widths:
            os.environ['OPA_WINO_X3_BN'] = str(bn)
            times[bn].append(time_ms(lambda: winograd.conv3x3_x3(x, u3, C, order=args.order, out=outs[bn]), args.reps))
    del os.environ['OPA_WINO_X3_BN']
    line = 'C %3d %3dx%3d B%d WGs %5d' % (C, H, H, args.batch, winograd.workgroups(x.shape, C, 4))
    for bn in sorted(widths):
        t = sorted(times[bn])
        line += ' | %3d: min %.4f med %.4f max %.4f' % (bn, t[0], t[len(t) // 2], t[-1])
    if len(widths) == 2:
        t64, t128 = sorted(times[64]), sorted(times[128])
        med = t128[len(t128) // 2]
        line += ' | med/med %+5.1f %% %s | bits %s' % (100.0 * (med / t64[len(t64) // 2] - 1.0),
                                                     'WIDE BELOW THE NARROW MINIMUM' if med < t64[0] else 'not below the narrow minimum',
                                                     'equal' if torch.equal(outs[64].view(torch.int32), outs[128].view(torch.int32)) else 'DIFFER')
    print(line, flush=True)


if args.bn:
    print('# B %d, order %d, %d rounds of %d launches per width, alternating; ms per launch' % (args.batch, args.order, args.rounds, args.reps), flush=True)
    for (C, H) in SHAPES:
        bn_ab(C, H)
    sys.exit(0)

for (C, H) in SHAPES:
    w = torch.randn((C, C, 3, 3), device='cuda') * (2.0 / (9 * C)) ** 0.5
    u, u3 = winograd.transform_filter(w, 2), winograd.split_filter(w)
    xs = torch.randn((2, C, H, H), device='cuda').contiguous(memory_format=torch.channels_last)
    ref = torch.nn.functional.conv2d(xs.double(), w.double(), padding=1)
    e2 = errors(winograd.conv3x3(xs, u, C, variant=2), ref)
    e4 = errors(winograd.conv3x3_x3(xs, u3, C), ref)
    del ref
    x = torch.randn((args.batch, C, H, H), device='cuda').contiguous(memory_format=torch.channels_last)
    out = torch.empty_like(x)
    t2 = time_ms(lambda: winograd.conv3x3(x, u, C, variant=2, out=out), args.reps)
    t4 = time_ms(lambda: winograd.conv3x3_x3(x, u3, C, out=out), args.reps)
    line = ('C %3d %3dx%3d B%d: v2 %.3f ms (max %.2e rms %.2e) | v4 %.3f ms (max %.2e rms %.2e) | v4/v2 %.3f'
            % (C, H, H, args.batch, t2, e2[0], e2[1], t4, e4[0], e4[1], t4 / t2))
    if args.diag:
        for variant, name in ((21, 'no split'), (22, 'leading products only'), (23, 'no fetches / transforms')):
            line += ' | %s %.3f ms' % (name, time_ms(lambda: winograd.conv3x3_x3(x, u3, C, variant=variant, out=out), args.reps))
    print(line, flush=True)
