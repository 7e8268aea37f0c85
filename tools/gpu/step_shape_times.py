"""Per-shape kernel times of steady-state bench steps from a ``rocprofv3 --kernel-trace --output-format csv`` run of ``bench.py``:
launches grouped by kernel AND grid size (i.e. by shape), averaged over the last STEPS timed steps -- a step is the stretch between
two consecutive association-kernel launches that holds a whole network forward -- with the lowest and highest per-step average as
the row's spread.  With two trace directories the second is printed beside the first, rows matched by the LAUNCH ORDER inside a
step (a shape that moved to another kernel or grid keeps its row).

    python tools/gpu/step_shape_times.py TRACE_DIR [TRACE_DIR_2] [--steps 6] [--only gemm_f32x3]
"""
import argparse
import csv
import glob
import os
import re
from collections import OrderedDict


def short(name):
    name = re.sub(r'^void ', '', name)
    name = re.sub(r'\(.*$', '', name)
    return name if len(name) <= 88 else name[:85] + '...'


def grid_of(r):
    for key in ('Grid_Size', 'Grid_Size_X'):
        if r.get(key):
            return int(r[key]) * int(r.get('Grid_Size_Y') or 1) * int(r.get('Grid_Size_Z') or 1)
    return 0


def steps_of(trace_dir, nsteps):
    paths = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    assert paths, 'no kernel_trace.csv under ' + trace_dir
    rows = list(csv.DictReader(open(paths[0])))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    idx = [i for i, r in enumerate(rows) if 'cifcaf_assoc' in r['Kernel_Name']]
    pairs = [(a, b) for a, b in zip(idx, idx[1:]) if b - a > 40]
    assert len(pairs) >= nsteps + 2, 'too few steps in the trace: %d' % len(pairs)
    steps = []
    for a, b in pairs[-nsteps - 1:-1]:
        seg = rows[a + 1:b + 1]
        steps.append([(short(r['Kernel_Name']), grid_of(r), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3) for r in seg])
    return steps


def table(steps):
    """-> OrderedDict (kernel, grid) -> (launches per step, mean us, lowest and highest per-step mean), in first-launch order;
    and per step the sum of kernel time in ms"""
    per_step = []
    for seg in steps:
        groups = OrderedDict()
        for name, grid, us in seg:
            groups.setdefault((name, grid), []).append(us)
        per_step.append(groups)
    out = OrderedDict()
    for key in per_step[-1]:
        means = [sum(g[key]) / len(g[key]) for g in per_step if key in g]
        out[key] = (len(per_step[-1][key]), sum(means) / len(means), min(means), max(means))
    return out, [sum(us for _, _, us in seg) / 1e3 for seg in steps]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('traces', nargs='+')
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--only', default=None, help='substring a kernel name must hold')
    args = ap.parse_args()
    tables = []
    for d in args.traces[:2]:
        t, sums = table(steps_of(d, args.steps))
        tables.append(t)
        print('%s: %d steady-state steps; sum of kernel time per step %s ms\n'
              % (os.path.basename(os.path.normpath(d)), args.steps, ' '.join('%.2f' % s for s in sums)))
    if len(tables) == 1:
        print('| kernel | grid | launches per step | avg us per launch | min..max of the per-step average |\n|---|---|---|---|---|')
        for (name, grid), (n, mean, lo, hi) in sorted(tables[0].items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            if not args.only or args.only in name:
                print('| `%s` | %d | %d | %.1f | %.1f..%.1f |' % (name, grid, n, mean, lo, hi))
        return
    # two traces: the i-th distinct (kernel, grid) of a step in launch order is the same layer group in both
    a, b = (list(t.items()) for t in tables)
    print('| first: kernel, grid | launches | avg us (min..max) | second: kernel, grid | launches | avg us (min..max) | second - first, us per step |\n|---|---|---|---|---|---|---|')
    total = 0.0
    if len(a) != len(b) or any(x[1][0] != y[1][0] for x, y in zip(a, b)):
        print('(the two steps do not have the same launch groups: printed one after the other)')
        for t in tables:
            for (name, grid), (n, mean, lo, hi) in t.items():
                print('| `%s`, %d | %d | %.1f (%.1f..%.1f) |' % (name, grid, n, mean, lo, hi))
        return
    for ((n1, g1), (c1, m1, lo1, hi1)), ((n2, g2), (c2, m2, lo2, hi2)) in zip(a, b):
        total += c2 * m2 - c1 * m1
        if args.only and args.only not in n1 and args.only not in n2:
            continue
        print('| `%s`, %d | %d | %.1f (%.1f..%.1f) | `%s`, %d | %d | %.1f (%.1f..%.1f) | %+.0f |'
              % (n1, g1, c1, m1, lo1, hi1, n2 if (n2, g2) != (n1, g1) else 'same', g2, c2, m2, lo2, hi2, c2 * m2 - c1 * m1))
    print('\nsum over every launch group of the step: %+.2f ms' % (total / 1e3))


if __name__ == '__main__':
    main()
