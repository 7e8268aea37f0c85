#!/bin/bash
# Counters of the split-operand GEMM's two tiles (csrc/gemm_f32x3.hip) on the layer-3 reduce and tail: ONE --pmc pass with
# --kernel-trace only, over tools/gpu/gemm_x3_tile_ab.py (which alternates OPA_X3_TILE=128 and 256 on the same operands).
# Per kernel and grid: instructions per MFMA instruction, MFMA busy cycles, and GRBM_GUI_ACTIVE over the launch's duration.
#     bash tools/gpu/gemm_x3_wide_pmc.sh OUTPUT_DIR          (from the repository root; OUTPUT_DIR/x3_wide_pmc is emptied first)
set -o pipefail
[ -n "$1" ] || { echo "usage: $0 OUTPUT_DIR"; exit 2; }
REPO="$PWD"; OUT="$1/x3_wide_pmc"; rm -rf "$OUT"; mkdir -p "$OUT"
SHAPES="reduce L3,tail L3" ROUNDS=2 REPS=5 timeout -k 10 300 rocprofv3 \
    --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv \
    -d "$OUT" -o pmc -- python "$REPO/tools/gpu/gemm_x3_tile_ab.py" > "$OUT.stdout.log" 2> "$OUT.stderr.log" || { echo "rocprofv3 failed"; tail -5 "$OUT.stderr.log"; exit 1; }
python - "$OUT" <<'P'
import collections, csv, glob, os, sys
out = sys.argv[1]
dur = {}
for f in glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True):
    for r in csv.DictReader(open(f)):
        dur[r['Dispatch_Id']] = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
rows = collections.defaultdict(lambda: collections.defaultdict(list))
seen = collections.defaultdict(set)
for f in glob.glob(os.path.join(out, '**', '*counter_collection.csv'), recursive=True):
    for r in csv.DictReader(open(f)):
        n = r.get('Kernel_Name', '')
        if 'gemm_f32x3' not in n:
            continue
        key = (n.split('(')[0].replace('void ', ''), r.get('Grid_Size', r.get('Grid_Size_X', '?')))
        rows[key][r['Counter_Name']].append(float(r['Counter_Value']))
        if r['Dispatch_Id'] not in seen[key] and r['Dispatch_Id'] in dur:
            seen[key].add(r['Dispatch_Id'])
            rows[key]['duration_us'].append(dur[r['Dispatch_Id']])
for key in sorted(rows):
    c = {name: sum(v) / len(v) for name, v in rows[key].items()}
    print('%s grid %s (%d launches)' % (key[0], key[1], len(rows[key].get('SQ_INSTS_MFMA', []))))
    for name in sorted(c):
        print('    %-28s %16.1f' % (name, c[name]))
    mfma = c.get('SQ_INSTS_MFMA') or float('nan')
    print('    VALU per MFMA %.3f   LDS per MFMA %.3f' % (c.get('SQ_INSTS_VALU', float('nan')) / mfma, c.get('SQ_INSTS_LDS', float('nan')) / mfma))
    if 'duration_us' in c and 'GRBM_GUI_ACTIVE' in c:
        print('    GRBM_GUI_ACTIVE / duration = %.0f cycles per us (the sum over the chip\'s dies, if the counter is summed)' % (c['GRBM_GUI_ACTIVE'] / c['duration_us']))
P
find "$OUT" -name '*.csv' -size +1M -delete
