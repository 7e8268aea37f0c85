#!/bin/bash
# Counters of variant 4's two workgroup widths (csrc/winograd.hip: 64 and 128 output channels) on the 128- and 256-channel
# ResNet-50 shapes: ONE --pmc pass with --kernel-trace only, over tools/gpu/winograd_x3_probe.py --bn 128 (which alternates
# OPA_WINO_X3_BN=128 and 64 on the same operands).  Per kernel and grid: VALU instructions per MFMA instruction, the MFMA-busy
# share of the launch (SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs over GRBM_GUI_ACTIVE / 8 dies), and the clock.
#     bash tools/gpu/winograd_x3_wide_pmc.sh OUTPUT_DIR        (from the repository root; OUTPUT_DIR/wino_x3_wide_pmc is emptied first)
set -o pipefail
[ -n "$1" ] || { echo "usage: $0 OUTPUT_DIR"; exit 2; }
REPO="$PWD"; OUT="$1/wino_x3_wide_pmc"; rm -rf "$OUT"; mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv \
    -d "$OUT" -o pmc -- python "$REPO/tools/gpu/winograd_x3_probe.py" --bn 128 --channels 128 256 --rounds 2 --reps 3 \
    > "$OUT.stdout.log" 2> "$OUT.stderr.log" || { echo "rocprofv3 failed"; tail -5 "$OUT.stderr.log"; exit 1; }
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
        if 'winograd_f23_w8x3' not in n:
            continue
        key = (n.split('(')[0].replace('void ', ''), int(r.get('Grid_Size') or r.get('Grid_Size_X') or 0) // 512)
        rows[key][r['Counter_Name']].append(float(r['Counter_Value']))
        if r['Dispatch_Id'] not in seen[key] and r['Dispatch_Id'] in dur:
            seen[key].add(r['Dispatch_Id'])
            rows[key]['duration_us'].append(dur[r['Dispatch_Id']])
print('%-36s %6s %3s %9s %6s %12s %12s %10s %9s' % ('kernel', 'wgs', 'n', 'us', 'GHz', 'INSTS_VALU', 'INSTS_MFMA', 'VALU/MFMA', 'MFMA busy'))
for key in sorted(rows, key=lambda k: (k[1] if 'w8x3w' not in k[0] else k[1] - 1, k[0])):
    c = {name: sum(v) / len(v) for name, v in rows[key].items()}
    mfma = c.get('SQ_INSTS_MFMA') or float('nan')
    cycles = c.get('GRBM_GUI_ACTIVE', float('nan')) / 8.0
    print('%-36s %6d %3d %9.1f %6.2f %12.4e %12.4e %10.2f %8.1f%%'
          % (key[0].replace('opa::', ''), key[1], len(rows[key].get('SQ_INSTS_MFMA', [])), c.get('duration_us', float('nan')),
             cycles / c.get('duration_us', float('nan')) / 1e3, c.get('SQ_INSTS_VALU', float('nan')), mfma,
             c.get('SQ_INSTS_VALU', float('nan')) / mfma, 100.0 * c.get('SQ_VALU_MFMA_BUSY_CYCLES', float('nan')) / 1024.0 / cycles))
P
find "$OUT" -name '*.csv' -size +1M -delete
