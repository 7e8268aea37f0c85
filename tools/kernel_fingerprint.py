#!/usr/bin/env python3
"""Which kernels did a change touch?  One line per kernel symbol of the given csrc/*.hip files:

    file  mangled-name  size=<bytes of code>  sha256=<of those bytes>  vgpr= sgpr= spill= scratch= lds=

sorted, so that two runs compare line by line.  The device code is compiled exactly as the library's is (build.FLAGS)
and never run: no GPU is needed.  The bytes are the symbol's range of .text, the numbers come from the code object's
metadata note (llvm-readelf); nothing is disassembled.  Host-side changes (the order of instantiations, a launcher's
structure) move kernels around in the code object and change the file as a whole, but not a kernel's bytes: the symbol
is the granularity at which "this kernel is unchanged" can be read off.

    tools/kernel_fingerprint.py gemm_f32x3.hip gemm_f32.hip              # this tree
    tools/kernel_fingerprint.py --against ../parent gemm_f32x3.hip       # the difference to another checkout (exit 1 if any)
"""
import argparse
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openpifpaf_amd import build  # noqa: E402

READELF = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'llvm-readelf')
# the fields of a kernel's entry in the metadata note, in the order they are printed
FIELDS = (('vgpr', '.vgpr_count'), ('sgpr', '.sgpr_count'), ('spill', '.vgpr_spill_count'),
          ('scratch', '.private_segment_fixed_size'), ('lds', '.group_segment_fixed_size'))


def readelf(*args):
    return subprocess.check_output([READELF, '--wide'] + list(args), text=True)


def kernel_metadata(code_object):
    """{symbol: {field: int}} from the amdhsa.kernels list of the code object's metadata note"""
    text = readelf('--notes', code_object)
    kernels = text.split('amdhsa.kernels:', 1)[1].split('amdhsa.target:', 1)[0]
    out = {}
    for entry in re.split(r'^  - ', kernels, flags=re.M)[1:]:              # the list's items; their scalar keys are four columns in
        keys = dict(re.findall(r'^    (\.\w+):\s+(\S+)$', '    ' + entry, re.M))
        out[keys['.name']] = {short: int(keys[key]) for short, key in FIELDS}
    return out


def fingerprint(tree, name):
    """the sorted lines of one source file of `tree`"""
    src = os.path.join(tree, 'openpifpaf_amd', 'csrc', os.path.basename(name))
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, 'device.co')
        subprocess.check_call([os.environ.get('HIPCC', 'hipcc')] + build.FLAGS +
                              ['--cuda-device-only', '--no-gpu-bundle-output', '-c', src, '-o', co])
        ndx, addr, offset = re.search(r'\[\s*(\d+)\] \.text\s+PROGBITS\s+(\w+) (\w+)', readelf('--sections', co)).groups()
        addr, offset = int(addr, 16), int(offset, 16)
        meta = kernel_metadata(co)
        with open(co, 'rb') as f:
            image = f.read()
        lines = []
        for row in (line.split() for line in readelf('--dyn-syms', co).splitlines()):
            # Num: Value Size Type Bind Vis Ndx Name
            if len(row) == 8 and row[3] == 'FUNC' and row[6] == ndx and row[7] in meta:
                value, size = int(row[1], 16), int(row[2])
                code = image[offset + value - addr: offset + value - addr + size]
                lines.append('%s %s size=%d sha256=%s %s' % (
                    os.path.basename(name), row[7], size, hashlib.sha256(code).hexdigest(),
                    ' '.join('%s=%d' % (short, meta[row[7]][short]) for short, _ in FIELDS)))
        assert len(lines) == len(meta), 'kernels in the metadata without a symbol in .text'
        return sorted(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('sources', nargs='+', help='names of files under openpifpaf_amd/csrc')
    ap.add_argument('--tree', default=ROOT, help='checkout to fingerprint (default: the one this tool lies in)')
    ap.add_argument('--against', help='a second checkout: print the difference to it instead')
    args = ap.parse_args()
    trees = [args.tree] + ([args.against] if args.against else [])
    with ThreadPoolExecutor(max_workers=8) as pool:                          # the compilations are what takes the time
        done = list(pool.map(lambda job: fingerprint(*job), [(t, s) for t in trees for s in args.sources]))
    here = [line for lines in done[:len(args.sources)] for line in lines]
    if not args.against:
        print('\n'.join(here))
        return 0
    there = [line for lines in done[len(args.sources):] for line in lines]
    diff = list(difflib.unified_diff(there, here, args.against, args.tree, lineterm='', n=0))
    print('\n'.join(diff) if diff else '%d kernels, no difference' % len(here))
    return 1 if diff else 0


if __name__ == '__main__':
    sys.exit(main())
