"""Generates tests/golden/launch_marshalling_unit_bf16.json: per case of tests/test_launch_marshalling_unit_bf16.py the native call that
``fused.conv1x1_unit_bf16`` makes -- the symbol, integers (the pitches among them), the parameter as a float, and per pointer the label
of the tensor it addresses -- recorded from the launcher as it is in the checkout this is run from.

    python tests/golden/make_golden_launch_marshalling_unit_bf16.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import test_launch_marshalling_unit_bf16 as tlm           # noqa: E402


def main():
    cases = tlm.record_all()
    with open(tlm.GOLDEN, 'w') as f:                      # (one case per line: a difference reads as one line of a diff)
        f.write('{"cases": {\n')
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(cases[k])) for k in sorted(cases)))
        f.write('\n}}\n')
    print('wrote %s: %d cases, %d calls' % (tlm.GOLDEN, len(cases), sum(len(c) for c in cases.values())))


if __name__ == '__main__':
    main()
