"""Writes ``tests/golden/routes16_truth.json``: what every predicate of the 16-bit MFMA routes answers over the grid of
``tests/test_routes16_truth_host.py`` (``record()``: the cases, the switch settings and the one-character answers are that module's),
from ``openpifpaf_amd/fused.py`` as it is in the checkout this is run from.

The file in the repository was written from the commit BEFORE the predicates were rearranged around ``fused.Route16`` and the shared
predicate pieces, and its test has to pass on every later commit: run this again only where a predicate's contract changes on purpose.
No GPU and no built library are needed.

    python tests/golden/make_golden_routes16.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import test_routes16_truth_host as truth                   # noqa: E402


def main():
    document = truth.record()
    with open(truth.GOLDEN, 'w') as f:
        json.dump(document, f, indent=1, sort_keys=False)
        f.write('\n')
    print('wrote %s: %s' % (truth.GOLDEN, document['about']))
    for predicate, entry in document['grid'].items():
        print('  %-34s %5d cases x %2d settings' % (predicate, entry['cases'], len(document['answers'][predicate])))


if __name__ == '__main__':
    main()
