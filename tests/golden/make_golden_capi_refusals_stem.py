"""Generates tests/golden/capi_refusals_stem.json: per row of tests/test_capi_refusals_stem.py the status and the message of
``opa_stem3x3_actp``, recorded from the library as it is built in the checkout this is run from, in a child process that sees no GPU.

Before anything is written: a refused row has the status OPA_ERR_INVALID_ARGUMENT (on a machine without a GPU, a row that slips past
the checks into the launcher answers OPA_ERR_HIP, "no ROCm-capable device is detected") and an empty row OPA_OK
(``test_capi_refusals_stem.check_kinds``).

    python tests/golden/make_golden_capi_refusals_stem.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import test_capi_refusals_stem as tcr                     # noqa: E402


def main():
    got = tcr.run_in_child()
    tcr.check_kinds(got)
    with open(tcr.GOLDEN, 'w') as f:                      # (one row per line: a difference reads as one line of a diff)
        f.write('{"rows": {\n')
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(got[k])) for k in sorted(got)))
        f.write('\n}}\n')
    print('wrote %s: %d rows, %d distinct messages' % (tcr.GOLDEN, len(got), len({m for _, m in got.values() if m})))


if __name__ == '__main__':
    main()
