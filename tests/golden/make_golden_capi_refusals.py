"""Generates tests/golden/capi_refusals.json: per row of tests/test_capi_refusals.py the status and the message of the C entry
point, recorded from the library as it is built in the checkout this is run from, in a child process that sees no GPU.  The file in
the repository was written from the commit BEFORE the trunk's entry points moved into ``csrc/capi_trunk.hip`` and their twins were
folded: the test passes there and has to pass on every later commit.

One prefix is written otherwise than that commit answered, on purpose: ``opa_dwconv_act`` with the activation codes 0 / 1 was refused
under the name of ``opa_dwconv_bias_act``, which it forwarded to, and is now refused under its own
(``test_capi_refusals.canonical``, applied to whatever was recorded).

Before anything is written: a refused row has a status other than OPA_ERR_HIP (on a machine without a GPU, a row that slips past
the checks into a launcher answers OPA_ERR_HIP, "no ROCm-capable device is detected"), an empty row OPA_OK, and only the listed
Winograd-variant rows OPA_ERR_HIP (``test_capi_refusals.check_kinds``).

    python tests/golden/make_golden_capi_refusals.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import test_capi_refusals as tcr                          # noqa: E402


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
