"""Generates tests/golden/capi_refusals_actp.json: per row of tests/test_capi_refusals_actp.py the status and the message of the C
entry point (``opa_gemm_unit_actp_f32x3``, ``opa_dwconv_actp``, and the older entry points asked for the new activation codes),
recorded from the library as it is built in the checkout this is run from, in a child process that sees no GPU.

Before anything is written: a refused row has a status other than OPA_ERR_HIP (on a machine without a GPU, a row that slips past
the checks into a launcher answers OPA_ERR_HIP, "no ROCm-capable device is detected") and an empty row OPA_OK
(``test_capi_refusals_actp.check_kinds``).

    python tests/golden/make_golden_capi_refusals_actp.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import test_capi_refusals_actp as tcr                     # noqa: E402


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
