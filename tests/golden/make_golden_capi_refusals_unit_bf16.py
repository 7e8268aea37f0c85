"""Generates tests/golden/capi_refusals_unit_bf16.json: per row of tests/test_capi_refusals_unit_bf16.py the status and the message of
``opa_gemm_unit_actp_bf16``, recorded from the library as it is built in the checkout this is run from, in a child process that sees no
GPU.

Before anything is written: a refused row has the status OPA_ERR_INVALID_ARGUMENT (on a machine without a GPU, a row that slips past
the checks into the launcher answers OPA_ERR_HIP, "no ROCm-capable device is detected") and an empty row OPA_OK
(``test_capi_refusals_unit_bf16.check_kinds``).

    python tests/golden/make_golden_capi_refusals_unit_bf16.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import test_capi_refusals_unit_bf16 as tcr                # noqa: E402


def main():
    rows = tcr.run_in_child()
    tcr.check_kinds(rows)
    with open(tcr.GOLDEN, 'w') as f:                      # (one row per line: a difference reads as one line of a diff)
        f.write('{"rows": {\n')
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(rows[k])) for k in sorted(rows)))
        f.write('\n}}\n')
    print('wrote %s: %d rows, %d distinct messages' % (tcr.GOLDEN, len(rows), len({m for _, m in rows.values() if m})))


if __name__ == '__main__':
    main()
