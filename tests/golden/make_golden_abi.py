"""Generates the golden files of the ABI-table tests (``tests/abi_tables.py``), each from the test module of its name:

    capi_refusals*.json        per row of ``tests/test_capi_refusals*.py`` the status and the message of the C entry point (group norm:
                               and the sizes ``opa_groupnorm_workspace_bytes`` answers), recorded from the library as it is built in
                               the checkout this is run from, in a child process that sees no GPU
    launch_marshalling*.json   per case of ``tests/test_launch_marshalling*.py`` the native calls a launcher makes -- symbol, integers,
                               floats, and per pointer the label of the tensor it addresses -- recorded from the launchers as they are
                               in the checkout this is run from

Before a refusal table is written it is checked against what it promises of its own rows (the test module's ``refusals``, through
``abi_tables.check_kinds``): a refused row has a status the test module allows (never OPA_ERR_HIP: on a machine without a GPU, a row
that slips past the checks into a launcher answers "no ROCm-capable device is detected"), an empty row OPA_OK, and only the listed
Winograd-variant rows OPA_ERR_HIP.

Two files in the repository were written from the commit BEFORE a rearrangement, and their tests have to pass on every later commit:
``capi_refusals.json`` from before the trunk's entry points moved into ``csrc/capi_trunk.hip`` and their twins were folded,
``launch_marshalling.json`` from before the route layer had one launcher and one activation code.  Three spellings in them are
written otherwise than those commits answered, on purpose, applied to whatever is recorded:
``opa_dwconv_act`` with the activation codes 0 / 1 was refused under the name of ``opa_dwconv_bias_act``, which it forwarded to, and is
now refused under its own (``test_capi_refusals.canonical``); ``conv1x1_unit_x3`` called ``opa_gemm_unit_bias_act_f32x3`` where it had
neither ``act`` nor a residual, and ``dwconv_bias_act`` called ``opa_dwconv_bias_act`` without ``act`` -- both now always call the
supersets ``opa_gemm_unit_act_f32x3`` / ``opa_dwconv_act``, and those entries are generated from the supersets' argument lists (a null
residual with pitch 0 put in; the activation code is ``int(bool(relu))``: ``abi_tables.canonical_call``).

    python tests/golden/make_golden_abi.py <table name> | all         (capi_refusals_actp, launch_marshalling, ...)
"""
import glob
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import abi_tables as at                                   # noqa: E402


def names():
    return sorted(os.path.basename(p)[len('test_'):-len('.py')] for kind in ('capi_refusals', 'launch_marshalling')
                  for p in glob.glob(os.path.join(TESTS, 'test_%s*.py' % kind)))


def main(name):
    module = importlib.import_module('test_' + name)
    if name.startswith('capi_refusals'):
        document = module.refusals()
    else:
        document = {'cases': module.record_all()}
    at.write_golden(module.GOLDEN, document)
    rows = list(document.values())[-1]
    print('wrote %s: %d rows' % (module.GOLDEN, len(rows)))


if __name__ == '__main__':
    if len(sys.argv) != 2 or sys.argv[1] not in names() + ['all']:
        sys.exit(__doc__)
    for table_name in names() if sys.argv[1] == 'all' else [sys.argv[1]]:
        main(table_name)
