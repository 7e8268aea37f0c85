"""Generates tests/golden/launch_marshalling.json: per case of tests/test_launch_marshalling.py the native calls a launcher of
``fused.py`` / ``winograd.py`` makes -- symbol, integers, and per pointer the label of the tensor it addresses -- recorded from the
launchers as they are in the checkout this is run from.  The file in the repository was written from the commit BEFORE the route
layer was rearranged (one launcher, one activation code): the test passes there and has to pass on every later commit.

Two symbols are written under another name than that commit called them by, on purpose.  ``conv1x1_unit_x3`` called
``opa_gemm_unit_bias_act_f32x3`` where it had neither ``act`` nor a residual, and ``dwconv_bias_act`` called ``opa_dwconv_bias_act``
without ``act``; both now always call the supersets ``opa_gemm_unit_act_f32x3`` / ``opa_dwconv_act``, which ``csrc/capi_trunk.hip``
forwards the old entry points to literally.  Those entries are generated from the supersets' argument lists (a null residual with
pitch 0 put in; the activation code is ``int(bool(relu))``): ``test_launch_marshalling.canonical``, applied to whatever was recorded.

    python tests/golden/make_golden_launch_marshalling.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import test_launch_marshalling as tlm                     # noqa: E402


def main():
    cases = tlm.record_all()
    with open(tlm.GOLDEN, 'w') as f:                      # (one case per line: a difference reads as one line of a diff)
        f.write('{"cases": {\n')
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(cases[k])) for k in sorted(cases)))
        f.write('\n}}\n')
    print('wrote %s: %d cases, %d calls' % (tlm.GOLDEN, len(cases), sum(len(c) for c in cases.values())))


if __name__ == '__main__':
    main()
