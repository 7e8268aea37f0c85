"""The load plan of the bf16 unit-mode GEMM (``csrc/unit_bf16_plan.hpp``, the header ``csrc/gemm_unit_bf16.hip`` takes every global
address of A, the partner and the residual from) touches no byte outside its operands: ``tests/host/unit_bf16_plan_main.cpp`` -- a
stand-alone program with its own ``main`` -- is compiled with g++ and the address and undefined-behaviour sanitizers (their runtimes
linked statically, so that it needs nothing preloaded and runs in the inherited environment as it is) and run.  It makes every access of every thread of a launch against an operand whose allocation ends with its last byte, for
m in {1, 127, 128, 129, 1311}, k (n) in {2, 24, 62, 64, 66, 174}, pitch in {k, k + 2, 2 k} and base addresses 0 / 4 / 8 / 12 mod 16, and
checks that every byte of the columns below k of every row is fetched exactly once per N-tile pass and no other byte ever, that no
access leaves [a, a + ((m - 1) pitch + k) 2), that none is wider than its address is aligned or than the launch's width, and that the
staged tile holds the operand where it exists and zeros from column k on.  The same for the partner / residual plan."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tests', 'host', 'unit_bf16_plan_main.cpp')
HEADER_DIR = os.path.join(ROOT, 'openpifpaf_amd', 'csrc')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ is needed to build the plan checker')
    exe = str(tmp_path_factory.mktemp('unit_bf16_plan') / 'unit_bf16_plan_main')
    # (the sanitizers' runtimes linked statically: the program runs in whatever environment the test inherits, which it leaves alone)
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
           '-static-libubsan', '-Wall', '-Wextra', '-Werror', '-I', HEADER_DIR, SOURCE, '-o', exe]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return exe


def test_the_plan_fetches_every_byte_once_and_none_outside(program):
    proc = subprocess.run([program], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, (proc.stdout[-4000:], proc.stderr[-4000:])
    assert 'AddressSanitizer' not in proc.stderr and 'runtime error' not in proc.stderr, proc.stderr[-4000:]
    m = re.search(r'unit_bf16_plan: (\d+) operands \(width 16: (\d+), 8: (\d+), 4: (\d+)\), 0 failures', proc.stdout)
    assert m, proc.stdout[-2000:]
    total, w16, w8, w4 = map(int, m.groups())
    assert total == 5 * 6 * 3 * 4 == w16 + w8 + w4 and min(w16, w8, w4) > 0              # every width is chosen by some launch


def test_the_kernel_takes_its_addresses_from_the_plan():
    """The kernel has no global access to A or to the partner / residual of its own: every one is an ``emit`` of the header."""
    with open(os.path.join(HEADER_DIR, 'gemm_unit_bf16.hip')) as f:
        kernel = f.read()
    assert '#include "unit_bf16_plan.hpp"' in kernel
    assert kernel.count('unit_bf16_plan_a<W_A>(') == 2 and kernel.count('unit_bf16_plan_third<WN>(') == 2
    body = kernel.split('gemm_unit_bf16_kernel(')[1].split('hipError_t launch_gemm_unit_act_bf16')[0]
    assert len(re.findall(r'\bA \+', body)) == 1 and 'const unsigned short* src = A + at;' in body          # inside load_a alone
    assert len(re.findall(r'\bthird \+', body)) == 1 and 'third + at' in body
