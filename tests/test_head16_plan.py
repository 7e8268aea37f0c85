"""The store plan of the 16-bit head kernel (``csrc/head16_plan.hpp``, the header ``csrc/head16.hip`` takes every output address from)
stores every element of the fields exactly once and touches no byte outside them: ``tests/host/head16_plan_main.cpp`` -- a stand-alone
program with its own ``main`` -- is compiled with g++ and the address and undefined-behaviour sanitizers (their runtimes linked
statically, so that it needs nothing preloaded and runs in the inherited environment as it is) and run.  It performs every store of
every thread of every workgroup against an output whose allocation ends at its last byte, for (B, hc, wc, F, C, us) in
{(2, 5, 7, 2, 5, 2): M = 70, one partial row tile, N = 40 inside one tile; (3, 9, 11, 3, 8, 2): M = 297, three row tiles, 32-row
blocks that cross image rows and images, N = 96; (1, 33, 4, 13, 6, 1): no upsampling, M = 132, N = 78; (1, 1, 1, 1, 5, 2): one pixel,
three of its four sub-pixels cropped; (1, 8, 16, 17, 5, 2): M = 128 exactly, N = 340, the last N-tile with 20 live columns}, and checks
that every element is stored exactly once, from the (m, n) the definition gives, that nothing is stored for m >= M, n >= N or a
cropped position, and that no offset lies outside the allocation."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tests', 'host', 'head16_plan_main.cpp')
HEADER_DIR = os.path.join(ROOT, 'openpifpaf_amd', 'csrc')

LAUNCHES = ((2, 5, 7, 2, 5, 2), (3, 9, 11, 3, 8, 2), (1, 33, 4, 13, 6, 1), (1, 1, 1, 1, 5, 2), (1, 8, 16, 17, 5, 2))   # B, hc, wc, F, C, us


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ is needed to build the plan checker')
    exe = str(tmp_path_factory.mktemp('head16_plan') / 'head16_plan_main')
    # (the sanitizers' runtimes linked statically: the program runs in whatever environment the test inherits, which it leaves alone)
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
           '-static-libubsan', '-Wall', '-Wextra', '-Werror', '-I', HEADER_DIR, SOURCE, '-o', exe]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return exe


def _counts():
    """(stores, tile rows behind M, weight rows behind N, cropped positions) of the program's launches, counted from the definition."""
    stores = dead_rows = dead_cols = cropped = 0
    for b, hc, wc, f, c, us in LAUNCHES:
        m, n = b * hc * wc, f * c * us * us
        elems = b * f * c * (hc * us - (us - 1)) * (wc * us - (us - 1))
        stores += elems
        dead_rows += -m % 128
        dead_cols += -n % 64
        cropped += m * n - elems
    return stores, dead_rows, dead_cols, cropped


def test_the_plan_stores_every_element_once_and_nothing_else(program):
    proc = subprocess.run([program], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, (proc.stdout[-4000:], proc.stderr[-4000:])
    assert 'AddressSanitizer' not in proc.stderr and 'runtime error' not in proc.stderr, proc.stderr[-4000:]
    m = re.search(r'head16_plan: (\d+) launches, (\d+) stores, (\d+) rows behind M, (\d+) columns behind N and (\d+) cropped positions left alone, '
                  r'0 failures', proc.stdout)
    assert m, proc.stdout[-2000:]
    launches, *counts = map(int, m.groups())
    assert launches == len(LAUNCHES)
    assert tuple(counts) == _counts() and min(counts) > 0


def test_the_kernel_takes_its_addresses_from_the_plan():
    """The kernel has no access to ``out`` of its own: the one there is stands inside the plan's ``emit``, at the plan's offset."""
    with open(os.path.join(HEADER_DIR, 'head16.hip')) as f:
        kernel = f.read()
    assert '#include "head16_plan.hpp"' in kernel
    assert kernel.count('head16_plan_rows(') == 1 and kernel.count('head16_plan_block(') == 1
    body = kernel.split('void head16_kernel(')[1].split('long long head16_workgroups')[0]
    emit = 'head16_plan_block(g, rows[i], n0, threadIdx.x, [&](int prow, int pcol, int at, int plane, int y, int x) {\n            out[at] = '
    assert emit in body                                                                       # inside the emit alone
    assert len(re.findall(r'\bout\b', body)) == 2 and not re.findall(r'\bout\s*\+', body)     # the parameter and the emit
    assert len(re.findall(r'\bout\[', body)) == 1
