"""The load plan of the bf16 two-source GEMM (``csrc/gemm2_bf16_plan.hpp``, the header ``csrc/gemm2_bf16.hip`` takes every global
address of ``A1`` and ``x`` from) touches no byte outside either tensor: ``tests/host/gemm2_bf16_plan_main.cpp`` -- a stand-alone
program with its own ``main`` -- is compiled with g++ and the address and undefined-behaviour sanitizers (their runtimes linked
statically, so that it needs nothing preloaded and runs in the inherited environment as it is) and run.  It makes every access of every
thread of every workgroup against an ``A1`` and an ``x`` whose allocations end at their last byte, for (batch, h_in, w_in, stride,
(k1, k2)) in {(3, 23, 19, 1, (64, 64)), (3, 23, 19, 2, (128, 192)), (2, 7, 5, 2, (0, 128)), (1, 1, 1, 2, (64, 64))}, and checks that
every (row < M, K chunk) is fetched exactly once from the right source and offset, that no access is made for a row >= M, and that
the staged 128 x 64 tile equals the plainly computed concatenated matrix with zeros in the rows from M on."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tests', 'host', 'gemm2_bf16_plan_main.cpp')
HEADER_DIR = os.path.join(ROOT, 'openpifpaf_amd', 'csrc')

LAUNCHES = ((3, 23, 19, 1, 64, 64), (3, 23, 19, 2, 128, 192), (2, 7, 5, 2, 0, 128), (1, 1, 1, 2, 64, 64))   # batch, h, w, s, k1, k2


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ is needed to build the plan checker')
    exe = str(tmp_path_factory.mktemp('gemm2_bf16_plan') / 'gemm2_bf16_plan_main')
    # (the sanitizers' runtimes linked statically: the program runs in whatever environment the test inherits, which it leaves alone)
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
           '-static-libubsan', '-Wall', '-Wextra', '-Werror', '-I', HEADER_DIR, SOURCE, '-o', exe]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return exe


def _counts():
    """(fetches, tile rows behind M) of the program's launches, counted from the definition: per output pixel (k1 + k2) / 8 chunks."""
    fetched = dead = 0
    for b, h, w, s, k1, k2 in LAUNCHES:
        m = b * ((h - 1) // s + 1) * ((w - 1) // s + 1)
        fetched += m * (k1 + k2) // 8
        dead += -m % 128
    return fetched, dead


def test_the_plan_fetches_every_chunk_of_every_row_once_and_nothing_else(program):
    proc = subprocess.run([program], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, (proc.stdout[-4000:], proc.stderr[-4000:])
    assert 'AddressSanitizer' not in proc.stderr and 'runtime error' not in proc.stderr, proc.stderr[-4000:]
    m = re.search(r'gemm2_bf16_plan: (\d+) launches, (\d+) fetches, (\d+) rows behind M left alone, 0 failures', proc.stdout)
    assert m, proc.stdout[-2000:]
    launches, fetches, dead = map(int, m.groups())
    assert launches == len(LAUNCHES)
    assert (fetches, dead) == _counts() and dead > 0


def test_the_kernel_takes_its_addresses_from_the_plan():
    """The kernel has no global access to ``A1`` or ``x`` of its own: every one is an ``emit`` of the header."""
    with open(os.path.join(HEADER_DIR, 'gemm2_bf16.hip')) as f:
        kernel = f.read()
    assert '#include "gemm2_bf16_plan.hpp"' in kernel
    assert kernel.count('gemm2_bf16_plan_rows(') == 1 and kernel.count('gemm2_bf16_plan_a(') == 1
    body = kernel.split('gemm2_bf16_kernel(')[1].split('long long gemm2_bf16_workgroups')[0]
    assert 'ra[p] = *reinterpret_cast<const u32x4_t*>((source == kGemm2Bf16A1 ? A1 : x) + at);' in body       # inside the emit alone
    assert len(re.findall(r'\bA1\b', body)) == 2 and len(re.findall(r'(?<![.\w])x\b', body)) == 2      # the parameter and the emit
    assert not re.findall(r'\b(A1|x)\[', body)
