"""The load plan of the bf16 7x7 stem implicit GEMM (``csrc/stem7x7_bf16_plan.hpp``, the header ``csrc/stem7x7_bf16.hip`` takes every
global address of ``x`` from) touches no element outside ``x`` and no tap outside the image: ``tests/host/stem7x7_bf16_plan_main.cpp``
-- a stand-alone program with its own ``main`` -- is compiled with g++ and the address and undefined-behaviour sanitizers (their
runtimes linked statically, so that it needs nothing preloaded and runs in the inherited environment as it is) and run.  It makes every
access of every thread of every workgroup against an ``x`` whose allocation begins at the first addressed element and ends at the
last, for (B, h, w) in {(1, 1, 1), (1, 3, 3), (2, 7, 5), (3, 23, 19)}, stride 1 and 2 and three layouts (NCHW, channels-last, a view
cropped out of a larger channels-last image), and checks that no access leaves the allocation, that every (row, valid tap, channel)
is fetched exactly once per N-tile pass, that no padded tap, zero column of K or row from M on is fetched at all, and that the staged
128 x 64 tiles equal a plainly computed im2col in the plan's K order."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tests', 'host', 'stem7x7_bf16_plan_main.cpp')
HEADER_DIR = os.path.join(ROOT, 'openpifpaf_amd', 'csrc')
SHAPES = ((1, 1, 1), (1, 3, 3), (2, 7, 5), (3, 23, 19))
LAYOUTS = 3


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ is needed to build the plan checker')
    exe = str(tmp_path_factory.mktemp('stem7x7_bf16_plan') / 'stem7x7_bf16_plan_main')
    # (the sanitizers' runtimes linked statically: the program runs in whatever environment the test inherits, which it leaves alone)
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
           '-static-libubsan', '-Wall', '-Wextra', '-Werror', '-I', HEADER_DIR, SOURCE, '-o', exe]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    return exe


def _counts():
    """(fetches, elements of padding, zero columns of K) of the program's launches, counted from the definition: per output pixel 49
    taps of 3 channels, inside the image or not, and 192 - 147 columns that hold no tap."""
    fetched = padding = zeros = 0
    for b, h, w in SHAPES:
        for s in (1, 2):
            for oy in range((h - 1) // s + 1):
                for ox in range((w - 1) // s + 1):
                    inside = sum(0 <= s * oy - 3 + ky < h and 0 <= s * ox - 3 + kx < w for ky in range(7) for kx in range(7))
                    fetched += LAYOUTS * b * inside * 3
                    padding += LAYOUTS * b * (49 - inside) * 3
                    zeros += LAYOUTS * b * (192 - 147)
    return fetched, padding, zeros


def test_the_plan_fetches_every_valid_tap_once_and_nothing_else(program):
    proc = subprocess.run([program], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, (proc.stdout[-4000:], proc.stderr[-4000:])
    assert 'AddressSanitizer' not in proc.stderr and 'runtime error' not in proc.stderr, proc.stderr[-4000:]
    m = re.search(r'stem7x7_bf16_plan: (\d+) launches, (\d+) fetches, (\d+) elements of padding left alone, (\d+) zero columns left alone, '
                  r'0 failures', proc.stdout)
    assert m, proc.stdout[-2000:]
    launches, fetches, padding, zeros = map(int, m.groups())
    assert launches == len(SHAPES) * 2 * LAYOUTS
    assert (fetches, padding, zeros) == _counts() and padding > 0 and zeros > 0


def test_the_kernel_takes_its_addresses_from_the_plan():
    """The kernel has no global access to ``x`` of its own: every one is an ``emit`` of the header."""
    with open(os.path.join(HEADER_DIR, 'stem7x7_bf16.hip')) as f:
        kernel = f.read()
    assert '#include "stem7x7_bf16_plan.hpp"' in kernel
    assert kernel.count('stem7x7_bf16_plan_rows(') == 1 and kernel.count('stem7x7_bf16_plan_a(') == 1
    body = kernel.split('stem7x7_bf16_kernel(')[1].split('long long stem7x7_bf16_workgroups')[0]
    assert len(re.findall(r'\bx \+', body)) == 1 and '[&](int p, int slot, long long at) { ra[p][slot >> 1] |= (unsigned)*(x + at)' in body
    assert not re.findall(r'\bx\[', body) and not re.findall(r'\*\s*x\b', body.replace('__restrict__ x', ''))
