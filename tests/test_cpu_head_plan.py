"""The fused head chains' launch planner (head_plan, csrc/smi_shapes.hpp) under
AddressSanitizer and UBSan: tests/head_plan_main.cpp (a stand-alone program
over the host-only header) sweeps rows 1 .. 70,000 and the layer widths
4 .. 512 and checks the row-tile threshold and grid against their formulas,
that LDS bytes x workgroups per CU fit a CU's 160 KiB, that the shared carve is
chosen only where it raises the workgroups per CU, and that the C3 shape
(21,504 rows, 100 -> 300 -> 200) gets three per CU in the forward (the
backward keeps its separate carve and two: sharing it measured no faster);
built with the sanitizers and run as a child process, it must end clean."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
# (the sanitizer runtimes linked into the program: nothing of theirs is preloaded)
SAN = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
       '-static-libasan', '-static-libubsan']


def test_head_plan_sweep_is_clean_under_asan_ubsan(tmp_path):
    trivial = tmp_path / 'trivial.cpp'
    trivial.write_text('int main() { return 0; }\n')
    try:
        ok = subprocess.run(SAN + [str(trivial), '-o', str(tmp_path / 'trivial')],
                            capture_output=True).returncode == 0
    except OSError:
        ok = False
    if not ok:
        pytest.skip('this toolchain cannot build a sanitized program')
    exe = tmp_path / 'head_plan_main'
    cc = subprocess.run(SAN + [os.path.join(HERE, 'head_plan_main.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'plans made' in run.stdout
