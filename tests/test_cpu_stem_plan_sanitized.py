"""The pixel-stem planner under AddressSanitizer and UBSan:
tests/stem_plan_main.cpp (a stand-alone program over csrc/stem_plan.hpp, which
has no device or runtime call in it) sweeps specs of 1 to 4 layers with k,
stride and channels at their range ends, frames from 1x8x8 over odd sizes to
256x256, and row counts; it paints the parameter, activation and scratch
regions into arrays of the planned size (no overlap, no gap), compares the
default spec with cnn_geom's offsets and stem_fused_ok with the fused kernels'
conditions restated; built with the sanitizers and run as a child process, it
must end clean."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
# (the sanitizer runtimes linked into the program, as tests/test_cpu_conv_plan_sanitized.py does)
SAN = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
       '-static-libasan', '-static-libubsan']


def test_stem_planner_sweep_is_clean_under_asan_ubsan(tmp_path):
    trivial = tmp_path / 'trivial.cpp'
    trivial.write_text('int main() { return 0; }\n')
    try:
        ok = subprocess.run(SAN + [str(trivial), '-o', str(tmp_path / 'trivial')],
                            capture_output=True).returncode == 0
    except OSError:
        ok = False
    if not ok:
        pytest.skip('this toolchain cannot build a sanitized program')
    exe = tmp_path / 'stem_plan_main'
    cc = subprocess.run(SAN + [os.path.join(HERE, 'stem_plan_main.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'plans made' in run.stdout
