"""The LSTM learner's shapes and scratch carve under AddressSanitizer and UBSan:
tests/rnn_layout_main.cpp (a stand-alone program over csrc/rnn_layout.hpp, which
has no device or runtime call in it) sweeps batch, window, width, layer, head
and pixel-stem shapes and checks the carve's order, alignment and bounds; built
with the sanitizers and run as a child process, it must end clean."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
# (the sanitizer runtimes linked into the program: it then runs whatever else the
# process environment loads ahead of it, with nothing of the sanitizers' preloaded)
SAN = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
       '-static-libasan', '-static-libubsan']


def test_layout_sweep_is_clean_under_asan_ubsan(tmp_path):
    trivial = tmp_path / 'trivial.cpp'
    trivial.write_text('int main() { return 0; }\n')
    try:
        ok = subprocess.run(SAN + [str(trivial), '-o', str(tmp_path / 'trivial')],
                            capture_output=True).returncode == 0
    except OSError:
        ok = False
    if not ok:
        pytest.skip('this toolchain cannot build a sanitized program')
    exe = tmp_path / 'rnn_layout_main'
    cc = subprocess.run(SAN + ['-Wall', os.path.join(HERE, 'rnn_layout_main.cpp'), '-o', str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'shapes carved' in run.stdout
