"""The native library takes every choice from its arguments: nothing under
surreal_amd/csrc or include reads the environment, and build.py carries the
product library and its two developer builds only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_sources_read_no_environment():
    hits = []
    for d in (os.path.join(ROOT, 'surreal_amd', 'csrc'), os.path.join(ROOT, 'include')):
        files = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs]
        assert files, d
        for path in sorted(files):
            with open(path, errors='replace') as fh:
                for no, line in enumerate(fh, 1):
                    if re.search(r'getenv', line):
                        hits.append(f'{os.path.relpath(path, ROOT)}:{no}: {line.strip()}')
    assert not hits, '\n'.join(hits)


def test_build_variants_are_product_prof_fault():
    from surreal_amd import build
    assert set(build.VARIANTS) == {None, 'prof', 'fault'}
