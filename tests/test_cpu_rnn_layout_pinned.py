"""The LSTM learner's scratch and exchange-buffer sizes, pinned: the learner
allocates by smi_ppo_rnn_scratch_bytes / smi_ppo_rnn_xbuf_floats and the phases
carve by the same formulas (csrc/rnn_layout.hpp), so a change that moves a
region or a parameter count must show here.  tests/golden/rnn_layout_pinned.json
holds the sizes of the commit it names (one crc32 per (B, T, horizon) over the
rest of the sweep); `python tests/test_cpu_rnn_layout_pinned.py --write COMMIT`
regenerates it from the library of the tree on sys.path (on purpose only: it
re-pins).  Neither entry point touches the device."""
import itertools
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'rnn_layout_pinned.json')

BS, TS = (1, 9, 19, 128, 1024), (1, 6, 25)
DS, HS, LS = (0, 1, 11, 42, 128), (0, 16, 100, 256), (1, 2, 3)
HEADS = ((1, 1), (30, 18), (32, 32), (300, 200), (520, 32))
AS, FS = (1, 4, 8, 32), (0, 64)
CAM = (3, 84, 84)                # the camera of tests/test_gpu_cnn.py


def _inner(T, Hz):
    """The shapes smi_ppo_rnn_phase accepts at (T, horizon), in a fixed order."""
    for D, H, L, (h1, h2), A, F in itertools.product(DS, HS, LS, HEADS, AS, FS):
        if (L > 1 and H == 0) or (D == 0 and F == 0) or (H == 0 and Hz != T):
            continue
        yield D, H, L, h1, h2, A, F


def _record(B, T, Hz):
    """-> [shapes, crc32 of their (scratch bytes, xbuf floats) as int64]."""
    from surreal_amd import _lib
    lib = _lib.lib()
    out = []
    for D, H, L, h1, h2, A, F in _inner(T, Hz):
        pc, ph, pw = CAM if F else (0, 0, 0)
        out.append(lib.smi_ppo_rnn_scratch_bytes(B, T, Hz, D, H, h1, h2, A, h1, h2, pc, ph, pw, F, L))
        out.append(lib.smi_ppo_rnn_xbuf_floats(D, H, h1, h2, A, h1, h2, pc, ph, pw, F, L))
    a = np.asarray(out, dtype=np.int64)
    assert (a > 0).all()
    return [len(a) // 2, zlib.crc32(a.tobytes())]


def _cases():
    return {f'B{B}/T{T}/Hz{Hz}': (B, T, Hz) for B in BS for T in TS for Hz in sorted({1, T})}


def test_sizes_match_the_pinned_commit():
    with open(GOLDEN) as f:
        gold = json.load(f)
    cases = _cases()
    assert sorted(gold['sizes']) == sorted(cases)
    bad = [name for name, case in cases.items() if _record(*case) != gold['sizes'][name]]
    assert not bad, f'{len(bad)} size tables differ from commit {gold["commit"]}: {bad[:8]}'


if __name__ == '__main__':
    if len(sys.argv) not in (2, 3) or sys.argv[1] != '--write':
        sys.exit('usage: test_cpu_rnn_layout_pinned.py --write [COMMIT]   (default: this checkout\'s HEAD)')
    sys.path.append(os.path.dirname(HERE))
    if len(sys.argv) == 2:
        import subprocess
        sys.argv.append(subprocess.check_output(['git', '-C', HERE, 'rev-parse', 'HEAD'], text=True).strip())
    sizes = {name: _record(*case) for name, case in _cases().items()}
    with open(GOLDEN, 'w') as f:
        f.write('{"commit": %s,\n "sizes": {\n' % json.dumps(sys.argv[2]))
        f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in sizes.items()))
        f.write('\n }}\n')
    from surreal_amd import _lib
    print(f'{len(sizes)} size tables of {sys.argv[2]} ({_lib.LIB_PATH}) written to {GOLDEN}')
