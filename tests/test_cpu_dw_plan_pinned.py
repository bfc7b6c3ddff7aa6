"""The grouped weight-gradient plans, pinned: slab lengths decide the rounding
of every weight gradient the learner produces, so a change to the planner
(csrc/dw_plan.hpp) that moves a single slab, rectangle or partial offset must
show here.  tests/golden/dw_plan_pinned.json holds the plans of the commit it
names; `python tests/test_cpu_dw_plan_pinned.py --write COMMIT` regenerates it
from the library of the tree on sys.path (on purpose only: it re-pins)."""
import ctypes
import itertools
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'dw_plan_pinned.json')
CAP = 1 << 26                    # floats of workspace

C3 = [(8, 201, 21504, 15, 1, -1), (200, 301, 21504, 15, 1, -1), (300, 101, 21504, 15, 1, -1),
      (400, 145, 21504, 15, 1, 44)]
LAUNCHES = ((4, 768), (8, 224))  # (waves, resident workgroups): the grouped launch, the BPTT's


def _cases():
    """name -> (gemms, waves, slots, max_ent, full): full rows, or one crc32."""
    cases = {}
    for K in (21504, 3200, 513):
        gemms = [(M, N, K, vec, ones, split) for M, N, _, vec, ones, split in C3]
        for (waves, slots), max_ent in itertools.product(LAUNCHES, (16, 8, 6)):
            cases[f'c3/K{K}/w{waves}/s{slots}/e{max_ent}'] = (gemms, waves, slots, max_ent, True)
    for g in ((400, 145, 21504, 15, 1, 44), (400, 100, 21504, 15, 1, 80), (400, 76, 21504, 15, 1, 70)):
        cases[f'two_source/N{g[1]}/split{g[5]}'] = ([g], 4, 768, 16, True)
    for M, N, ones, vec, K, waves in itertools.product((8, 72, 200, 300, 400), (79, 101, 145, 301),
                                                       (0, 1), (15, 0), (1100, 21504), (4, 8)):
        cases[f'single/{M}x{N}/ones{ones}/vec{vec}/K{K}/w{waves}'] = (
            [(M, N, K, vec, ones, -1)], waves, 768, 16, False)
    return cases


def _plan(gemms, waves, slots, max_ent):
    """-> (rows [n][12], totals [4]) as int64 arrays, or None when no plan fits."""
    from surreal_amd import _lib
    lib = _lib.lib()
    lib.smi_diag_dw_plan.restype = ctypes.c_int
    lib.smi_diag_dw_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    g = np.asarray(gemms, dtype=np.int32).reshape(-1, 6).copy()
    out = np.zeros((16, 12), dtype=np.int64)
    tot = np.zeros(4, dtype=np.int64)
    n = lib.smi_diag_dw_plan(g.ctypes.data, len(g), waves, slots, CAP, max_ent, out.ctypes.data,
                             tot.ctypes.data)
    return (out[:n].copy(), tot) if n > 0 else None


def _record(case):
    gemms, waves, slots, max_ent, full = case
    p = _plan(gemms, waves, slots, max_ent)
    if p is None:
        return None
    rows, tot = p
    if full:
        return {'rows': rows.tolist(), 'tot': tot.tolist()}
    return zlib.crc32(rows.tobytes() + tot.tobytes())


def test_plans_match_the_pinned_commit():
    with open(GOLDEN) as f:
        gold = json.load(f)
    cases = _cases()
    assert sorted(gold['plans']) == sorted(cases)
    bad = []
    for name, case in cases.items():
        got = _record(case)
        if got != gold['plans'][name]:
            p = _plan(*case[:4])
            shown = None if p is None else {'rows': p[0].tolist(), 'tot': p[1].tolist()}
            print(f'{name}: gemms {case[0]}\n  pinned {gold["plans"][name]}\n  got    {got}\n  plan   {shown}')
            bad.append(name)
    assert not bad, f'{len(bad)} plans differ from commit {gold["commit"]}: {bad[:8]}'


if __name__ == '__main__':
    if len(sys.argv) not in (2, 3) or sys.argv[1] != '--write':
        sys.exit('usage: test_cpu_dw_plan_pinned.py --write [COMMIT]   (default: this checkout\'s HEAD)')
    sys.path.append(os.path.dirname(HERE))
    if len(sys.argv) == 2:
        import subprocess
        sys.argv.append(subprocess.check_output(['git', '-C', HERE, 'rev-parse', 'HEAD'], text=True).strip())
    plans = {name: _record(case) for name, case in _cases().items()}
    with open(GOLDEN, 'w') as f:
        f.write('{"commit": %s,\n "plans": {\n' % json.dumps(sys.argv[2]))
        f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':')))
                           for k, v in plans.items()))
        f.write('\n }}\n')
    from surreal_amd import _lib
    print(f'{len(plans)} plans of {sys.argv[2]} ({_lib.LIB_PATH}) written to {GOLDEN}')
