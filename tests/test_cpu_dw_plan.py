"""The grouped weight-gradient launch's plan (smi_diag_dw_plan: host arithmetic
only, no device call): every GEMM cut into full 64 x 64 tiles, an M edge, an N
edge and their corner with edge tiles fitted to the remainder, each rectangle
with balanced split-K slabs.  For a sweep of shapes the plan must tile the
output exactly once, slice the rows exactly once in whole prefetch windows, and
keep its workgroup / reducer prefixes and partial offsets consistent."""
import ctypes
import itertools

import numpy as np
import pytest

from surreal_amd import _lib

MS = (1, 8, 16, 17, 64, 72, 90, 108, 128, 200, 300, 400)
NS = (16, 79, 91, 101, 128, 143, 201, 301)
KS = (513, 1100, 21504)
SLOTS = 768                      # 256 CUs x 3 resident workgroups (the C3 launch)
CAP = 1 << 26                    # floats of workspace
RED_BLOCK = 256                  # elements per reducer block (64 x 4)
F = ('gi', 'm0', 'n0', 'M', 'N', 'mt', 'nt', 'kchunk', 'S', 'wg0', 'rb0', 'part_off')


def _plan(gemms, waves=4, slots=SLOTS, cap=CAP, max_ent=16):
    """gemms: [(M, N, K, vec, ones, split_col)] -> (entries as dicts, totals)."""
    lib = _lib.lib()
    lib.smi_diag_dw_plan.restype = ctypes.c_int
    lib.smi_diag_dw_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    g = np.asarray(gemms, dtype=np.int32).reshape(-1, 6).copy()
    out = np.zeros((16, 12), dtype=np.int64)
    tot = np.zeros(4, dtype=np.int64)
    n = lib.smi_diag_dw_plan(g.ctypes.data, len(g), waves, slots, cap, max_ent, out.ctypes.data,
                             tot.ctypes.data)
    assert n > 0, lib.smi_last_error().decode()
    return [dict(zip(F, map(int, out[i]))) for i in range(n)], [int(t) for t in tot]


def _check(gemms, ents, tot, waves):
    rs = tot[3]
    assert rs == 16 * waves                      # 4 rows x waves x 4 steps in flight
    cover = [np.zeros((g[0], g[1]), dtype=np.int32) for g in gemms]
    wg, rb, spans = 0, 0, []
    for e in ents:
        M, N, K, _, ones, _ = gemms[e['gi']]
        assert e['M'] >= 1 and e['N'] >= 1
        assert e['m0'] >= 0 and e['n0'] >= 0 and e['m0'] + e['M'] <= M and e['n0'] + e['N'] <= N
        cover[e['gi']][e['m0']:e['m0'] + e['M'], e['n0']:e['n0'] + e['N']] += 1
        # tile class and the conditions the fitted loads rely on
        assert 1 <= e['mt'] <= 4 and 1 <= e['nt'] <= 4
        if e['mt'] in (2, 3):                    # a clamped run of mt rows ends at M
            assert e['m0'] + e['M'] == M and e['M'] <= 16 * e['mt'] and e['M'] >= e['mt']
        if e['nt'] < 4:                          # fitted N edge: one tile, the bias column in a lane of its own
            assert e['n0'] + e['N'] == N and e['N'] <= 16 * e['nt']
            data = e['N'] - (1 if ones else 0)
            assert data == 0 or data >= e['nt']
            assert -(-data // e['nt']) + (1 if ones else 0) <= 16
        # slabs cover [0, K) exactly once in whole prefetch windows
        assert e['S'] >= 1 and e['kchunk'] % rs == 0
        assert (e['S'] - 1) * e['kchunk'] < K <= e['S'] * e['kchunk']
        # prefixes
        gm, gn = -(-e['M'] // (16 * e['mt'])), -(-e['N'] // (16 * e['nt']))
        assert e['wg0'] == wg and e['rb0'] == rb
        wg += gm * gn * e['S']
        rb += -(-(e['M'] * e['N']) // RED_BLOCK)
        spans.append((e['part_off'], e['part_off'] + e['S'] * e['M'] * e['N']))
    assert tot[0] == wg and tot[1] == rb
    for c in cover:
        assert (c == 1).all()
    spans.sort()
    assert spans[0][0] >= 0 and spans[-1][1] <= tot[2] <= CAP
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0
    return wg


@pytest.mark.parametrize('waves', [4, 8])
@pytest.mark.parametrize('K', KS)
def test_plan_sweep(K, waves):
    for M, N, ones, vec in itertools.product(MS, NS, (0, 1), (15, 0)):
        gemms = [(M, N, K, vec, ones, -1)]
        ents, tot = _plan(gemms, waves=waves)
        assert len(ents) <= 4
        _check(gemms, ents, tot, waves)


def test_plan_fits_edges_to_sixteen():
    """the C3 head layer 1 (300 x 101 with the bias column): 4 x 4 interior,
    3-sub-tile M and N edges and their corner."""
    ents, _ = _plan([(300, 101, 21504, 15, 1, -1)])
    got = sorted((e['m0'], e['n0'], e['M'], e['N'], e['mt'], e['nt']) for e in ents)
    assert got == [(0, 0, 256, 64, 4, 4), (0, 64, 256, 37, 4, 3),
                   (256, 0, 44, 64, 3, 4), (256, 64, 44, 37, 3, 3)]
    # the 8-wave launch cuts off a <= 16-row tail only
    ents, _ = _plan([(200, 301, 21504, 15, 1, -1)], waves=8)
    got = sorted((e['m0'], e['n0'], e['M'], e['N'], e['mt'], e['nt']) for e in ents)
    assert got == [(0, 0, 192, 301, 4, 4), (192, 0, 8, 301, 1, 4)]


def test_plan_two_source_edge():
    """[x | h] with the sources split at column 44: an N edge wholly in the
    second source is fitted; one that would straddle the split keeps 4-wide tiles
    unless a lane holds a single column."""
    ents, _ = _plan([(400, 145, 21504, 15, 1, 44)])
    assert {(e['n0'], e['nt']) for e in ents} == {(0, 4), (128, 2)}
    ents, _ = _plan([(400, 100, 21504, 15, 1, 80)])     # edge 64..99 straddles column 80
    assert {(e['n0'], e['nt']) for e in ents} == {(0, 4), (64, 4)}
    ents, _ = _plan([(400, 76, 21504, 15, 1, 70)])      # 11 data columns + bias: one per lane
    assert {(e['n0'], e['nt']) for e in ents} == {(0, 4), (64, 1)}


def test_plan_c3_group_is_one_round():
    """the four GEMMs of a C3 backward phase: 14 entries, one resident round."""
    gemms = [(8, 201, 21504, 15, 1, -1), (200, 301, 21504, 15, 1, -1), (300, 101, 21504, 15, 1, -1),
             (400, 145, 21504, 15, 1, 44)]
    ents, tot = _plan(gemms)
    assert len(ents) == 14
    assert _check(gemms, ents, tot, 4) <= SLOTS
    # with room for fewer entries the later GEMMs stay whole (padded tiles)
    ents, tot = _plan(gemms, max_ent=6)
    assert len(ents) <= 6
    _check(gemms, ents, tot, 4)


def test_plan_slabs_follow_row_bands():
    """Slab lengths decide which rows an element sums in one chain, so every
    rectangle takes the slabs of its row band (the full 64-row tiles, or a cut
    <= 16-row tail with its longer slabs): fitting an edge never moves a slab
    boundary.  The C3 group: the 200- and 400-row GEMMs' tails are cut, the
    300-row one (44-row remainder) and the 8-row one are one band each."""
    gemms = [(8, 201, 21504, 15, 1, -1), (200, 301, 21504, 15, 1, -1), (300, 101, 21504, 15, 1, -1),
             (400, 145, 21504, 15, 1, 44)]
    ents, _ = _plan(gemms)
    bands = {}
    for e in ents:
        M = gemms[e['gi']][0]
        tail = M > 64 and 1 <= M % 64 <= 16 and e['m0'] == M // 64 * 64
        bands.setdefault((e['gi'], tail), set()).add((e['kchunk'], e['S']))
    assert all(len(v) == 1 for v in bands.values()), bands
    assert sorted(bands) == [(0, False), (1, False), (1, True), (2, False), (3, False), (3, True)]
    for gi in (1, 3):                                  # a tail's slabs are the longer ones
        assert min(bands[(gi, True)])[0] > min(bands[(gi, False)])[0]
    # with room for fewer entries (later GEMMs cut less or not at all) the slabs stay
    ents8, _ = _plan(gemms, max_ent=8)
    for e in ents8:
        M = gemms[e['gi']][0]
        tail = M > 64 and 1 <= M % 64 <= 16 and e['m0'] == M // 64 * 64
        assert {(e['kchunk'], e['S'])} == bands[(e['gi'], tail)]
