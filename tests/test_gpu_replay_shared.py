"""Frame-shared pixel replay on the device: smi_replay_gather_shared and
smi_replay_insert_shared against numpy models, and UniformReplay /
PrioritizedReplay with replay.share_frames against the unshared replays.  A
gather moves bytes, so every comparison is exact."""
import copy
import random

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd.config import DDPG_DEFAULT_LEARNER_CONFIG, gym_env_config, pixel_env_config
from surreal_amd.replay import PrioritizedReplay, UniformReplay

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
S = 3
CHUNKS = (1, 3, 18, 9, 1, 3, 18, 9)         # 62 transitions into 7 slots: 8 wraps


def _cfg(B=64, memory_size=200, share=False, frame_slots=None):
    lc = copy.deepcopy(DDPG_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = B
    lc.replay.memory_size = memory_size
    lc.replay.sampling_start_size = 10
    lc.replay.alpha = 0.6
    lc.algo.network.target_update = {'type': 'hard', 'interval': 2}
    if share:
        lc.replay.share_frames = True
        if frame_slots:
            lc.replay.frame_slots = frame_slots
    return lc


def _env(D, A, cam, stacks=S):
    ec = pixel_env_config(D, A, cam)
    ec['frame_stacks'] = stacks
    return ec


# ------------------------------------------------------------- the kernels
def _gather(table, cols, store, fid, stack, fbytes, idx, rows_out, pix_out, pix_next_out):
    L.call('smi_replay_gather_shared', L.ptr(table), cols, L.ptr(store), L.ptr(fid), stack, fbytes,
           L.ptr(idx), idx.numel(), L.ptr(rows_out), L.ptr(pix_out), L.ptr(pix_next_out),
           L.stream(idx.device))
    torch.cuda.synchronize()


def _shared_ring(fbytes, stack, cols, slots=16, fslots=23, batch=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    store = torch.randint(0, 256, (fslots, fbytes), generator=g, dtype=torch.uint8)
    fid = torch.randint(0, fslots, (slots, 2, stack), generator=g, dtype=torch.int32)
    fid[0, 0, :] = 5                                   # a reset observation: S equal ids
    fid[0, 1, 0], fid[0, 1, -1] = 0, fslots - 1        # both ends of the store
    fid[slots - 1, 0, -1], fid[slots - 1, 1, 0] = 0, fslots - 1
    table = torch.randn(slots, cols, generator=g) if cols else None
    idx = torch.randint(0, slots, (batch,), generator=g)
    idx[0], idx[1], idx[-1], idx[-2] = 0, slots - 1, 0, slots - 1    # repeats of both ends
    return store, fid, table, idx


def _expected(store, fid, idx, side):
    return store[fid[idx, side].long()].reshape(idx.numel(), -1)


@pytest.mark.parametrize('fbytes,stack,cols', [(400, 3, 12), (21168, 3, 42), (21168, 1, 0),
                                               (35, 3, 7), (1200, 4, 12)])
def test_replay_gather_shared_abi_exact(fbytes, stack, cols):
    """(400, 3, 12): 25 vectors per frame, a side smaller than one chunk, frame
    boundaries inside a lane group; (21168, 3, 42): the 3 x 84 x 84 frame, 1,323
    vectors per frame, 3,969 per side = 3 full chunks + 897, float2 rows;
    (21168, 1, 0): no stacking, no table; (35, 3, 7): the byte path, scalar
    rows; (1200, 4, 12): the largest stack.  The outputs are one sample longer
    than the batch and pre-filled: the extra sample must come back untouched."""
    batch = 37
    store, fid, table, idx = _shared_ring(fbytes, stack, cols, batch=batch)
    dev, side = 'cuda', stack * fbytes
    pix = torch.full((batch + 1, side), SENTINEL, dtype=torch.uint8, device=dev)
    pix_next = torch.full((batch + 1, side), SENTINEL, dtype=torch.uint8, device=dev)
    rows = torch.full((batch + 1, cols), -7.0, device=dev) if cols else None
    _gather(table.to(dev) if cols else None, cols, store.to(dev), fid.to(dev), stack, fbytes,
            idx.to(dev), rows, pix, pix_next)
    assert torch.equal(pix[:batch].cpu(), _expected(store, fid, idx, 0))
    assert torch.equal(pix_next[:batch].cpu(), _expected(store, fid, idx, 1))
    assert bool((pix[batch] == SENTINEL).all()) and bool((pix_next[batch] == SENTINEL).all())
    if cols:
        assert torch.equal(rows[:batch].cpu(), table[idx])
        assert bool((rows[batch] == -7.0).all())


def test_replay_gather_shared_misaligned_falls_back():
    """pix_out 4 bytes off a 16-byte boundary: the byte path must give the same
    exact result and leave the guard bytes alone."""
    fbytes, stack, cols, batch = 400, 3, 12, 37
    store, fid, table, idx = _shared_ring(fbytes, stack, cols, batch=batch, seed=1)
    dev, side = 'cuda', stack * fbytes
    buf = torch.full((4 + (batch + 1) * side,), SENTINEL, dtype=torch.uint8, device=dev)
    pix = buf[4:].view(batch + 1, side)
    assert pix.data_ptr() % 16 == 4
    pix_next = torch.full((batch + 1, side), SENTINEL, dtype=torch.uint8, device=dev)
    rows = torch.empty(batch, cols, device=dev)
    _gather(table.to(dev), cols, store.to(dev), fid.to(dev), stack, fbytes, idx.to(dev), rows, pix,
            pix_next)
    assert torch.equal(pix[:batch].cpu(), _expected(store, fid, idx, 0))
    assert torch.equal(pix_next[:batch].cpu(), _expected(store, fid, idx, 1))
    assert torch.equal(rows.cpu(), table[idx])
    assert bool((buf[:4] == SENTINEL).all()) and bool((pix[batch] == SENTINEL).all())
    assert bool((pix_next[batch] == SENTINEL).all())


def test_replay_gather_shared_offsets_beyond_4gib():
    """A 3,600,000 x 1200 B store (4.32 GB).  Slot 3,579,139 starts at byte
    4,294,966,800 and straddles 2^32; 3,579,140 is the first wholly beyond it;
    3,599,999 is the last.  A 32-bit source offset would wrap each of them into
    the zero-filled low store.  Every marked frame is named from both sides and
    from different stack positions."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 1024 ** 3:
        pytest.skip(f'needs 6 GB of free HBM for the 4.32 GB store, {free / 1024 ** 3:.1f} GB free')
    fslots, fbytes, dev = 3600000, 1200, 'cuda'
    store = torch.zeros(fslots, fbytes, dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(2)
    m = [0, 3579139, 3579140, 3599999]
    marks = {s: torch.randint(1, 256, (fbytes,), generator=g, dtype=torch.uint8) for s in m}
    for s, f in marks.items():
        store[s] = f.to(dev)
    fid = torch.tensor([[[m[0], m[1], m[2]], [m[3], m[2], m[1]]],
                        [[m[3], m[3], m[0]], [m[1], m[0], m[3]]],
                        [[m[2], m[3], m[1]], [m[0], m[1], m[2]]],
                        [[m[1], m[0], m[3]], [m[2], m[3], m[0]]]], dtype=torch.int32)
    idx = torch.tensor([3, 0, 2, 1, 0])
    pix = torch.empty(idx.numel(), 3 * fbytes, dtype=torch.uint8, device=dev)
    pix_next = torch.empty_like(pix)
    _gather(None, 0, store, fid.to(dev), 3, fbytes, idx.to(dev), None, pix, pix_next)
    for side, out in ((0, pix), (1, pix_next)):
        exp = torch.stack([torch.cat([marks[int(s)] for s in fid[i, side]]) for i in idx.tolist()])
        assert torch.equal(out.cpu(), exp)
    del store
    torch.cuda.empty_cache()


@pytest.mark.parametrize('fbytes,cols', [(400, 12), (35, 7)])
def test_replay_insert_shared_exact(fbytes, cols):
    """A ring of 7 transitions and a store of 16 frames, pre-filled; n = 5 rows
    from slot 5 on (wraps) with m = 4 new frames, then n = 9 > 7 rows with no
    frame: table, ids and store equal a numpy model and every slot not named
    keeps its sentinel."""
    mem, fslots_n, dev = 7, 16, 'cuda'
    g = torch.Generator().manual_seed(3)
    table = torch.full((mem, cols), -7.0)
    fid = torch.full((mem, 2, S), -1, dtype=torch.int32)
    store = torch.full((fslots_n, fbytes), SENTINEL, dtype=torch.uint8)
    d_table, d_fid, d_store = table.to(dev), fid.to(dev), store.to(dev)

    def insert(first, n, slots):
        rows = torch.randn(n, cols, generator=g)
        ids = torch.randint(0, fslots_n, (n, 2, S), generator=g, dtype=torch.int32)
        frames = torch.randint(0, 256, (len(slots), fbytes), generator=g, dtype=torch.uint8)
        fs = torch.tensor(slots, dtype=torch.int32)
        d = [t.to(dev) if t.numel() else None for t in (rows, ids, frames, fs)]
        L.call('smi_replay_insert_shared', L.ptr(d_table), cols, L.ptr(d_fid), S, L.ptr(d_store),
               fbytes, mem, first, L.ptr(d[0]), L.ptr(d[1]), n, L.ptr(d[2]), L.ptr(d[3]),
               len(slots), L.stream(d_table.device))
        torch.cuda.synchronize()
        for e in range(max(0, n - mem), n):
            table[(first + e) % mem] = rows[e]
            fid[(first + e) % mem] = ids[e]
        for j, s in enumerate(slots):
            store[s] = frames[j]

    insert(5, 5, [15, 0, 7, 3])
    assert torch.equal(d_table.cpu(), table) and torch.equal(d_fid.cpu(), fid)
    assert torch.equal(d_store.cpu(), store)
    assert bool((d_table[3:5] == -7.0).all()) and bool((d_fid[3:5] == -1).all())
    untouched = [s for s in range(fslots_n) if s not in (15, 0, 7, 3)]
    assert bool((d_store[untouched] == SENTINEL).all())
    insert(3, 9, [])                       # more rows than slots: the last 7 survive
    assert torch.equal(d_table.cpu(), table) and torch.equal(d_fid.cpu(), fid)
    assert torch.equal(d_store.cpu(), store)


# ------------------------------------------------------------- the replays
def rolling_stream(n_step, total, frame_shape, seed=0, actors=2):
    """the stream of tests/test_cpu_replay_shared.py: `actors` interleaved
    actors, episodes of 1..9 steps from a reset observation of S equal frames,
    obs_next n_step steps after obs, shared frames being shared objects"""
    rs = np.random.RandomState(seed)
    rnd = random.Random(seed)

    def frame():
        return rs.randint(0, 256, frame_shape).astype(np.uint8)

    def episodes():
        while True:
            steps = rnd.randint(1, 9)
            hist = [frame()] * S
            obs = [list(hist)]
            for _ in range(steps):
                hist = hist[1:] + [frame()]
                obs.append(list(hist))
                if len(obs) > n_step:
                    yield obs[-1 - n_step], obs[-1]
                else:
                    yield None
    gens = [episodes() for _ in range(actors)]
    out = []
    while len(out) < total:
        for g in gens:
            t = next(g)
            if t is not None and len(out) < total:
                out.append(t)
    return out


def _exps(stream, D, A, seed, as_array=False):
    """SSAR experience dicts over the stream's observations; camera0 is the
    list of S frames (the reference's form) or, as_array, one (C, H, W) array"""
    g = torch.Generator().manual_seed(seed)
    n = len(stream)
    rows = torch.randn(n, 2 * D + A + 2, generator=g)
    rows[:, D:D + A] = torch.tanh(rows[:, D:D + A])
    rows[:, 2 * D + A + 1] = (torch.rand(n, generator=g) < 0.1).float()
    r = rows.numpy()
    out = []
    for i, (f0, f1) in enumerate(stream):
        cams = [np.concatenate(f, axis=0) if as_array else f for f in (f0, f1)]
        o0, o1 = {'pixel': {'camera0': cams[0]}}, {'pixel': {'camera0': cams[1]}}
        if D:
            o0['low_dim'] = {'flat_inputs': r[i, :D]}
            o1['low_dim'] = {'flat_inputs': r[i, D + A + 1:2 * D + A + 1]}
        out.append({'obs': [o0, o1], 'action': r[i, D:D + A], 'reward': r[i, D + A],
                    'done': bool(r[i, 2 * D + A + 1])})
    return out, rows


def _leaves(batch):
    out = {}

    def walk(path, v):
        if isinstance(v, dict):
            for k in v:
                walk(path + (k,), v[k])
        else:
            out[path] = v
    walk((), batch)
    return out


def _same_batch(a, b):
    la, lb = _leaves(a), _leaves(b)
    assert sorted(la) == sorted(lb)
    for k in la:
        assert la[k].dtype == lb[k].dtype and la[k].shape == lb[k].shape, k
        assert torch.equal(la[k], lb[k]), k


def _distinct_live(stream, pos, mem):
    live = stream[max(0, pos - mem):pos]
    return len({f.tobytes() for t in live for side in t for f in side})


@pytest.mark.parametrize('D,n_step', [(5, 1), (5, 3), (0, 1)])
def test_shared_replay_equals_unshared(D, n_step):
    A, cam, mem = 2, (9, 20, 20), 7
    ec = _env(D, A, cam)
    plain = UniformReplay(_cfg(8, mem), ec, seed=42)
    shared = UniformReplay(_cfg(8, mem, share=True), ec, seed=42)
    assert shared.share_frames and not plain.share_frames
    assert not hasattr(shared, 'frames') and not hasattr(shared, 'frames_next')
    assert shared.frame_slots == mem + mem // 4
    assert tuple(shared.frame_store.shape) == (mem + mem // 4, 3, 20, 20)
    assert tuple(shared.frame_ids.shape) == (mem, 2, S) and shared.frame_ids.dtype == torch.int32
    # the default store of 8 frames is small for 7 transitions of two actors
    shared = UniformReplay(_cfg(8, mem, share=True, frame_slots=48), ec, seed=42)
    stream = rolling_stream(n_step, sum(CHUNKS), (3, 20, 20), seed=20 + n_step)
    exps, _ = _exps(stream, D, A, seed=1)
    arr_exps, _ = _exps(stream, D, A, seed=1, as_array=True)
    pos = 0
    for step, n in enumerate(CHUNKS):
        chunk = exps[pos:pos + n]
        plain.insert_rows(*plain.pack(chunk))
        if step == 1:                                   # one experience at a time
            for e in chunk:
                shared.insert(e)
        elif step == 3:                                 # whole (C, H, W) cameras
            shared.insert_rows(*shared.pack(arr_exps[pos:pos + n]))
        elif step == 5:                                 # the unshared ring's arrays
            shared.insert_rows(*plain.pack(chunk))
        else:
            shared.insert_rows(*shared.pack(chunk))
        pos += n
        assert len(shared) == len(plain) and shared._next_idx == plain._next_idx
        ia, ba = plain.sample_batch(8)
        ib, bb = shared.sample_batch(8)
        assert torch.equal(ia, ib)
        _same_batch(ba, bb)
        assert shared.frames_in_use == _distinct_live(stream, pos, mem)
    assert shared.frames_in_use < 2 * S * len(shared)
    with pytest.raises(ValueError, match='sample_batch'):
        shared.sample(4)


def test_share_frames_config_errors_on_the_replay():
    with pytest.raises(ValueError, match='pixel'):
        UniformReplay(_cfg(8, 7, share=True), gym_env_config(5, 2), seed=0)
    with pytest.raises(ValueError, match='frame_stacks'):
        UniformReplay(_cfg(8, 7, share=True), _env(5, 2, (9, 20, 20), stacks=2), seed=0)


@pytest.fixture(scope='module')
def stream_84():
    """150 transitions of a rolling 9 x 84 x 84 stream (shared, never modified):
    (experience dicts, rows, pix, pix_next)"""
    D, A = 17, 6
    stream = rolling_stream(1, 150, (3, 84, 84), seed=5)
    exps, rows = _exps(stream, D, A, seed=6)
    pix = torch.from_numpy(np.stack([np.concatenate(t[0], axis=0) for t in stream]))
    pix_next = torch.from_numpy(np.stack([np.concatenate(t[1], axis=0) for t in stream]))
    return exps, rows, pix, pix_next


def _check_batch(batch, idx, rows, pix, pix_next, D, A, cam):
    n = len(idx)
    cam0, cam1 = batch['obs']['pixel']['camera0'], batch['obs_next']['pixel']['camera0']
    for t in (cam0, cam1):
        assert t.dtype == torch.uint8 and tuple(t.shape) == (n,) + cam and t.is_cuda
        assert t.is_contiguous()
    assert torch.equal(cam0.cpu(), pix[idx])
    assert torch.equal(cam1.cpu(), pix_next[idx])
    r = rows[idx]
    low0 = batch['obs']['low_dim']['flat_inputs']
    low1 = batch['obs_next']['low_dim']['flat_inputs']
    assert low0.dtype == torch.float32 and tuple(low0.shape) == (n, D)
    assert torch.equal(low0.cpu(), r[:, :D])
    assert torch.equal(low1.cpu(), r[:, D + A + 1:2 * D + A + 1])
    assert torch.equal(batch['actions'].cpu(), r[:, D:D + A])
    assert torch.equal(batch['rewards'].cpu(), r[:, D + A:D + A + 1])
    assert torch.equal(batch['dones'].cpu(), r[:, 2 * D + A + 1:])


def _shared_84(stream_84, seed, cls=UniformReplay, share=True):
    D, A, cam, B = 17, 6, (9, 84, 84), 64
    rep = cls(_cfg(B, 200, share=share), _env(D, A, cam), seed=seed)
    rep.insert_rows(*rep.pack(stream_84[0]))
    return rep


def test_shared_replay_workload_frame_matches_cpython(stream_84):
    D, A, cam, B = 17, 6, (9, 84, 84), 64
    _, rows, pix, pix_next = stream_84
    rep = _shared_84(stream_84, 1234)
    assert len(rep) == 150 and rep.start_sample_condition()
    assert rep.frames_in_use < 250 and rep.frame_slots == 250
    idx, batch = rep.sample_batch(B)
    random.seed(1234)
    exp = [random.randint(0, 149) for _ in range(B)]
    assert idx.cpu().tolist() == exp
    _check_batch(batch, exp, rows, pix, pix_next, D, A, cam)
    # the second draw continues the stream and reuses the output buffers
    ptr = batch['obs']['pixel']['camera0'].data_ptr()
    idx2, batch2 = rep.sample_batch(B)
    exp2 = [random.randint(0, 149) for _ in range(B)]
    assert idx2.cpu().tolist() == exp2
    assert batch2['obs']['pixel']['camera0'].data_ptr() == ptr
    _check_batch(batch2, exp2, rows, pix, pix_next, D, A, cam)


def test_shared_replay_rank_shards_concatenate(stream_84):
    B, world = 64, 4
    idx1, whole = _shared_84(stream_84, 77).sample_batch(B)
    shards = [_shared_84(stream_84, 77).sample_batch(B, rank=r, world=world) for r in range(world)]
    assert torch.equal(torch.cat([s[0] for s in shards]), idx1)
    lw = _leaves(whole)
    for k in lw:
        assert torch.equal(torch.cat([_leaves(s[1])[k] for s in shards]), lw[k]), k
    _check_batch(whole, idx1.cpu().tolist(), stream_84[1], stream_84[2], stream_84[3], 17, 6,
                 (9, 84, 84))


def test_prioritized_replay_shared_equals_unshared():
    D, A, cam, mem, B, beta = 5, 2, (9, 20, 20), 7, 8, 0.4
    ec = _env(D, A, cam)
    plain = PrioritizedReplay(_cfg(B, mem), ec, seed=9)
    shared = PrioritizedReplay(_cfg(B, mem, share=True, frame_slots=48), ec, seed=9)
    stream = rolling_stream(1, sum(CHUNKS), (3, 20, 20), seed=31)
    exps, _ = _exps(stream, D, A, seed=2)
    g = torch.Generator().manual_seed(4)
    pos = 0
    for n in CHUNKS:
        plain.insert_rows(*plain.pack(exps[pos:pos + n]))
        shared.insert_rows(*shared.pack(exps[pos:pos + n]))
        pos += n
        if len(plain) < 2:
            continue
        for _ in range(2):                              # before and after a TD round
            ia, ba = plain.sample_batch(B, beta=beta)
            ib, bb = shared.sample_batch(B, beta=beta)
            assert torch.equal(ia, ib)
            assert 'weights' in bb
            _same_batch(ba, bb)
            td = torch.randn(B, generator=g).cuda()
            plain.update_priorities_from_td(ia, td)
            shared.update_priorities_from_td(ib, td)
        assert torch.equal(plain.tree, shared.tree)


def test_store_full_leaves_replay_and_trees_untouched():
    D, A, cam, mem = 5, 2, (9, 20, 20), 7
    rep = PrioritizedReplay(_cfg(8, mem, share=True, frame_slots=12), _env(D, A, cam), seed=0)
    stream = rolling_stream(1, 7, (3, 20, 20), seed=40)
    exps, _ = _exps(stream, D, A, seed=3)
    rep.insert_rows(*rep.pack(exps[:4]))
    rs = np.random.RandomState(1)
    distinct = [([rs.randint(0, 256, (3, 20, 20)).astype(np.uint8) for _ in range(S)],
                 [rs.randint(0, 256, (3, 20, 20)).astype(np.uint8) for _ in range(S)])
                for _ in range(3)]
    big, _ = _exps(distinct, D, A, seed=4)
    torch.cuda.synchronize()
    before = [t.clone() for t in (rep.tree, rep.table, rep.frame_store, rep.frame_ids)]
    state = (len(rep), rep._next_idx, rep.frames_in_use)
    rep.sample_batch(8)
    with pytest.raises(RuntimeError, match='frame_slots'):
        rep.insert_rows(*rep.pack(big))                 # 18 new frames into 12 slots
    torch.cuda.synchronize()
    for was, now in zip(before, (rep.tree, rep.table, rep.frame_store, rep.frame_ids)):
        assert torch.equal(was, now)
    assert (len(rep), rep._next_idx, rep.frames_in_use) == state
    rep.insert_rows(*rep.pack(exps[4:5]))               # one that fits goes in
    assert len(rep) == 5
    fresh = PrioritizedReplay(_cfg(8, mem, share=True, frame_slots=12), _env(D, A, cam), seed=0)
    fresh.insert_rows(*fresh.pack(exps[:4]))
    fresh.sample_batch(8)
    fresh.insert_rows(*fresh.pack(exps[4:5]))
    _same_batch(rep.sample_batch(8)[1], fresh.sample_batch(8)[1])
    assert torch.equal(rep.tree, fresh.tree)


def _flats(learner):
    out = []
    for model in (learner.model, learner.model_target):
        for m in model.modules():
            f = m.__dict__.get('flat')
            if isinstance(f, torch.Tensor):
                out.append(f)
    return out


def test_shared_replay_feeds_learner_identically(stream_84):
    """one learn() from the shared replay's batch and one, in a second learner
    with the same seed, from the unshared replay's: identical bytes in, so
    bit-identical parameters out"""
    from surreal_amd.ddpg import DDPGLearner
    D, A, cam, B = 17, 6, (9, 84, 84), 64
    ec = _env(D, A, cam)
    shared = _shared_84(stream_84, 11)
    plain = _shared_84(stream_84, 11, share=False)
    assert hasattr(plain, 'frames') and not hasattr(shared, 'frames')
    ia, ba = plain.sample_batch(B)
    ib, bb = shared.sample_batch(B)
    assert torch.equal(ia, ib)
    _same_batch(ba, bb)
    la, lb = DDPGLearner(_cfg(B, 200), ec, seed=0), DDPGLearner(_cfg(B, 200, share=True), ec, seed=0)
    assert la.is_pixel_input
    start = [f.clone() for f in _flats(la)]
    la.learn(ba)
    lb.learn(bb)
    torch.cuda.synchronize()
    fa, fb = _flats(la), _flats(lb)
    assert len(fa) == len(fb) >= 2
    for x, y in zip(fa, fb):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, s) for x, s in zip(fa, start))     # and they trained
