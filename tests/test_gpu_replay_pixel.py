"""Device-resident pixel replay: smi_replay_gather (frames of both observations
and the float side rows of a sample, one launch) and UniformReplay's pixel mode
feeding DDPGLearner.  A gather moves bytes, so every comparison is exact
(torch.equal) against numpy / torch indexing of host copies."""
import copy
import random

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd.config import DDPG_DEFAULT_LEARNER_CONFIG, gym_env_config, pixel_env_config
from surreal_amd.replay import UniformReplay

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _cfg(B=64, memory_size=200):
    lc = copy.deepcopy(DDPG_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = B
    lc.replay.memory_size = memory_size
    lc.replay.sampling_start_size = 10
    lc.algo.network.target_update = {'type': 'hard', 'interval': 2}
    return lc


def _gather(table, cols, frames, frames_next, frame_bytes, idx, rows_out, pix_out, pix_next_out):
    L.call('smi_replay_gather', L.ptr(table), cols, L.ptr(frames), L.ptr(frames_next), frame_bytes,
           L.ptr(idx), idx.numel(), L.ptr(rows_out), L.ptr(pix_out), L.ptr(pix_next_out),
           L.stream(idx.device))
    torch.cuda.synchronize()


def _ring(frame_bytes, cols, slots=16, batch=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (slots, frame_bytes), generator=g, dtype=torch.uint8)
    frames_next = torch.randint(0, 256, (slots, frame_bytes), generator=g, dtype=torch.uint8)
    table = torch.randn(slots, cols, generator=g) if cols else None
    idx = torch.randint(0, slots, (batch,), generator=g)
    idx[0], idx[1], idx[-1], idx[-2] = 0, slots - 1, 0, slots - 1    # repeats of both ends
    return frames, frames_next, table, idx


@pytest.mark.parametrize('frame_bytes,cols', [(1200, 12), (63504, 42), (63504, 0), (105, 7)])
def test_replay_gather_abi_exact(frame_bytes, cols):
    """(1200, 12): 75 16-byte chunks, less than one workgroup pass, float4 rows;
    (63504, 42): the 9 x 84 x 84 frame, 3969 = 15 * 256 + 129 chunks, float2
    rows; (63504, 0): no table; (105, 7): the byte path, scalar rows.  The
    outputs are one frame longer than the batch and pre-filled: the extra frame
    must come back untouched."""
    batch = 37
    frames, frames_next, table, idx = _ring(frame_bytes, cols, batch=batch)
    dev = 'cuda'
    pix = torch.full((batch + 1, frame_bytes), SENTINEL, dtype=torch.uint8, device=dev)
    pix_next = torch.full((batch + 1, frame_bytes), SENTINEL, dtype=torch.uint8, device=dev)
    rows = torch.full((batch + 1, cols), -7.0, device=dev) if cols else None
    _gather(table.to(dev) if cols else None, cols, frames.to(dev), frames_next.to(dev), frame_bytes,
            idx.to(dev), rows, pix, pix_next)
    assert torch.equal(pix[:batch].cpu(), frames[idx])
    assert torch.equal(pix_next[:batch].cpu(), frames_next[idx])
    assert bool((pix[batch] == SENTINEL).all()) and bool((pix_next[batch] == SENTINEL).all())
    if cols:
        assert torch.equal(rows[:batch].cpu(), table[idx])
        assert bool((rows[batch] == -7.0).all())


def test_replay_gather_misaligned_falls_back():
    """pix_out 4 bytes off a 16-byte boundary: the 16-byte path does not apply
    and the byte path must give the same exact result."""
    frame_bytes, cols, batch = 1200, 12, 37
    frames, frames_next, table, idx = _ring(frame_bytes, cols, batch=batch, seed=1)
    dev = 'cuda'
    buf = torch.full((4 + (batch + 1) * frame_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    pix = buf[4:].view(batch + 1, frame_bytes)
    assert pix.data_ptr() % 16 == 4
    pix_next = torch.full((batch + 1, frame_bytes), SENTINEL, dtype=torch.uint8, device=dev)
    rows = torch.empty(batch, cols, device=dev)
    _gather(table.to(dev), cols, frames.to(dev), frames_next.to(dev), frame_bytes, idx.to(dev),
            rows, pix, pix_next)
    assert torch.equal(pix[:batch].cpu(), frames[idx])
    assert torch.equal(pix_next[:batch].cpu(), frames_next[idx])
    assert torch.equal(rows.cpu(), table[idx])
    assert bool((buf[:4] == SENTINEL).all()) and bool((pix[batch] == SENTINEL).all())
    assert bool((pix_next[batch] == SENTINEL).all())


def test_replay_gather_offsets_beyond_4gib():
    """One 3,600,000 x 1200 B ring (4.32 GB) as both sides.  Slot 3,579,139
    starts at byte 4,294,966,800 and straddles 2^32; slot 3,579,140 is the
    first that lies wholly beyond it; 3,599,999 is the last slot.  A 32-bit
    source offset would wrap each of them into the zero-filled low ring."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 1024 ** 3:
        pytest.skip(f'needs 6 GB of free HBM for the 4.32 GB ring, {free / 1024 ** 3:.1f} GB free')
    slots, frame_bytes = 3600000, 1200
    dev = 'cuda'
    ring = torch.zeros(slots, frame_bytes, dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(2)
    marks = {s: torch.randint(1, 256, (frame_bytes,), generator=g, dtype=torch.uint8)
             for s in (0, 3579139, 3579140, 3599999)}
    for s, f in marks.items():
        ring[s] = f.to(dev)
    order = [3599999, 0, 3579139, 3579140]
    idx = torch.tensor(order, device=dev)
    pix = torch.empty(len(order), frame_bytes, dtype=torch.uint8, device=dev)
    pix_next = torch.empty_like(pix)
    _gather(None, 0, ring, ring, frame_bytes, idx, None, pix, pix_next)
    exp = torch.stack([marks[s] for s in order])
    assert torch.equal(pix.cpu(), exp)
    assert torch.equal(pix_next.cpu(), exp)
    del ring
    torch.cuda.empty_cache()


def _experience(n, D, A, cam, seed):
    """n transitions as host arrays: (rows [n, 2D+A+2], pix, pix_next)"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(n, 2 * D + A + 2, generator=g)
    rows[:, D:D + A] = torch.tanh(rows[:, D:D + A])
    rows[:, 2 * D + A + 1] = (torch.rand(n, generator=g) < 0.1).float()
    pix = torch.randint(0, 256, (n,) + cam, generator=g, dtype=torch.uint8)
    pix_next = torch.randint(0, 256, (n,) + cam, generator=g, dtype=torch.uint8)
    return rows, pix, pix_next


def _as_exps(rows, pix, pix_next, D, A):
    """the same transitions as SSAR experience dicts"""
    rows = rows.numpy()
    out = []
    for i in range(rows.shape[0]):
        o0, o1 = {'pixel': {'camera0': pix[i].numpy()}}, {'pixel': {'camera0': pix_next[i].numpy()}}
        if D:
            o0['low_dim'] = {'flat_inputs': rows[i, :D]}
            o1['low_dim'] = {'flat_inputs': rows[i, D + A + 1:2 * D + A + 1]}
        out.append({'obs': [o0, o1], 'action': rows[i, D:D + A], 'reward': rows[i, D + A],
                    'done': bool(rows[i, 2 * D + A + 1])})
    return out


@pytest.fixture(scope='module')
def experience_84():
    """150 transitions of the 9 x 84 x 84 configuration (shared, never modified)"""
    return _experience(150, 17, 6, (9, 84, 84), seed=5)


def _check_batch(batch, idx, rows, pix, pix_next, D, A, cam):
    n = len(idx)
    cam0, cam1 = batch['obs']['pixel']['camera0'], batch['obs_next']['pixel']['camera0']
    for t in (cam0, cam1):
        assert t.dtype == torch.uint8 and tuple(t.shape) == (n,) + cam and t.is_cuda
        assert t.is_contiguous()
    assert torch.equal(cam0.cpu(), pix[idx])
    assert torch.equal(cam1.cpu(), pix_next[idx])
    r = rows[idx]
    if D:
        low0 = batch['obs']['low_dim']['flat_inputs']
        low1 = batch['obs_next']['low_dim']['flat_inputs']
        assert low0.dtype == torch.float32 and tuple(low0.shape) == (n, D)
        assert torch.equal(low0.cpu(), r[:, :D])
        assert torch.equal(low1.cpu(), r[:, D + A + 1:2 * D + A + 1])
    else:
        assert 'low_dim' not in batch['obs'] and 'low_dim' not in batch['obs_next']
    assert tuple(batch['actions'].shape) == (n, A)
    assert tuple(batch['rewards'].shape) == (n, 1) and tuple(batch['dones'].shape) == (n, 1)
    assert torch.equal(batch['actions'].cpu(), r[:, D:D + A])
    assert torch.equal(batch['rewards'].cpu(), r[:, D + A:D + A + 1])
    assert torch.equal(batch['dones'].cpu(), r[:, 2 * D + A + 1:])


def test_pixel_replay_sample_batch_matches_cpython(experience_84):
    D, A, cam, B = 17, 6, (9, 84, 84), 64
    rows, pix, pix_next = experience_84
    rep = UniformReplay(_cfg(B, 200), pixel_env_config(D, A, cam), seed=1234)
    assert rep.is_pixel and rep.width == 2 * D + A + 2
    assert tuple(rep.frames.shape) == (200,) + cam and rep.frames.dtype == torch.uint8
    packed = rep.pack(_as_exps(rows, pix, pix_next, D, A))
    assert np.array_equal(packed[0], rows.numpy())
    rep.insert_rows(*packed)
    assert len(rep) == 150 and rep.start_sample_condition()
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


def test_pixel_replay_wraps_like_single_inserts():
    """uniform_replay.py:36-41 in pixel mode: the three rings advance together,
    and a bulk insert of more transitions than slots keeps the last
    memory_size in the slots repeated single inserts leave them in."""
    D, A, cam = 5, 2, (3, 20, 20)
    ec = pixel_env_config(D, A, cam)
    bulk = UniformReplay(_cfg(8, 7), ec, seed=1)
    single = UniformReplay(_cfg(8, 7), ec, seed=1)
    for step, n in enumerate((3, 18, 1, 9)):
        rows, pix, pix_next = _experience(n, D, A, cam, seed=30 + step)
        bulk.insert_rows(rows, pix, pix_next)
        for e in _as_exps(rows, pix, pix_next, D, A):
            single.insert(e)
        assert torch.equal(bulk.table.cpu(), single.table.cpu()), n
        assert torch.equal(bulk.frames.cpu(), single.frames.cpu()), n
        assert torch.equal(bulk.frames_next.cpu(), single.frames_next.cpu()), n
        assert len(bulk) == len(single) and bulk._next_idx == single._next_idx
    assert len(bulk) == 7 and bulk._next_idx == 31 % 7
    # the rings hold the last 7 transitions of the last two inserts
    last = _experience(9, D, A, cam, seed=33)
    slots = [(22 + i) % 7 for i in range(2, 9)]
    assert torch.equal(bulk.frames.cpu()[slots], last[1][2:])
    assert torch.equal(bulk.frames_next.cpu()[slots], last[2][2:])
    assert torch.equal(bulk.table.cpu()[slots], last[0][2:])
    with pytest.raises(ValueError):
        bulk.insert_rows(last[0])                                 # frames missing
    with pytest.raises(ValueError):
        bulk.insert_rows(last[0], last[1][:, :, :10], last[2])    # mis-shaped
    with pytest.raises(ValueError):
        bulk.insert_rows(last[0], last[1].float(), last[2])       # not uint8


def test_pixel_replay_rank_shards_concatenate(experience_84):
    D, A, cam, B, world = 17, 6, (9, 84, 84), 64, 4
    rows, pix, pix_next = experience_84
    ec = pixel_env_config(D, A, cam)

    def replay():
        rep = UniformReplay(_cfg(B, 200), ec, seed=77)
        rep.insert_rows(rows, pix, pix_next)
        return rep
    idx1, whole = replay().sample_batch(B)
    shards = [replay().sample_batch(B, rank=r, world=world) for r in range(world)]
    assert torch.equal(torch.cat([s[0] for s in shards]), idx1)
    for s in shards:
        assert s[0].numel() == B // world

    def cat(f):
        return torch.cat([f(s[1]) for s in shards])
    for f in (lambda b: b['obs']['pixel']['camera0'], lambda b: b['obs_next']['pixel']['camera0'],
              lambda b: b['obs']['low_dim']['flat_inputs'],
              lambda b: b['obs_next']['low_dim']['flat_inputs'],
              lambda b: b['actions'], lambda b: b['rewards'], lambda b: b['dones']):
        assert torch.equal(cat(f), f(whole))
    _check_batch(whole, idx1.cpu().tolist(), rows, pix, pix_next, D, A, cam)
    with pytest.raises(ValueError):
        replay().sample_batch(B, rank=0, world=3)


def test_pixel_only_spec():
    A, cam, B = 3, (3, 20, 20), 24
    rows, pix, pix_next = _experience(40, 0, A, cam, seed=9)
    rep = UniformReplay(_cfg(B, 50), pixel_env_config(0, A, cam), seed=3)
    assert rep.obs_dim == 0 and rep.width == A + 2
    rep.insert_rows(*rep.pack(_as_exps(rows, pix, pix_next, 0, A)))
    idx, batch = rep.sample_batch(B)
    random.seed(3)
    exp = [random.randint(0, 39) for _ in range(B)]
    assert idx.cpu().tolist() == exp
    _check_batch(batch, exp, rows, pix, pix_next, 0, A, cam)


def test_pixel_replay_feeds_learner(experience_84):
    from surreal_amd.ddpg import DDPGLearner
    D, A, cam, B = 17, 6, (9, 84, 84), 64
    lc, ec = _cfg(B, 200), pixel_env_config(D, A, cam)
    rep = UniformReplay(lc, ec, seed=11)
    rep.insert_rows(*experience_84)
    learner = DDPGLearner(lc, ec, seed=0)
    assert learner.is_pixel_input
    before = learner.model.perception.flat.detach().clone()
    for _ in range(2):
        learner.learn(rep.sample_batch(B)[1])
        stats = learner.last_stats()
        assert stats and np.isfinite(list(stats.values())).all()
    assert not torch.equal(learner.model.perception.flat, before)    # the stem trained


def test_low_dim_sample_batch_equals_split_sample():
    D, A, B = 17, 6, 512
    lc, ec = _cfg(B, 5000), gym_env_config(D, A)
    a, b = UniformReplay(lc, ec, seed=21), UniformReplay(lc, ec, seed=21)
    rows = np.random.RandomState(4).randn(3000, a.width).astype(np.float32)
    a.insert_rows(rows)
    b.insert_rows(rows)
    idx_a, batch = a.sample_batch(B)
    idx_b, got = b.sample(B)
    ref = b.split(got)
    assert torch.equal(idx_a, idx_b)
    assert sorted(batch) == sorted(ref)
    for k in ref:
        assert torch.equal(batch[k], ref[k]), k
    assert torch.equal(got.cpu(), torch.from_numpy(rows[idx_b.cpu().numpy()]))


def test_pixel_mode_sample_raises():
    rep = UniformReplay(_cfg(8, 16), pixel_env_config(5, 2, (3, 20, 20)), seed=0)
    rep.insert_rows(*_experience(4, 5, 2, (3, 20, 20), seed=1))
    with pytest.raises(ValueError, match='sample_batch'):
        rep.sample(4)
