"""Replay buffers of the learner hot path.

UniformReplay mirrors surreal/replay/uniform_replay.py:6-74 with the memory as
a device-resident ring of fixed-width rows (obs | action | reward | obs_next |
done) in HBM and the index draw done by the CPython-exact MT19937 HIP kernel
(smi_mt_randint), so `sample()` returns exactly the rows the reference's
`[random.randint(0, len-1) for _ in range(B)]` would pick after
`random.seed(seed)`.  With camera observations (a 'pixel' entry in the obs
spec) the ring also holds the uint8 frames of both observations on the device
and `sample_batch()` gathers rows and frames in one launch (smi_replay_gather)
into the batch form DDPGLearner.learn() takes.  PrioritizedReplay adds the
proportional draw of prioritized_replay.py / segment_tree.py on the same ring:
fp64 sum and min trees in HBM, the draw and its importance-sampling weights in
one kernel (smi_per_sample), priorities from the learner's TD errors without a
host round trip (smi_per_update_td).  FIFOReplay mirrors fifo_replay.py:6-49
(host deque; the PPO path consumes batches in insertion order).
"""
import ctypes
from collections import deque

import numpy as np
import torch

from . import _lib as L
from .frame_store import FrameAllocator, frame_sharing, split_camera


class CPythonRandom(object):
    """Host+device MT19937 state that reproduces `random.seed(s); random.randint`."""

    def __init__(self, seed=0, device=None):
        self.device = device
        self.host = np.zeros(625, dtype=np.uint32)
        L.check(L.lib().smi_mt_seed(abs(int(seed)), self.host.ctypes.data), 'smi_mt_seed')
        self.dev = None
        if device is not None:
            self.dev = torch.from_numpy(self.host.view(np.int32).copy()).to(device)

    def randint_host(self, n, batch):
        out = np.zeros(batch, dtype=np.int64)
        L.check(L.lib().smi_mt_randint_host(self.host.ctypes.data, int(n), int(batch),
                                            out.ctypes.data), 'smi_mt_randint_host')
        return out

    def randint_device(self, n, batch, out=None):
        if out is None:
            out = torch.empty(batch, dtype=torch.int64, device=self.device)
        L.call('smi_mt_randint', L.ptr(self.dev), int(n), int(batch), L.ptr(out),
               L.stream(self.device))
        return out


def _camera_u8(cam, shape):
    """camera0 of one observation -> uint8 (C, H, W); a list of per-frame arrays
    is concatenated along channels (frame_stack_concatenate_on_env: False), and
    a non-uint8 array must hold integral values in [0, 255] (the rule of
    DDPGAgentBatch._camera)"""
    if isinstance(cam, (list, tuple)):
        cam = np.concatenate([np.asarray(f) for f in cam], axis=0)
    a = np.asarray(cam)
    if a.dtype != np.uint8:
        if not (np.all(a == np.round(a)) and a.min() >= 0 and a.max() <= 255):
            raise TypeError('camera observations must hold uint8 pixel values')
        a = a.astype(np.uint8)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f'camera0 has shape {tuple(a.shape)}, the obs spec says {tuple(shape)}')
    return a


def _low_dim(obs):
    return np.concatenate([np.ravel(v) for v in obs['low_dim'].values()])


def pack_rows(exps, obs_dim, act_dim):
    """SSAR experience dicts {'obs': [o0, o1], 'action', 'reward', 'done'} ->
    rows float32 [n, W] on the host, W = 2 * obs_dim + act_dim + 2, in
    UniformReplay's layout [obs | action | reward | obs_next | done] (obs_dim
    0, a pixel-only spec: [action | reward | done])."""
    D, A = int(obs_dim), int(act_dim)
    rows = np.zeros((len(exps), 2 * D + A + 2), dtype=np.float32)
    for i, e in enumerate(exps):
        if D:
            rows[i, :D] = _low_dim(e['obs'][0])
            rows[i, D + A + 1:2 * D + A + 1] = _low_dim(e['obs'][1])
        rows[i, D:D + A] = e['action']
        rows[i, D + A] = e['reward']
        rows[i, 2 * D + A + 1] = float(e['done'])
    return rows


def pack_pixel_exps(exps, obs_dim, act_dim, camera_shape):
    """SSAR experience dicts with camera observations -> (pack_rows' rows, pix
    uint8 [n, C, H, W], pix_next uint8 [n, C, H, W]) on the host."""
    shape = tuple(int(c) for c in camera_shape)
    pix = np.zeros((len(exps),) + shape, dtype=np.uint8)
    pix_next = np.zeros((len(exps),) + shape, dtype=np.uint8)
    for i, e in enumerate(exps):
        pix[i] = _camera_u8(e['obs'][0]['pixel']['camera0'], shape)
        pix_next[i] = _camera_u8(e['obs'][1]['pixel']['camera0'], shape)
    return pack_rows(exps, obs_dim, act_dim), pix, pix_next


class UniformReplay(object):
    """Ring buffer with CPython-exact uniform sampling (uniform_replay.py:36-47).

    Rows are fixed-width float32 records laid out [obs(D) | action(A) |
    reward(1) | obs_next(D) | done(1)] in one (memory_size, W) device tensor.
    For an action spec of type 'discrete' A is 1: the column holds the action
    index (pack() takes a Python or numpy integer), as DQNLearner reads it.

    Pixel mode (a 'pixel' entry in env_config['obs_spec']; only camera0 is
    read, as DDPGModel does): two more device rings, `frames` and
    `frames_next`, uint8 (memory_size, C, H, W), hold the camera observation
    before and after each transition; D is the low-dim width and may be 0
    (W = A + 2).  The three rings always advance together.  The frame rings
    take 2 * memory_size * C*H*W bytes: 42 GB at the reference defaults
    (memory_size 333,333, 9 x 84 x 84), because every transition stores both
    of its observations whole.

    Frame-shared pixel mode (learner_config.replay.share_frames = True) keeps
    every camera frame once, as the reference sender's per-frame hashing does
    (distributed/exp_sender.py:45-59).  With S = env_config.frame_stacks an
    observation is S frames of (C/S, H, W); `frame_store`, uint8 (frame_slots,
    C/S, H, W), holds each distinct frame once and `frame_ids`, int32
    (memory_size, 2, S), names the store slots of obs and obs_next of every
    transition; `frames` and `frames_next` do not exist.  frame_slots is
    learner_config.replay.frame_slots, by default memory_size + memory_size //
    4: 8.8 GB at the reference defaults.  The host side (frame_store.py:
    digests, reference counts, free list) decides which frames of an insert
    are new; those, the rows and the ids go up in one pinned buffer, one copy
    and one launch (smi_replay_insert_shared), and sample_batch() gathers
    through the ids (smi_replay_gather_shared) into the same batch.  Sampling
    draws transition slots, which have not moved, so it is unchanged.  A full
    store raises RuntimeError and leaves the replay as it was."""

    def __init__(self, learner_config, env_config, session_config=None, index=0, seed=0,
                 device=None):
        L.require_gpu()
        self.learner_config = learner_config
        self.memory_size = int(learner_config['replay']['memory_size'])
        self.sampling_start_size = int(learner_config['replay']['sampling_start_size'])
        spec = env_config['obs_spec']
        self.is_pixel = 'pixel' in spec
        if self.is_pixel:
            self.camera_shape = tuple(int(c) for c in spec['pixel']['camera0'])
            self.obs_dim = int(sum(v[0] for v in spec['low_dim'].values())) if 'low_dim' in spec else 0
        else:
            self.obs_dim = int(sum(v[0] for v in spec['low_dim'].values()))
        # a discrete spec's dim[0] is the NUMBER of actions: the row holds the
        # action index in one column (DQNLearner reads it as a float32 column)
        self.discrete = env_config['action_spec'].get('type') == 'discrete'
        self.act_dim = 1 if self.discrete else int(env_config['action_spec']['dim'][0])
        self.width = 2 * self.obs_dim + self.act_dim + 2
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        self.table = torch.zeros(self.memory_size, self.width, dtype=torch.float32,
                                 device=self.device)
        if self.is_pixel:
            self.frame_bytes = int(np.prod(self.camera_shape))
        self.share_frames = False
        shared = frame_sharing(learner_config, env_config)
        if shared is not None:
            self._init_shared(*shared)
        elif self.is_pixel:
            self.frames = torch.zeros((self.memory_size,) + self.camera_shape, dtype=torch.uint8,
                                      device=self.device)
            self.frames_next = torch.zeros_like(self.frames)
        self._len = 0
        self._next_idx = 0
        self.rng = CPythonRandom(seed, self.device)
        self._idx = None
        self._out = None

    def _init_shared(self, stack, frame_shape, frame_slots):
        self.share_frames = True
        self.frame_stacks, self.frame_shape = stack, frame_shape
        self.fbytes = int(np.prod(frame_shape))
        self._alloc = FrameAllocator(self.memory_size, frame_slots, stack)
        self.frame_store = torch.zeros((frame_slots,) + frame_shape, dtype=torch.uint8,
                                       device=self.device)
        self.frame_ids = torch.zeros(self.memory_size, 2, stack, dtype=torch.int32,
                                     device=self.device)
        self._stage = None                 # (pinned host bytes, device bytes, copy-done event)

    @property
    def frame_slots(self):
        return self._alloc.frame_slots

    @property
    def frames_in_use(self):
        """store slots that hold a frame some live transition names"""
        return self._alloc.frames_in_use

    def __len__(self):
        return self._len

    def insert(self, exp_dict):
        """uniform_replay.py:36-41 for one SSAR experience dict."""
        if self.is_pixel:
            self.insert_rows(*self.pack([exp_dict]))
            return
        row = self.pack([exp_dict])
        self.insert_rows(row)

    def pack(self, exps):
        if self.share_frames:
            return self._pack_shared(exps)
        if self.is_pixel:
            return pack_pixel_exps(exps, self.obs_dim, self.act_dim, self.camera_shape)
        return pack_rows(exps, self.obs_dim, self.act_dim)

    def _pack_shared(self, exps):
        """pack() of the frame-shared mode: (rows, frames of obs, frames of
        obs_next), the frames as one list of S uint8 arrays per experience.
        camera0 may be a list of S frames or one (C, H, W) array; an object
        that several experiences share comes back as the same arrays, so
        insert_rows digests it once."""
        S = self.frame_stacks
        pix, pix_next, cache = [], [], {}
        for e in exps:
            o0, o1 = e['obs']
            pix.append(split_camera(o0['pixel']['camera0'], S, self.frame_shape, cache))
            pix_next.append(split_camera(o1['pixel']['camera0'], S, self.frame_shape, cache))
        return pack_rows(exps, self.obs_dim, self.act_dim), pix, pix_next

    def _check_insert(self, rows, pix, pix_next):
        """insert_rows of a pixel replay: rows [n, W] come with pix and pix_next,
        each uint8 (n, C, H, W) (returned as tensors) or, frame-shared, a list
        of n lists of S frames (returned as given)"""
        n = rows.shape[0]
        if pix is None or pix_next is None:
            raise ValueError('a pixel replay inserts rows together with pix and pix_next')
        sides = []
        for name, f in (('pix', pix), ('pix_next', pix_next)):
            if self.share_frames and isinstance(f, (list, tuple)) and (
                    not len(f) or isinstance(f[0], (list, tuple))):
                if len(f) != n:
                    raise ValueError(f'{name} holds {len(f)} observations for {n} rows')
            else:
                f = torch.as_tensor(f)
                if f.dtype != torch.uint8 or tuple(f.shape) != (n,) + self.camera_shape:
                    raise ValueError(f'{name} must be uint8 {(n,) + self.camera_shape}, got '
                                     f'{f.dtype} {tuple(f.shape)}')
            sides.append(f)
        if tuple(rows.shape) != (n, self.width):
            raise ValueError(f'rows must be ({n}, {self.width}), got {tuple(rows.shape)}')
        return sides

    def _side_frames(self, pix, n):
        """one checked side of insert_rows -> n lists of S contiguous uint8 frames"""
        S = self.frame_stacks
        if not isinstance(pix, torch.Tensor):
            return [split_camera(f, S, self.frame_shape) for f in pix]
        a = np.ascontiguousarray(pix.cpu().numpy()).reshape((n, S) + self.frame_shape)
        return [[a[i, k] for k in range(S)] for i in range(n)]

    def _insert_shared(self, rows, pix, pix_next):
        rows = np.ascontiguousarray(torch.as_tensor(rows, dtype=torch.float32).cpu().numpy())
        n = rows.shape[0]
        pix, pix_next = self._check_insert(rows, pix, pix_next)
        skip = max(0, n - self.memory_size)
        sides = list(zip(self._side_frames(pix, n)[skip:], self._side_frames(pix_next, n)[skip:]))
        # raises RuntimeError, with nothing changed, when the store is full
        first, ids, fslots, new = self._alloc.insert(sides, skipped=skip)
        cnt, m, fb = n - skip, len(new), self.fbytes
        # one pinned block [new frames | rows | ids | fslots], the float and
        # int parts from a 16-byte boundary on
        o_rows = (m * fb + 15) // 16 * 16
        o_ids = o_rows + cnt * self.width * 4
        o_slots = o_ids + ids.size * 4
        total = o_slots + m * 4
        if total:
            if self._stage is None or self._stage[0].numel() < total:
                cap = max(total, 2 * self._stage[0].numel() if self._stage else 0)
                if self._stage is not None and self._stage[2] is not None:
                    self._stage[2].synchronize()
                self._stage = (torch.empty(cap, dtype=torch.uint8).pin_memory(),
                               torch.empty(cap, dtype=torch.uint8, device=self.device), None)
            host, dev, done = self._stage
            if done is not None:
                done.synchronize()         # the previous copy has read the pinned block
            h = host.numpy()
            for j, f in enumerate(new):
                h[j * fb:(j + 1) * fb] = f.reshape(-1)
            h[o_rows:o_ids].view(np.float32)[:] = rows[skip:].reshape(-1)
            h[o_ids:o_slots].view(np.int32)[:] = ids.reshape(-1)
            h[o_slots:total].view(np.int32)[:] = fslots
            dev[:total].copy_(host[:total], non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            self._stage = (host, dev, done)
            base = dev.data_ptr()

            def at(off, count):
                return ctypes.c_void_p(base + off) if count else None
            L.call('smi_replay_insert_shared', L.ptr(self.table), self.width,
                   L.ptr(self.frame_ids), self.frame_stacks, L.ptr(self.frame_store), fb,
                   self.memory_size, first, at(o_rows, cnt), at(o_ids, cnt), cnt, at(0, m),
                   at(o_slots, m), m, L.stream(self.device))
        self._len = min(self.memory_size, self._len + n)
        self._next_idx = int((self._next_idx + n) % self.memory_size)

    def insert_rows(self, rows, pix=None, pix_next=None):
        """Bulk ring insert of packed rows (same slot sequence as repeated insert);
        pixel mode: with their uint8 (n, C, H, W) frames.  Frame-shared mode
        also takes what its pack() returns (per experience a list of S frames)
        and stores only the frames the store does not hold yet."""
        if self.share_frames:
            return self._insert_shared(rows, pix, pix_next)
        rows = torch.as_tensor(rows, dtype=torch.float32)
        n = rows.shape[0]
        if self.is_pixel:
            pix, pix_next = self._check_insert(rows, pix, pix_next)
        elif pix is not None or pix_next is not None:
            raise ValueError('this replay has no pixel observations (no "pixel" in the obs spec)')
        # more rows than slots: only the last memory_size survive a sequence of
        # single inserts; scatter just those (no duplicate slot indices)
        skip = max(0, n - self.memory_size)
        slots = (self._next_idx + np.arange(skip, n)) % self.memory_size
        slots = torch.as_tensor(slots, device=self.device)
        self.table[slots] = rows[skip:].to(self.device)
        if self.is_pixel:
            self.frames[slots] = pix[skip:].to(self.device)
            self.frames_next[slots] = pix_next[skip:].to(self.device)
        self._len = min(self.memory_size, self._len + n)
        self._next_idx = int((self._next_idx + n) % self.memory_size)

    def start_sample_condition(self):
        return len(self) > self.sampling_start_size

    def sample_indices(self, batch_size):
        if self._idx is None or self._idx.numel() != batch_size:
            self._idx = torch.empty(batch_size, dtype=torch.int64, device=self.device)
        return self.rng.randint_device(len(self), batch_size, self._idx)

    def _draw_indices(self, batch_size, rank, world, **draw):
        """(idx_all, this rank's slice of it, n = batch_size / world): the whole
        draw of sample_indices(batch_size, **draw), which every rank makes.
        ValueError, before anything is drawn, unless batch_size % world == 0
        and 0 <= rank < world."""
        if world < 1 or not 0 <= rank < world or batch_size % world:
            raise ValueError(f'batch_size {batch_size} must split evenly over {world} ranks')
        idx = self.sample_indices(batch_size, **draw)
        n = batch_size // world
        return idx, idx[rank * n:(rank + 1) * n], n

    def _draw(self, batch_size, rank, world, **draw):
        """The one draw path of sample_batch and sample_shard: (idx_all, mine,
        batch), the batch gathered for this rank's n slots into buffers that
        are allocated once per n and overwritten by the next call."""
        idx, mine, n = self._draw_indices(batch_size, rank, world, **draw)
        if self._out is None or self._out[0].shape[0] != n:
            self._out = (torch.empty(n, self.width, dtype=torch.float32, device=self.device),)
            if self.is_pixel:
                self._out += tuple(torch.empty((n,) + self.camera_shape, dtype=torch.uint8,
                                               device=self.device) for _ in range(2))
        return idx, mine, self._gather_batch(mine, n)

    def sample(self, batch_size, out=None, rank=0, world=1, **draw):
        """Returns (indices, rows[batch, W]) on device; rows gathered by kernel.

        Data parallel (world > 1, SURVEY §8(e) DDPG row): every rank holds the
        same replicated ring and the same MT19937 state (same seed, same
        inserts), so all ranks draw the SAME `batch_size` global indices -- the
        one CPython-exact stream a single learner draws
        (uniform_replay.py:43-47) -- and gather only their own slice of
        batch_size / world rows: the sampling stays bit-exact and the shards
        concatenate to the single learner's batch."""
        if self.is_pixel:
            raise ValueError('a pixel replay samples rows together with their frames: '
                             'use sample_batch()')
        _, mine, n = self._draw_indices(batch_size, rank, world, **draw)
        if out is None:
            out = torch.empty(n, self.width, dtype=torch.float32, device=self.device)
        if tuple(out.shape) != (n, self.width) or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous ({n}, {self.width}) tensor')
        L.call('smi_gather_rows', L.ptr(self.table), self.width, L.ptr(mine), n, L.ptr(out),
               L.stream(self.device))
        return mine, out

    def sample_batch(self, batch_size, rank=0, world=1, **draw):
        """Returns (indices, batch): the draw of sample() (same CPython-exact
        stream, same rank slicing) gathered into the batch DDPGLearner.learn()
        takes.  Low-dim: split(rows), one smi_gather_rows.  Pixel: one
        smi_replay_gather (frame-shared: smi_replay_gather_shared, through the
        frame ids) moves this rank's rows and both frames of each;
        batch = {'obs': {'pixel': {'camera0': u8 [n, C, H, W]}, 'low_dim':
        {'flat_inputs': [n, D]}}, 'obs_next': likewise, 'actions', 'rewards',
        'dones'} ('low_dim' omitted when D == 0).  The output buffers are
        allocated once per n and overwritten by the next call."""
        _, mine, batch = self._draw(batch_size, rank, world, **draw)
        return mine, batch

    def sample_shard(self, batch_size, rank, world, **draw):
        """Returns (idx_all, batch) for one rank of a data-parallel learner
        (DQNLearner / DDPGLearner(dp=...)): idx_all is the WHOLE draw, int64
        [batch_size] on the device (overwritten by the next draw), and batch is
        sample_batch's dict for rows [rank * n, (rank + 1) * n) of it, n =
        batch_size / world, gathered by the same kernels over the index slice.
        Every replica draws all batch_size indices from the one CPython-exact
        stream, so replicas seeded and fed alike keep identical generators."""
        idx_all, _, batch = self._draw(batch_size, rank, world, **draw)
        return idx_all, batch

    def _gather_batch(self, mine, n):
        """sample_batch's dict for the n drawn slots `mine`, into self._out"""
        if not self.is_pixel:
            rows = self._out[0]
            L.call('smi_gather_rows', L.ptr(self.table), self.width, L.ptr(mine), n, L.ptr(rows),
                   L.stream(self.device))
            return self.split(rows)
        rows, pix, pix_next = self._out
        if self.share_frames:
            L.call('smi_replay_gather_shared', L.ptr(self.table), self.width,
                   L.ptr(self.frame_store), L.ptr(self.frame_ids), self.frame_stacks, self.fbytes,
                   L.ptr(mine), n, L.ptr(rows), L.ptr(pix), L.ptr(pix_next), L.stream(self.device))
        else:
            L.call('smi_replay_gather', L.ptr(self.table), self.width, L.ptr(self.frames),
                   L.ptr(self.frames_next), self.frame_bytes, L.ptr(mine), n, L.ptr(rows),
                   L.ptr(pix), L.ptr(pix_next), L.stream(self.device))
        flat = self.split(rows)
        obs, obs_next = {'pixel': {'camera0': pix}}, {'pixel': {'camera0': pix_next}}
        if self.obs_dim:
            obs['low_dim'] = {'flat_inputs': flat['obs']}
            obs_next['low_dim'] = {'flat_inputs': flat['obs_next']}
        return {'obs': obs, 'obs_next': obs_next, 'actions': flat['actions'],
                'rewards': flat['rewards'], 'dones': flat['dones']}

    def split(self, rows):
        D, A = self.obs_dim, self.act_dim
        return {'obs': rows[:, :D], 'actions': rows[:, D:D + A],
                'rewards': rows[:, D + A:D + A + 1], 'obs_next': rows[:, D + A + 1:2 * D + A + 1],
                'dones': rows[:, 2 * D + A + 1:2 * D + A + 2]}


class PrioritizedReplay(UniformReplay):
    """Proportional prioritized replay (prioritized_replay.py, segment_tree.py)
    on the device ring.  The reference class cannot be constructed (its super()
    names another class, it reads self._storage, sample returns only the
    experiences), so its text is read as the openai/baselines code it was
    adapted from; the decisions are listed in csrc/per_kernels.hip and
    INTEGRATION.md.  In short: fp64 trees over capacity = the smallest power
    of two >= memory_size; a written slot gets max_priority ** alpha; a draw is
    find_prefixsum_idx(random.random() * sum(slots 0 .. len-2)) on the
    CPython-exact stream (slot len-1 is never drawn, as in baselines); weights
    (p_i * len) ** -beta / max_w; a repeated index keeps its last priority.

    alpha is read from learner_config.replay.alpha, as the reference does.
    Data parallel: every rank keeps a replicated replay (same seed, same
    inserts) and calls sample_shard(), which draws the whole global batch on
    every rank and gathers the rank's rows; after DQNLearner / DDPGLearner
    (dp=...).learn() every rank applies update_priorities_from_td(idx_all, learner.td_error),
    the TD errors of the whole draw in draw order, so the trees stay
    bit-identical.  sample() and sample_batch() are the one-rank calls:
    world != 1 raises ValueError there."""

    def __init__(self, learner_config, env_config, session_config=None, index=0, seed=0,
                 device=None):
        super().__init__(learner_config, env_config, session_config, index, seed, device)
        self.alpha = float(learner_config['replay']['alpha'])
        if not self.alpha > 0:
            raise ValueError(f'replay.alpha must be > 0, got {self.alpha}')
        self.capacity = 1
        while self.capacity < self.memory_size:
            self.capacity *= 2
        self.tree = torch.empty(int(L.lib().smi_per_tree_doubles(self.capacity)),
                                dtype=torch.float64, device=self.device)
        L.call('smi_per_init', L.ptr(self.tree), self.capacity, L.stream(self.device))
        self.weights = None

    @property
    def max_priority(self):
        """host copy of the running maximum priority (synchronises)"""
        return float(self.tree[0].item())

    def insert_rows(self, rows, pix=None, pix_next=None):
        """UniformReplay.insert_rows; the written slots get max_priority ** alpha"""
        first = self._next_idx
        n = int(torch.as_tensor(rows).shape[0])
        super().insert_rows(rows, pix, pix_next)
        L.call('smi_per_insert', L.ptr(self.tree), self.capacity, first, n, self.memory_size,
               self.alpha, L.stream(self.device))

    def sample_indices(self, batch_size, beta=0):
        """batch_size proportional draws; their weights are kept in self.weights"""
        if self._idx is None or self._idx.numel() != batch_size:
            self._idx = torch.empty(batch_size, dtype=torch.int64, device=self.device)
            self.weights = torch.empty(batch_size, dtype=torch.float32, device=self.device)
        L.call('smi_per_sample', L.ptr(self.tree), self.capacity, len(self), L.ptr(self.rng.dev),
               int(batch_size), float(beta), L.ptr(self._idx), L.ptr(self.weights),
               L.stream(self.device))
        return self._idx

    @staticmethod
    def _one_rank(world):
        if world != 1:
            raise ValueError('sample() and sample_batch() of a prioritized replay take world = 1: '
                             'a data-parallel rank calls sample_shard(batch_size, rank, world), '
                             'which keeps the replicated trees identical')

    def _draw(self, batch_size, rank, world, beta=0):
        """UniformReplay._draw over the proportional draw: smi_per_sample draws
        the whole batch on every rank, and batch['weights'] is this rank's
        slice, float32 [n, 1], where the learners read it (the weights are
        normalised by the tree minimum, not by the batch, so they do not depend
        on the shard).  After learn(), every rank of sample_shard() calls
        update_priorities_from_td(idx_all, learner.td_error)."""
        idx_all, mine, batch = super()._draw(batch_size, rank, world, beta=beta)
        n = batch_size // world
        batch['weights'] = self.weights[rank * n:(rank + 1) * n].view(-1, 1)
        return idx_all, mine, batch

    def sample(self, batch_size, out=None, rank=0, world=1, beta=0):
        """(indices, rows, weights [batch] float32) on the device"""
        self._one_rank(world)
        idx, rows = super().sample(batch_size, out=out, beta=beta)
        return idx, rows, self.weights

    def sample_batch(self, batch_size, rank=0, world=1, beta=0):
        """UniformReplay.sample_batch over the prioritized draw, for one rank"""
        self._one_rank(world)
        return super().sample_batch(batch_size, beta=beta)

    def _indices(self, indices):
        if isinstance(indices, torch.Tensor):
            return indices.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        return torch.as_tensor(np.asarray(indices, dtype=np.int64).reshape(-1), device=self.device)

    def update_priorities(self, indices, priorities):
        """tree[idx] = priority ** alpha in the sequential loop's meaning (a
        repeated index keeps its last priority), max_priority raised to the
        largest one.  Host floats are raised to alpha on the host in fp64;
        device tensors stay on the device."""
        idx = self._indices(indices)
        if not idx.numel() and not len(priorities):
            return
        if isinstance(priorities, torch.Tensor) and priorities.is_cuda:
            p = priorities.to(torch.float64).contiguous().view(-1)
            leaf = p.pow(self.alpha)
            top = p.max().view(1)
        else:
            p = np.asarray(priorities, dtype=np.float64).reshape(-1)
            if not np.all(p > 0):
                raise ValueError('priorities must be > 0')
            leaf = torch.as_tensor(np.array([float(v) ** self.alpha for v in p], dtype=np.float64),
                                   device=self.device)
            top = torch.as_tensor(np.array([p.max()]), device=self.device)
        if idx.numel() != leaf.numel():
            raise ValueError(f'{idx.numel()} indices, {leaf.numel()} priorities')
        L.call('smi_per_set', L.ptr(self.tree), self.capacity, L.ptr(idx), L.ptr(leaf), idx.numel(),
               L.stream(self.device))
        torch.maximum(self.tree[0:1], top, out=self.tree[0:1])

    def update_priorities_from_td(self, indices, td, eps=1e-6):
        """priority = |td| + eps from a float32 device tensor of TD errors
        (DDPGLearner.td_error), one launch, no synchronisation"""
        idx = self._indices(indices)
        if not (isinstance(td, torch.Tensor) and td.is_cuda and td.dtype == torch.float32):
            raise ValueError('td must be a float32 device tensor')
        if td.dim() == 2 and td.shape[1] == 1:
            td = td[:, 0]
        if td.dim() != 1 or td.shape[0] != idx.numel():
            raise ValueError(f'{idx.numel()} indices, td of shape {tuple(td.shape)}')
        L.call('smi_per_update_td', L.ptr(self.tree), self.capacity, L.ptr(idx), L.ptr(td),
               td.stride(0) if td.numel() > 1 else 1, idx.numel(), float(eps), self.alpha,
               L.stream(self.device))


class FIFOReplay(object):
    """fifo_replay.py:6-49: popleft x batch in insertion order."""

    def __init__(self, learner_config, env_config=None, session_config=None, index=0):
        self.batch_size = learner_config['replay']['batch_size']
        self.memory_size = learner_config['replay']['memory_size']
        self._memory = deque(maxlen=self.memory_size + 3)

    def insert(self, exp_tuple):
        self._memory.append(exp_tuple)

    def sample(self, batch_size):
        assert batch_size <= self.memory_size
        return [self._memory.popleft() for _ in range(batch_size)]

    def start_sample_condition(self):
        return len(self._memory) >= self.batch_size

    def __len__(self):
        return len(self._memory)
