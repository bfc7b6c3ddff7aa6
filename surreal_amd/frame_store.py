"""Host bookkeeping of the frame-shared pixel replay (numpy + stdlib, no GPU).

The reference never stores a camera frame twice: with
frame_stack_concatenate_on_env False an observation's camera0 is a list of
frame_stacks single frames, ExpBuffer._hash_nested (distributed/exp_sender.py:
45-59) hashes every leaf, and exp_collector._retrieve_storage hands every
experience that names a hash the same object.  FrameAllocator gives the device
replay the same storage model: a store of single (C/S, H, W) frames, a
reference count per store slot, and for every transition slot the 2 x S store
slots of its two observations.  A frame is recognised by a 128-bit digest of
its bytes (equal digests are taken as equal frames, the bet binary_hash makes)
or, within one call, by the identity of the array object."""
import hashlib
from collections import deque

import numpy as np


def frame_digest(frame):
    """128-bit content key of one contiguous uint8 frame"""
    return hashlib.blake2b(frame, digest_size=16).digest()


def frame_sharing(learner_config, env_config):
    """The frame-shared layout a replay is configured for: None when
    learner_config.replay.share_frames is absent or False, else
    (S, (C/S, H, W), frame_slots).  ValueError for share_frames without a
    'pixel' obs spec, C % S != 0 or frame_slots < 1."""
    rc = learner_config['replay']
    if not ('share_frames' in rc and rc['share_frames']):
        return None
    spec = env_config['obs_spec']
    if 'pixel' not in spec:
        raise ValueError('replay.share_frames needs camera observations (a "pixel" entry in the '
                         'obs spec)')
    C, H, W = (int(c) for c in spec['pixel']['camera0'])
    S = int(env_config['frame_stacks'])
    if S < 1 or S > 4 or C % S:
        raise ValueError(f'replay.share_frames: the {C} camera channels do not split into '
                         f'frame_stacks = {S} frames (1 <= frame_stacks <= 4, C % frame_stacks == 0)')
    memory_size = int(rc['memory_size'])
    # M consecutive transitions of one actor name M + S frames; episode ends
    # and interleaved actors add a few each: a quarter on top is a generous,
    # documented (not measured) default
    slots = int(rc['frame_slots']) if 'frame_slots' in rc and rc['frame_slots'] else \
        memory_size + memory_size // 4
    if slots < 1:
        raise ValueError(f'replay.frame_slots must be >= 1, got {slots}')
    return S, (C // S, H, W), slots


def _frame_u8(f, shape):
    """one frame -> contiguous uint8 of `shape`, by the rules of replay._camera_u8"""
    a = np.asarray(f)
    if a.dtype != np.uint8:
        if not (np.all(a == np.round(a)) and a.min() >= 0 and a.max() <= 255):
            raise TypeError('camera observations must hold uint8 pixel values')
        a = a.astype(np.uint8)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f'a camera0 frame has shape {tuple(a.shape)}, the obs spec and '
                         f'frame_stacks say {tuple(shape)}')
    return np.ascontiguousarray(a)


def split_camera(cam, stack, frame_shape, cache=None):
    """camera0 of one observation -> list of `stack` uint8 frames.  cam is a
    list of `stack` per-frame arrays or one (C, H, W) array, split along
    channels.  `cache` (id(object) -> result, for the length of one call) keeps
    the frames of an object that several experiences share the same objects."""
    key = id(cam)
    if cache is not None and key in cache:
        return cache[key][1]
    c = frame_shape[0]
    if isinstance(cam, (list, tuple)) and len(cam) == stack:
        out = []
        for f in cam:
            if cache is not None and id(f) in cache:
                out.append(cache[id(f)][1])
                continue
            u = _frame_u8(f, frame_shape)
            if cache is not None:
                cache[id(f)] = (f, u)             # f is kept alive: its id stays its own
            out.append(u)
    else:
        if isinstance(cam, (list, tuple)):
            cam = np.concatenate([np.asarray(f) for f in cam], axis=0)
        a = np.asarray(cam)
        full = (stack * c,) + tuple(frame_shape[1:])
        if tuple(a.shape) != full:
            raise ValueError(f'camera0 has shape {tuple(a.shape)}, the obs spec says {full}')
        out = [_frame_u8(a[k * c:(k + 1) * c], frame_shape) for k in range(stack)]
    if cache is not None:
        cache[key] = (cam, out)
    return out


class FrameAllocator(object):
    """Reference counts, FIFO free list, key -> slot dictionary and the host
    mirror of frame_ids ([memory_size][2][S] int32) of a frame-shared replay.

    insert() takes the surviving transitions of one call in ring order; each
    acquires its 2 S frames first (a known key adds a reference, an unknown one
    takes a free slot and is listed as new) and only then releases the 2 S
    references of the transition it overwrites, so a frame both of them name
    is never dropped and re-uploaded, and a slot is written at most once per
    call.  A full store raises RuntimeError and leaves every field as it was."""

    def __init__(self, memory_size, frame_slots, stack):
        self.memory_size = int(memory_size)
        self.frame_slots = int(frame_slots)
        self.stack = int(stack)
        self.refcount = np.zeros(self.frame_slots, dtype=np.int32)
        self.free = deque(range(self.frame_slots))
        self.slot_of = {}                               # key -> slot of every live frame
        self.key_of = [None] * self.frame_slots         # slot -> key
        self.ids = np.full((self.memory_size, 2, self.stack), -1, dtype=np.int32)
        self._len = 0
        self._next_idx = 0

    def __len__(self):
        return self._len

    @property
    def frames_in_use(self):
        return self.frame_slots - len(self.free)

    def insert(self, transitions, skipped=0):
        """transitions: per surviving transition (frames of obs, frames of
        obs_next), each a list of S contiguous uint8 arrays; skipped: how many
        transitions of the call went before them and did not survive (n >
        memory_size).  Returns (first ring slot written, ids int32 [cnt][2][S],
        store slots of the new frames int32 [m], the m new frames)."""
        M, S = self.memory_size, self.stack
        cnt = len(transitions)
        if cnt > M:
            raise ValueError(f'{cnt} transitions for a ring of {M}: pass the last {M} only')
        first = (self._next_idx + skipped) % M
        ids = np.empty((cnt, 2, S), dtype=np.int32)
        new_slots, new_frames = [], []
        key_by_id = {}                                  # id(array) -> key, this call only
        journal = []          # (took?, slot, key when the slot entered / left the dictionary)
        old_rows = self.ids[(first + np.arange(cnt)) % M].copy()
        try:
            for e, sides in enumerate(transitions):
                for j, frames in enumerate(sides):
                    if len(frames) != S:
                        raise ValueError(f'an observation has {len(frames)} frames, frame_stacks '
                                         f'is {S}')
                    for k, f in enumerate(frames):
                        key = key_by_id.get(id(f))
                        if key is None:
                            key = frame_digest(f)
                            key_by_id[id(f)] = key
                        slot = self.slot_of.get(key)
                        if slot is None:
                            if not self.free:
                                raise RuntimeError(
                                    f'the frame store is full: all replay.frame_slots = '
                                    f'{self.frame_slots} hold live frames; raise replay.frame_slots')
                            slot = self.free.popleft()
                            self.slot_of[key] = slot
                            self.key_of[slot] = key
                            new_slots.append(slot)
                            new_frames.append(f)
                            journal.append((True, slot, key))
                        else:
                            journal.append((True, slot, None))
                        self.refcount[slot] += 1
                        ids[e, j, k] = slot
                ring = (first + e) % M
                # the ring slot holds a live transition once the ring is full
                # or, before that, never (slots fill in order from 0)
                if self._len == M or ring < self._len:
                    for slot in self.ids[ring].ravel():
                        slot = int(slot)
                        self.refcount[slot] -= 1
                        if self.refcount[slot] == 0:
                            key = self.key_of[slot]
                            del self.slot_of[key]
                            self.key_of[slot] = None
                            self.free.append(slot)
                            journal.append((False, slot, key))
                        else:
                            journal.append((False, slot, None))
                self.ids[ring] = ids[e]
        except BaseException:
            for took, slot, key in reversed(journal):
                if took:
                    self.refcount[slot] -= 1
                    if key is not None:
                        del self.slot_of[key]
                        self.key_of[slot] = None
                        self.free.appendleft(slot)
                else:
                    if key is not None:
                        self.free.pop()
                        self.slot_of[key] = slot
                        self.key_of[slot] = key
                    self.refcount[slot] += 1
            self.ids[(first + np.arange(cnt)) % M] = old_rows
            raise
        total = skipped + cnt
        self._len = min(M, self._len + total)
        self._next_idx = (self._next_idx + total) % M
        return first, ids, np.asarray(new_slots, dtype=np.int32), new_frames
