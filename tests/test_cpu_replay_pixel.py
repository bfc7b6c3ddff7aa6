"""CPU tests of the pixel replay: the argument checks of smi_replay_gather (no
launch is made) and the host-side packing of camera experiences."""
import ctypes

import numpy as np
import pytest


def test_replay_gather_rejects_bad_args():
    from surreal_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)                  # never dereferenced: no launch is made

    def bad(*args):
        assert lib.smi_replay_gather(*args) == -1
        assert b'replay_gather' in lib.smi_last_error()

    #   table cols frames next fb   idx batch rows pix pixn stream
    bad(None, 0, None, None, 1200, p, 4, None, None, None, None)       # NULL pixel pointers
    bad(None, 0, p, p, 1200, p, 4, None, p, None, None)                # one NULL output
    bad(None, 0, p, p, 1200, None, 4, None, p, p, None)                # NULL idx
    bad(None, 0, p, p, 0, p, 4, None, p, p, None)                      # frame_bytes = 0
    bad(None, 0, p, p, 1200, p, -1, None, p, p, None)                  # batch = -1
    bad(None, -1, p, p, 1200, p, 4, None, p, p, None)                  # cols = -1
    bad(None, 4, p, p, 1200, p, 4, p, p, p, None)                      # cols = 4, NULL table
    bad(p, 4, p, p, 1200, p, 4, None, p, p, None)                      # cols = 4, NULL rows_out
    assert lib.smi_replay_gather(p, 4, p, p, 1200, p, 0, p, p, p, None) == 0   # batch = 0
    assert lib.smi_replay_gather(None, 0, p, p, 1200, p, 0, None, p, p, None) == 0


def _exps():
    rs = np.random.RandomState(0)
    D, A, cam = 5, 2, (9, 20, 20)
    frames = rs.randint(0, 256, (3, 2) + cam).astype(np.uint8)
    low = rs.randn(3, 2, D).astype(np.float32)
    act = rs.randn(3, A).astype(np.float32)
    rew = rs.randn(3)
    done = [False, True, False]

    def cam_of(i, j):
        f = frames[i, j]
        if (i, j) == (0, 1):                     # per-frame list, concatenated along channels
            return [f[0:3], f[3:6], f[6:9]]
        if (i, j) == (2, 0):                     # float array of integral values
            return f.astype(np.float64)
        return f
    exps = [{'obs': [{'low_dim': {'flat_inputs': low[i, j]}, 'pixel': {'camera0': cam_of(i, j)}}
                     for j in range(2)],
             'action': act[i], 'reward': rew[i], 'done': done[i]} for i in range(3)]
    return exps, frames, low, act, rew, done


def test_pack_pixel_exps():
    from surreal_amd.replay import pack_pixel_exps
    D, A, cam = 5, 2, (9, 20, 20)
    exps, frames, low, act, rew, done = _exps()
    rows, pix, pix_next = pack_pixel_exps(exps, D, A, cam)
    assert rows.dtype == np.float32 and rows.shape == (3, 2 * D + A + 2)
    assert pix.dtype == np.uint8 and pix_next.dtype == np.uint8
    assert pix.shape == (3,) + cam and pix_next.shape == (3,) + cam
    exp_rows = np.concatenate([low[:, 0], act, rew.astype(np.float32)[:, None], low[:, 1],
                               np.asarray(done, np.float32)[:, None]], axis=1)
    assert rows.tobytes() == exp_rows.tobytes()
    assert pix.tobytes() == frames[:, 0].tobytes()
    assert pix_next.tobytes() == frames[:, 1].tobytes()

    half = [dict(e) for e in exps]
    half[1] = dict(half[1], obs=[half[1]['obs'][0],
                                 {'low_dim': half[1]['obs'][1]['low_dim'],
                                  'pixel': {'camera0': np.full(cam, 0.5)}}])
    with pytest.raises(TypeError):
        pack_pixel_exps(half, D, A, cam)
    for v in (-1.0, 256.0):
        half[1]['obs'][1]['pixel']['camera0'] = np.full(cam, v)
        with pytest.raises(TypeError):
            pack_pixel_exps(half, D, A, cam)

    # pixel-only spec: D = 0, the row is [action | reward | done]
    only = [{'obs': [{'pixel': o['pixel']} for o in e['obs']], 'action': e['action'],
             'reward': e['reward'], 'done': e['done']} for e in exps]
    rows0, pix0, pixn0 = pack_pixel_exps(only, 0, A, cam)
    assert rows0.shape == (3, A + 2)
    exp0 = np.concatenate([act, rew.astype(np.float32)[:, None],
                           np.asarray(done, np.float32)[:, None]], axis=1)
    assert rows0.tobytes() == exp0.tobytes()
    assert pix0.tobytes() == pix.tobytes() and pixn0.tobytes() == pix_next.tobytes()
