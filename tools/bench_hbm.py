"""HBM-roofline sweep of the streaming kernels on the learner path.

Each kernel runs on working sets well beyond the 256 MiB Infinity Cache, timed
with HIP events on the stream it is launched on (median of --iters launches
after warm-up).  achieved GB/s = ALGORITHMIC bytes per launch / duration, where
the algorithmic bytes are the §8(d) per-unit figures:

  gae_windows (non-RNN, T=50, H=T)  r,d 8 B + V 4(T+1)/T B + adv,ret 8/T B per env-step
  gae_windows (RNN, T=25, H=5)      r,d 8 B + V 4(T+1)/T B + adv,ret 8E/T B per env-step
  zfilter_apply (D=42)              8 D B per row (read x, write out)
  zfilter_update (D=42)             4 D B per row (read x; 2D+1 floats written)
  diag_gauss kl+loglik+ent (A=8)    a 4A + p0 8A + p1 8A read, 3 x 4 B written per row
  adam_clip                         p,g,m,v read 16 B + p,m,v written 12 B per param: SURVEY
                                    §8(d)'s 28 B (the norm pass's second read of g, 4 B more
                                    moved, is NOT counted; frac_moved adds it); g spans 3 x 2^26
                                    floats (768 MiB, > 2 x the MALL) so that re-read cannot hit
                                    the Infinity Cache
  adam_noclip                       p,g,m,v read 16 B + p,m,v written 12 B per param
  gather_rows (W=42 floats)         8 idx + 2 x 4 W B per gathered row
  replay_gather (9x84x84 u8, W=42)  8 idx + 2 sides x 2 x 63504 B + 2 x 4 W B per sample (B = 512,
                                    8,192-slot rings); replay_gather_baseline3 is the same
                                    gather as two torch.index_select + one smi_gather_rows
  replay_gather_shared              the same sample from the frame-shared store (3x84x84 frames,
                                    S = 3, ids of a rolling stream: the two sides of a transition
                                    share two frames): 8 idx + 2 x S x 4 id B + 2 sides x 2 x
                                    63504 B + 2 x 4 W B per sample; replay_gather_shared_distinct
                                    gives every transition 2 S frames of its own (a store as
                                    large as the two rings, no frame read twice)
  replay_insert                     host wall time of one insert call of 64 rolling-stream
                                    transitions of 9x84x84 ending in a synchronise, frame-shared
                                    against unshared, with the bytes each uploads and the host
                                    time of the digests
  moments                           4 B per element

peak = 8000 GB/s (MI355X HBM3E spec, MI355X_MICROARCH.md).  Prints one JSON line
per kernel.  Usage: python tools/bench_hbm.py [--iters 20] [--only name,...]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from surreal_amd import _lib as L  # noqa: E402

PEAK = 8000.0


def timed(fn, iters, warm=3, spread=False):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) for s, e in evs)
    return ts if spread else ts[len(ts) // 2]     # spread: every repeat, sorted


def report(name, nbytes, ms, **extra):
    gbs = nbytes / (ms * 1e-3) / 1e9
    out = {'kernel': name, 'algorithmic_bytes': int(nbytes), 'median_ms': round(ms, 4),
           'achieved_GBs': round(gbs, 1), 'peak_GBs': PEAK, 'frac': round(gbs / PEAK, 4)}
    out.update(extra)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    only = set(args.only.split(',')) if args.only else None
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    L.ensure_workspace(dev)
    st = L.stream(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    P = L.ptr

    def want(n):
        return only is None or n in only

    for name, B, T, H in (('gae_windows_nonrnn', 1 << 20, 50, 50), ('gae_windows_rnn', 1 << 21, 25, 5)):
        if not want(name):
            continue
        E = T - H + 1
        r = torch.randn(B, T, device=dev, generator=g)
        d = (torch.rand(B, T, device=dev, generator=g) < 0.02).float()
        v = torch.randn(B, T + 1, device=dev, generator=g)
        gt = torch.pow(0.99, torch.arange(T, dtype=torch.float32)).to(dev)
        lt = torch.pow(0.95, torch.arange(T, dtype=torch.float32)).to(dev)
        adv = torch.empty(B, E, device=dev)
        ret = torch.empty(B, E, device=dev)
        npart = L.lib().smi_gae_windows_max_partials(B, T)
        parts = torch.empty(2 * npart, dtype=torch.float64, device=dev)
        np_out = ctypes.c_int(0)
        fn = lambda: L.call('smi_gae_windows', P(v), None, P(r), P(d), B, T, H, P(gt), P(lt), 0.99,  # noqa
                            float(0.99 ** H), P(adv), P(ret), P(parts), ctypes.byref(np_out), st)
        ms = timed(fn, args.iters)
        nbytes = B * T * 8 + B * (T + 1) * 4 + B * E * 8
        report(name, nbytes, ms, B=B, T=T, horizon=H, env_steps=B * T,
               bytes_per_env_step=round(nbytes / (B * T), 3))
        del r, d, v, adv, ret, parts

    D = 42
    if want('zfilter_apply'):
        rows = 1 << 22
        x = torch.randn(rows, D, device=dev, generator=g)
        out = torch.empty_like(x)
        zs, zq, zc = x[:1000].sum(0), (x[:1000] ** 2).sum(0), torch.tensor([1000.0], device=dev)
        fn = lambda: L.call('smi_zfilter_apply', P(x), P(out), rows, D, P(zs), P(zq), P(zc), 1e-5, st)  # noqa
        report('zfilter_apply', rows * D * 8, timed(fn, args.iters), rows=rows, dim=D)
        del x, out
    if want('zfilter_update'):
        rows = 1 << 22
        x = torch.randn(rows, D, device=dev, generator=g)
        zs, zq, zc = torch.zeros(D, device=dev), torch.zeros(D, device=dev), torch.ones(1, device=dev)
        fn = lambda: L.call('smi_zfilter_update', P(x), rows, D, D, P(zs), P(zq), P(zc), st)  # noqa
        report('zfilter_update', rows * D * 4, timed(fn, args.iters), rows=rows, dim=D)
        del x

    if want('diag_gauss'):
        rows, A = 1 << 23, 8
        a = torch.randn(rows, A, device=dev, generator=g)
        p0 = torch.rand(rows, 2 * A, device=dev, generator=g) + 0.5
        p1 = torch.rand(rows, 2 * A, device=dev, generator=g) + 0.5
        ll, kl, en = (torch.empty(rows, device=dev) for _ in range(3))
        fn = lambda: L.call('smi_diag_gauss', P(a), P(p0), P(p1), rows, A, P(ll), None, P(kl), P(en), st)  # noqa
        report('diag_gauss', rows * (4 * A + 16 * A + 12), timed(fn, args.iters), rows=rows, act_dim=A)
        del a, p0, p1, ll, kl, en

    if want('adam_clip'):
        n = 3 << 26
        p = torch.randn(n, device=dev, generator=g)
        gr = torch.randn(n, device=dev, generator=g)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        lr = torch.tensor([1e-4], device=dev)
        norm = torch.zeros(1, device=dev)
        fn = lambda: L.call('smi_adam_clip', P(p), P(gr), P(m), P(v), n, P(step), P(lr), 0.9,  # noqa
                            0.999, 1e-8, 0.0, 10.0, 0.0, None, P(norm), st)
        ms = timed(fn, args.iters)
        report('adam_clip', n * 28, ms, params=n,
               frac_moved=round(n * 32 / (ms * 1e-3) / 1e9 / PEAK, 4),
               note='28 B/param algorithmic (SURVEY 8(d)); frac_moved counts the norm pass (32 B)')
        fn2 = lambda: L.call('smi_adam_clip', P(p), P(gr), P(m), P(v), n, P(step), P(lr), 0.9,  # noqa
                             0.999, 1e-8, 0.0, 0.0, 0.0, None, None, st)
        report('adam_noclip', n * 28, timed(fn2, args.iters), params=n)
        del p, gr, m, v

    if want('gather_rows'):
        n_tab, W, batch = 1 << 22, 42, 1 << 21
        tab = torch.randn(n_tab, W, device=dev, generator=g)
        idx = torch.randint(0, n_tab, (batch,), device=dev, generator=g)
        out = torch.empty(batch, W, device=dev)
        fn = lambda: L.call('smi_gather_rows', P(tab), W, P(idx), batch, P(out), st)  # noqa
        report('gather_rows', batch * (8 + 8 * W), timed(fn, args.iters), table_rows=n_tab,
               cols=W, batch=batch)
        del tab, idx, out

    if want('replay_gather'):
        # the pixel DDPG sample: B = 512 transitions of 9 x 84 x 84 frames (both
        # observations) + the 42-float side row, from 8,192-slot rings (520 MB per
        # side, beyond the Infinity Cache).  Successive launches draw disjoint
        # index sets that sweep the whole ring, so no launch finds its frames
        # cached by an earlier one.  Fused launch against what the tree had
        # before it: two torch.index_select + one smi_gather_rows.
        slots, batch, W = 8192, 512, 42
        fb = 9 * 84 * 84
        fr = torch.randint(0, 256, (slots, fb), device=dev, generator=g, dtype=torch.uint8)
        fn_ = torch.randint(0, 256, (slots, fb), device=dev, generator=g, dtype=torch.uint8)
        tab = torch.randn(slots, W, device=dev, generator=g)
        sets = torch.randperm(slots, device=dev, generator=g).view(slots // batch, batch)
        turn = [0]

        def draw():
            turn[0] = (turn[0] + 1) % sets.shape[0]
            return sets[turn[0]]
        rows = torch.empty(batch, W, device=dev)
        po = torch.empty(batch, fb, dtype=torch.uint8, device=dev)
        pn = torch.empty(batch, fb, dtype=torch.uint8, device=dev)
        nbytes = batch * (8 + 2 * 2 * fb + 8 * W)

        def fused():
            idx = draw()
            L.call('smi_replay_gather', P(tab), W, P(fr), P(fn_), fb, P(idx), batch, P(rows), P(po),
                   P(pn), st)

        def three():
            idx = draw()
            torch.index_select(fr, 0, idx, out=po)
            torch.index_select(fn_, 0, idx, out=pn)
            L.call('smi_gather_rows', P(tab), W, P(idx), batch, P(rows), st)

        # bench.py's calibrated stream (float4 read + write over 2 x 1 GiB), same process
        n = 1 << 28
        x, y = torch.rand(n, device=dev, generator=g), torch.empty(n, device=dev)
        calib = 8.0 * n / (timed(lambda: L.call('smi_calib_stream', P(x), P(y), n, st), 5,
                                 spread=True)[0] * 1e-3) / 1e9
        del x, y
        for name, fn in (('replay_gather', fused), ('replay_gather_baseline3', three)):
            ts = timed(fn, max(args.iters, 20), spread=True)
            med = ts[len(ts) // 2]
            report(name, nbytes, med, slots=slots, batch=batch, frame_bytes=fb, cols=W,
                   repeats=len(ts), min_ms=round(ts[0], 4), p25_ms=round(ts[len(ts) // 4], 4),
                   p75_ms=round(ts[(3 * len(ts)) // 4], 4), max_ms=round(ts[-1], 4),
                   calib_stream_GBs=round(calib, 1),
                   frac_of_calib_stream=round(nbytes / (med * 1e-3) / 1e9 / calib, 4))
        del fr, fn_, tab, sets, rows, po, pn

    if want('replay_gather_shared'):
        # the protocol of replay_gather on the frame-shared store
        slots, batch, W, S = 8192, 512, 42, 3
        fbytes = 3 * 84 * 84
        tab = torch.randn(slots, W, device=dev, generator=g)
        sets = torch.randperm(slots, device=dev, generator=g).view(slots // batch, batch)
        rows = torch.empty(batch, W, device=dev)
        po = torch.empty(batch, S * fbytes, dtype=torch.uint8, device=dev)
        pn = torch.empty(batch, S * fbytes, dtype=torch.uint8, device=dev)
        nbytes = batch * (8 + 2 * S * 4 + 2 * 2 * S * fbytes + 8 * W)
        t = torch.arange(slots, dtype=torch.int32).view(slots, 1, 1)
        k = torch.arange(S, dtype=torch.int32).view(1, 1, S)
        side = torch.arange(2, dtype=torch.int32).view(1, 2, 1)
        layouts = (('replay_gather_shared', t + side + k, slots + S),           # frames t .. t + S
                   ('replay_gather_shared_distinct', t * (2 * S) + side * S + k, slots * 2 * S))
        for name, fid, fslots in layouts:
            store = torch.randint(0, 256, (fslots, fbytes), device=dev, generator=g,
                                  dtype=torch.uint8)
            fid = fid.contiguous().to(dev)
            turn = [0]

            def shared():
                turn[0] = (turn[0] + 1) % sets.shape[0]
                idx = sets[turn[0]]
                L.call('smi_replay_gather_shared', P(tab), W, P(store), P(fid), S, fbytes, P(idx),
                       batch, P(rows), P(po), P(pn), st)
            ts = timed(shared, max(args.iters, 20), spread=True)
            med = ts[len(ts) // 2]
            report(name, nbytes, med, slots=slots, batch=batch, frame_bytes=S * fbytes, stack=S,
                   cols=W, store_slots=fslots, store_bytes=fslots * fbytes, repeats=len(ts),
                   min_ms=round(ts[0], 4), p25_ms=round(ts[len(ts) // 4], 4),
                   p75_ms=round(ts[(3 * len(ts)) // 4], 4), max_ms=round(ts[-1], 4))
            del store, fid
        del tab, sets, rows, po, pn

    if want('replay_insert'):
        import copy
        import time
        import numpy as np
        from surreal_amd.config import DDPG_DEFAULT_LEARNER_CONFIG, pixel_env_config
        from surreal_amd.frame_store import frame_digest
        from surreal_amd.replay import UniformReplay
        D, A, S, n, calls = 17, 6, 3, 64, 23
        rs = np.random.RandomState(0)
        fr = [rs.randint(0, 256, (3, 84, 84)).astype(np.uint8) for _ in range(n * calls + S + 1)]
        exps = []
        for i in range(n * calls):
            low = rs.randn(2, D).astype(np.float32)
            exps.append({'obs': [{'low_dim': {'flat_inputs': low[j]},
                                  'pixel': {'camera0': fr[i + j:i + j + S]}} for j in range(2)],
                         'action': rs.randn(A).astype(np.float32), 'reward': 0.5, 'done': False})
        ec = pixel_env_config(D, A, (9, 84, 84))
        ec['frame_stacks'] = S
        for name, share in (('replay_insert_shared', True), ('replay_insert_unshared', False)):
            lc = copy.deepcopy(DDPG_DEFAULT_LEARNER_CONFIG)
            lc.replay.memory_size = 4096
            lc.replay.share_frames = share
            rep = UniformReplay(lc, ec, seed=0, device=dev)
            ts, packs = [], []
            for c in range(calls):
                chunk = exps[c * n:(c + 1) * n]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                packed = rep.pack(chunk)
                t1 = time.perf_counter()
                rep.insert_rows(*packed)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if c >= 3:
                    ts.append((t2 - t1) * 1e3)
                    packs.append((t1 - t0) * 1e3)
            ts.sort()
            packs.sort()
            t0 = time.perf_counter()
            for f in fr[:n + 1]:
                frame_digest(f)
            dig = (time.perf_counter() - t0) * 1e3
            fb = 3 * 84 * 84
            up = n * rep.width * 4 + ((n + 1) * fb + n * 2 * S * 4 + (n + 1) * 4 if share
                                      else 2 * n * S * fb)
            print(json.dumps({'kernel': name, 'transitions': n, 'repeats': len(ts),
                              'insert_rows_median_ms': round(ts[len(ts) // 2], 4),
                              'insert_rows_min_ms': round(ts[0], 4),
                              'insert_rows_max_ms': round(ts[-1], 4),
                              'pack_median_ms': round(packs[len(packs) // 2], 4),
                              'uploaded_bytes': int(up),
                              'digest_ms_of_65_frames': round(dig, 4) if share else None}),
                  flush=True)
            del rep

    if want('moments'):
        n = 1 << 27
        x = torch.randn(n, device=dev, generator=g)
        o = torch.empty(3, dtype=torch.float64, device=dev)
        fn = lambda: L.call('smi_moments', P(x), n, None, 0, P(o), st)  # noqa
        report('moments', n * 4, timed(fn, args.iters), n=n)
        del x


if __name__ == '__main__':
    main()
