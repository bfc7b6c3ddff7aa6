"""Per-layer timing of the general convolution layer (smi_conv2d_forward /
_backward_input / _backward_weight) at the Atari stem's three layers
(4x84x84 -> 32@8/4 -> 64@4/2 -> 64@3/1, SAME padding, first layer on uint8
frames / 255) against torch.nn.functional.conv2d forward and
aten.convolution_backward (MIOpen, fp32) in the same process: the two are
timed alternately, call by call, with HIP events after a warm-up, and the
median is reported with the share of the fp32 MFMA peak (157.3 TFLOP/s) that
2 n Ho Wo cin k k cout FLOP in that time amount to.

The same tool runs the first two layers of the fixed PPO / DDPG stem
(3x84x84 -> 16@8/4 -> 32@4/2, pad 0) on the general kernels against
smi_cnn_forward / smi_cnn_backward, whose launch also holds the stem's Linear
layer (F = 8 here, 0.1 % of the FLOP).

--ours-only runs each general kernel --iters times and nothing else (for a
rocprofv3 --kernel-trace --stats run of its own).  When MIOpen cannot run, that
is printed and the project's numbers stand alone.  One JSON line per measurement.

Usage: python tools/bench_conv.py [--batch 512] [--iters 30] [--warmup 5] [--ours-only]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from surreal_amd import _lib as L  # noqa: E402

PEAK = 157.3e12
P = L.ptr


def alternate(fns, iters, warm):
    """median ms of each fn, timed in turn within every iteration"""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    evs = [[] for _ in fns]
    for _ in range(iters):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            evs[i].append((s, e))
    torch.cuda.synchronize()
    out = []
    for ev in evs:
        ts = sorted(s.elapsed_time(e) for s, e in ev)
        out.append(ts[len(ts) // 2])
    return out


class Layer(object):
    def __init__(self, n, cin, H, W, cout, k, s, p, u8, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.geom = (cin, H, W, cout, k, s, p)
        self.n, self.u8 = n, u8
        self.ho, self.wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        if u8:
            self.x = torch.randint(0, 256, (n, cin, H, W), generator=g, dtype=torch.uint8).cuda()
            self.xf = self.x.float() / 255.0
        else:
            self.x = torch.relu(torch.randn(n, cin, H, W, generator=g)).cuda()
            self.xf = self.x
        self.w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).cuda()
        self.b = torch.randn(cout, generator=g).cuda()
        self.dy = torch.randn(n, cout, self.ho, self.wo, generator=g).cuda()
        self.y = torch.empty_like(self.dy)
        self.dx = torch.empty(n, cin, H, W).cuda()
        self.dw, self.db = torch.empty_like(self.w), torch.empty_like(self.b)
        self.nbytes = int(L.lib().smi_conv2d_scratch_bytes(n, *self.geom))
        self.scratch = torch.empty(self.nbytes // 4 + 1).cuda()
        self.flop = 2.0 * n * self.ho * self.wo * cin * k * k * cout
        self.st = L.stream()

    def fwd(self):
        cin, H, W, cout, k, s, p = self.geom
        L.call('smi_conv2d_forward', P(self.x), int(self.u8), int(self.u8), self.n, cin, H, W,
               P(self.w), P(self.b), cout, k, s, p, 1, P(self.y), self.st)

    def bwd_input(self):
        cin, H, W, cout, k, s, p = self.geom
        L.call('smi_conv2d_backward_input', P(self.dy), self.n, cin, H, W, P(self.w), cout, k, s, p,
               P(self.xf), P(self.dx), self.st)

    def bwd_weight(self):
        cin, H, W, cout, k, s, p = self.geom
        L.call('smi_conv2d_backward_weight', P(self.dy), P(self.x), int(self.u8), int(self.u8),
               self.n, cin, H, W, cout, k, s, p, P(self.dw), P(self.db), P(self.scratch),
               self.nbytes, self.st)

    def t_fwd(self):
        s, p = self.geom[5], self.geom[6]
        return torch.relu_(F.conv2d(self.xf, self.w, self.b, stride=s, padding=p))

    def t_bwd(self, mask):
        s, p = self.geom[5], self.geom[6]
        return torch.ops.aten.convolution_backward(
            self.dy, self.xf, self.w, [self.geom[3]], [s, s], [p, p], [1, 1], False, [0, 0], 1, mask)


def report(name, layer, ours_ms, torch_ms=None, **extra):
    d = {'measurement': name, 'n': layer.n, 'geom': list(layer.geom), 'ours_ms': round(ours_ms, 4),
         'ours_share_of_fp32_mfma_peak': round(layer.flop / (ours_ms * 1e-3) / PEAK, 4)}
    if torch_ms is not None:
        d['torch_miopen_ms'] = round(torch_ms, 4)
    d.update(extra)
    print(json.dumps(d), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--ours-only', action='store_true')
    args = ap.parse_args()
    n = args.batch
    L.ensure_workspace(torch.device('cuda', torch.cuda.current_device()))
    atari = [('atari_l1', Layer(n, 4, 84, 84, 32, 8, 4, 4, True)),
             ('atari_l2', Layer(n, 32, 22, 22, 64, 4, 2, 2, False)),
             ('atari_l3', Layer(n, 64, 12, 12, 64, 3, 1, 1, False))]
    if args.ours_only:
        for name, l in atari:
            for _ in range(args.iters):
                l.fwd()
                l.bwd_weight()
                if name != 'atari_l1':
                    l.bwd_input()
        torch.cuda.synchronize()
        print(json.dumps({'measurement': 'ours_only', 'n': n, 'iters': args.iters}), flush=True)
        return
    miopen = True
    try:
        atari[2][1].t_fwd()
        torch.cuda.synchronize()
    except RuntimeError as e:
        miopen = False
        print(json.dumps({'measurement': 'torch_miopen', 'not_measured': str(e).splitlines()[0][:200]}),
              flush=True)
    for name, l in atari:
        kinds = [('forward', l.fwd, l.t_fwd), ('backward_weight', l.bwd_weight,
                                               lambda l=l: l.t_bwd([False, True, True]))]
        if name != 'atari_l1':
            kinds.append(('backward_input', l.bwd_input, lambda l=l: l.t_bwd([True, False, False])))
        for kind, ours, ref in kinds:
            if miopen:
                a, b = alternate([ours, ref], args.iters, args.warmup)
                report(f'{name}_{kind}', l, a, b)
            else:
                report(f'{name}_{kind}', l, alternate([ours], args.iters, args.warmup)[0])
    # ---- the fixed stem's two convolutions (pad 0, C = 3) on the general kernels
    Fd = 8
    l1 = Layer(n, 3, 84, 84, 16, 8, 4, 0, True)
    l2 = Layer(n, 16, 20, 20, 32, 4, 2, 0, False)
    lib = L.lib()
    flat = (0.05 * torch.randn(int(lib.smi_cnn_param_count(3, 84, 84, Fd)))).cuda()
    a1 = torch.empty(n, 16, 400).cuda()
    a2 = torch.empty(n, 32 * 81).cuda()
    feat = torch.empty(n, Fd).cuda()
    dz = torch.randn(n, Fd).cuda()
    grad = torch.empty_like(flat)
    nb = int(lib.smi_cnn_scratch_bytes(n, 3, 84, 84, Fd))
    scr = torch.empty(nb // 4 + 1).cuda()
    st = L.stream()

    def stem_fwd():
        L.call('smi_cnn_forward', P(flat), P(l1.x), None, n, 1, n, 3, 84, 84, Fd, P(a1), P(a2), P(feat),
               Fd, st)

    def stem_bwd():
        L.call('smi_cnn_backward', P(flat), P(l1.x), None, n, 1, n, 3, 84, 84, Fd, P(a1), P(a2), P(dz),
               Fd, P(grad), P(scr), nb, st)

    def gen_fwd():
        l1.fwd()
        l2.fwd()

    def gen_bwd():
        l2.bwd_weight()
        l2.bwd_input()
        l1.bwd_weight()
    stem_fwd()
    a, b = alternate([gen_fwd, stem_fwd], args.iters, args.warmup)
    print(json.dumps({'measurement': 'stem_shape_forward', 'n': n, 'general_two_layers_ms': round(a, 4),
                      'fixed_stem_ms': round(b, 4)}), flush=True)
    a, b = alternate([gen_bwd, stem_bwd], args.iters, args.warmup)
    print(json.dumps({'measurement': 'stem_shape_backward', 'n': n, 'general_two_layers_ms': round(a, 4),
                      'fixed_stem_ms': round(b, 4)}), flush=True)


if __name__ == '__main__':
    main()
