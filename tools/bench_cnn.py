"""Developer tool: time smi_cnn_forward / smi_cnn_backward at the C5 row counts
(JSON lines: rows, us per call, TF/s).  SMI_LIB_VARIANT selects a build variant.

--general: the dispatch measurement of the pixel stem.  At
3x84x84 and 9x84x84, where both implementations run, it times one whole stem
call (device events around 20 calls, the Linear layer included) of
  fused    smi_stem_forward / smi_stem_backward (the dispatch picks the fused
           kernels there), and
  general  the same stem as the general form runs it: one smi_conv2d_* launch
           per layer and direction and the Linear layer on the GEMM engine
           (composed here from the layer ABI over a contiguous batch: the
           row-mapped first layer differs in its image base only)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from surreal_amd import _lib as L  # noqa: E402

H, W, F = 84, 84, 256
dev = 'cuda'


def kernel_classes():
    C = 3
    n = int(L.lib().smi_cnn_param_count(C, H, W, F))
    g = torch.Generator(device=dev).manual_seed(0)
    flat = (torch.rand(n, device=dev, generator=g) - 0.5) * 0.05
    st = L.stream()
    for rows in (2688, 3328):
        pix = torch.randint(0, 256, (rows, C, H, W), device=dev, dtype=torch.uint8, generator=g)
        a1 = torch.empty(rows, 16, 400, device=dev)
        a2 = torch.empty(rows, 2592, device=dev)
        feat = torch.empty(rows, F, device=dev)
        dz = torch.randn(rows, F, device=dev, generator=g)
        nb = int(L.lib().smi_cnn_scratch_bytes(rows, C, H, W, F))
        scratch = torch.empty(nb // 4 + 1, device=dev)
        grad = torch.empty(n, device=dev)

        def fwd():
            L.call('smi_cnn_forward', L.ptr(flat), L.ptr(pix), None, rows, 1, rows, C, H, W, F,
                   L.ptr(a1), L.ptr(a2), L.ptr(feat), F, st)

        def bwd():
            L.call('smi_cnn_backward', L.ptr(flat), L.ptr(pix), None, rows, 1, rows, C, H, W, F,
                   L.ptr(a1), L.ptr(a2), L.ptr(dz), F, L.ptr(grad), L.ptr(scratch), nb, st)
        for name, fn, conv_flops in (('fwd', fwd, 2 * (16 * 400 * 192 + 32 * 81 * 256)),
                                     ('bwd', bwd, 2 * (2 * 32 * 81 * 256 + 16 * 400 * 192))):
            for _ in range(3):
                fn()
            L.kernel_timing(True)
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            L.kernel_timing(False)
            rep = L.kernel_timing_report()
            k = 'cnn_' + name
            c, ms, fl = rep[k]
            print(json.dumps({'variant': os.environ.get('SMI_LIB_VARIANT'), 'op': name, 'rows': rows,
                              'conv_us': round(ms / c * 1e3, 1),
                              'conv_tflops': round(fl / (ms * 1e-3) / 1e12, 1)}), flush=True)


def _time(fn, reps=20, rounds=5):
    """us per call: the median of `rounds` device-event timings of `reps` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    out.sort()
    return round(out[len(out) // 2], 1), round(out[0], 1), round(out[-1], 1)


def dispatch(rows=2688):
    L.ensure_workspace(torch.device(dev))
    st = L.stream()
    g = torch.Generator(device=dev).manual_seed(0)
    layers = [(16, 8, 4), (32, 4, 2)]
    for C in (3, 9):
        spec = L.stem_spec([16, 32], [8, 4], [4, 2]) + (C, H, W, F)
        assert int(L.lib().smi_stem_fused(*spec)) == 1
        n = int(L.lib().smi_stem_param_count(*spec))
        flat = (torch.rand(n, device=dev, generator=g) - 0.5) * 0.05
        pix = torch.randint(0, 256, (rows, C, H, W), device=dev, dtype=torch.uint8, generator=g)
        act = torch.empty(int(L.lib().smi_stem_act_floats(rows, *spec)), device=dev)
        feat = torch.empty(rows, F, device=dev)
        dz = torch.randn(rows, F, device=dev, generator=g)
        nb = int(L.lib().smi_stem_scratch_bytes(rows, *spec))
        scratch = torch.empty(nb // 4 + 1, device=dev)
        grad = torch.empty(n, device=dev)

        def fused_fwd():
            L.call('smi_stem_forward', L.ptr(flat), L.ptr(pix), None, rows, 1, rows, *spec, L.ptr(act),
                   L.ptr(scratch), nb, L.ptr(feat), F, None, st)

        def fused_bwd():
            L.call('smi_stem_backward', L.ptr(flat), L.ptr(pix), None, rows, 1, rows, *spec,
                   L.ptr(act), L.ptr(dz), F, L.ptr(grad), L.ptr(scratch), nb, None, st)

        # the general form: geometry, parameter offsets, activations and gradient images
        geo, offs, o, cin, h, w = [], [], 0, C, H, W
        for co, k, s in layers:
            geo.append((cin, h, w, co, k, s, 0))
            offs.append((o, o + co * cin * k * k))
            o += co * cin * k * k + co
            cin, h, w = co, (h - k) // s + 1, (w - k) // s + 1
        flat_dim = cin * h * w
        oWf, obf = o, o + F * flat_dim
        A = [torch.empty(rows, 16 * 400, device=dev), torch.empty(rows, flat_dim, device=dev)]
        dA = [torch.empty_like(a) for a in A]
        gfeat = torch.empty(rows, F, device=dev)
        ggrad = torch.empty(n, device=dev)
        pb = max(int(L.lib().smi_conv2d_scratch_bytes(rows, *ge)) for ge in geo)
        part = torch.empty(pb // 4 + 1, device=dev)

        def general_fwd():
            x = pix
            for i, (ci, hh, ww, co, k, s, _) in enumerate(geo):
                L.call('smi_conv2d_forward', L.ptr(x), int(i == 0), int(i == 0), rows, ci, hh, ww,
                       L.ptr(flat[offs[i][0]:]), L.ptr(flat[offs[i][1]:]), co, k, s, 0, 1, L.ptr(A[i]),
                       st)
                x = A[i]
            L.call('smi_linear_forward', L.ptr(A[1]), flat_dim, rows, flat_dim, L.ptr(flat[oWf:]),
                   flat_dim, L.ptr(flat[obf:]), F, 1, L.ptr(gfeat), F, st)

        def general_bwd():
            L.call('smi_linear_backward_weight', L.ptr(dz), F, rows, F, L.ptr(A[1]), flat_dim, flat_dim,
                   L.ptr(ggrad[oWf:]), flat_dim, L.ptr(ggrad[obf:]), 0, st)
            L.call('smi_linear_backward_input', L.ptr(dz), F, rows, F, L.ptr(flat[oWf:]), flat_dim,
                   flat_dim, L.ptr(A[1]), flat_dim, L.ptr(dA[1]), flat_dim, st)
            for i in (1, 0):
                ci, hh, ww, co, k, s, _ = geo[i]
                x = pix if i == 0 else A[i - 1]
                L.call('smi_conv2d_backward_weight', L.ptr(dA[i]), L.ptr(x), int(i == 0), int(i == 0),
                       rows, ci, hh, ww, co, k, s, 0, L.ptr(ggrad[offs[i][0]:]),
                       L.ptr(ggrad[offs[i][1]:]), L.ptr(part), pb, st)
                if i > 0:
                    L.call('smi_conv2d_backward_input', L.ptr(dA[i]), rows, ci, hh, ww,
                           L.ptr(flat[offs[i][0]:]), co, k, s, 0, L.ptr(A[i - 1]), L.ptr(dA[i - 1]), st)

        fused_fwd()
        general_fwd()
        torch.cuda.synchronize()
        err = float((feat - gfeat).abs().max()) / max(float(feat.abs().max()), 1e-30)
        for op, ff, gf in (('fwd', fused_fwd, general_fwd), ('bwd', fused_bwd, general_bwd)):
            # alternate the two forms: A B A B, the medians of each form's rounds
            f1, g1, f2, g2 = _time(ff), _time(gf), _time(ff), _time(gf)
            print(json.dumps({'op': op, 'C': C, 'rows': rows, 'fused_us': [f1[0], f2[0]],
                              'general_us': [g1[0], g2[0]], 'fused_min_max': [f1[1:], f2[1:]],
                              'general_min_max': [g1[1:], g2[1:]], 'feat_rel_diff': err}), flush=True)
        fused_bwd()
        general_bwd()
        torch.cuda.synchronize()
        print(json.dumps({'C': C, 'grad_rel_diff': float((grad - ggrad).abs().max()) /
                          max(float(grad.abs().max()), 1e-30)}), flush=True)


if __name__ == '__main__':
    if '--general' in sys.argv:
        dispatch()
    else:
        kernel_classes()
