"""The pixel-stem parity bars against emulations (host only).

tests/test_gpu_cnn_geometry.py compares smi_cnn_forward / smi_cnn_backward with
torch at frames other than 3x84x84.  Here the same checks (the same references,
bars and images, tests/cnn_ref.py) run against a plain-torch fp32 emulation of
the kernels' arithmetic:

  * the unfaulted emulation passes every output's bar at every geometry of the
    GPU case table, so the bars are not tighter than fp32 itself allows at
    these shapes (raw bytes, / 255 in the epilogue, another summation order);
  * each one-line fault (H / W swapped in a window offset, a stale image row,
    pix_next ignored, an unwritten last pixel, a dropped dW2 pixel, a missing
    / 255, a `>=` ReLU mask) fails at least one bar, so a kernel with that
    fault cannot pass the GPU file;
  * geom() agrees with torch's Conv2d output shapes.
"""
import pytest
import torch

from tests import cnn_ref as CR

# (B, T, rows) per table geometry: rows = (T + 1) * B reads pix_next for every
# segment, rows < B * T with rows % B != 0 ends inside a time step
ROWS = {(3, 20, 20): (3, 2, 9), (3, 24, 20): (4, 2, 7), (3, 64, 36): (5, 1, 5),
        (3, 36, 52): (2, 3, 8), (3, 68, 116): (2, 2, 5), (3, 28, 324): (5, 1, 5),
        (9, 20, 20): (3, 3, 7), (9, 36, 52): (2, 2, 6), (9, 40, 212): (4, 1, 4),
        (9, 84, 84): (2, 1, 4)}
F = 24


def _check(cam, B, T, rows, fault=None, seed=0):
    """run the emulated stem (with `fault`) through the checks of the GPU file;
    returns the outputs that miss their bar."""
    g = CR.geom(*cam)
    torch.manual_seed(100 * B + rows + seed)
    net, net64 = CR.nets(*cam, F)
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    pix, pixn = CR.images(B, T, cam, seed + rows, rows)
    x = CR.timemajor_images(pix, pixn, rows)
    x_emu = CR.timemajor_images(pix, pixn, rows, fault)
    a1, a2, feat = CR.emu_forward(flat, x_emu, g, F, fault)
    s32, s64 = CR.stages(net, x), CR.stages(net64, x)
    bad = CR.failures(CR.FWD_NAMES, (a1, a2, feat), s32, s64, CR.FWD_SLACK)
    dy = torch.randn(rows, F, generator=torch.Generator().manual_seed(7))
    dz = (dy * (s32[2] > 0)).contiguous()
    grads = CR.emu_backward(flat, x_emu, g, F, a1, a2, dz, fault)
    m1, m2 = a1 > 0, a2 > 0
    g32 = CR.masked_grads(net, x, m1, m2, dz)
    g64 = CR.masked_grads(net64, x, m1, m2, dz)
    bad += CR.failures(CR.GRAD_NAMES, grads, g32, g64, CR.BWD_SLACK)
    for t in (a1, a2, feat, *grads):
        assert bool(torch.isfinite(t).all())
    return bad


@pytest.mark.parametrize('cam', CR.TABLE, ids=lambda c: 'x'.join(map(str, c)))
def test_emulated_stem_passes_the_bars(cam):
    assert CR.geom(*cam).ok
    bad = _check(cam, *ROWS[cam])
    assert not bad, bad


@pytest.mark.parametrize('cam,rows', [((3, 20, 20), 2051), ((9, 36, 52), 1795), ((3, 84, 84), 771),
                                      ((9, 84, 84), 259), ((3, 28, 324), 515)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_emulated_stem_passes_with_many_rows(cam, rows):
    # the multi-image cases of the GPU file at the rows a 256-CU part gives them
    # (7 segments, the last rows on pix_next): gradient sums of up to 308,400 terms
    bad = _check(cam, 7, (rows - 1) // 7, rows)
    assert not bad, bad


# fault -> (frame, (B, T, rows)): a rectangular frame for the H / W swap, a
# conv-1 pixel count that is no multiple of 16 for the dropped pixel, rows
# beyond B * T for pix_next
FAULT_CASES = {
    'hw_swap': ((3, 64, 36), (5, 1, 5)),
    'prev_row': ((3, 36, 52), (2, 3, 8)),
    'no_pix_next': ((3, 20, 20), (3, 2, 9)),
    'a1_last_pixel': ((3, 24, 20), (4, 2, 7)),
    'dw2_last_pixel': ((3, 36, 52), (2, 3, 8)),
    'dw1_no_255': ((9, 20, 20), (3, 3, 7)),
    'mask_ge': ((3, 64, 36), (5, 1, 5)),
}


@pytest.mark.parametrize('fault', CR.FAULTS)
def test_fault_fails_a_bar(fault):
    cam, (B, T, rows) = FAULT_CASES[fault]
    g = CR.geom(*cam)
    if fault == 'hw_swap':
        assert g.H != g.W
    if fault == 'a1_last_pixel':
        assert g.P1 % 16 != 0
    if fault == 'no_pix_next':
        assert rows > B * T
    assert not _check(cam, B, T, rows)              # the same case passes unfaulted
    bad = _check(cam, B, T, rows, fault)
    print(fault, [n for n, _ in bad])
    assert bad, f'{fault}: every output still passes its bar'


def test_hw_swap_is_invisible_on_a_square_frame():
    # why the table needs rectangular frames: at H == W the fault changes nothing
    assert not _check((3, 20, 20), 3, 2, 9, 'hw_swap')


def test_geom_matches_conv2d_shapes():
    frames = CR.TABLE + [(3, 84, 84), (3, 21, 23), (9, 47, 33), (3, 100, 84)]
    for C, H, W in frames:
        g = CR.geom(C, H, W)
        net = CR.R.cnn_stem_ref(C, H, W, 4)
        with torch.no_grad():
            y1 = net[0](torch.zeros(1, C, H, W))
            y2 = net[2](y1)
        assert tuple(y1.shape) == (1, 16, g.H1, g.W1), (C, H, W)
        assert tuple(y2.shape) == (1, 32, g.H2, g.W2), (C, H, W)
        assert g.P1 == g.H1 * g.W1 and g.P2 == g.H2 * g.W2
        assert net[5].in_features == 32 * g.P2
        assert g.img == C * H * W and g.fwd_lds == (g.img + 15) // 16 * 16 + 64 * g.P1


def test_table_geometry_matches_its_purposes():
    G = {cam: CR.geom(*cam) for cam in CR.TABLE}
    assert (G[3, 20, 20].P1, G[3, 20, 20].P2) == (16, 1)
    assert G[3, 24, 20].H1 == 5 and G[3, 24, 20].P1 % 16 != 0
    g = G[3, 64, 36]
    assert (g.H1, g.W1, g.H2, g.W2) == (15, 8, 6, 3) and 2 * (g.H2 - 1) + 3 < g.H1 - 1
    assert (G[3, 36, 52].H1, G[3, 36, 52].W1) == (8, 12) and G[3, 36, 52].P2 == 15
    assert G[3, 68, 116].P1 == 448 and G[3, 68, 116].P2 == 91
    assert G[3, 28, 324].P1 == 480 and G[3, 28, 324].img // 16 > 6 * 256
    assert G[3, 28, 324].bwd_lds == 71176 > 64 * 1024
    assert all(g.bwd_lds <= CR.CU_LDS for g in G.values())
    assert G[9, 40, 212].P1 == 468 and G[9, 40, 212].H1 == 9 and G[9, 40, 212].fwd_lds == 106272
    assert G[9, 84, 84].P1 == 400 and G[9, 84, 84].img // 16 > 2 * 6 * 256
