"""The general pixel stem's parity rule against emulations, its state dict and
its configuration errors (host only).

tests/test_gpu_stem.py compares smi_stem_forward / smi_stem_backward with torch
(tests/stem_ref.py).  Here the same checks (references, failure rule, slacks,
images, row counts) run against a plain-torch fp32 emulation of the kernels'
arithmetic:

  * the unfaulted emulation passes every output's bar at every case of the GPU
    table, so the bars are not tighter than fp32 allows at these shapes;
  * each one-line fault (H / W swapped in a window offset, pix_next ignored, a
    stale row of the row map, a missing / 255, a `>=` ReLU mask, a layer's
    stride off by one, two layers' biases swapped) fails at least one bar, so a
    kernel with that fault cannot pass the GPU file.

CNNStemNetwork: for specs of 1, 2 and 3 layers the state dict has the keys,
shapes and order of the equivalent nn.Sequential and load_state_dict
round-trips through the flat buffer; every invalid conv_spec raises
ConfigError naming the layer, with no GPU present.
"""
import pytest
import torch

from surreal_amd.config import ConfigError
from surreal_amd.model import CNNStemNetwork
from tests import cnn_ref as CR
from tests import stem_ref as SR

BY_ID = {c.id: c for c in SR.CASES}


def _check(case, fault=None):
    """run the emulated stem (with `fault`) through the checks of the GPU file;
    returns the outputs that miss their bar."""
    spec, cam, F, B, T, rows = case.spec, case.cam, case.F, case.B, case.T, case.rows
    n = len(spec[0])
    torch.manual_seed(100 * B + rows)
    net, net64 = SR.nets(spec, cam, F)
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    pix, pixn = SR.images(B, T, cam, rows, rows)
    x = SR.timemajor_images(pix, pixn, rows)
    x_emu = SR.timemajor_images(pix, pixn, rows, fault)
    outs = SR.emu_forward(flat, x_emu, spec, cam, F, fault)
    s32, s64 = SR.stages(net, x, n), SR.stages(net64, x, n)
    bad = SR.failures(SR.fwd_names(n), outs, s32, s64, CR.FWD_SLACK)
    dy = torch.randn(rows, F, generator=torch.Generator().manual_seed(7))
    dz = (dy * (s32[n] > 0)).contiguous()
    grads = SR.emu_backward(flat, x_emu, spec, cam, F, outs[:n], dz, fault)
    masks = [a > 0 for a in outs[:n]]
    g32 = SR.masked_grads(net, x, masks, dz, n)
    g64 = SR.masked_grads(net64, x, masks, dz, n)
    bad += SR.failures(SR.grad_names(n), grads, g32, g64, CR.BWD_SLACK)
    for t in (*outs, *grads):
        assert bool(torch.isfinite(t).all())
    return bad


@pytest.mark.parametrize('case', SR.CASES, ids=[c.id for c in SR.CASES])
def test_emulated_stem_passes_the_bars(case):
    bad = _check(case)
    assert not bad, bad


# fault -> case: a rectangular frame for the H / W swap, rows beyond B * T for
# pix_next, at least two layers for the stride fault's layer to have a producer
FAULT_CASES = {'hw_swap': 'w22', 'no_pix_next': 'c4-20x20', 'prev_row': 'three-layers',
               'no_255': 'one-layer', 'mask_ge': 'three-layers', 'stride_off': 'three-layers',
               'bias_swap': 'four-layers'}


@pytest.mark.parametrize('fault', SR.FAULTS)
def test_fault_fails_a_bar(fault):
    case = BY_ID[FAULT_CASES[fault]]
    if fault == 'hw_swap':
        assert case.cam[1] != case.cam[2]
    if fault == 'no_pix_next':
        assert case.rows > case.B * case.T
    assert not _check(case)                         # the same case passes unfaulted
    bad = _check(case, fault)
    print(fault, [n for n, _ in bad])
    assert bad, f'{fault}: every output still passes its bar'


def test_default_factory_is_the_oracle_stem():
    a, b = SR.factory(3, 36, 52, 24), CR.R.cnn_stem_ref(3, 36, 52, 24)
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == \
        [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
    assert [type(m) for m in a] == [type(m) for m in b]


def test_table_shapes_match_their_purposes():
    sh = {c.id: SR.layer_shapes(c.spec, c.cam) for c in SR.CASES}
    assert sh['84x100'][1][6:] == (9, 11)                       # conv-2 output of 99 pixels
    assert sh['w22'][0][2] % 4 != 0
    c = sh['c1-21x23-off1'][0]
    assert c[0] == 1 and (c[7] - 1) * c[5] + c[4] < c[2]       # trailing columns no window covers
    assert len(sh['one-layer']) == 1 and len(sh['three-layers']) == 3 and len(sh['four-layers']) == 4
    assert sh['72ch-k4s3'][0][3] > 64 and sh['72ch-k4s3'][0][4] % sh['72ch-k4s3'][0][5] != 0
    for c in SR.CASES:
        assert c.rows <= (c.T + 1) * c.B


# ---------------------------------------------------------------- state dict
@pytest.mark.parametrize('spec,cam', [(((8,), (3,), (1,)), (2, 9, 11)), (SR.DEFAULT, (3, 36, 52)),
                                      (((8, 12, 20), (5, 3, 2), (2, 1, 2)), (3, 30, 26))],
                         ids=['1-layer', '2-layers', '3-layers'])
def test_state_dict_is_the_sequentials(spec, cam):
    F, n = 16, len(spec[0])
    torch.manual_seed(3)
    ref = SR.factory(*cam, F, *spec)
    net = CNNStemNetwork(cam, F, *spec)
    sd, rd = net.state_dict(), ref.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == \
        [('model.' + k, tuple(v.shape)) for k, v in rd.items()]
    assert 'model.{}.weight'.format(2 * n + 1) in sd and 'model.{}.weight'.format(2 * (n - 1)) in sd
    net.load_state_dict({'model.' + k: v for k, v in rd.items()})
    # the flat buffer is the module-order concatenation (the planner's layout) ...
    assert torch.equal(net.flat, torch.cat([p.detach().reshape(-1) for p in ref.parameters()]))
    # ... and what was loaded comes back
    for k, v in net.state_dict().items():
        assert torch.equal(v, rd[k[len('model.'):]])
    assert net.flat_dim == ref[2 * n + 1].in_features
    other = CNNStemNetwork(cam, F, *spec, flat=net.flat.clone())
    other.flat.zero_()
    other.load_state_dict(net.state_dict())
    assert torch.equal(other.flat, net.flat)


def test_default_spec_keeps_todays_keys():
    assert list(CNNStemNetwork((3, 84, 84), 8).state_dict()) == [
        'model.0.weight', 'model.0.bias', 'model.2.weight', 'model.2.bias', 'model.5.weight',
        'model.5.bias']


# --------------------------------------------------------------- ConfigError
@pytest.mark.parametrize('cam,spec,what', [
    ((3, 84, 84), ((16, 32), (8,), (4, 2)), 'one length'),
    ((3, 84, 84), ((4,) * 5, (2,) * 5, (1,) * 5), '1 to 4 layers'),
    ((3, 84, 84), ((), (), ()), '1 to 4 layers'),
    ((3, 84, 84), ((16, 32), (8, 9), (4, 2)), 'layer 2'),          # k > 8
    ((3, 84, 84), ((16, 32), (8, 4), (5, 2)), 'layer 1'),          # stride > 4
    ((3, 84, 84), ((16, 32), (8, 2), (4, 3)), 'layer 2'),          # stride > k
    ((3, 84, 84), ((16, 129), (8, 4), (4, 2)), 'layer 2'),         # channels > 128
    ((3, 84, 84), ((0, 32), (8, 4), (4, 2)), 'layer 1'),
    ((3, 84, 84), ((16, 32), (8, 4), (0, 2)), 'layer 1'),
    ((3, 16, 16), SR.DEFAULT, 'layer 2'),                          # conv-1 output 3 x 3 < 4 x 4
    ((3, 7, 84), SR.DEFAULT, 'layer 1'),
    ((3, 12, 12), ((4,) * 4, (2,) * 4, (4, 1, 1, 1)), 'layer 1'),
    ((200, 84, 84), SR.DEFAULT, 'layer 1'),                        # input channels > 128
], ids=lambda v: None)
def test_invalid_conv_spec_is_a_config_error(cam, spec, what):
    with pytest.raises(ConfigError, match=what):
        CNNStemNetwork(cam, 8, *spec)


def test_no_not_implemented_left():
    import inspect
    from surreal_amd import model
    assert 'NotImplementedError' not in inspect.getsource(model.CNNStemNetwork)
