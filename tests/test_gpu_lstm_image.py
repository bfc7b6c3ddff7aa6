"""The 4-segment LSTM forward's image form (lstm_fwd_r4_kernel<KP,KX,img>): the
weight columns loaded from the transposed image [W_ihT | W_hhT | zeros]
instead of one row per lane.

Form parity: smi_lstm_forward_x_image on an image from smi_lstm_weight_image
against smi_lstm_forward_x on the same weights, bitwise (the registers hold the
same values and the MFMA order is the same), one case per instantiation, with
smi_last_launch() naming the form on both sides.

Image maintenance: after every learn() of a PPOLearner whose batch runs that
form, the image in the learner's scratch (smi_ppo_rnn_wimage_offset) is the
transpose of the current stem weights bitwise: Adam's transposed stores, and
the GAE phase's rebuild after the parameters were replaced from outside."""
import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd import synthetic
from surreal_amd.learner import PPOLearner
from tests.helpers import env_config, ppo_config

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
E_NOFIT = -2


def setup_module(m):
    L.ensure_workspace(DEV)       # the unfused form's xproj GEMM


def _last():
    return L.lib().smi_last_launch().decode()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _r4(kp, kx, tag):
    return f'lstm_fwd_r4_kernel<{kp},{kx}{"," + tag if tag else ""}>'


def _at(t, off):
    """a copy of t that starts `off` floats into a fresh allocation"""
    buf = torch.empty(t.numel() + off, device=DEV)
    buf[off:] = t.reshape(-1)
    return buf[off:]


def _inputs(B, S, D, H, seed, off=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.empty(*shape).uniform_(-0.4, 0.4, generator=g)  # noqa: E731
    w = {'Wih': _at(u(4 * H, D).to(DEV), off), 'Whh': _at(u(4 * H, H).to(DEV), off),
         'bih': u(4 * H).to(DEV), 'bhh': u(4 * H).to(DEV),
         'x': torch.randn(S * B, D, generator=g).to(DEV),
         'h0': (0.3 * torch.randn(B, H, generator=g)).to(DEV),
         'c0': (0.3 * torch.randn(B, H, generator=g)).to(DEV)}
    # NaN behind the image: a read past its zero row shows in the outputs
    img = torch.full((off + 4 * H * (D + H + 1) + 64,), NAN, device=DEV)
    w['img'] = img[off:]
    return w


def _outs(B, S, H):
    return (torch.full((S + 1, B, H), NAN, device=DEV), torch.full((S + 1, B, H), NAN, device=DEV),
            torch.full((S, B, 4 * H), NAN, device=DEV), torch.full((max(S, 1), B, 4 * H), NAN, device=DEV))


def _fwd(name, w, wslot, B, S, D, H, o):
    """smi_lstm_forward_x (wslot: W_hh) or smi_lstm_forward_x_image (wslot: the image)"""
    return getattr(L.lib(), name)(L.ptr(w['x']), D, D, L.ptr(w['Wih']), L.ptr(w['bih']), L.ptr(wslot),
                                  L.ptr(w['bhh']), L.ptr(w['h0']), L.ptr(w['c0']), S, B, H,
                                  L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.stream())


def _parity(B, S, D, H, f_nat, f_img, seed, off=0):
    w = _inputs(B, S, D, H, seed, off)
    L.call('smi_lstm_weight_image', L.ptr(w['Wih']), L.ptr(w['Whh']), D, H, L.ptr(w['img']),
           L.stream())
    n = 4 * H * D
    img = w['img']
    assert torch.equal(img[:n].reshape(D, 4 * H), w['Wih'].reshape(4 * H, D).t())
    assert torch.equal(img[n:n + 4 * H * H].reshape(H, 4 * H), w['Whh'].reshape(4 * H, H).t())
    assert bool((img[n + 4 * H * H:n + 4 * H * (H + 1)] == 0).all())
    assert bool(torch.isnan(img[4 * H * (D + H + 1):]).all())
    nat, got = _outs(B, S, H), _outs(B, S, H)
    assert _fwd('smi_lstm_forward_x', w, w['Whh'], B, S, D, H, nat) == 0
    assert _last() == f_nat
    assert _fwd('smi_lstm_forward_x_image', w, img, B, S, D, H, got) == 0
    assert _last() == f_img
    for name, a, b in zip(('hbuf', 'cbuf', 'gates_act'), nat, got):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), f'{name}: the image form differs from the row form'


# (din, H, the row form smi_lstm_forward_x runs, the image form): the learner's
# shapes and the odd ones first, then one for each remaining image instantiation
IMAGE_CASES = [
    (42, 100, _r4(104, 48, 'vf'), _r4(104, 48, 'img')),     # the C3 form
    (47, 102, _r4(104, 48, ''), _r4(104, 48, 'img')),       # H % 4 != 0, odd din: no vector rows
    (8, 20, _r4(64, 48, 'vf'), _r4(64, 48, 'img')),         # 4H = 80: two of eight waves active
    (64, 64, _r4(64, 64, 'vf'), _r4(64, 64, 'img')),
    (70, 100, _r4(104, 0, 'vf'), _r4(104, 0, 'img')),       # din > 64: xproj GEMM + KX == 0
    (9, 126, _r4(128, 0, ''), _r4(128, 0, 'img')),          # H > 104: KP 128, KX == 0
    (70, 20, _r4(32, 0, 'vf'), _r4(32, 0, 'img')),
    (70, 64, _r4(64, 0, 'vf'), _r4(64, 0, 'img')),
    (50, 100, _r4(104, 64, 'vf'), _r4(104, 64, 'img')),
]


@pytest.mark.parametrize('extra', [1, 6], ids=['cu1', 'cu6'])
@pytest.mark.parametrize('D,H,f_nat,f_img', IMAGE_CASES, ids=[f'D{c[0]}-H{c[1]}' for c in IMAGE_CASES])
def test_image_form_parity(D, H, f_nat, f_img, extra):
    """S = 3 at CUs + 1 segments (the last workgroup holds one) and CUs + 6."""
    _parity(_cus() + extra, 3, D, H, f_nat, f_img, seed=1000 * H + D + extra)


def test_image_form_parity_unaligned_weights():
    """weights and image 4 bytes past a 16-byte boundary: the row form falls
    back to its alignment-branching loads, the image form has no requirement"""
    _parity(_cus() + 1, 3, 42, 100, _r4(104, 48, ''), _r4(104, 48, 'img'), seed=11, off=1)


def test_image_form_zero_steps_and_small_batch():
    """S = 0 launches nothing and leaves every buffer untouched; B <= CUs (the
    one-segment forms' batch) is SMI_E_NOFIT, likewise nothing launched."""
    D, H = 8, 20
    for B, S, rc_exp in ((_cus() + 1, 0, 0), (3, 2, E_NOFIT)):
        w = _inputs(B, max(S, 1), D, H, seed=5)
        L.call('smi_lstm_weight_image', L.ptr(w['Wih']), L.ptr(w['Whh']), D, H, L.ptr(w['img']),
               L.stream())
        before = _last()
        assert before == 'lstm_weight_image_kernel'
        o = _outs(B, S, H)
        assert _fwd('smi_lstm_forward_x_image', w, w['img'], B, S, D, H, o) == rc_exp
        assert _last() == before
        for t in o:
            assert bool(torch.isnan(t).all())


def _image_matches(learner, off, D, H):
    stem = learner.model.stem_flat.detach()
    img = learner._bufs['rnn_scratch'][off:off + 4 * H * (D + H + 1)]
    n = 4 * H * D
    assert torch.equal(img[:n].reshape(D, 4 * H), stem[:n].reshape(4 * H, D).t()), 'W_ihT'
    assert torch.equal(img[n:n + 4 * H * H].reshape(H, 4 * H),
                       stem[n:n + 4 * H * H].reshape(4 * H, H).t()), 'W_hhT'
    assert bool((img[n + 4 * H * H:] == 0).all()), 'zero row'


def test_learner_keeps_the_image_current():
    B, T, Hz, D, A, H = _cus() + 1, 6, 2, 8, 3, 20
    lc = ppo_config(B=B, T=T, mode='adapt', use_z_filter=True, hidden=(32, 32), lam=1.0,
                    epochs=(2, 2), rnn=True, rnn_hidden=H, horizon=Hz)
    learner = PPOLearner(lc, env_config(D, A), seed=3, device=DEV)
    batch = synthetic.to_device(synthetic.ppo_batch(B, T, D, A, seed=2, rnn_hidden=H), DEV)
    off = L.lib().smi_ppo_rnn_wimage_offset(B, T, Hz, D, H, 32, 32, A, 32, 32, 0, 0, 0, 0, 1)
    assert off > 0
    assert off * 4 + 4 * H * (D + H + 1) * 4 <= L.lib().smi_ppo_rnn_scratch_bytes(
        B, T, Hz, D, H, 32, 32, A, 32, 32, 0, 0, 0, 0, 1)
    # shapes without an image: two layers, H > 128, no LSTM
    assert L.lib().smi_ppo_rnn_wimage_offset(B, T, Hz, D, H, 32, 32, A, 32, 32, 0, 0, 0, 0, 2) == -1
    assert L.lib().smi_ppo_rnn_wimage_offset(B, T, Hz, D, 129, 32, 32, A, 32, 32, 0, 0, 0, 0, 1) == -1
    assert L.lib().smi_ppo_rnn_wimage_offset(B, T, T, D, 0, 32, 32, A, 32, 32, 0, 0, 0, 0, 1) == -1
    prev = learner.model.stem_flat.detach().clone()
    for _ in range(2):
        learner.learn(batch)
        torch.cuda.synchronize()
        assert not torch.equal(prev, learner.model.stem_flat.detach()), 'the stem did not train'
        prev = learner.model.stem_flat.detach().clone()
        _image_matches(learner, off, D, H)
    # the parameters replaced from outside (a checkpoint load): the GAE phase
    # rebuilds the image before the epoch forwards read it
    g = torch.Generator().manual_seed(9)
    new = torch.empty(learner.model.stem_flat.numel()).uniform_(-0.3, 0.3, generator=g)
    with torch.no_grad():
        learner.model.stem_flat.copy_(new.to(DEV))
    # (every Adam step rewrites the whole image, so a stale one would not show
    # afterwards: poisoned, it shows in the parameters unless GAE rebuilt it)
    learner._bufs['rnn_scratch'][off:off + 4 * H * (D + H + 1)].fill_(NAN)
    learner.learn(batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(learner.model.stem_flat).all())
    assert not torch.equal(new.to(DEV), learner.model.stem_flat.detach())
    _image_matches(learner, off, D, H)
