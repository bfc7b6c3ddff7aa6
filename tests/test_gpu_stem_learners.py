"""The learners on the general pixel stem: cameras the fused stem refuses, and
model.conv_spec.

  * PPO (the reference's default layers, ppo_net.py:139) on a 3x32x22 camera
    (W % 4 != 0) without the LSTM and on a 4x20x24 camera (4 channels) with it:
    tests/test_gpu_cnn._run_pixel and its bars, at the shapes of
    test_pixel_mlp_learn_off_the_square / test_pixel_mlp_learn_matches_oracle
    (the LSTM case adds that file's 16-wide LSTM with horizon 2);
  * DDPG with the default spec on a 4x24x22 camera, batch 8: one learn() against
    oracle.ddpg_ref.DDPGLearnerRef on the envelope bars of
    tests/test_gpu_ddpg.test_ddpg_pixel_envelope;
  * DDPG with conv_spec {[8, 12], [5, 3], [2, 1], 16} on 3x30x26: the oracle's
    stem factory (oracle.ppo_ref.cnn_stem_ref) is the general factory of
    tests/stem_ref.py while the references are constructed; critic, perception,
    actor and the target perception after a hard update on the envelope bars,
    td_error against the references' Q - y, and the same steps under
    use_graph=True bit-equal to the eager learner;
  * the PPO learner under use_graph=True on the general stem captures and gives
    the eager bits;
  * DDPGAgentBatch.act with that spec equals the learner model's forward_actor.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import ddpg_ref as R
from oracle import ppo_ref
from surreal_amd import synthetic
from surreal_amd.agent import DDPGAgentBatch
from surreal_amd.config import pixel_env_config
from surreal_amd.ddpg import DDPGLearner
from tests import stem_ref as SR
from tests import test_gpu_ddpg as TD
from tests.test_gpu_cnn import _run_pixel

pytestmark = pytest.mark.gpu

SPEC = {'out_channels': [8, 12], 'kernel_sizes': [5, 3], 'strides': [2, 1], 'hidden_output_dim': 16}
SPEC_CAM = (3, 30, 26)


# ------------------------------------------------------------------------ PPO
def test_ppo_mlp_learn_on_a_camera_the_fused_stem_refuses():
    rep = _run_pixel('adapt', B=24, T=6, H=6, D=7, A=3, Hd=0, hidden=(32, 24), F=32, iters=1,
                     epochs=(1, 1), rnn=False, cam=(3, 32, 22))
    print('pixel mlp parity, 3x32x22:', rep)


def test_ppo_rnn_learn_on_a_four_channel_camera():
    rep = _run_pixel('adapt', B=24, T=6, H=2, D=7, A=3, Hd=16, hidden=(32, 24), F=32, iters=1,
                     epochs=(1, 1), rnn=True, cam=(4, 20, 24))
    print('pixel rnn parity, 4x20x24:', rep)


def test_ppo_graph_replay_with_the_general_stem_bit_exact():
    """the pixel branch of tests/test_gpu_boundary.test_ppo_graph_replay_bit_exact
    on a camera the general stem takes: every buffer and the stem's scratch are
    allocated before the capture, so use_graph=True still captures and replays
    the eager learner's bits."""
    from tests.test_gpu_boundary import _same, _state, ppo_config
    from surreal_amd.learner import PPOLearner
    lc = ppo_config(B=8, T=6, mode='adapt', use_z_filter=True, hidden=(32, 24), lam=1.0,
                    epochs=(2, 2), rnn=True, rnn_hidden=16, horizon=2, cnn_feat=16)
    D, A, Hd, pix = 9, 3, 16, (4, 20, 24)
    ec = pixel_env_config(D, A, pix)
    B, T = lc.replay.batch_size, lc.algo.n_step
    eager = PPOLearner(lc, ec, seed=4)
    graph = PPOLearner(lc, ec, seed=4, use_graph=True)
    for it in range(3):
        b = synthetic.to_device(synthetic.ppo_batch(B, T, D, A, seed=60 + it, rnn_hidden=Hd, pixel=pix),
                                'cuda')
        eager.learn(b)
        graph.learn(b)
        torch.cuda.synchronize()
        assert _same(_state(eager), _state(graph)), it
        assert eager.last_stats() == graph.last_stats(), it
    assert graph._graph is not None


# ----------------------------------------------------------------------- DDPG
def _batch(B, D, A, cam, seed):
    b = {k: v.numpy() for k, v in synthetic.ddpg_batch(B, D, A, seed=seed).items()}
    g = torch.Generator().manual_seed(100 + seed)
    b['pix'] = torch.randint(0, 256, (B,) + cam, generator=g, dtype=torch.uint8).numpy()
    b['pix_next'] = torch.randint(0, 256, (B,) + cam, generator=g, dtype=torch.uint8).numpy()
    return b


def _device_batch(b):
    dev = {k: torch.as_tensor(b[k], dtype=torch.float32).cuda() for k in ('actions', 'rewards', 'dones')}
    for k, pk in (('obs', 'pix'), ('obs_next', 'pix_next')):
        dev[k] = {'low_dim': {'flat_inputs': torch.as_tensor(b[k], dtype=torch.float32).cuda()},
                  'pixel': {'camera0': torch.as_tensor(b[pk]).cuda()}}
    return dev


def test_ddpg_learn_on_a_camera_the_fused_stem_refuses():
    B, D, A, cam = 8, 17, 6, (4, 24, 22)
    lc = TD._cfg(B, 'hard', False)
    learner = TD.ddpg_envelope_run(lc, D, A, batches=[_batch(B, D, A, cam, 70)], pixel=cam, n_ulp=3)
    assert learner.is_pixel_input
    p = learner.model.perception
    from surreal_amd import _lib as L
    assert int(L.lib().smi_stem_fused(*p.spec_args())) == 0


def _spec_cfg(B):
    lc = TD._cfg(B, 'hard', False)
    lc.algo.network.target_update = {'type': 'hard', 'interval': 1}    # the hard update follows step 1
    lc.model.conv_spec = copy.deepcopy(SPEC)
    return lc


def _td_reference(lc, D, A, init, b, dtype):
    """Q(obs, a) - y at the step's starting parameters (ddpg.py:267-296)."""
    ref = R.DDPGLearnerRef(lc, D, A, dtype=dtype, pixel=SPEC_CAM)
    TD._load_ddpg(ref, init)
    cv = lambda k: torch.as_tensor(b[k], dtype=torch.float32).to(dtype)  # noqa: E731
    with torch.no_grad():
        pt = ref.perception(ref.perc_t, (cv('obs_next'), torch.as_tensor(b['pix_next'])))
        y = cv('rewards') + pow(ref.gamma, ref.n_step) * ref.critic_t(pt, ref.actor_t(pt)) * \
            (1.0 - cv('dones'))
        q = ref.critic(ref.perception(ref.perc, (cv('obs'), torch.as_tensor(b['pix']))), cv('actions'))
    return (q - y).reshape(-1), float((q.abs() + y.abs()).max())


def test_ddpg_learn_with_a_conv_spec(monkeypatch):
    B, D, A, cam = 8, 17, 6, SPEC_CAM
    monkeypatch.setattr(ppo_ref, 'cnn_stem_ref', functools.partial(
        SR.factory, channels=SPEC['out_channels'], kernel_sizes=SPEC['kernel_sizes'],
        strides=SPEC['strides']))
    lc = _spec_cfg(B)
    ec = pixel_env_config(D, A, cam)
    learner = DDPGLearner(lc, ec, seed=2)
    p = learner.model.perception
    assert (p.conv_channels, p.kernel_sizes, p.strides, p.D_out) == ((8, 12), (5, 3), (2, 1), 16)
    assert list(p.state_dict()) == ['model.0.weight', 'model.0.bias', 'model.2.weight', 'model.2.bias',
                                    'model.5.weight', 'model.5.bias']
    assert tuple(p.state_dict()['model.2.weight'].shape) == (12, 8, 3, 3)
    init = {k: v for k, v in TD._ddpg_state(learner).items()
            if k in ('actor', 'critic', 'perc', 'perc_t')}
    b = _batch(B, D, A, cam, 71)
    np.random.seed(100)
    learner.learn(_device_batch(b))
    got = TD._ddpg_state(learner)
    td = learner.td_error.detach().cpu().clone()
    # critic, perception, actor, and the targets (perc_t: the hard update of step 1)
    report = TD.ddpg_envelope_check(lc, D, A, init, [b], [(got, learner.last_stats())], n_ulp=3,
                                    pixel=cam)
    assert not report.get('_fail'), report['_fail']
    assert torch.equal(torch.as_tensor(got['perc_t']), torch.as_tensor(got['perc']))
    assert not np.array_equal(np.asarray(got['perc']), np.asarray(init['perc']))
    # td_error: as good as torch's own fp32 step against fp64, on the scale of |Q| + |y|
    t32, _ = _td_reference(lc, D, A, init, b, torch.float32)
    t64, mag = _td_reference(lc, D, A, init, b, torch.float64)
    print('td_error: e_gpu', float((td.double() - t64).abs().max()), 'e_torch32',
          float((t32.double() - t64).abs().max()), 'mag', mag)
    TD._fp32_as_good_as_torch(td, t32, t64, 1e-6, mag)


def test_ddpg_conv_spec_graph_replay_bit_exact():
    """the same steps under use_graph=True give the eager learner's bits (a
    pixel DDPG step keeps running eagerly under use_graph, as with the fused
    stem: its observations are dicts, not the graph's static inputs)."""
    B, D, A, cam = 8, 17, 6, SPEC_CAM
    lc = _spec_cfg(B)
    ec = pixel_env_config(D, A, cam)
    eager = DDPGLearner(lc, ec, seed=3)
    graph = DDPGLearner(lc, ec, seed=3, use_graph=True)
    for it in range(3):
        b = _device_batch(_batch(B, D, A, cam, 80 + it))
        eager.learn(b)
        graph.learn(b)
        torch.cuda.synchronize()
        se, sg = TD._ddpg_state(eager), TD._ddpg_state(graph)
        for k in se:
            assert torch.equal(se[k], sg[k]), (it, k)
        assert torch.equal(eager.td_error, graph.td_error), it
        assert eager.last_stats() == graph.last_stats(), it


def test_agent_acts_with_the_conv_spec():
    N, D, A, cam = 5, 17, 6, SPEC_CAM
    lc = _spec_cfg(8)
    ec = pixel_env_config(D, A, cam)
    learner = DDPGLearner(lc, ec, seed=4)
    agent = DDPGAgentBatch(lc, ec, N, agent_mode='eval_deterministic', seed=9)
    assert agent.model.perception.conv_channels == (8, 12)
    agent.model.load_state_dict(learner.model.state_dict())
    g = torch.Generator().manual_seed(5)
    pix = torch.randint(0, 256, (N,) + cam, generator=g, dtype=torch.uint8)
    low = torch.randn(N, D, generator=g)
    act = agent.act({'low_dim': {'flat_inputs': low.numpy()}, 'pixel': {'camera0': pix.numpy()}})
    m = learner.model
    x = m.forward_perception({'low_dim': {'flat_inputs': low.cuda()}, 'pixel': {'camera0': pix.cuda()}})
    exp = m.forward_actor(x).cpu().numpy().clip(-1, 1)
    assert act.shape == (N, A)
    assert np.array_equal(act, exp)
    assert float(np.abs(act).max()) > 0
