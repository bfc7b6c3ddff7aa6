"""Shared test helpers: configs and oracle <-> product weight transfer."""
import copy

import numpy as np
import torch

from surreal_amd.config import (DDPG_DEFAULT_LEARNER_CONFIG, PPO_DEFAULT_LEARNER_CONFIG, Config,
                                gym_env_config)


def ppo_config(B=64, T=50, mode='clip', use_z_filter=True, hidden=(64, 64), lam=0.95,
               gamma=0.99, epochs=(10, 10), norm_adv=True, use_r_filter=False, reward_scale=1.0,
               kl_target=0.02, lr=(3e-4, 3e-4), wd=(0.0, 0.0), rnn=False, rnn_hidden=100,
               horizon=5, critic_hidden=None, cnn_feat=256, rnn_layer=1):
    lc = copy.deepcopy(PPO_DEFAULT_LEARNER_CONFIG)
    lc.model.actor_fc_hidden_sizes = list(hidden)
    lc.model.critic_fc_hidden_sizes = list(critic_hidden if critic_hidden is not None else hidden)
    lc.algo.use_z_filter = use_z_filter
    lc.algo.use_r_filter = use_r_filter
    lc.algo.gamma = gamma
    lc.algo.n_step = T
    lc.algo.ppo_mode = mode
    lc.algo.advantage.lam = lam
    lc.algo.advantage.norm_adv = norm_adv
    lc.algo.advantage.reward_scale = reward_scale
    lc.algo.rnn.if_rnn_policy = bool(rnn)
    lc.algo.rnn.rnn_hidden = rnn_hidden
    lc.algo.rnn.rnn_layer = rnn_layer
    lc.algo.rnn.horizon = horizon
    lc.algo.consts.epoch_policy = epochs[0]
    lc.algo.consts.epoch_baseline = epochs[1]
    lc.algo.consts.kl_target = kl_target
    lc.algo.network.lr_actor = lr[0]
    lc.algo.network.lr_critic = lr[1]
    lc.algo.network.anneal.min_lr = min(lr)
    lc.algo.network.actor_regularization = wd[0]
    lc.algo.network.critic_regularization = wd[1]
    lc.replay.batch_size = B
    lc.model.cnn_feature_dim = cnn_feat
    return lc


def env_config(D=17, A=6):
    return gym_env_config(D, A)


def ddpg_config(B=512, target='hard', clip_critic=False, layernorm=False):
    lc = copy.deepcopy(DDPG_DEFAULT_LEARNER_CONFIG)
    lc.replay.batch_size = B
    lc.model.use_layernorm = layernorm
    lc.algo.network.clip_critic_gradient = clip_critic
    if target == 'soft':
        lc.algo.network.target_update = {'type': 'soft', 'tau': 1e-3}
    else:
        lc.algo.network.target_update = {'type': 'hard', 'interval': 2}
    return lc


def per_cfg(B=64, memory_size=200, double=False, action_reg=False):
    """ddpg_config for a learner fed by a PrioritizedReplay"""
    lc = ddpg_config(B, 'hard')
    lc.replay.memory_size = memory_size
    lc.replay.sampling_start_size = 10
    lc.replay.alpha = 0.6
    lc.algo.network.use_double_critic = double
    lc.algo.network.use_action_regularization = action_reg
    return lc


def replay_rows(n, D, A, seed):
    """n packed replay rows [obs | action | reward | obs_next | done] on the host"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(n, 2 * D + A + 2, generator=g)
    rows[:, D:D + A] = torch.tanh(rows[:, D:D + A])
    rows[:, 2 * D + A + 1] = (torch.rand(n, generator=g) < 0.1).float()
    return rows


def copy_weights_to_oracle(learner, ref):
    """product (device flat buffers) -> oracle (CPU torch modules)."""
    ref.model.actor.load_flat(learner.model.actor.flat.detach().cpu())
    ref.model.critic.load_flat(learner.model.critic.flat.detach().cpu())
    ref.ref_target_model.actor.load_flat(learner.ref_target_model.actor.flat.detach().cpu())
    ref.ref_target_model.critic.load_flat(learner.ref_target_model.critic.flat.detach().cpu())
    if getattr(learner, 'if_rnn_policy', False):
        for src, dst in ((learner.model, ref.model), (learner.ref_target_model, ref.ref_target_model)):
            load_lstm_flat(dst.rnn_stem, src.rnn_stem.flat.detach().cpu())
    if getattr(learner, 'if_pixel_input', False):
        for src, dst in ((learner.model, ref.model), (learner.ref_target_model, ref.ref_target_model)):
            load_seq_flat(dst.cnn_stem, src.cnn_stem.flat.detach().cpu())
    if learner.use_z_filter:
        for a, b in ((learner.model.z_filter, ref.model.z_filter),
                     (learner.ref_target_model.z_filter, ref.ref_target_model.z_filter)):
            b.running_sum.copy_(a.running_sum.cpu())
            b.running_sumsq.copy_(a.running_sumsq.cpu())
            b.count.copy_(a.count.cpu())


def load_lstm_flat(lstm, flat):
    """C-ABI LSTM layout (per layer [W_ih | W_hh | b_ih | b_hh]) -> a torch nn.LSTM
    (nn.LSTM.parameters() has exactly that order)."""
    o = 0
    with torch.no_grad():
        for p in lstm.parameters():
            n = p.numel()
            p.copy_(flat[o:o + n].reshape(p.shape))
            o += n


def load_seq_flat(module, flat):
    """flat buffer -> module.parameters() in order (the C-ABI CNN layout)."""
    o = 0
    with torch.no_grad():
        for p in module.parameters():
            n = p.numel()
            p.copy_(flat[o:o + n].reshape(p.shape))
            o += n
    assert o == flat.numel()


def seq_flat(module):
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()])


def lstm_flat(lstm):
    return torch.cat([p.detach().reshape(-1) for p in lstm.parameters()])


def oracle_batch(batch):
    """Synthetic batch (surreal_amd.synthetic layout) -> oracle learn() dict."""
    out = {'obs': None, 'obs_next': None,
           'actions': batch['actions'], 'rewards': batch['rewards'], 'dones': batch['dones'],
           'pds': batch['persistent_infos'][-1], 'onetime': batch['onetime_infos']}
    if 'low_dim' in batch['obs']:
        key = list(batch['obs']['low_dim'])[0]
        out['obs'] = batch['obs']['low_dim'][key]
        out['obs_next'] = batch['obs_next']['low_dim'][key]
    if 'pixel' in batch['obs']:
        out['pixels'] = batch['obs']['pixel']['camera0']
        out['pixels_next'] = batch['obs_next']['pixel']['camera0']
    return out


def max_rel_err(x, ref, floor=None):
    """max |x - ref| / (|ref| + floor); floor defaults to 1e-2 * max|ref|, so an
    entry that cancels to ~0 is judged relative to the tensor's scale (fp32
    summation-order noise is ~1e-7 of the summed magnitudes, not of the result)."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if floor is None:
        floor = 1e-2 * max(1e-30, float(np.max(np.abs(ref))) if ref.size else 1.0)
    return float(np.max(np.abs(x - ref) / (np.abs(ref) + floor))) if ref.size else 0.0
