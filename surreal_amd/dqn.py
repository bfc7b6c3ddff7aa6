"""FFQfunc / DQNLearner mirrors (surreal/model/q_net.py, surreal/learner/dqn.py)
on the MFMA GEMM layers of linear_kernels.hip and the fused TD kernel of
dqn_kernels.hip.

One DQN learn() (dqn.py:42-92; dueling double-Q, batch 512, 17-128-128-{6, 1})
is ~25 launches on one stream and no host sync: target net forward on
obs_next, online forward on obs (and on obs_next with algo.double_q),
smi_dqn_td (dueling combination, double-Q arg-max and gather, Bellman target,
Huber loss and its gradient, statistics: one launch), the input gradients of
both streams, every weight gradient of the step as ONE grouped launch
(smi_dw_group_*), and smi_adam_clip (eps 1e-4, L2 norm clip) on the flat
buffer.  The target network is a copy of the flat buffer, made whenever the
host-side sample counter enters the next multiple of
algo.target_network_update_freq (PeriodicTracker.track_increment,
session/tracker.py:22-36).

Parameter layout of FFQfunc (flat, torch (out, in) order; hidden widths h1..hn
from model.fc_hidden_sizes, 1 <= n <= 3; both streams use the same widths,
q_net.py:24-39):
  dueling : W1[2 h1][D] b1[2 h1]       the two streams' FIRST layers stacked:
                                       rows 0..h1-1 are fc_action_layers.0,
                                       rows h1..2 h1-1 are fc_state_layers.0
            action stream  Wk[hk][hk-1] bk (k = 2..n)  WA[A][hn] bA
            state stream   Wk[hk][hk-1] bk (k = 2..n)  WV[1][hn] bV
  plain   : W1[h1][D] b1  Wk[hk][hk-1] bk (k = 2..n)  WA[A][hn] bA
One smi_linear_forward produces H1 [B][2 h1] for both streams and one
weight-gradient GEMM covers both first layers; the deeper layers read their
half of H1 (and write their half of dH1) through its leading dimension.
state_dict names are the reference's: fc_action_layers.k.{weight,bias} and
fc_state_layers.k.{weight,bias}, each an nn.Parameter view of the flat buffer.

Out of scope (ConfigError): model.convs (the reference's Q-net convolutions
are SAME-padded and of free shape; the CNN kernels here are the fixed
VALID-padded PPO / DDPG stem), a 'pixel' obs spec, a non-discrete action spec.
There is no data-parallel form.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .session import LearnerHooks
from .config import Config, ConfigError
from .model import _LinearView

RELU, NONE = 1, 0


def _p(t):
    return L.ptr(t)


class _LinearAt(_LinearView):
    """weight [d_out][d_in] at w_off and bias [d_out] at b_off of a flat buffer
    (a row block of a stacked layer: the two are not adjacent)."""

    def __init__(self, flat, w_off, b_off, d_in, d_out):
        nn.Module.__init__(self)
        self.in_features, self.out_features = d_in, d_out
        self.weight = nn.Parameter(flat[w_off:w_off + d_out * d_in].view(d_out, d_in))
        self.bias = nn.Parameter(flat[b_off:b_off + d_out])


def dqn_specs(learner_config, env_config):
    """(D, A, hidden sizes, dueling) of build_ffqfunc (q_net.py:122-134) for the
    configurations this package runs; everything else raises ConfigError."""
    lc, ec = learner_config, env_config
    spec = ec['action_spec']
    if spec.get('type') != 'discrete':
        raise ConfigError('DQN needs a discrete action spec, got {!r}'.format(spec.get('type')))
    if len(spec['dim']) != 1:
        raise ConfigError('DQN action_spec.dim must have one entry')
    if list(lc['model'].get('convs') or []):
        raise ConfigError('DQN model.convs is not supported (SAME-padded free-shape convolutions; '
                          'only low-dimensional observations)')
    obs = ec['obs_spec']
    if 'pixel' in obs or bool(ec.get('pixel_input', False)):
        raise ConfigError('DQN pixel observations are not supported')
    D = int(sum(v[0] for v in obs['low_dim'].values()))
    hidden = [int(h) for h in lc['model']['fc_hidden_sizes']]
    if not 1 <= len(hidden) <= 3 or min(hidden) < 1:
        raise ConfigError('DQN model.fc_hidden_sizes must hold 1 to 3 positive widths')
    return D, int(spec['dim'][0]), hidden, bool(lc['model']['dueling'])


class FFQfunc(nn.Module):
    """q_net.py:9-119 for low-dimensional observations over ONE flat fp32
    buffer (layout: module docstring)."""

    def __init__(self, D_in, action_dim, fc_hidden_sizes, dueling, device=None, generator=None):
        super().__init__()
        L.require_gpu()
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        hs = [int(h) for h in fc_hidden_sizes]
        if not 1 <= len(hs) <= 3:
            raise ConfigError('FFQfunc takes 1 to 3 hidden widths')
        self.dims = (int(D_in), tuple(hs), int(action_dim))
        self.dueling = bool(dueling)
        D, A, S = int(D_in), int(action_dim), 2 if dueling else 1
        h1 = hs[0]
        deep = lambda out: sum(hs[k] * hs[k - 1] + hs[k] for k in range(1, len(hs))) + \
            out * hs[-1] + out                                              # noqa: E731
        n = S * h1 * D + S * h1 + deep(A) + (deep(1) if dueling else 0)
        flat = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.__dict__['flat'] = flat
        b1 = S * h1 * D
        self.__dict__['w1'] = flat[:b1].view(S * h1, D)
        self.__dict__['b1'] = flat[b1:b1 + S * h1]
        off = b1 + S * h1
        streams = []
        for s, out in enumerate((A, 1)[:S]):
            layers = [_LinearAt(flat, s * h1 * D, b1 + s * h1, D, h1)]
            for k in range(1, len(hs)):
                layers.append(_LinearView(flat, off, hs[k - 1], hs[k]))
                off = layers[-1].end
            layers.append(_LinearView(flat, off, hs[-1], out))
            off = layers[-1].end
            streams.append(layers)
        assert off == n
        # construction (and so initialisation) order of q_net.py:25-39
        self.fc_action_layers = nn.ModuleList(streams[0])
        for lin in self.fc_action_layers:
            lin.reset_parameters(generator)
        if dueling:
            self.fc_state_layers = nn.ModuleList(streams[1])
            for lin in self.fc_state_layers:
                lin.reset_parameters(generator)

    def streams(self):
        return [self.fc_action_layers] + ([self.fc_state_layers] if self.dueling else [])

    def off(self, p):
        """offset of a parameter view in the flat buffer (= in a gradient image)"""
        return (p.data_ptr() - self.flat.data_ptr()) // 4

    def copy_from(self, other):                      # nnx.Module.copy_from / clone
        with torch.no_grad():
            self.flat.copy_(other.flat)

    def clone(self):
        D, hs, A = self.dims
        c = FFQfunc(D, A, hs, self.dueling, self.device)
        c.copy_from(self)
        return c

    def forward(self, x):
        """q values [rows][A] (q_net.py:41-65) of a float32 device matrix"""
        x = x if x.stride(-1) == 1 else x.contiguous()
        adv, val = _QNet(self, {}).fwd(x, x.shape[0], 'f')
        if not self.dueling:
            return adv.clone()
        return (adv - adv.mean(dim=1, keepdim=True)) + val


class _QNet(object):
    """Launch helpers over an FFQfunc's flat buffer."""

    def __init__(self, model, bufs):
        self.m = model
        self.st = L.stream(model.device)
        self.bufs = bufs

    def buf(self, name, shape):
        t = self.bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.zeros(shape, dtype=torch.float32, device=self.m.device)
            self.bufs[name] = t
        return t

    def lin(self, x, ldx, rows, k, w, ldw, b, n, act, y, ldy):
        L.call('smi_linear_forward', _p(x), ldx, rows, k, _p(w), ldw, _p(b), n, act, _p(y), ldy,
               self.st)

    def fwd(self, x, rows, pre):
        """(ADV [rows][A], VAL [rows][1] | None); the hidden activations stay in
        the buffers pre_h1 ([rows][S h1], both streams) and pre_h{k}_{s}"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        if (x.dim() != 2 or x.shape[0] < rows or x.shape[1] != D or x.stride(1) != 1
                or x.dtype != torch.float32):
            raise ValueError(f'q_func input: expected a float32 [{rows}][{D}] matrix, got '
                             f'{x.dtype} {tuple(x.shape)}')
        H1 = self.buf(pre + '_h1', (rows, S * hs[0]))
        self.lin(x, x.stride(0), rows, D, m.w1, D, m.b1, S * hs[0], RELU, H1, S * hs[0])
        outs = []
        for s, layers in enumerate(m.streams()):
            prev, ld = H1[:, s * hs[0]:], S * hs[0]
            for k in range(1, len(hs)):
                H = self.buf(f'{pre}_h{k + 1}_{s}', (rows, hs[k]))
                lin = layers[k]
                self.lin(prev, ld, rows, hs[k - 1], lin.weight, hs[k - 1], lin.bias, hs[k], RELU,
                         H, hs[k])
                prev, ld = H, hs[k]
            lin = layers[-1]
            n_out = lin.out_features
            out = self.buf(f'{pre}_out_{s}', (rows, n_out))
            self.lin(prev, ld, rows, hs[-1], lin.weight, hs[-1], lin.bias, n_out, NONE, out, n_out)
            outs.append(out)
        return outs[0], (outs[1] if m.dueling else None)

    def bwd(self, x, rows, pre, douts, g):
        """from douts[s] = d loss / d (stream s's output) into the gradient image
        g (the flat layout); the weight-gradient calls queue into the caller's
        open group, so every dY / X buffer is written once and left alone"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        st = self.st
        H1 = self.bufs[pre + '_h1']
        dH1 = self.buf(pre + '_dh1', (rows, S * hs[0]))
        for s, layers in enumerate(m.streams()):
            acts = [(H1[:, s * hs[0]:], S * hs[0])] + \
                [(self.bufs[f'{pre}_h{k + 1}_{s}'], hs[k]) for k in range(1, len(hs))]
            grads = [(dH1[:, s * hs[0]:], S * hs[0])] + \
                [(self.buf(f'{pre}_dh{k + 1}_{s}', (rows, hs[k])), hs[k]) for k in range(1, len(hs))]
            dy, ldg = douts[s], douts[s].shape[1]
            for k in range(len(hs), 0, -1):           # layers[k]: hs[k-1] -> out
                lin = layers[k]
                n_out = lin.out_features
                xk, ldx = acts[k - 1]
                dx, lddx = grads[k - 1]
                L.call('smi_linear_backward_weight', _p(dy), ldg, rows, n_out, _p(xk), ldx, hs[k - 1],
                       _p(g[m.off(lin.weight):]), hs[k - 1], _p(g[m.off(lin.bias):]), 0, st)
                L.call('smi_linear_backward_input', _p(dy), ldg, rows, n_out, _p(lin.weight),
                       hs[k - 1], hs[k - 1], _p(xk), ldx, _p(dx), lddx, st)
                dy, ldg = dx, lddx
        # both streams' first layers: one weight-gradient GEMM over dH1 [rows][S h1]
        L.call('smi_linear_backward_weight', _p(dH1), S * hs[0], rows, S * hs[0], _p(x), x.stride(0),
               D, _p(g), D, _p(g[S * hs[0] * D:]), 0, st)


class TargetUpdateTracker(object):
    """PeriodicTracker.track_increment (session/tracker.py:22-36) on host
    integers: True when value += incr has entered the next period."""

    def __init__(self, period, value=0, endpoint=0):
        if int(period) < 1:
            raise ConfigError('target_network_update_freq must be a positive integer')
        self.period, self.value, self.endpoint = int(period), int(value), int(endpoint)

    def track_increment(self, incr=1):
        self.value += int(incr)
        if self.value >= self.endpoint + self.period:
            self.endpoint += (self.value - self.endpoint) // self.period * self.period
            return True
        return False


def _column(t, B, what):
    """(tensor, row stride) of a float32 device column [B] or [B, 1]"""
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or t.shape[0] != B or t.dtype != torch.float32:
        raise ValueError(f'{what}: expected float32 [{B}] or [{B}, 1], got {t.dtype} {tuple(t.shape)}')
    return t, (t.stride(0) if B > 1 else 1)


class DQNLearner(LearnerHooks):
    """dqn.py:9-126 on MI355X (low-dimensional observations, discrete
    actions).  A batch with a 'weights' entry (float32 [B] or [B, 1],
    replay.PrioritizedReplay.sample_batch) weights the Huber loss; after every
    learn() `td_error` is a device view [B] of Q(s, a) - y
    (PrioritizedReplay.update_priorities_from_td)."""

    def __init__(self, learner_config, env_config, session_config=None, metrics=None,
                 device=None, seed=0, use_graph=False, checkpoint=None,
                 checkpoint_full_state=False):
        self.learner_config = lc = learner_config if isinstance(learner_config, Config) \
            else Config(learner_config)
        self.env_config = ec = env_config if isinstance(env_config, Config) else Config(env_config)
        D, A, hidden, dueling = dqn_specs(lc, ec)
        self.algo = algo = lc.algo
        self.target_update_tracker = TargetUpdateTracker(algo.target_network_update_freq)
        L.require_gpu()
        self.checkpoint_full_state = bool(checkpoint_full_state)
        self.session_config = session_config
        self._init_hooks(metrics, checkpoint)
        self.device = torch.device(device) if device is not None else \
            torch.device('cuda', torch.cuda.current_device())
        L.ensure_workspace(self.device)
        self._ctx = L.Context(self.device)      # this learner's own workspace (re-entrancy)
        self.current_iteration = 0
        self.action_dim, self.obs_dim = A, D
        self.double_q = bool(algo.double_q)
        clip = algo.get('grad_norm_clipping')
        self.max_norm = float(clip) if clip else 0.0          # None or 0: no clip (dqn.py:33-35)
        gen = torch.Generator().manual_seed(seed)
        self.q_func = FFQfunc(D, A, hidden, dueling, self.device, gen)
        self.q_target = self.q_func.clone()                   # dqn.py:17
        flat, dev = self.q_func.flat, self.device
        self.opt = {'m': torch.zeros_like(flat), 'v': torch.zeros_like(flat),
                    'step': torch.zeros(1, dtype=torch.int32, device=dev),
                    'lr': torch.tensor([algo.lr], dtype=torch.float32, device=dev),
                    'g': torch.zeros_like(flat)}
        self.stats_buf = torch.zeros(2, dtype=torch.float32, device=dev)
        self.td_error = None
        self._bufs = {}
        self.use_graph = bool(use_graph)
        self._graph = None
        self._gin = None

    # ------------------------------------------------------------ helpers
    def _update_target(self):                                            # dqn.py:27-28
        self.q_target.copy_from(self.q_func)

    def preprocess(self, batch):
        """host batch (SSARAggregator.aggregate: int32 actions) -> device
        tensors; the action indices become the float32 column the kernel reads.
        Actions outside [0, A) raise ValueError before anything is launched."""
        a = np.asarray(batch['actions'].cpu() if isinstance(batch['actions'], torch.Tensor)
                       else batch['actions'])
        if a.size and (not np.all(a == np.round(a)) or a.min() < 0 or a.max() >= self.action_dim):
            raise ValueError(f'actions must be integers in [0, {self.action_dim})')
        out = {}
        for k in ('obs', 'obs_next'):
            v = batch[k]
            if isinstance(v, dict):
                v = v['low_dim']['flat_inputs']
            out[k] = torch.as_tensor(v, dtype=torch.float32).to(self.device, non_blocking=True)
        out['actions'] = torch.as_tensor(a.astype(np.float32).reshape(-1, 1)).to(
            self.device, non_blocking=True)
        for k in ('rewards', 'dones'):
            out[k] = torch.as_tensor(batch[k], dtype=torch.float32).to(self.device, non_blocking=True)
        if batch.get('weights') is not None:
            out['weights'] = torch.as_tensor(batch['weights'], dtype=torch.float32).to(
                self.device, non_blocking=True)
        return Config(out)

    # --------------------------------------------------------- _optimize
    def _optimize(self, obs, actions, rewards, obs_next, dones, weights=None):   # dqn.py:42-73
        B, A = obs.shape[0], self.action_dim
        act, a_s = _column(actions, B, 'actions')
        rew, r_s = _column(rewards, B, 'rewards')
        don, d_s = _column(dones, B, 'dones')
        if weights is not None:
            weights, w_s = _column(weights, B, 'weights')
            if w_s != 1:
                raise ValueError('weights must be contiguous')
        st = L.stream(self.device)
        dueling = self.q_func.dueling
        net, tnet = _QNet(self.q_func, self._bufs), _QNet(self.q_target, self._bufs)
        adv_t, val_t = tnet.fwd(obs_next, B, 't')
        adv, val = net.fwd(obs, B, 'q')
        adv_n = val_n = None
        if self.double_q:
            adv_n, val_n = net.fwd(obs_next, B, 'n')
        dadv = net.buf('dadv', (B, A))
        dval = net.buf('dval', (B, 1)) if dueling else None
        self.td_error = net.buf('td', (B,))
        L.call('smi_dqn_td', _p(adv), A, _p(adv_n), A, _p(adv_t), A, _p(val), 1, _p(val_n), 1,
               _p(val_t), 1, _p(act), a_s, _p(rew), r_s, _p(don), d_s, _p(weights), B, A,
               float(self.algo.gamma), int(dueling), int(self.double_q), _p(dadv), A, _p(dval),
               _p(self.td_error), None, _p(self.stats_buf), st)
        o = self.opt
        L.call('smi_dw_group_begin')
        try:
            net.bwd(obs, B, 'q', [dadv, dval] if dueling else [dadv], o['g'])
        finally:
            L.call('smi_dw_group_flush', st)       # always flush: nothing stays queued
        flat = self.q_func.flat
        L.call('smi_adam_clip', _p(flat), _p(o['g']), _p(o['m']), _p(o['v']), flat.numel(),
               _p(o['step']), _p(o['lr']), 0.9, 0.999, 1e-4, 0.0, self.max_norm, 0.0, None, None, st)

    # ------------------------------------------------------- reference API
    def learn(self, batch):                                              # dqn.py:75-92
        self.current_iteration += 1
        self._ctx.make_current()
        if not isinstance(batch['actions'], torch.Tensor) or not batch['actions'].is_cuda:
            batch = self.preprocess(batch)
        obs, obs_next = batch['obs'], batch['obs_next']
        obs = obs['low_dim']['flat_inputs'] if isinstance(obs, dict) else obs
        obs_next = obs_next['low_dim']['flat_inputs'] if isinstance(obs_next, dict) else obs_next
        actions = batch['actions']
        if actions.dtype != torch.float32:
            actions = actions.to(torch.float32)
        ins = (obs, actions, batch['rewards'], obs_next, batch['dones'])
        weights = batch.get('weights')
        if self.use_graph:
            self._optimize_graphed(*ins, weights=weights)
        else:
            self._optimize(*ins, weights=weights)
        if self.target_update_tracker.track_increment(int(obs.shape[0])):
            self._update_target()
        self._report_metrics(self.current_iteration)
        self.periodic_checkpoint(global_steps=self.current_iteration, score=None)

    def _optimize_graphed(self, obs, actions, rewards, obs_next, dones, weights=None):
        """One _optimize as a hipGraph replay, as DDPGLearner._optimize_graphed:
        the first call runs eagerly (it is that call's update and sizes every
        buffer), then the same launch sequence is captured over static input
        buffers; later calls copy their inputs in and replay.  The weights are
        one more static input (a graph captured without them is captured again
        when they appear, and the other way round).  The target copy stays on
        the host, where its counter lives."""
        ins = (obs, actions, rewards, obs_next, dones)
        if weights is not None:
            ins = ins + (weights,)
        if self._graph is not None and (len(self._gin) != len(ins) or
                                        self._gin[0].shape[0] != obs.shape[0]):
            self._graph = None
        if self._graph is None:
            self._optimize(*ins[:5], weights=weights)
            self._gin = [torch.zeros(tuple(t.shape), dtype=torch.float32, device=self.device)
                         for t in ins]
            g = torch.cuda.CUDAGraph()
            with L.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
                self._optimize(*self._gin[:5], weights=self._gin[5] if weights is not None else None)
            self._graph = g
            return
        for s, t in zip(self._gin, ins):
            if s.data_ptr() != t.data_ptr():
                s.copy_(t)
        self._graph.replay()

    def graph_inputs(self):
        """Static (obs, actions, rewards, obs_next, dones[, weights]) buffers of
        the captured step (None before the first learn() in graph mode)."""
        return None if self._gin is None else dict(zip(
            ('obs', 'actions', 'rewards', 'obs_next', 'dones', 'weights'), self._gin))

    def _host_scalars(self):
        return {}

    def last_stats(self):
        return self._stats_dict(self.stats_buf.cpu().numpy(), {})

    def _stats_dict(self, v, host):
        """'td_error' is the reference's scalar mean |td| (dqn.py:89-92)"""
        return {'loss': float(v[0]), 'td_error': float(v[1])}

    def module_dict(self):                                               # dqn.py:123-126
        return {'q_func': self.q_func}

    def checkpoint_attributes(self):
        """q_func, q_target and the optimizer state (the step count and learning
        rate; a restored learner starts from fresh moments, as a restored
        torch.optim.Adam without its state would); checkpoint_full_state adds
        the Adam moments and the target tracker for a bit-identical
        continuation."""
        return ['current_iteration', 'q_func', 'q_target', 'optimizer_state_host']

    @property
    def optimizer_state_host(self):
        o = self.opt
        out = {'lr': o['lr'].detach().cpu().clone()}
        if self.checkpoint_full_state:
            out.update({k: o[k].detach().cpu().clone() for k in ('m', 'v', 'step')})
            t = self.target_update_tracker
            out['tracker'] = (t.value, t.endpoint)
        return out

    @optimizer_state_host.setter
    def optimizer_state_host(self, d):
        with torch.no_grad():
            for k in ('m', 'v', 'step', 'lr'):
                if k in d:
                    self.opt[k].copy_(torch.as_tensor(d[k]).to(self.device))
        if 'tracker' in d:
            self.target_update_tracker.value, self.target_update_tracker.endpoint = d['tracker']

    def _prefetcher_preprocess(self, batch):
        from .aggregator import SSARAggregator
        return SSARAggregator(self.env_config.obs_spec, self.env_config.action_spec).aggregate(batch)
