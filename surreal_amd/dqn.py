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

Pixel observations (model.convs on a pixel-only obs spec; dqn_conv_specs): the
reference's conv_layers (q_net.py:82-102,112-119: nn.Conv2d(padding = k // 2),
'SAME' mode, ReLU after each, U.flatten_conv) run on the general convolution
layer of conv_kernels.hip (smi_conv2d_*), one launch per layer and direction.
The flat buffer then starts with the conv layers, [w (cout, cin, k, k) | b]
each, followed by the layout above with D = prod(pre-FC shape); state_dict
names and order are the reference's: conv_layers.k.{weight,bias}, then
fc_action_layers.*, then fc_state_layers.*.  One learn() is: target stem +
heads on obs_next, online stem + heads on obs (activations kept), online on
obs_next with double_q, smi_dqn_td, the heads' backward, the first FC layer's
input gradient masked by the last conv activation, per conv layer the weight
gradient and (except layer 0) the input gradient into the same gradient image,
and the one smi_adam_clip over the whole flat buffer: the norm clip covers
conv and FC parameters together, as clip_grad_norm_ over q_func.parameters().
Frames stay uint8 on the device and are read in place (a replay's
sample_batch() output is not copied); model.is_uint8 (x / 255.0, q_net.py:
113-115) defaults to True here, where the reference's build_ffqfunc leaves
FFQfunc.is_uint8 at False and so feeds 0..255 to the first convolution: Atari
frames are bytes and the scaled input is what the class documents; False runs
the reference builder's behaviour.  The 1 / 255 is folded into the kernels'
epilogues (conv_kernels.hip).
Initialisation of every view (Linear and Conv) is this build's own rule,
torch's default for nn.Linear / nn.Conv2d (U(+-1/sqrt(fan_in)) for weight and
bias); U.conv_fc_init is torchx-side and unpinned, parity tests load weights.

Out of scope (ConfigError): model.convs on a low-dimensional obs spec, a
'pixel' obs spec without convs or together with 'low_dim' (FFQfunc has one
input), more than 4 conv layers or a layer outside the kernel's ranges
(1 <= k <= 8, 1 <= stride <= min(k, 4), 1 <= channels <= 128), a non-discrete
action spec.

Data parallel (DQNLearner(dp=...); DeviceLearner owns the learn() frame and the
layout of the exchange image): N ranks each learn on B / N rows of one global
draw (replay.sample_shard) and end with the parameters, statistics, TD errors
and, through
update_priorities_from_td(idx_all, learner.td_error), the priority trees that
one learner on the B rows would have.  smi_dqn_td_shard divides by the global
batch, so the SUM of the ranks' gradient images is the global-batch gradient;
it writes its rows of td_all [B] and +0.0 elsewhere, so the same SUM gathers
the TD errors exactly; its statistics sum to the global means.  The three sit
in ONE exchange image [gradient | td_all | stats] and one all-reduce per
learn(), between the backward and smi_adam_clip, so the norm clip acts on the
global-batch gradient.  Every rank then runs the same Adam on the same bits.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .config import Config, ConfigError
from .device_learner import DeviceLearner, LaunchNet, as_config, exchange_image, p
from .model import _LinearView

RELU, NONE = 1, 0


class _LinearAt(_LinearView):
    """weight [d_out][d_in] at w_off and bias [d_out] at b_off of a flat buffer
    (a row block of a stacked layer: the two are not adjacent)."""

    def __init__(self, flat, w_off, b_off, d_in, d_out):
        nn.Module.__init__(self)
        self.in_features, self.out_features = d_in, d_out
        self.weight = nn.Parameter(flat[w_off:w_off + d_out * d_in].view(d_out, d_in))
        self.bias = nn.Parameter(flat[b_off:b_off + d_out])


def _action_dim(ec):
    spec = ec['action_spec']
    if spec.get('type') != 'discrete':
        raise ConfigError('DQN needs a discrete action spec, got {!r}'.format(spec.get('type')))
    if len(spec['dim']) != 1:
        raise ConfigError('DQN action_spec.dim must have one entry')
    return int(spec['dim'][0])


def _hidden_sizes(lc):
    hidden = [int(h) for h in lc['model']['fc_hidden_sizes']]
    if not 1 <= len(hidden) <= 3 or min(hidden) < 1:
        raise ConfigError('DQN model.fc_hidden_sizes must hold 1 to 3 positive widths')
    return hidden


def dqn_specs(learner_config, env_config):
    """(D, A, hidden sizes, dueling) of build_ffqfunc (q_net.py:122-134) for a
    low-dimensional obs spec; everything else raises ConfigError (a pixel-only
    spec with model.convs goes through dqn_conv_specs)."""
    lc, ec = learner_config, env_config
    A = _action_dim(ec)
    if list(lc['model'].get('convs') or []):
        raise ConfigError('DQN model.convs needs a pixel-only obs spec (SAME-padded convolutions '
                          'over camera0); this spec is low-dimensional')
    obs = ec['obs_spec']
    if 'pixel' in obs or bool(ec.get('pixel_input', False)):
        raise ConfigError('DQN pixel observations need model.convs and no low_dim modality '
                          '(dqn_conv_specs)')
    D = int(sum(v[0] for v in obs['low_dim'].values()))
    return D, A, _hidden_sizes(lc), bool(lc['model']['dueling'])


MAX_CONVS = 4


def conv_chain(input_shape, convs):
    """([(cin, H, W, cout, k, stride, pad)] per layer, pre-FC shape (C, H, W)) of
    q_net.py:85-102: pad = k // 2 and U.infer_shape_conv2d's
    (H + 2 pad - k) // stride + 1.  ValueError for an invalid input or pre-FC
    shape (q_net.py:83,104-105)."""
    if len(input_shape) != 3:
        raise ValueError('convs need a 3-D input_shape (C, H, W), got {}'.format(tuple(input_shape)))
    C, H, W = (int(v) for v in input_shape)
    layers = []
    for cout, k, s in convs:
        cout, k, s = int(cout), int(k), int(s)
        if min(C, H, W) < 1:
            break
        layers.append((C, H, W, cout, k, s, k // 2))
        H, W = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        C = cout
    if min(C, H, W) < 1:
        raise ValueError('Pre-FC shape has invalid size: {}'.format((C, H, W)))
    return layers, (C, H, W)


def check_convs(convs, in_channels):
    """model.convs as [[cout, k, stride]] within the ranges of smi_conv2d_*"""
    convs = [list(c) for c in (convs or [])]
    if not 1 <= len(convs) <= MAX_CONVS:
        raise ConfigError('DQN model.convs must hold 1 to {} layers, got {}'.format(MAX_CONVS,
                                                                                    len(convs)))
    if not 1 <= int(in_channels) <= 128:
        raise ConfigError('DQN pixel input must have 1 to 128 channels, got {}'.format(in_channels))
    for c in convs:
        if len(c) != 3:
            raise ConfigError('DQN model.convs entries are [cout, kernel_size, stride], got '
                              '{!r}'.format(c))
        cout, k, s = (int(v) for v in c)
        if not (1 <= cout <= 128 and 1 <= k <= 8 and 1 <= s <= min(k, 4)):
            raise ConfigError('DQN model.convs layer {!r} is outside 1 <= cout <= 128, 1 <= k <= 8, '
                              '1 <= stride <= min(k, 4)'.format(c))
    return [[int(v) for v in c] for c in convs]


def dqn_conv_specs(learner_config, env_config):
    """(input shape (C, H, W), convs, A, hidden sizes, dueling, is_uint8) of
    build_ffqfunc for a pixel-only obs spec with 1 to 4 conv layers and discrete
    actions.  model.is_uint8 defaults to True (module docstring)."""
    lc, ec = learner_config, env_config
    A = _action_dim(ec)
    obs = ec['obs_spec']
    if 'pixel' not in obs:
        raise ConfigError('dqn_conv_specs takes a pixel obs spec')
    if 'low_dim' in obs:
        raise ConfigError('DQN takes a pixel-only obs spec or a low_dim-only one (FFQfunc has one '
                          'input), got both')
    if len(obs['pixel']) != 1:
        raise ConfigError('DQN pixel observations: exactly one camera, got {}'.format(
            sorted(obs['pixel'])))
    convs = list(lc['model'].get('convs') or [])
    if not convs:
        raise ConfigError('DQN pixel observations need model.convs')
    shape = tuple(int(v) for v in list(obs['pixel'].values())[0])
    if len(shape) != 3:
        raise ConfigError('DQN pixel observations are (C, H, W), got {}'.format(shape))
    convs = check_convs(convs, shape[0])
    conv_chain(shape, convs)
    return (shape, convs, A, _hidden_sizes(lc), bool(lc['model']['dueling']),
            bool(lc['model'].get('is_uint8', True)))


def dqn_model_kwargs(learner_config, env_config):
    """(D, A, hidden, dueling, FFQfunc keyword arguments): dqn_conv_specs for a
    spec with pixels, dqn_specs otherwise.  Host only."""
    if 'pixel' in env_config['obs_spec']:
        shape, convs, A, hidden, dueling, u8 = dqn_conv_specs(learner_config, env_config)
        D = int(np.prod(conv_chain(shape, convs)[1]))
        return D, A, hidden, dueling, {'convs': convs, 'input_shape': shape, 'is_uint8': u8}
    D, A, hidden, dueling = dqn_specs(learner_config, env_config)
    return D, A, hidden, dueling, {}


def ffq_param_names(n_convs, n_hidden, dueling):
    """state_dict keys in the reference's construction order (q_net.py:25-39,87-98)"""
    names = [f'conv_layers.{i}.{p}' for i in range(n_convs) for p in ('weight', 'bias')]
    for stream in ('fc_action_layers', 'fc_state_layers')[:2 if dueling else 1]:
        names += [f'{stream}.{i}.{p}' for i in range(n_hidden + 1) for p in ('weight', 'bias')]
    return names


class _ConvAt(_LinearView):
    """weight (cout, cin, k, k) and bias (cout) at `off` of a flat buffer"""

    def __init__(self, flat, off, cin, cout, k):
        nn.Module.__init__(self)
        self.in_features, self.out_features = cin * k * k, cout      # fan-in of reset_parameters
        self.weight = nn.Parameter(flat[off:off + cout * cin * k * k].view(cout, cin, k, k))
        off += cout * cin * k * k
        self.bias = nn.Parameter(flat[off:off + cout])
        self.end = off + cout


class FFQfunc(nn.Module):
    """q_net.py:9-119 over ONE flat fp32 buffer (layout: module docstring).
    With convs ([[cout, k, stride]], input_shape (C, H, W)) the input is a
    uint8 or float32 (rows, C, H, W) device tensor and D_in is ignored."""

    def __init__(self, D_in, action_dim, fc_hidden_sizes, dueling, device=None, generator=None,
                 convs=None, input_shape=None, is_uint8=False):
        super().__init__()
        hs = [int(h) for h in fc_hidden_sizes]
        if not 1 <= len(hs) <= 3:
            raise ConfigError('FFQfunc takes 1 to 3 hidden widths')
        self.convs = [[int(v) for v in c] for c in (convs or [])]
        self.is_uint8 = bool(is_uint8)
        self.input_shape = None
        self.conv_geoms = []
        if self.convs:
            if input_shape is None or len(tuple(input_shape)) != 3:          # q_net.py:82-83
                raise ValueError('convs need a 3-D input_shape (C, H, W), got {!r}'.format(input_shape))
            self.input_shape = tuple(int(v) for v in input_shape)
            check_convs(self.convs, max(self.input_shape[0], 1))
            self.conv_geoms, pre = conv_chain(self.input_shape, self.convs)
            D_in = int(np.prod(pre))
        L.require_gpu()
        self.device = torch.device(device) if device is not None else torch.device('cuda')
        self.dims = (int(D_in), tuple(hs), int(action_dim))
        self.dueling = bool(dueling)
        D, A, S = int(D_in), int(action_dim), 2 if dueling else 1
        h1 = hs[0]
        deep = lambda out: sum(hs[k] * hs[k - 1] + hs[k] for k in range(1, len(hs))) + \
            out * hs[-1] + out                                              # noqa: E731
        fc0 = sum(co * ci * k * k + co for ci, _, _, co, k, _, _ in self.conv_geoms)
        n = fc0 + S * h1 * D + S * h1 + deep(A) + (deep(1) if dueling else 0)
        flat = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.__dict__['flat'] = flat
        if self.convs:
            off, cl = 0, []
            for ci, _, _, co, k, _, _ in self.conv_geoms:
                cl.append(_ConvAt(flat, off, ci, co, k))
                off = cl[-1].end
            assert off == fc0
            self.conv_layers = nn.ModuleList(cl)                  # q_net.py:87-98, built first
            for conv in self.conv_layers:
                conv.reset_parameters(generator)
        b1 = fc0 + S * h1 * D
        self.__dict__['w1'] = flat[fc0:b1].view(S * h1, D)
        self.__dict__['b1'] = flat[b1:b1 + S * h1]
        off = b1 + S * h1
        streams = []
        for s, out in enumerate((A, 1)[:S]):
            layers = [_LinearAt(flat, fc0 + s * h1 * D, b1 + s * h1, D, h1)]
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
        c = FFQfunc(D, A, hs, self.dueling, self.device, convs=self.convs,
                    input_shape=self.input_shape, is_uint8=self.is_uint8)
        c.copy_from(self)
        return c

    def forward(self, x):
        """q values [rows][A] (q_net.py:41-65,112-119) of a float32 device matrix
        (with convs: of a uint8 or float32 (rows, C, H, W) device tensor)"""
        x = x.contiguous() if self.convs else (x if x.stride(-1) == 1 else x.contiguous())
        adv, val = _QNet(self, {}).fwd(x, x.shape[0], 'f')
        if not self.dueling:
            return adv.clone()
        return (adv - adv.mean(dim=1, keepdim=True)) + val


class _QNet(LaunchNet):
    """Launch helpers over an FFQfunc's flat buffer."""

    def __init__(self, model, bufs):
        super().__init__(model.device, bufs)
        self.m = model

    def conv_fwd(self, x, rows, pre):
        """the conv stem on (rows, C, H, W) uint8 or float32 frames, read in
        place; layer i's ReLU output stays in pre_c{i} and the last one, seen
        as [rows][F], is the feature matrix (U.flatten_conv)"""
        m = self.m
        if (x.dim() != 4 or x.shape[0] < rows or tuple(x.shape[1:]) != m.input_shape
                or x.dtype not in (torch.uint8, torch.float32) or not x.is_contiguous()):
            raise ValueError(f'q_func input: expected contiguous uint8 or float32 frames '
                             f'({rows}, {m.input_shape}), got {x.dtype} {tuple(x.shape)}')
        for i, (ci, H, W, co, k, s, pad) in enumerate(m.conv_geoms):
            ho, wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
            y = self.buf(f'{pre}_c{i}', (rows, co, ho, wo))
            conv = m.conv_layers[i]
            L.call('smi_conv2d_forward', p(x), int(x.dtype == torch.uint8),
                   int(i == 0 and m.is_uint8), rows, ci, H, W, p(conv.weight), p(conv.bias), co, k,
                   s, pad, RELU, p(y), self.st)
            x = y
        return x.view(rows, -1)

    def conv_bwd(self, x, rows, pre, dH1, g):
        """from dH1 (both streams' first-layer gradient) through the stem: the
        first FC layer's input gradient masked by the last conv activation, then
        per layer the weight gradient and (except layer 0) the input gradient"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        n = len(m.conv_geoms)
        acts = [x] + [self.bufs[f'{pre}_c{i}'] for i in range(n)]
        need = max(int(L.lib().smi_conv2d_scratch_bytes(rows, *geo)) for geo in m.conv_geoms)
        scratch = self.buf('conv_scratch', ((need + 3) // 4,))
        dy = self.buf(f'{pre}_dc{n - 1}', tuple(acts[n].shape))
        L.call('smi_linear_backward_input', p(dH1), S * hs[0], rows, S * hs[0], p(m.w1), D, D,
               p(acts[n]), D, p(dy), D, self.st)
        for i in range(n - 1, -1, -1):
            ci, H, W, co, k, s, pad = m.conv_geoms[i]
            conv, xi = m.conv_layers[i], acts[i]
            L.call('smi_conv2d_backward_weight', p(dy), p(xi), int(xi.dtype == torch.uint8),
                   int(i == 0 and m.is_uint8), rows, ci, H, W, co, k, s, pad,
                   p(g[m.off(conv.weight):]), p(g[m.off(conv.bias):]), p(scratch), need, self.st)
            if i:
                dx = self.buf(f'{pre}_dc{i - 1}', tuple(xi.shape))
                L.call('smi_conv2d_backward_input', p(dy), rows, ci, H, W, p(conv.weight), co, k, s,
                       pad, p(xi), p(dx), self.st)
                dy = dx

    def fwd(self, x, rows, pre):
        """(ADV [rows][A], VAL [rows][1] | None); the hidden activations stay in
        the buffers pre_h1 ([rows][S h1], both streams) and pre_h{k}_{s}"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        if m.convs:
            x = self.conv_fwd(x, rows, pre)
        self.check_rows(x, rows, D, 'q_func')
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
        frames = x
        if m.convs:
            x = self.bufs[f'{pre}_c{len(m.convs) - 1}'].view(rows, -1)
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
                L.call('smi_linear_backward_weight', p(dy), ldg, rows, n_out, p(xk), ldx, hs[k - 1],
                       p(g[m.off(lin.weight):]), hs[k - 1], p(g[m.off(lin.bias):]), 0, st)
                L.call('smi_linear_backward_input', p(dy), ldg, rows, n_out, p(lin.weight),
                       hs[k - 1], hs[k - 1], p(xk), ldx, p(dx), lddx, st)
                dy, ldg = dx, lddx
        # both streams' first layers: one weight-gradient GEMM over dH1 [rows][S h1]
        L.call('smi_linear_backward_weight', p(dH1), S * hs[0], rows, S * hs[0], p(x), x.stride(0),
               D, p(g[m.off(m.w1):]), D, p(g[m.off(m.b1):]), 0, st)
        if m.convs:
            self.conv_bwd(frames, rows, pre, dH1, g)


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


class DQNLearner(DeviceLearner):
    """dqn.py:9-126 on MI355X (low-dimensional observations, or uint8 frames
    with model.convs; discrete actions).  A batch with a 'weights' entry (float32 [B] or [B, 1],
    replay.PrioritizedReplay.sample_batch) weights the Huber loss; after every
    learn() `td_error` is a device view [B] of Q(s, a) - y
    (PrioritizedReplay.update_priorities_from_td).  With dp, `td_error` is
    [B_global]: the TD errors of the WHOLE draw, in draw order, on every rank
    (replay.sample_shard's idx_all names their slots)."""

    def __init__(self, learner_config, env_config, session_config=None, metrics=None,
                 device=None, seed=0, use_graph=False, checkpoint=None,
                 checkpoint_full_state=False, *, dp=None):
        """dp (keyword only): None (one GPU) or a data-parallel group exposing
        `world_size`, `rank` and `allreduce_(tensor)` (in-place SUM, stream-ordered), e.g.
        learner.TorchDistAllReduce().  Each rank passes its own
        replay.batch_size = B_global / world rows of one global draw
        (sample_shard); initial weights are broadcast from rank 0.  A group of
        world 1 is dp=None.  use_graph with world > 1 runs eagerly (the
        collective is not captured)."""
        lc, ec = as_config(learner_config), as_config(env_config)
        D, A, hidden, dueling, conv_kw = dqn_model_kwargs(lc, ec)      # host checks come first
        self.algo = algo = lc.algo
        self.target_update_tracker = TargetUpdateTracker(algo.target_network_update_freq)
        self._init_device(lc, ec, session_config, metrics, checkpoint, device, checkpoint_full_state)
        self.action_dim, self.obs_dim = A, D
        self.double_q = bool(algo.double_q)
        clip = algo.get('grad_norm_clipping')
        self.max_norm = float(clip) if clip else 0.0          # None or 0: no clip (dqn.py:33-35)
        gen = torch.Generator().manual_seed(seed)
        self.q_func = FFQfunc(D, A, hidden, dueling, self.device, gen, **conv_kw)
        self.pixel = bool(conv_kw)
        self.q_target = self.q_func.clone()                   # dqn.py:17
        self.dp = self._dp_group(dp, [self.q_func.flat, self.q_target.flat])
        self.opt = self.adam_state(self.q_func.flat, algo.lr)
        self.stats_buf = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.td_error = None
        self._xbuf = None             # the exchange image (dp only), sized by the first batch
        self.use_graph = bool(use_graph) and self.dp is None

    # ------------------------------------------------------------ helpers
    def _update_target(self):                                            # dqn.py:27-28
        self.q_target.copy_from(self.q_func)

    def _obs_of(self, v):
        """the one input of FFQfunc inside an obs dict: the camera of a pixel
        model ({'pixel': {'camera0': uint8 (B, C, H, W)}}), low_dim.flat_inputs
        otherwise; anything else is returned as given"""
        if not isinstance(v, dict):
            return v
        if self.pixel:
            return list(v['pixel'].values())[0]
        return v['low_dim']['flat_inputs']

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
            v = self._obs_of(batch[k])
            if self.pixel:
                v = torch.as_tensor(v)
                if v.dtype != torch.uint8 or v.dim() != 4:
                    raise ValueError(f'{k}: pixel observations are uint8 (B, C, H, W), got '
                                     f'{v.dtype} {tuple(v.shape)}')
                out[k] = v.contiguous().to(self.device, non_blocking=True)
            else:
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
        self._gradient(obs, actions, rewards, obs_next, dones, weights)
        self._apply()

    def _apply(self):
        self.adam_step(self.opt, self.q_func.flat, 1e-4, self.max_norm, 0.0, L.stream(self.device))

    def _gradient(self, obs, actions, rewards, obs_next, dones, weights=None):
        """everything of _optimize before the Adam step: the gradient image, the
        TD errors and the statistics of this learner's rows (with dp: its shard's
        part of the exchange image)"""
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
        if self.dp is None:
            self.td_error = net.buf('td', (B,))
            L.call('smi_dqn_td', p(adv), A, p(adv_n), A, p(adv_t), A, p(val), 1, p(val_n), 1,
                   p(val_t), 1, p(act), a_s, p(rew), r_s, p(don), d_s, p(weights), B, A,
                   float(self.algo.gamma), int(dueling), int(self.double_q), p(dadv), A, p(dval),
                   p(self.td_error), None, p(self.stats_buf), st)
        else:
            world = self.dp.world_size
            if self._xbuf is None or self.td_error.numel() != B * world:
                # what the one all-reduce per learn() carries: [gradient | pad |
                # td_all (B_global) | stats (2)], the three as views of it
                self._xbuf, self.opt['g'], (self.td_error, self.stats_buf) = exchange_image(
                    self.device, self.q_func.flat.numel(), (B * world, 2))
            L.call('smi_dqn_td_shard', p(adv), A, p(adv_n), A, p(adv_t), A, p(val), 1, p(val_n), 1,
                   p(val_t), 1, p(act), a_s, p(rew), r_s, p(don), d_s, p(weights), B, B * world,
                   self.dp.rank * B, A, float(self.algo.gamma), int(dueling), int(self.double_q),
                   p(dadv), A, p(dval), p(self.td_error), None, p(self.stats_buf), st)
        with L.dw_group(st):
            net.bwd(obs, B, 'q', [dadv, dval] if dueling else [dadv], self.opt['g'])

    # ------------------------------------------------------- reference API
    def _update_phases(self, batch):
        """the data-parallel update: the exchange image is all-reduced once,
        after the backward and before smi_adam_clip"""
        ins = self._inputs(batch)
        self._gradient(*ins, weights=batch.get('weights'))
        yield self._xbuf
        self._ctx.make_current()      # whatever ran on this thread meanwhile
        self._apply()
        # samples of the GLOBAL batch: every rank copies the target on the
        # step the single learner would
        if self.target_update_tracker.track_increment(
                int(ins[0].shape[0]) * self.dp.world_size):
            self._update_target()

    def _inputs(self, batch):
        """(obs, actions, rewards, obs_next, dones) of a device batch"""
        obs, obs_next = self._obs_of(batch['obs']), self._obs_of(batch['obs_next'])
        actions = batch['actions']
        if actions.dtype != torch.float32:
            actions = actions.to(torch.float32)
        return (obs, actions, batch['rewards'], obs_next, batch['dones'])

    def _learn_device(self, batch):                                      # dqn.py:75-92
        ins = self._inputs(batch)
        weights = batch.get('weights')
        if self.use_graph:      # the weights are one more static input (uint8 frames stay uint8)
            self._graph_step(ins if weights is None else ins + (weights,), self._optimize)
        else:
            self._optimize(*ins, weights=weights)
        # the target copy stays on the host, where its counter lives
        if self.target_update_tracker.track_increment(int(ins[0].shape[0])):
            self._update_target()

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
