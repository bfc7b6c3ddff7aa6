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

Categorical heads (algo.distributional.enabled; C51, Bellemare et al. 2017;
this build's own specification, dqn_dist_kernels.hip): the last layer of the
action stream has A N outputs, action major (column a N + i is atom i of
action a), the last layer of the state stream N; state_dict names are
unchanged, only these two shapes grow.  forward() returns the expected values
sum_i z_i softmax(l[a, .])_i over the support z_i = v_min + i (v_max - v_min) /
(N - 1) (smi_dqn_c51_q), logits() the raw streams.  learn() runs the same three
forwards, then smi_dqn_c51_td (smi_dqn_c51_td_shard under dp, inside the same
exchange image) in place of smi_dqn_td and the same backward: the loss is the
cross-entropy of the projected target distribution against the online net's
log-softmax at the action taken, and `td_error` holds each row's loss (>= 0):
the priority signal update_priorities_from_td reads.

Quantile heads (algo.distributional.kind = 'quantile'; QR-DQN, Dabney et al.
2018; this build's own specification, dqn_quant_kernels.hip): the same head
layout with `atoms` quantile values per action (1 to 256, A atoms <= 4096) and
no support, so v_min / v_max are not read.  forward() returns the mean
quantiles (smi_dqn_qr_q), the agents act on their arg-max, and learn() runs
smi_dqn_qr_td (smi_dqn_qr_td_shard under dp) in the same place: the loss of a
row is the quantile-Huber loss (threshold algo.distributional.kappa; 0 is the
pinball loss) summed over the online quantiles of the action taken and
averaged over the target quantiles r + gamma (1 - d) theta_target(s')[a*, .],
and `td_error` holds it (>= 0).  dp, the exchange image, graph replay and
checkpoints are the categorical head's: nothing in them knows the head.

Implicit quantile heads (algo.distributional.kind = 'implicit'; IQN, Dabney et
al. 2018b; this build's own specification, dqn_iqn_kernels.hip): the net takes
a quantile fraction tau per sample, so heads stay scalar (A and 1 outputs) and
one new pair fc_tau_layer.{weight [d][embed_dim], bias [d]}, d = S h1, sits at
the END of the flat buffer and of the state_dict (every other offset is the
scalar model's).  A forward is: the first layer (after the conv stem, if any)
to H1 [B][d]; smi_iqn_embed_forward, Z [B N][d] = H1[b] (.) relu(bias + cos(pi
i tau) W^T) for the N fractions of each row; the deeper layers on the B N
sample rows, so adv is [B N][A] and val [B N][1] (sample major).  learn()
draws three sets of fractions (smi_iqn_taus, streams 0 online / 1 selecting /
2 target, counter = the device Adam step, so a graph replay draws new ones and
a dp rank draws the global draw's fractions of its rows), runs the three
forwards (atoms online samples, target_atoms for the other two), smi_iqn_td
(smi_iqn_td_shard under dp), the usual backward on the B N rows down to dZ
(the layer above masks by Z > 0, which leaves every gradient unchanged),
smi_iqn_embed_backward (dH1 and fc_tau_layer's gradients, written at their
offsets of the gradient image), the first layer's weight gradient (and the
conv backward) from dH1, and the one smi_adam_clip.  The fractions used stay
readable as learner.tau / tau_next / tau_target.  forward() and the agents
draw act_atoms fractions per row from a counter of their own and take the
mean over them (smi_iqn_q).  v_min / v_max are not read.

Noisy linear layers (model.noisy.enabled; NoisyNet, factorised Gaussian noise,
noisy_kernels.hip): every FC layer computes with W_mu + W_sig (.) (f_out f_in^T)
and b_mu + b_sig (.) f_out without writing either; the sigma parameters are a
second image of the FC range appended at the very end of the flat buffer
(ffq_sigma_shift) and of the state_dict (ffq_sigma_names), so the target copy,
the exchange image, Adam with its norm clip and the checkpoints cover them as
part of the one buffer.  learn() draws three noise images per step from the
device Adam step (smi_noisy_draw; streams 0 online at s, 1 online at s' with
double-Q, 2 target; learner.noise, noise_next, noise_target; key = the seed XOR
NOISE_KEY, apart from the implicit heads' fractions), the same on every
data-parallel rank, and after the grouped mu weight gradients one
smi_noisy_sigma_grad fills the sigma range of the gradient image.

bf16 convolutions (model.conv_dtype = 'bf16', default 'fp32'; pixel models
only, anything else is a ConfigError; conv_bf16_kernels.hip): every conv
launch above becomes its smi_conv2d_*_bf16 twin, same arguments and one launch
each, with a scratch size of its own.  The frames (exactly), the weights, the
float activations a layer reads and the gradients arriving at a layer's output
are rounded to bf16 (nearest even) while the kernels stage them for
v_mfma_f32_16x16x32_bf16; sums, bias, / 255, ReLU, masks and db are fp32.
Parameters, activations, gradients, Adam, the target copy, checkpoints, the
exchange image and the publisher stay fp32: nothing outside the conv launches
knows the option, so graph replay and dp are the fp32 model's.  The noisy
layers and fc_tau_layer are untouched; the FC layers and the heads have a
switch of their own:

bf16 dense layers (model.fc_dtype = 'bf16', default 'fp32'; with
model.noisy.enabled a ConfigError: the noisy layers have kernels of their own;
linear_bf16_kernels.hip): every smi_linear_forward and smi_linear_backward_input
of the FC stack above (the first layer after the observation or the stem, the
deeper layers of both streams and the heads of every head kind, for implicit
heads on the B N sample rows too) becomes its _bf16 twin, same arguments and
one launch each.  The activations, the weights and the gradients arriving at a
layer's output are rounded to bf16 (nearest even) while the kernels stage them
for v_mfma_f32_16x16x32_bf16; sums, bias, ReLU and masks are fp32.  Every
weight gradient stays on the grouped fp32 launch and reads the unrounded
activations and output gradients; the IQN embedding kernels, fc_tau_layer, the
convolutions (conv_dtype), the TD kernels, Adam, the target copy, checkpoints,
the exchange image and the publisher are untouched: nothing outside the two
launch sites (_QNet.lin, _QNet.ndx) knows the option.

model.fc_dtype = 'bf16_all' is 'bf16' plus the weight gradients: every
smi_linear_backward_weight of _QNet.bwd (the per-layer calls of both streams
and the joint first-layer GEMM over dH1) becomes smi_linear_backward_weight_bf16,
which rounds dy and x while staging them, sums db in fp32 from the unrounded
dy, and launches where it stands instead of queueing into the grouped launch
(the group's flush then has nothing to run for them).  The forward and the
input gradients are those of 'bf16', bit for bit; fc_tau_layer's gradient stays
in smi_iqn_embed_backward.  The small 512-row layers lose the grouped launch
under this value and are not routed back: a model's numerics do not depend on
a dispatch threshold.

bf16 noisy layers (model.noisy.dtype = 'bf16', an optional key of the noisy
table read only when it is enabled; absent or 'fp32': the fp32 kernels;
noisy_bf16_kernels.hip): every smi_noisy_forward and smi_noisy_backward_input
(every launch of _QNet.nlin / _QNet.ndx that takes a noise image) becomes its
_bf16 twin, same arguments and one launch each (a split reduction adds its
reducer).  x, x (.) f_in, dy, dy (.) f_out, W_mu and W_sig are rounded to bf16
(nearest even) while the kernel stages them, the product with the noise being
one fp32 multiply of the unrounded value rounded once; sums, biases, f_out /
f_in in the epilogue, ReLU and masks are fp32.  'bf16_all' also puts the mu
weight gradients of _QNet.bwd (plain dy^T x) on smi_linear_backward_weight_bf16,
launched where they stand as under fc_dtype 'bf16_all'; smi_noisy_sigma_grad
runs after them, unchanged.  Without a noise image (eval agents, forward() in
eval mode) the plain fp32 layers run on the mu parameters as before.  The
value is kept as q_func.noisy_dtype and carried by clone(); nothing outside
those launch sites knows it: QAgentBatch, data parallelism, graph replay,
checkpoints and the publisher are the fp32 noisy model's.  model.fc_dtype
other than 'fp32' with noisy layers stays a ConfigError.
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
# model.conv_dtype -> suffix of the smi_conv2d_* symbols the conv layers run on
CONV_DTYPES = {'fp32': '', 'bf16': '_bf16'}
# model.fc_dtype -> suffixes of the FC stack's smi_linear_forward, smi_linear_backward_input
# and smi_linear_backward_weight
FC_DTYPES = {'fp32': ('', '', ''), 'bf16': ('_bf16', '_bf16', ''),
             'bf16_all': ('_bf16', '_bf16', '_bf16')}
# model.noisy.dtype -> suffixes of smi_noisy_forward / smi_noisy_backward_input and of the mu
# weight gradients' smi_linear_backward_weight, of the launches that take a noise image
NOISY_DTYPES = {'fp32': ('', ''), 'bf16': ('_bf16', ''), 'bf16_all': ('_bf16', '_bf16')}


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


C51_MAX_ATOMS = 64        # one lane per atom (dqn_dist_kernels.hip: kC51MaxAtoms)
C51_MAX_SLAB = 3072       # A * atoms: the LDS slabs of a workgroup (kC51LdsBytes)


def check_atoms(A, atoms, v_min, v_max):
    """the ranges smi_dqn_c51_* serve, as (atoms, v_min, v_max)"""
    atoms, v_min, v_max = int(atoms), float(v_min), float(v_max)
    if not 2 <= atoms <= C51_MAX_ATOMS:
        raise ConfigError('DQN algo.distributional.atoms must be in [2, {}], got {}'.format(
            C51_MAX_ATOMS, atoms))
    if not v_max > v_min:
        raise ConfigError('DQN algo.distributional needs v_max > v_min, got [{}, {}]'.format(
            v_min, v_max))
    if A * atoms > C51_MAX_SLAB:
        raise ConfigError('DQN algo.distributional: {} actions x {} atoms is over the kernel\'s '
                          '{} logits per row'.format(A, atoms, C51_MAX_SLAB))
    return atoms, v_min, v_max


QR_MAX_QUANTILES = 256    # one thread of a workgroup per quantile (dqn_quant_kernels.hip: kQrMaxN)
QR_MAX_SLAB = 4096        # A * quantiles (kQrMaxSlab)


def check_quantiles(A, quantiles, kappa, kind='quantile'):
    """the ranges smi_dqn_qr_* serve, as (quantiles, kappa)"""
    if kind != 'quantile':
        raise ConfigError("DQN algo.distributional.kind must be 'categorical' or 'quantile', got "
                          '{!r}'.format(kind))
    quantiles, kappa = int(quantiles), float(kappa)
    if not 1 <= quantiles <= QR_MAX_QUANTILES:
        raise ConfigError('DQN algo.distributional.atoms (the quantile count) must be in [1, {}], '
                          'got {}'.format(QR_MAX_QUANTILES, quantiles))
    if A * quantiles > QR_MAX_SLAB:
        raise ConfigError('DQN algo.distributional: {} actions x {} quantiles is over the '
                          'kernel\'s {} values per row'.format(A, quantiles, QR_MAX_SLAB))
    if not kappa >= 0.0:
        raise ConfigError('DQN algo.distributional.kappa must be >= 0, got {}'.format(kappa))
    return quantiles, kappa


IQN_MAX_SAMPLES = 64      # one lane per sample (dqn_iqn_kernels.hip: kIqnMaxN)
IQN_MAX_SLAB = 4096       # A * samples (kIqnMaxSlab)
IQN_MAX_COS = 64          # cosines of the embedding (kIqnMaxCos)


def check_implicit(A, atoms=8, target_atoms=None, act_atoms=32, embed_dim=64, kappa=1.0):
    """the ranges smi_iqn_* serve, as the dict FFQfunc(implicit=...) takes"""
    out = {'atoms': int(atoms), 'target_atoms': int(atoms if target_atoms is None else target_atoms),
           'act_atoms': int(act_atoms), 'embed_dim': int(embed_dim), 'kappa': float(kappa)}
    for k in ('atoms', 'target_atoms', 'act_atoms'):
        if not 1 <= out[k] <= IQN_MAX_SAMPLES:
            raise ConfigError('DQN algo.distributional.{} must be in [1, {}], got {}'.format(
                k, IQN_MAX_SAMPLES, out[k]))
    if not 4 <= out['embed_dim'] <= IQN_MAX_COS or out['embed_dim'] % 4:
        raise ConfigError('DQN algo.distributional.embed_dim must be a multiple of 4 in [4, {}], '
                          'got {}'.format(IQN_MAX_COS, out['embed_dim']))
    most = max(out['atoms'], out['target_atoms'], out['act_atoms'])
    if A * most > IQN_MAX_SLAB:
        raise ConfigError('DQN algo.distributional: {} actions x {} samples is over the kernel\'s '
                          '{} values per row'.format(A, most, IQN_MAX_SLAB))
    if not out['kappa'] >= 0.0:
        raise ConfigError('DQN algo.distributional.kappa must be >= 0, got {}'.format(out['kappa']))
    return out


NOISE_KEY = 0x6E6F697379          # XORed into a seed for the noise draws ('noisy')


def check_noisy(sigma0):
    """model.noisy.sigma0 as a float: positive and finite"""
    try:
        sigma0 = float(sigma0)
    except (TypeError, ValueError):
        raise ConfigError('DQN model.noisy.sigma0 must be a number, got {!r}'.format(sigma0))
    if not (sigma0 > 0.0 and np.isfinite(sigma0)):
        raise ConfigError('DQN model.noisy.sigma0 must be positive and finite, got {}'.format(sigma0))
    return sigma0


def ffq_sigma_names(n_hidden, dueling):
    """what a noisy model appends to the state_dict, after every other name: the
    FC layers' sigma entries in the layer order of ffq_param_names"""
    return [f'{stream}.{i}.{p}_sigma' for stream in ('fc_action_layers', 'fc_state_layers')[:2 if dueling else 1]
            for i in range(n_hidden + 1) for p in ('weight', 'bias')]


def ffq_sigma_shift(fc0, n, n_tau):
    """a noisy model's flat buffer is [convs (fc0) | FC range [fc0, n) | fc_tau_layer
    (n_tau) | the FC range's sigma image]: the FC parameter at offset o has its
    sigma at o + this shift.  Host only."""
    return n + n_tau - fc0


def ffq_noisy_layers(D, hidden, dueling, out_widths):
    """the noisy layers of a net in noise-image order, [(in, out)]: the stacked
    first layer, then per stream its deeper layers; out_widths: the streams'
    output widths.  Host only."""
    S = 2 if dueling else 1
    layers = [(D, S * hidden[0])]
    for s in range(S):
        layers += [(hidden[k - 1], hidden[k]) for k in range(1, len(hidden))]
        layers.append((hidden[-1], out_widths[s]))
    return layers


def dqn_model_kwargs(learner_config, env_config):
    """(D, A, hidden, dueling, FFQfunc keyword arguments): dqn_conv_specs for a
    spec with pixels, dqn_specs otherwise; algo.distributional.enabled adds
    atoms, v_min and v_max, with kind 'quantile' quantiles and kappa instead,
    with kind 'implicit' the dict of check_implicit; model.noisy.enabled adds
    noisy = sigma0 and, with model.noisy.dtype = 'bf16' or 'bf16_all' (an optional
    key, read only then), noisy_dtype; model.conv_dtype = 'bf16' (pixels only) adds conv_dtype;
    model.fc_dtype = 'bf16' or 'bf16_all' (not with noisy layers) adds fc_dtype.
    Host only."""
    if 'pixel' in env_config['obs_spec']:
        shape, convs, A, hidden, dueling, u8 = dqn_conv_specs(learner_config, env_config)
        D = int(np.prod(conv_chain(shape, convs)[1]))
        kw = {'convs': convs, 'input_shape': shape, 'is_uint8': u8}
    else:
        D, A, hidden, dueling = dqn_specs(learner_config, env_config)
        kw = {}
    conv_dtype = learner_config['model'].get('conv_dtype', 'fp32')
    if conv_dtype not in CONV_DTYPES:
        raise ConfigError("DQN model.conv_dtype must be 'fp32' or 'bf16', got {!r}".format(conv_dtype))
    if conv_dtype != 'fp32':
        if 'convs' not in kw:
            raise ConfigError("DQN model.conv_dtype = 'bf16' needs model.convs: it is the operand "
                              'type of the convolution layers')
        kw['conv_dtype'] = conv_dtype
    dist = learner_config['algo'].get('distributional') or {}
    kind = dist.get('kind', 'categorical')
    if dist.get('enabled', False) and kind == 'implicit':
        kw['implicit'] = check_implicit(A, dist.get('atoms', 8), dist.get('target_atoms'),
                                        dist.get('act_atoms', 32), dist.get('embed_dim', 64),
                                        dist.get('kappa', 1.0))
    elif dist.get('enabled', False) and kind != 'categorical':
        kw['quantiles'], kw['kappa'] = check_quantiles(A, dist.get('atoms', 51),
                                                       dist.get('kappa', 1.0), kind)
    elif dist.get('enabled', False):
        kw['atoms'], kw['v_min'], kw['v_max'] = check_atoms(
            A, dist.get('atoms', 51), dist.get('v_min', -10.0), dist.get('v_max', 10.0))
    noisy = learner_config['model'].get('noisy') or {}
    if noisy.get('enabled', False):
        kw['noisy'] = check_noisy(noisy.get('sigma0', 0.5))
        noisy_dtype = noisy.get('dtype', 'fp32')
        if noisy_dtype not in NOISY_DTYPES:
            raise ConfigError("DQN model.noisy.dtype must be 'fp32', 'bf16' or 'bf16_all', got "
                              '{!r}'.format(noisy_dtype))
        if noisy_dtype != 'fp32':
            kw['noisy_dtype'] = noisy_dtype
    fc_dtype = learner_config['model'].get('fc_dtype', 'fp32')
    if fc_dtype not in FC_DTYPES:
        raise ConfigError("DQN model.fc_dtype must be 'fp32', 'bf16' or 'bf16_all', got "
                          '{!r}'.format(fc_dtype))
    if fc_dtype != 'fp32':
        if 'noisy' in kw:
            raise ConfigError('DQN model.fc_dtype = {!r} does not combine with model.noisy: the '
                              'noisy layers run on kernels of their own'.format(fc_dtype))
        kw['fc_dtype'] = fc_dtype
    return D, A, hidden, dueling, kw


def ffq_param_names(n_convs, n_hidden, dueling):
    """state_dict keys in the reference's construction order (q_net.py:25-39,87-98)"""
    names = [f'conv_layers.{i}.{p}' for i in range(n_convs) for p in ('weight', 'bias')]
    for stream in ('fc_action_layers', 'fc_state_layers')[:2 if dueling else 1]:
        names += [f'{stream}.{i}.{p}' for i in range(n_hidden + 1) for p in ('weight', 'bias')]
    return names            # (an implicit model appends fc_tau_layer.{weight, bias})


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
    uint8 or float32 (rows, C, H, W) device tensor and D_in is ignored.  With
    atoms (categorical heads over the support [v_min, v_max]) the action
    stream ends in A * atoms logits and the state stream in atoms; with
    quantiles (quantile heads with Huber threshold kappa; not together with
    atoms) in A * quantiles values and quantiles.  With implicit (the dict of
    check_implicit; not together with either) the heads stay scalar and
    fc_tau_layer embeds a quantile fraction per sample row (module docstring).
    With noisy (sigma0) every FC layer is a noisy linear layer (noisy_kernels.hip;
    the stacked first layer is one layer of S h1 outputs, fc_tau_layer and the
    convolutions stay plain): the sigma parameters are a second image of the FC
    range at the end of the flat buffer (ffq_sigma_shift), every entry sigma0 /
    sqrt(in_features), and the state_dict ends in ffq_sigma_names.  In train()
    mode forward() / logits() draw one noise image per call from a counter of
    the model's own (noise_step; the last image stays in `noise`); in eval()
    mode they run the mu parameters through the plain layers."""

    def __init__(self, D_in, action_dim, fc_hidden_sizes, dueling, device=None, generator=None,
                 convs=None, input_shape=None, is_uint8=False, atoms=None, v_min=None, v_max=None,
                 quantiles=None, kappa=1.0, implicit=None, noisy=None, conv_dtype='fp32',
                 fc_dtype='fp32', noisy_dtype='fp32'):
        super().__init__()
        if noisy_dtype not in NOISY_DTYPES or (noisy_dtype != 'fp32' and noisy is None):
            raise ConfigError("FFQfunc noisy_dtype is 'fp32' or, with noisy layers, 'bf16' or "
                              "'bf16_all'; got {!r}".format(noisy_dtype))
        self.noisy_dtype = noisy_dtype
        if fc_dtype not in FC_DTYPES or (fc_dtype != 'fp32' and noisy is not None):
            raise ConfigError("FFQfunc fc_dtype is 'fp32' or, without noisy layers, 'bf16' or "
                              "'bf16_all'; got {!r}".format(fc_dtype))
        self.fc_dtype = fc_dtype
        if conv_dtype not in CONV_DTYPES or (conv_dtype != 'fp32' and not convs):
            raise ConfigError("FFQfunc conv_dtype is 'fp32' or, with convs, 'bf16'; got "
                              '{!r}'.format(conv_dtype))
        self.conv_dtype = conv_dtype
        self.noisy = None if noisy is None else check_noisy(noisy)
        self.atoms, self.v_min, self.v_max = None, None, None
        self.quantiles, self.kappa = None, None
        self.implicit = None
        if (atoms is not None) + (quantiles is not None) + (implicit is not None) > 1:
            raise ConfigError('FFQfunc takes atoms (categorical heads), quantiles or implicit, '
                              'not two of them')
        if implicit is not None:
            self.implicit = check_implicit(int(action_dim), **dict(implicit))
            self.kappa = self.implicit['kappa']
        if atoms is not None:
            self.atoms, self.v_min, self.v_max = check_atoms(int(action_dim), atoms, v_min, v_max)
        if quantiles is not None:
            self.quantiles, self.kappa = check_quantiles(int(action_dim), quantiles, kappa)
        N = self.atoms or self.quantiles or 1
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
        n = fc0 + S * h1 * D + S * h1 + deep(A * N) + (deep(N) if dueling else 0)
        n_cos = self.implicit['embed_dim'] if self.implicit else 0
        n_tau = S * h1 * n_cos + S * h1 if self.implicit else 0       # fc_tau_layer, at the end
        n_sig = n - fc0 if self.noisy else 0                          # the sigma image, at the very end
        flat = torch.zeros(n + n_tau + n_sig, dtype=torch.float32, device=self.device)
        self.__dict__['flat'] = flat
        self.sig_shift = ffq_sigma_shift(fc0, n, n_tau)
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
        for s, out in enumerate((A * N, N)[:S]):
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
        if self.implicit:
            self.fc_tau_layer = _LinearView(flat, n, n_cos, S * h1)
            self.fc_tau_layer.reset_parameters(generator)
            # the counter of forward()'s own fraction draws
            self.__dict__['tau_step'] = torch.zeros(1, dtype=torch.int32, device=self.device)
        if self.noisy:
            self.noisy_layers = ffq_noisy_layers(D, hs, self.dueling, (A * N, N))
            with torch.no_grad():
                flat[fc0 + self.sig_shift:b1 + S * h1 + self.sig_shift] = self.noisy / D ** 0.5
                for layers in self.streams():
                    for lin in layers[1:]:
                        for t in self.sigma_of(lin):
                            t.fill_(self.noisy / lin.in_features ** 0.5)
            # the counter of forward()'s own noise draws and the last image drawn
            self.__dict__['noise_step'] = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.__dict__['noise'] = None
            self.noise_seed = 0          # of forward()'s draws; set it per process

    def sigma_of(self, lin):
        """(weight_sigma, bias_sigma) views of an FC layer of a noisy model"""
        w = self.flat[self.off(lin.weight) + self.sig_shift:][:lin.weight.numel()]
        b = self.flat[self.off(lin.bias) + self.sig_shift:][:lin.bias.numel()]
        return w.view(lin.weight.shape), b

    def _sigma_items(self):
        names = ffq_sigma_names(len(self.dims[1]), self.dueling)
        views = [t for layers in self.streams() for lin in layers for t in self.sigma_of(lin)]
        return list(zip(names, views))

    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        if self.noisy:
            keep, prefix = kwargs.get('keep_vars', False), kwargs.get('prefix', '')
            for name, t in self._sigma_items():
                sd[prefix + name] = t if keep else t.detach().clone()
        return sd

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        state_dict = dict(state_dict)
        if self.noisy:
            with torch.no_grad():
                for name, t in self._sigma_items():
                    if name in state_dict:
                        t.copy_(torch.as_tensor(state_dict.pop(name)).to(self.device))
                    elif strict:
                        raise RuntimeError(f'FFQfunc.load_state_dict: missing {name!r}')
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

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
                    input_shape=self.input_shape, is_uint8=self.is_uint8, atoms=self.atoms,
                    v_min=self.v_min, v_max=self.v_max, quantiles=self.quantiles,
                    kappa=self.kappa if self.quantiles else 1.0, implicit=self.implicit,
                    noisy=self.noisy, conv_dtype=self.conv_dtype, fc_dtype=self.fc_dtype,
                    noisy_dtype=self.noisy_dtype)
        c.copy_from(self)
        return c

    def logits(self, x, tau=None):
        """the raw streams (adv [rows][A * atoms] action major, val [rows][atoms]
        | None); for scalar heads (adv [rows][A], val [rows][1] | None); for an
        implicit model at the fractions tau (float32 device [rows * N], row
        major): (adv [rows * N][A], val [rows * N][1] | None)"""
        x = x.contiguous() if self.convs else (x if x.stride(-1) == 1 else x.contiguous())
        net, noise = _QNet(self, {}), None
        if self.noisy and self.training:
            noise = self.__dict__['noise'] = net.draw(self.noise_seed ^ NOISE_KEY, self.noise_step, 0,
                                                      'f_noise')
            self.noise_step.add_(1)
        return net.fwd(x, x.shape[0], 'f', tau, noise=noise)

    def forward(self, x):
        """q values [rows][A] (q_net.py:41-65,112-119) of a float32 device matrix
        (with convs: of a uint8 or float32 (rows, C, H, W) device tensor); with
        atoms the expected values of the categorical heads (smi_dqn_c51_q), with
        quantiles their means (smi_dqn_qr_q), with implicit the means over
        act_atoms sampled fractions (smi_iqn_q)"""
        if self.implicit:      # the mean over act_atoms fractions per row, drawn here
            net, rows = _QNet(self, {}), x.shape[0]
            tau = net.taus(0, self.tau_step, 0, 0, rows, self.implicit['act_atoms'], 'f_tau')
            self.tau_step.add_(1)
            adv, val = self.logits(x, tau)
            return net.expected_q(adv, val, rows, 'f')
        adv, val = self.logits(x)
        if self.atoms or self.quantiles:
            return _QNet(self, {}).expected_q(adv, val, adv.shape[0], 'f')
        if not self.dueling:
            return adv.clone()
        return (adv - adv.mean(dim=1, keepdim=True)) + val


class _QNet(LaunchNet):
    """Launch helpers over an FFQfunc's flat buffer."""

    def __init__(self, model, bufs):
        super().__init__(model.device, bufs)
        self.m = model

    def lin(self, x, ldx, rows, k, w, ldw, b, n, act, y, ldy):
        """a dense layer's forward on the model's fc_dtype"""
        L.call('smi_linear_forward' + FC_DTYPES[self.m.fc_dtype][0], p(x), ldx, rows, k, p(w), ldw, p(b),
               n, act, p(y), ldy, self.st)

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
            L.call('smi_conv2d_forward' + CONV_DTYPES[m.conv_dtype], p(x), int(x.dtype == torch.uint8),
                   int(i == 0 and m.is_uint8), rows, ci, H, W, p(conv.weight), p(conv.bias), co, k,
                   s, pad, RELU, p(y), self.st)
            x = y
        return x.view(rows, -1)

    def conv_bwd(self, x, rows, pre, dH1, g, noise=None):
        """from dH1 (both streams' first-layer gradient) through the stem: the
        first FC layer's input gradient masked by the last conv activation, then
        per layer the weight gradient and (except layer 0) the input gradient"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        n = len(m.conv_geoms)
        acts = [x] + [self.bufs[f'{pre}_c{i}'] for i in range(n)]
        sfx = CONV_DTYPES[m.conv_dtype]
        scratch_bytes = getattr(L.lib(), 'smi_conv2d_scratch_bytes' + sfx)
        need = max(int(scratch_bytes(rows, *geo)) for geo in m.conv_geoms)
        scratch = self.buf('conv_scratch', ((need + 3) // 4,))
        dy = self.buf(f'{pre}_dc{n - 1}', tuple(acts[n].shape))
        self.ndx(noise, 0, dH1, S * hs[0], rows, S * hs[0], m.w1, D, D, acts[n], D, dy, D)
        for i in range(n - 1, -1, -1):
            ci, H, W, co, k, s, pad = m.conv_geoms[i]
            conv, xi = m.conv_layers[i], acts[i]
            L.call('smi_conv2d_backward_weight' + sfx, p(dy), p(xi), int(xi.dtype == torch.uint8),
                   int(i == 0 and m.is_uint8), rows, ci, H, W, co, k, s, pad,
                   p(g[m.off(conv.weight):]), p(g[m.off(conv.bias):]), p(scratch), need, self.st)
            if i:
                dx = self.buf(f'{pre}_dc{i - 1}', tuple(xi.shape))
                L.call('smi_conv2d_backward_input' + sfx, p(dy), rows, ci, H, W, p(conv.weight), co, k, s,
                       pad, p(xi), p(dx), self.st)
                dy = dx

    def expected_q(self, adv, val, rows, pre, greedy=None):
        """Q [rows][A] of a categorical or quantile model's head outputs (fwd's);
        greedy (int32 [rows], optional) receives each row's first arg-max"""
        m = self.m
        A = m.dims[2]
        q = self.buf(pre + '_q', (rows, A))
        if m.implicit:
            L.call('smi_iqn_q', p(adv), adv.stride(0), p(val), rows, A, adv.shape[0] // rows,
                   int(m.dueling), p(q), A, p(greedy), self.st)
            return q
        if m.quantiles:
            L.call('smi_dqn_qr_q', p(adv), adv.stride(0), p(val), m.quantiles, rows, A, m.quantiles,
                   int(m.dueling), p(q), A, p(greedy), self.st)
            return q
        L.call('smi_dqn_c51_q', p(adv), adv.stride(0), p(val), m.atoms, rows, A, m.atoms, m.v_min,
               m.v_max, int(m.dueling), p(q), A, p(greedy), self.st)
        return q

    def draw(self, seed, step, stream_id, name):
        """the noise image of a noisy model's layers (smi_noisy_draw): per layer
        [f_in | f_out]; the same on every data-parallel rank"""
        nl, dims = L.noisy_dims(self.m.noisy_layers)
        f = self.buf(name, (sum(k + n for k, n in self.m.noisy_layers),))
        L.call('smi_noisy_draw', int(seed), p(step), stream_id, nl, dims, p(f), None, self.st)
        return f

    def _f(self, noise, li):
        """(f_in, f_out) of noisy layer li in a noise image"""
        lay = self.m.noisy_layers
        o = sum(k + n for k, n in lay[:li])
        return noise[o:], noise[o + lay[li][0]:]

    def nlin(self, noise, li, x, ldx, rows, k, w, ldw, b, n, act, y, ldy):
        """layer li's forward: LaunchNet.lin on the mu parameters without a
        noise image, smi_noisy_forward (on the model's noisy_dtype) with one"""
        if noise is None:
            return self.lin(x, ldx, rows, k, w, ldw, b, n, act, y, ldy)
        sh = self.m.sig_shift
        fi, fo = self._f(noise, li)
        L.call('smi_noisy_forward' + NOISY_DTYPES[self.m.noisy_dtype][0], p(x), ldx, rows, k, p(w),
               p(self.m.flat[self.m.off(w) + sh:]),
               ldw, p(b), p(self.m.flat[self.m.off(b) + sh:]), p(fi), p(fo), n, act, p(y), ldy,
               self.st)

    def ndx(self, noise, li, dy, ldg, rows, n_out, w, ldw, k, mask, ldm, dx, lddx):
        """layer li's input gradient, plain (on the model's fc_dtype) or noisy as nlin"""
        if noise is None:
            return L.call('smi_linear_backward_input' + FC_DTYPES[self.m.fc_dtype][1], p(dy), ldg,
                          rows, n_out, p(w), ldw, k, p(mask), ldm, p(dx), lddx, self.st)
        fi, fo = self._f(noise, li)
        L.call('smi_noisy_backward_input' + NOISY_DTYPES[self.m.noisy_dtype][0], p(dy), ldg, rows,
               n_out, p(w),
               p(self.m.flat[self.m.off(w) + self.m.sig_shift:]), ldw, k, p(fi), p(fo), p(mask), ldm,
               p(dx), lddx, self.st)

    def sigma_grad(self, g, noise):
        """the sigma ranges of the gradient image g from its mu ranges, one launch
        (after the weight-gradient group's flush)"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        tab = [(m.off(m.w1), m.off(m.b1), D, S * hs[0])]
        for layers in m.streams():
            tab += [(m.off(lin.weight), m.off(lin.bias), lin.in_features, lin.out_features)
                    for lin in layers[1:]]
        nl, t = L.noisy_table(tab)
        L.call('smi_noisy_sigma_grad', p(g), p(g[m.sig_shift:]), p(noise), nl, t, self.st)

    def taus(self, seed, step, stream_id, row0, rows, N, name):
        """rows * N quantile fractions of an implicit model (smi_iqn_taus)"""
        tau = self.buf(name, (rows * N,))
        L.call('smi_iqn_taus', int(seed), p(step), stream_id, row0, rows, N, p(tau), self.st)
        return tau

    def fwd(self, x, rows, pre, tau=None, keep_phi=False, noise=None):
        """(ADV [rows][A], VAL [rows][1] | None), with atoms (ADV [rows][A * atoms],
        VAL [rows][atoms] | None); the hidden activations stay in
        the buffers pre_h1 ([rows][S h1], both streams) and pre_h{k}_{s}.  An
        implicit model takes tau [rows * N]: H1 is embedded into pre_z [rows *
        N][S h1] (phi into pre_phi with keep_phi, for bwd) and every later
        layer, ADV and VAL have rows * N sample rows.  noise: a noisy model's
        noise image (draw); None runs the mu parameters through the plain layers"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        if m.convs:
            x = self.conv_fwd(x, rows, pre)
        self.check_rows(x, rows, D, 'q_func')
        H1 = self.buf(pre + '_h1', (rows, S * hs[0]))
        self.nlin(noise, 0, x, x.stride(0), rows, D, m.w1, D, m.b1, S * hs[0], RELU, H1, S * hs[0])
        if m.implicit:
            if (tau is None or tau.dtype != torch.float32 or tau.dim() != 1 or not tau.is_contiguous()
                    or tau.numel() % rows or not 1 <= tau.numel() // rows <= IQN_MAX_SAMPLES):
                raise ValueError(f'q_func: an implicit model takes float32 fractions [{rows} * N], '
                                 f'1 <= N <= {IQN_MAX_SAMPLES}')
            N, d, tl = tau.numel() // rows, S * hs[0], m.fc_tau_layer
            Z = self.buf(pre + '_z', (rows * N, d))
            phi = self.buf(pre + '_phi', (rows * N, d)) if keep_phi else None
            L.call('smi_iqn_embed_forward', p(tau), p(H1), d, rows, N, p(tl.weight), p(tl.bias),
                   m.implicit['embed_dim'], d, p(Z), d, p(phi), d, self.st)
            self.bufs[pre + '_tau'] = tau
            H1, rows = Z, rows * N
        outs = []
        for s, layers in enumerate(m.streams()):
            prev, ld = H1[:, s * hs[0]:], S * hs[0]
            for k in range(1, len(hs)):
                H = self.buf(f'{pre}_h{k + 1}_{s}', (rows, hs[k]))
                lin = layers[k]
                self.nlin(noise, s * len(hs) + k, prev, ld, rows, hs[k - 1], lin.weight, hs[k - 1],
                          lin.bias, hs[k], RELU, H, hs[k])
                prev, ld = H, hs[k]
            lin = layers[-1]
            n_out = lin.out_features
            out = self.buf(f'{pre}_out_{s}', (rows, n_out))
            self.nlin(noise, (s + 1) * len(hs), prev, ld, rows, hs[-1], lin.weight, hs[-1], lin.bias,
                      n_out, NONE, out, n_out)
            outs.append(out)
        return outs[0], (outs[1] if m.dueling else None)

    def bwd(self, x, rows, pre, douts, g, noise=None):
        """from douts[s] = d loss / d (stream s's output) into the gradient image
        g (the flat layout); the weight-gradient calls queue into the caller's
        open group, so every dY / X buffer is written once and left alone (with
        fc_dtype 'bf16_all', or noisy_dtype 'bf16_all' and a noise image, they
        launch where they stand, on the _bf16 twin)"""
        m = self.m
        D, hs, A = m.dims
        S = 2 if m.dueling else 1
        st = self.st
        dw_call = 'smi_linear_backward_weight' + (
            FC_DTYPES[m.fc_dtype][2] if noise is None else NOISY_DTYPES[m.noisy_dtype][1])
        frames = x
        if m.convs:
            x = self.bufs[f'{pre}_c{len(m.convs) - 1}'].view(rows, -1)
        H1 = self.bufs[pre + '_h1']
        dH1 = self.buf(pre + '_dh1', (rows, S * hs[0]))
        B, hid, dhid = rows, H1, dH1
        if m.implicit:           # the streams run on the sample rows, from Z down to dZ
            H1 = self.bufs[pre + '_z']
            rows = H1.shape[0]
            dH1 = self.buf(pre + '_dz', (rows, S * hs[0]))
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
                L.call(dw_call, p(dy), ldg, rows, n_out, p(xk), ldx, hs[k - 1],
                       p(g[m.off(lin.weight):]), hs[k - 1], p(g[m.off(lin.bias):]), 0, st)
                self.ndx(noise, s * len(hs) + k, dy, ldg, rows, n_out, lin.weight, hs[k - 1],
                         hs[k - 1], xk, ldx, dx, lddx)
                dy, ldg = dx, lddx
        if m.implicit:
            tau, phi, tl, d = self.bufs[pre + '_tau'], self.bufs[pre + '_phi'], m.fc_tau_layer, S * hs[0]
            n_cos, N = m.implicit['embed_dim'], rows // B
            need = int(L.lib().smi_iqn_embed_scratch_bytes(B, N, n_cos, d))
            scratch = self.buf('iqn_scratch', (max(need // 4, 1),))
            L.call('smi_iqn_embed_backward', p(dH1), d, p(tau), p(hid), d, p(phi), d, B, N,
                   p(g[m.off(tl.weight):]), p(g[m.off(tl.bias):]), n_cos, d, p(dhid), d, p(scratch),
                   need, st)
            rows, dH1 = B, dhid
        # both streams' first layers: one weight-gradient GEMM over dH1 [rows][S h1]
        L.call(dw_call, p(dH1), S * hs[0], rows, S * hs[0], p(x), x.stride(0),
               D, p(g[m.off(m.w1):]), D, p(g[m.off(m.b1):]), 0, st)
        if m.convs:
            self.conv_bwd(frames, rows, pre, dH1, g, noise)


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
    learn() `td_error` is a device view [B] of Q(s, a) - y, with categorical
    heads of each row's cross-entropy (>= 0), with quantile heads of each row's
    quantile-Huber loss (>= 0)
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
        self.pixel = 'convs' in conv_kw
        self.atoms, self.quantiles = self.q_func.atoms, self.q_func.quantiles
        self.implicit = self.q_func.implicit
        self._tau_seed = int(seed)
        self.tau = self.tau_next = self.tau_target = None     # the fractions of the last learn()
        self.noisy = self.q_func.noisy
        # the noise draws take a key of their own: with the learner's seed they would share
        # Philox blocks with the implicit heads' fractions (same step, streams 0 / 1 / 2)
        self._noise_seed = int(seed) ^ NOISE_KEY
        self.noise = self.noise_next = self.noise_target = None   # the noise images of the last learn()
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
        if self.implicit:
            # the whole draw's fractions of this learner's rows: streams 0 online,
            # 1 selecting, 2 target, counted by the device Adam step
            q, row0 = self.implicit, (self.dp.rank * B if self.dp is not None else 0)
            draw = lambda sid, n, name: net.taus(self._tau_seed, self.opt['step'], sid, row0, B,   # noqa: E731
                                                 n, name)
            self.tau = draw(0, q['atoms'], 'tau')
            self.tau_next = draw(1, q['target_atoms'], 'tau_next') if self.double_q else None
            self.tau_target = draw(2, q['target_atoms'], 'tau_target')
        if self.noisy:
            # one noise image per forward, the same on every rank: streams 0 online
            # at s, 1 online at s' (double-Q), 2 target, counted by the device Adam step
            ndraw = lambda sid, name: net.draw(self._noise_seed, self.opt['step'], sid, name)   # noqa: E731
            self.noise = ndraw(0, 'noise')
            self.noise_next = ndraw(1, 'noise_next') if self.double_q else None
            self.noise_target = ndraw(2, 'noise_target')
        adv_t, val_t = tnet.fwd(obs_next, B, 't', self.tau_target, noise=self.noise_target)
        adv, val = net.fwd(obs, B, 'q', self.tau, keep_phi=True, noise=self.noise)
        adv_n = val_n = None
        if self.double_q:
            adv_n, val_n = net.fwd(obs_next, B, 'n', self.tau_next, noise=self.noise_next)
        N = self.atoms or self.quantiles or 1
        if self.implicit:                        # sample rows, scalar heads
            dadv = net.buf('dadv', (B * self.implicit['atoms'], A))
            dval = net.buf('dval', (B * self.implicit['atoms'], 1)) if dueling else None
        else:
            dadv = net.buf('dadv', (B, A * N))
            dval = net.buf('dval', (B, N)) if dueling else None
        if self.dp is not None and (self._xbuf is None
                                    or self.td_error.numel() != B * self.dp.world_size):
            # what the one all-reduce per learn() carries: [gradient | pad |
            # td_all (B_global) | stats (2)], the three as views of it
            self._xbuf, self.opt['g'], (self.td_error, self.stats_buf) = exchange_image(
                self.device, self.q_func.flat.numel(), (B * self.dp.world_size, 2))
        if self.atoms or self.quantiles or self.implicit:
            (self._gradient_c51 if self.atoms else self._gradient_qr if self.quantiles
             else self._gradient_iqn)(
                net, B, (adv, adv_n, adv_t), (val, val_n, val_t), (act, a_s), (rew, r_s), (don, d_s),
                weights, dadv, dval)
        elif self.dp is None:
            self.td_error = net.buf('td', (B,))
            L.call('smi_dqn_td', p(adv), A, p(adv_n), A, p(adv_t), A, p(val), 1, p(val_n), 1,
                   p(val_t), 1, p(act), a_s, p(rew), r_s, p(don), d_s, p(weights), B, A,
                   float(self.algo.gamma), int(dueling), int(self.double_q), p(dadv), A, p(dval),
                   p(self.td_error), None, p(self.stats_buf), st)
        else:
            world = self.dp.world_size
            L.call('smi_dqn_td_shard', p(adv), A, p(adv_n), A, p(adv_t), A, p(val), 1, p(val_n), 1,
                   p(val_t), 1, p(act), a_s, p(rew), r_s, p(don), d_s, p(weights), B, B * world,
                   self.dp.rank * B, A, float(self.algo.gamma), int(dueling), int(self.double_q),
                   p(dadv), A, p(dval), p(self.td_error), None, p(self.stats_buf), st)
        with L.dw_group(st):
            net.bwd(obs, B, 'q', [dadv, dval] if dueling else [dadv], self.opt['g'], self.noise)
        if self.noisy:
            net.sigma_grad(self.opt['g'], self.noise)

    def _gradient_c51(self, net, B, advs, vals, act, rew, don, weights, dadv, dval):
        """_gradient's TD step for categorical heads: smi_dqn_c51_td and its
        statistics launch, or the shard form into the exchange image's views"""
        A, N, q = self.action_dim, self.atoms, self.q_func
        (adv, adv_n, adv_t), (val, val_n, val_t) = advs, vals
        need = int(L.lib().smi_dqn_c51_partials_bytes(B))
        part = net.buf('c51_partials', (need // 8,), torch.float64)
        args = [p(adv), A * N, p(adv_n), A * N, p(adv_t), A * N, p(val), N, p(val_n), N, p(val_t), N,
                p(act[0]), act[1], p(rew[0]), rew[1], p(don[0]), don[1], p(weights), B]
        tail = [A, N, q.v_min, q.v_max, float(self.algo.gamma), int(q.dueling), int(self.double_q),
                p(dadv), A * N, p(dval), N]
        if self.dp is None:
            self.td_error = net.buf('td', (B,))
            L.call('smi_dqn_c51_td', *args, *tail, p(self.td_error), None, None, p(part), need,
                   p(self.stats_buf), net.st)
        else:
            L.call('smi_dqn_c51_td_shard', *args, B * self.dp.world_size, self.dp.rank * B, *tail,
                   p(self.td_error), None, None, p(part), need, p(self.stats_buf), net.st)

    def _gradient_qr(self, net, B, advs, vals, act, rew, don, weights, dadv, dval):
        """_gradient's TD step for quantile heads: smi_dqn_qr_td and the
        statistics launch, or the shard form into the exchange image's views"""
        A, N, q = self.action_dim, self.quantiles, self.q_func
        (adv, adv_n, adv_t), (val, val_n, val_t) = advs, vals
        need = int(L.lib().smi_dqn_qr_partials_bytes(B))
        part = net.buf('qr_partials', (need // 8,), torch.float64)
        args = [p(adv), A * N, p(adv_n), A * N, p(adv_t), A * N, p(val), N, p(val_n), N, p(val_t), N,
                p(act[0]), act[1], p(rew[0]), rew[1], p(don[0]), don[1], p(weights), B]
        tail = [A, N, q.kappa, float(self.algo.gamma), int(q.dueling), int(self.double_q),
                p(dadv), A * N, p(dval), N]
        if self.dp is None:
            self.td_error = net.buf('td', (B,))
            L.call('smi_dqn_qr_td', *args, *tail, p(self.td_error), None, None, p(part), need,
                   p(self.stats_buf), net.st)
        else:
            L.call('smi_dqn_qr_td_shard', *args, B * self.dp.world_size, self.dp.rank * B, *tail,
                   p(self.td_error), None, None, p(part), need, p(self.stats_buf), net.st)

    def _gradient_iqn(self, net, B, advs, vals, act, rew, don, weights, dadv, dval):
        """_gradient's TD step for implicit quantile heads: smi_iqn_td and the
        statistics launch, or the shard form into the exchange image's views"""
        A, q = self.action_dim, self.implicit
        (adv, adv_n, adv_t), (val, val_n, val_t) = advs, vals
        need = int(L.lib().smi_iqn_partials_bytes(B))
        part = net.buf('iqn_partials', (need // 8,), torch.float64)
        args = [p(adv), A, p(adv_n), A, p(adv_t), A, p(val), p(val_n), p(val_t), p(self.tau),
                p(act[0]), act[1], p(rew[0]), rew[1], p(don[0]), don[1], p(weights), B]
        tail = [A, q['atoms'], q['target_atoms'], q['kappa'], float(self.algo.gamma),
                int(self.q_func.dueling), int(self.double_q), p(dadv), A, p(dval)]
        if self.dp is None:
            self.td_error = net.buf('td', (B,))
            L.call('smi_iqn_td', *args, *tail, p(self.td_error), None, None, p(part), need,
                   p(self.stats_buf), net.st)
        else:
            L.call('smi_iqn_td_shard', *args, B * self.dp.world_size, self.dp.rank * B, *tail,
                   p(self.td_error), None, None, p(part), need, p(self.stats_buf), net.st)

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
        """'td_error' is the reference's scalar mean |td| (dqn.py:89-92); with
        categorical heads it is the mean cross-entropy of the rows (the
        unweighted mean of what `td_error` holds per row)"""
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
