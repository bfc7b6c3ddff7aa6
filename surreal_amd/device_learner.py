"""What the learners share on the host side of their launches: config
coercion, named scratch buffers, the dense-layer launch helpers (LaunchNet)
and, for the off-policy learners, the learn() frame with and without a
data-parallel group, the layout of an exchange image, the Adam state and the
one hipGraph capture-and-replay routine (DeviceLearner)."""
import torch

from . import _lib as L
from .config import Config
from .session import LearnerHooks

p = L.ptr


def as_config(c):
    return c if isinstance(c, Config) else Config(c or {})


def named_buf(bufs, device, name, shape, dtype=torch.float32):
    """bufs[name]: a zero-filled scratch tensor, made anew when the shape changes"""
    t = bufs.get(name)
    if t is None or tuple(t.shape) != tuple(shape):
        t = torch.zeros(shape, dtype=dtype, device=device)
        bufs[name] = t
    return t


def exchange_image(device, n_grad, tails):
    """What one all-reduce of a data-parallel learn() carries: the zero-filled
    buffer [gradient (n_grad) | pad to a multiple of 4 floats | tails...], its
    gradient view and the views of the tails (their lengths in `tails`)"""
    off = (n_grad + 3) // 4 * 4
    buf = torch.zeros(off + sum(tails), dtype=torch.float32, device=device)
    views = []
    for n in tails:
        views.append(buf[off:off + n])
        off += n
    return buf, buf[:n_grad], views


class LaunchNet(object):
    """Launch helpers over a model's flat buffers and a dict of named scratch."""

    def __init__(self, device, bufs):
        self.device = device
        self.st = L.stream(device)
        self.bufs = bufs

    def buf(self, name, shape, dtype=torch.float32):
        return named_buf(self.bufs, self.device, name, shape, dtype)

    def lin(self, x, ldx, rows, k, w, ldw, b, n, act, y, ldy):
        L.call('smi_linear_forward', p(x), ldx, rows, k, p(w), ldw, p(b), n, act, p(y), ldy, self.st)

    @staticmethod
    def check_rows(x, rows, width, what):
        """x must be a [>= rows][width] fp32 device matrix with unit column stride
        (the kernels read rows x width through its row stride)"""
        if (x.dim() != 2 or x.shape[0] < rows or x.shape[1] != width or x.stride(1) != 1
                or x.dtype != torch.float32):
            raise ValueError(f'{what} input: expected a float32 [{rows}][{width}] matrix, got '
                             f'{x.dtype} {tuple(x.shape)}')


class DeviceLearner(LearnerHooks):
    """An off-policy learner whose update is one launch sequence on one stream.
    The host class provides preprocess(host batch), _learn_device(device batch)
    and _stats_dict; use_graph routes the update through _graph_step.  A
    data-parallel learner (self.dp: a group exposing world_size, rank and
    allreduce_, see _dp_group) also provides _update_phases(device batch): the
    update as a generator of the buffers to all-reduce (SUM) between its
    launches."""
    dp = None                     # one GPU, unless the constructor sets a group

    def _init_device(self, learner_config, env_config, session_config, metrics, checkpoint,
                     device, checkpoint_full_state):
        """the constructor preamble; returns (learner_config, env_config) as Configs"""
        L.require_gpu()
        self.checkpoint_full_state = bool(checkpoint_full_state)
        self.learner_config = as_config(learner_config)
        self.env_config = as_config(env_config)
        self.session_config = session_config
        self._init_hooks(metrics, checkpoint)
        self.device = torch.device(device) if device is not None else \
            torch.device('cuda', torch.cuda.current_device())
        L.ensure_workspace(self.device)
        self._ctx = L.Context(self.device)      # this learner's own workspace (re-entrancy)
        self.current_iteration = 0
        self._bufs = {}
        self._graph = None
        self._gin = None
        return self.learner_config, self.env_config

    @staticmethod
    def _dp_group(dp, tensors):
        """a constructor's data-parallel group: None for one rank (dp=None or a
        group of world 1); the tensors start as rank 0's on every rank"""
        from .learner import replicate_from_rank0
        dp = dp if dp is not None and dp.world_size > 1 else None
        replicate_from_rank0(dp, tensors)
        return dp

    # ---------------------------------------------------------------- Adam
    @staticmethod
    def adam_state(flat, lr, g=None, wd=0.0):
        """moments, device step counter and learning rate of one flat parameter
        buffer; g: its gradient image (a view of a packed buffer, or its own)"""
        dev = flat.device
        return {'m': torch.zeros_like(flat), 'v': torch.zeros_like(flat),
                'step': torch.zeros(1, dtype=torch.int32, device=dev),
                'lr': torch.tensor([lr], dtype=torch.float32, device=dev),
                'wd': float(wd), 'g': g if g is not None else torch.zeros_like(flat)}

    @staticmethod
    def adam_step(o, flat, eps, max_norm, clip_value, st):
        """torch.optim.Adam (betas (0.9, 0.999)) on flat from o['g'], after an L2
        norm clip (max_norm) or a value clip (clip_value); 0 turns either off"""
        L.call('smi_adam_clip', p(flat), p(o['g']), p(o['m']), p(o['v']), flat.numel(),
               p(o['step']), p(o['lr']), 0.9, 0.999, eps, o['wd'], max_norm, float(clip_value),
               None, None, st)

    # ------------------------------------------------------- reference API
    def learn(self, batch):                               # ddpg.py:354-376, dqn.py:75-92
        if self.dp is not None:
            for buf in self._learn_phases(batch):
                self.dp.allreduce_(buf)
            return
        self.current_iteration += 1           # one GPU: the frame without a generator
        self._ctx.make_current()
        if not isinstance(batch['actions'], torch.Tensor) or not batch['actions'].is_cuda:
            batch = self.preprocess(batch)
        self._learn_device(batch)
        self._report_metrics(self.current_iteration)
        self.periodic_checkpoint(global_steps=self.current_iteration, score=None)

    def _learn_phases(self, batch):
        """learn() as a generator of the buffers a data-parallel learner must
        all-reduce (SUM) between its launches (_update_phases); a caller that
        is not learn() sums them itself.  Without dp it yields nothing."""
        self.current_iteration += 1
        self._ctx.make_current()
        if not isinstance(batch['actions'], torch.Tensor) or not batch['actions'].is_cuda:
            batch = self.preprocess(batch)
        if self.dp is None:
            self._learn_device(batch)
        else:
            yield from self._update_phases(batch)
        self._report_metrics(self.current_iteration)
        self.periodic_checkpoint(global_steps=self.current_iteration, score=None)

    def _host_scalars(self):
        return {}

    def last_stats(self):
        return self._stats_dict(self.stats_buf.cpu().numpy(), {})

    # ------------------------------------------------------- hipGraph replay
    def _graph_step(self, ins, run, after=None):
        """One update as a hipGraph replay (the step is a few dozen small
        launches, so host launch overhead, not the GPU, bounds it).  ins: the
        step's device inputs; run(*inputs) issues its launches.  The first call
        for a given input count, shapes and dtypes runs eagerly (it is that
        call's update, and it sizes every scratch buffer), then captures the
        same launch sequence over static input buffers; later calls copy their
        inputs in (skipped when the caller already wrote them: graph_inputs())
        and replay.  after() is the host part of the step that follows a replay
        (the eager call's run has done it)."""
        sig = [(t.shape, t.dtype) for t in ins]
        if self._graph is None or sig != [(t.shape, t.dtype) for t in self._gin]:
            self._graph = None
            run(*ins)
            self._gin = [torch.zeros(s, dtype=d, device=self.device) for s, d in sig]
            g = torch.cuda.CUDAGraph()
            with L.gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
                run(*self._gin)
            self._graph = g
            return
        for s, t in zip(self._gin, ins):
            if s.data_ptr() != t.data_ptr():
                s.copy_(t)
        self._graph.replay()
        if after is not None:
            after()

    def graph_inputs(self):
        """Static (obs, actions, rewards, obs_next, dones[, weights]) buffers of
        the captured step (None before the first learn() in graph mode)."""
        return None if self._gin is None else dict(zip(
            ('obs', 'actions', 'rewards', 'obs_next', 'dones', 'weights'), self._gin))
