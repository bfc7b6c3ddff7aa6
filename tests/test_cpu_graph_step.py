"""DeviceLearner._graph_step, the one capture-and-replay routine of the
off-policy learners, on the CPU (no GPU): torch.cuda's graph API is replaced by
the fakes of test_cpu_capture_fallback, the inputs are CPU tensors and `run`
counts its calls and keeps the tensors it was handed."""
import torch

from surreal_amd.device_learner import DeviceLearner
from tests.test_cpu_capture_fallback import FakeGraph, fake_cuda  # noqa: F401  (fixture)


def shell():
    ln = object.__new__(DeviceLearner)
    ln.device = torch.device('cpu')
    ln._graph = ln._gin = None
    ln.runs, ln.afters = [], 0

    def run(*a):
        ln.runs.append(a)

    def after():
        ln.afters += 1
    ln.run, ln.after = run, after
    return ln


def _ins(B=8, weights=False, obs_dtype=torch.float32, fill=1.0):
    t = [torch.full((B, 5), fill).to(obs_dtype), torch.full((B, 3), fill), torch.full((B, 1), fill),
         torch.full((B, 5), fill).to(obs_dtype), torch.full((B, 1), fill)]
    if weights:
        t.append(torch.full((B, 1), fill))
    return tuple(t)


def _step(ln, ins):
    ln.runs.clear()
    ln._graph_step(ins, ln.run, ln.after)


def _same(a, b):
    return len(a) == len(b) and all(x is y for x, y in zip(a, b))


def test_first_call_eager_then_capture_then_replay(fake_cuda):
    ln = shell()
    ins = _ins()
    _step(ln, ins)
    # once eager on the live inputs, once (the capture) on the static ones
    assert len(ln.runs) == 2 and _same(ln.runs[0], ins) and _same(ln.runs[1], ln._gin)
    assert isinstance(ln._graph, FakeGraph) and ln._graph.replays == 0 and ln.afters == 0
    assert isinstance(ln._gin, list) and all(s is not t for s, t in zip(ln._gin, ins))
    g, gin = ln._graph, ln._gin
    nxt = _ins(fill=2.0)
    _step(ln, nxt)
    assert ln.runs == [] and g.replays == 1 and ln.afters == 1
    assert ln._graph is g and ln._gin is gin
    assert all(torch.equal(s, t) for s, t in zip(gin, nxt))          # copied in before the replay
    _step(ln, _ins(fill=3.0))
    assert ln.runs == [] and g.replays == 2 and ln.afters == 2


def test_after_is_optional(fake_cuda):
    ln = shell()
    ln._graph_step(_ins(), ln.run)
    ln._graph_step(_ins(), ln.run)
    assert ln._graph.replays == 1 and len(ln.runs) == 2


def test_input_that_is_the_static_tensor_is_not_copied(fake_cuda, monkeypatch):
    ln = shell()
    _step(ln, _ins())
    gin = ln._gin
    gin[1].fill_(7.0)                       # the caller wrote the static actions itself
    # a live twin at the same address with other contents: a copy would show
    twin = torch.full((8, 3), -1.0)
    monkeypatch.setattr(twin, 'data_ptr', gin[1].data_ptr)
    nxt = list(_ins(fill=2.0))
    nxt[1] = twin
    _step(ln, tuple(nxt))
    assert ln._graph.replays == 1
    assert torch.equal(gin[1], torch.full((8, 3), 7.0))               # kept its own
    assert torch.equal(gin[0], nxt[0]) and torch.equal(gin[4], nxt[4])
    # and the static tensor itself as an input
    gin[2].fill_(5.0)
    nxt = list(_ins(fill=4.0))
    nxt[2] = gin[2]
    _step(ln, tuple(nxt))
    assert torch.equal(gin[2], torch.full((8, 1), 5.0)) and torch.equal(gin[0], nxt[0])


def test_sixth_input_captures_again_and_back(fake_cuda):
    ln = shell()
    _step(ln, _ins())
    g5 = ln._graph
    w = _ins(weights=True, fill=2.0)
    _step(ln, w)
    assert len(ln.runs) == 2 and _same(ln.runs[0], w) and _same(ln.runs[1], ln._gin)
    assert ln._graph is not g5 and len(ln._gin) == 6 and ln._graph.replays == 0 and ln.afters == 0
    g6 = ln._graph
    _step(ln, _ins(weights=True, fill=3.0))
    assert ln.runs == [] and g6.replays == 1
    _step(ln, _ins())                                   # the weights disappear: again
    assert len(ln.runs) == 2 and ln._graph is not g6 and len(ln._gin) == 5


def test_leading_dimension_captures_again(fake_cuda):
    ln = shell()
    _step(ln, _ins(B=8))
    g = ln._graph
    small = _ins(B=4)
    _step(ln, small)
    assert len(ln.runs) == 2 and _same(ln.runs[0], small) and ln._graph is not g
    assert [tuple(s.shape) for s in ln._gin] == [tuple(t.shape) for t in small]
    # one input alone
    one = list(_ins(B=4))
    one[2] = torch.zeros(6, 1)
    _step(ln, tuple(one))
    assert len(ln.runs) == 2 and tuple(ln._gin[2].shape) == (6, 1) and g.replays == 0


def test_dtype_captures_again_with_a_uint8_static_buffer(fake_cuda):
    ln = shell()
    _step(ln, _ins())
    g = ln._graph
    assert ln._gin[0].dtype == torch.float32
    frames = list(_ins(fill=2.0))
    frames[0] = torch.full((8, 5), 200, dtype=torch.uint8)
    _step(ln, tuple(frames))
    assert len(ln.runs) == 2 and ln._graph is not g and g.replays == 0
    assert ln._gin[0].dtype == torch.uint8 and ln._gin[3].dtype == torch.float32
    nxt = list(_ins(fill=3.0))
    nxt[0] = torch.full((8, 5), 201, dtype=torch.uint8)
    _step(ln, tuple(nxt))
    assert ln.runs == [] and ln._graph.replays == 1 and torch.equal(ln._gin[0], nxt[0])


def test_graph_inputs_names(fake_cuda):
    ln = shell()
    assert ln.graph_inputs() is None
    _step(ln, _ins())
    gi = ln.graph_inputs()
    assert list(gi) == ['obs', 'actions', 'rewards', 'obs_next', 'dones']
    assert all(gi[k] is s for k, s in zip(gi, ln._gin))
    _step(ln, _ins(weights=True))
    gi = ln.graph_inputs()
    assert list(gi) == ['obs', 'actions', 'rewards', 'obs_next', 'dones', 'weights']
    assert gi['weights'] is ln._gin[5]
