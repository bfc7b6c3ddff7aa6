"""DeviceLearner.learn and _learn_phases, the one learn() frame of the
off-policy learners, on the CPU (no GPU): a shell whose hooks append to a log,
a fake group that keeps what it is asked to all-reduce."""
import torch

from surreal_amd.device_learner import DeviceLearner


class _Ctx(object):
    def __init__(self, log):
        self.log = log

    def make_current(self):
        self.log.append('make_current')


class _Sum(object):
    def __init__(self, world, log):
        self.world_size, self.rank, self.log, self.seen = world, 0, log, []

    def allreduce_(self, t):
        self.log.append('allreduce')
        self.seen.append(t)
        return t


class Shell(DeviceLearner):
    """the frame's hooks, logged; no constructor of the product's runs"""

    def __init__(self, phases=()):
        self.log, self.current_iteration, self.phases = [], 0, list(phases)
        self._ctx = _Ctx(self.log)

    def preprocess(self, batch):
        self.log.append(('preprocess', self.current_iteration))
        return dict(batch, on_device=True)

    def _learn_device(self, batch):
        assert batch['on_device']
        self.log.append('learn_device')

    def _update_phases(self, batch):
        assert batch['on_device']
        for t in self.phases:
            self.log.append('launches')
            yield t
        self.log.append('launches')

    def _report_metrics(self, it):
        self.log.append(('metrics', it))

    def periodic_checkpoint(self, global_steps, score):
        self.log.append(('checkpoint', global_steps, score))


BATCH = {'actions': torch.zeros(4, 1)}
def test_without_dp_the_frame_runs_in_order_and_dp_is_never_set():
    ln = Shell()
    ln.learn(BATCH)
    # ('preprocess', 1): the counter had advanced before anything else ran
    assert ln.log == ['make_current', ('preprocess', 1), 'learn_device', ('metrics', 1),
                      ('checkpoint', 1, None)]
    assert ln.current_iteration == 1
    assert 'dp' not in vars(ln) and ln.dp is None          # a learner that never heard of dp


def test_without_dp_learn_phases_yields_nothing_and_is_the_same_frame():
    ln = Shell()
    assert list(ln._learn_phases(BATCH)) == []
    plain = Shell()
    plain.learn(BATCH)
    assert ln.log == plain.log and ln.current_iteration == 1


def test_with_dp_exactly_the_yielded_buffers_are_all_reduced_in_order():
    a, b = torch.zeros(3), torch.ones(5)
    ln = Shell([a, b])
    ln.dp = _Sum(2, ln.log)
    ln.learn(BATCH)
    assert len(ln.dp.seen) == 2 and ln.dp.seen[0] is a and ln.dp.seen[1] is b
    assert ln.log == ['make_current', ('preprocess', 1), 'launches', 'allreduce', 'launches',
                      'allreduce', 'launches', ('metrics', 1), ('checkpoint', 1, None)]
    assert ln.current_iteration == 1
    ln.learn(BATCH)
    assert ln.current_iteration == 2 and ln.log.count(('metrics', 2)) == 1
    assert 'learn_device' not in ln.log


def test_a_group_of_world_1_is_no_group(monkeypatch):
    import surreal_amd.learner as learner_mod
    seen = []
    monkeypatch.setattr(learner_mod, 'replicate_from_rank0', lambda dp, ts: seen.append((dp, ts)))
    ln = Shell()
    t = [torch.zeros(2), torch.ones(2)]
    assert ln._dp_group(_Sum(1, ln.log), t) is None
    assert ln._dp_group(None, t) is None
    two = _Sum(2, ln.log)
    assert ln._dp_group(two, t) is two
    # the learner's tensors, in its order, with the group that will be used
    assert [d for d, _ in seen] == [None, None, two] and all(ts is t for _, ts in seen)
    ln.dp = ln._dp_group(_Sum(1, ln.log), t)
    ln.learn(BATCH)
    assert 'learn_device' in ln.log and 'allreduce' not in ln.log
