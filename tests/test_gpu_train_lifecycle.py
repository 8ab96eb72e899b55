"""The lifetime of a captured training step (``core.trainer.CapturedStep``): what a real run does BETWEEN steps -- resume,
validation, a second batch signature, zero_grad, eager epochs, frozen parameters, parameter groups, a changed
hyperparameter -- on the tiny architecture and batches of tests/_train_run.py (64 x 64, N = 2 and N = 1).

Every test plays one scripted sequence of events twice from the same initial state, once through the eager loop
(``do_train(graph=False)``) and once through a ``CapturedStep``, with the same ``litepose_amd.optim`` class, and requires
the same bits for every parameter, BatchNorm buffer, optimizer state tensor, ``p.grad`` and returned dict.  The eager loop
is held to fp64 by test_gpu_layer_grad.py, test_gpu_conv_grad.py, test_gpu_optim.py and test_gpu_train_net.py, so bitwise
equality carries that accuracy over; what is tested here is that a replay trains the memory the caller believes it trains.
"Lockstep" tests compare after every step.  DESIGN.md 4f has the table of events these tests pin."""
import io

import pytest
import torch

import _poison as po
from _train_run import _assert_same, _loader, _module, make_cfg, setup  # noqa: F401  (setup: the module-scoped fixture)
from litepose_amd import config, optim
from litepose_amd.core.loss import MultiLossFactory
from litepose_amd.core.trainer import CapturedStep, _flat, do_train

pytestmark = pytest.mark.gpu


def ADAM(m):
    return optim.Adam(m.parameters(), lr=1e-3)


def SGD(m):
    return optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)


OPTIMIZERS = {'adam': ADAM, 'sgd': SGD}


class Run(object):
    """A module from the golden weights, its optimizer and, for the captured run, a kept ``CapturedStep``.  ``step`` is
    ``do_train`` over one batch, ``epoch`` over several; ``got`` is the last returned dict."""

    def __init__(self, setup, make_opt, graph, cfg=None):
        self.cfg = setup['cfg'] if cfg is None else cfg
        self.model = _module(setup['case'])
        self.opt = make_opt(self.model)
        self.factory = MultiLossFactory(self.cfg)
        self.stepper = CapturedStep(self.cfg, self.model, self.factory, self.opt) if graph else False
        self.got = None

    def epoch(self, batches):
        self.got = do_train(self.cfg, self.model, _loader(batches, False), self.factory, self.opt, 0, None, None,
                            self.stepper)
        return self.got

    def step(self, batch):
        return self.epoch([batch])

    def counters(self):
        s = self.stepper
        return s.captures, s.replays, s.eager_steps, s.invalidations

    def view(self):
        return dict(model=self.model, opt=self.opt, got=self.got)


def _pair(setup, make_opt, cfg=None):
    return Run(setup, make_opt, False, cfg), Run(setup, make_opt, True, cfg)


def _same(eager, graph, every_parameter=True):
    torch.cuda.synchronize()
    _assert_same(graph.view(), eager.view(), every_parameter)


def _steps_of(opt):
    """index -> Adam's step count, read from ``state_dict()``."""
    return {i: float(st['step']) for i, st in opt.state_dict()['state'].items()}


def _same_state(state, want):
    assert sorted(state) == sorted(want)
    for i in want:
        assert sorted(state[i]) == sorted(want[i])
        for name, v in want[i].items():
            assert po.bitwise_equal(state[i][name].cpu(), v.cpu()), (i, name)


# ------------------------------------------------------------------ 1. optimizer.load_state_dict into live objects
@pytest.mark.parametrize('which', ['adam', 'sgd'])
def test_resume_into_live_objects(setup, which):
    B = setup['batches']
    eager, graph = _pair(setup, OPTIMIZERS[which])
    for r in (eager, graph):
        for i in range(3):                                  # eager, captured, replayed
            r.step(B[i])
        sd = r.opt.state_dict()
        r.step(B[3])
        r.step(B[0])
        r.opt.load_state_dict(sd)                           # rewinds the moments and the counts; the parameters stay
        _same_state(r.opt.state_dict()['state'], sd['state'])
        if which == 'adam':
            assert set(_steps_of(r.opt).values()) == {3.0}
        for i in (1, 2, 3):
            r.step(B[i])
    assert graph.counters() == (2, 6, 2, 1)
    _same(eager, graph)
    if which == 'adam':                                     # sd's counts advanced by three steps, not the five + three run
        assert set(_steps_of(graph.opt).values()) == {6.0} and set(_steps_of(eager.opt).values()) == {6.0}


# ------------------------------------------------------------------ 2. a checkpoint into fresh objects
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'captured'])
def test_full_checkpoint_resume(setup, graph):
    B = setup['batches']
    seq = [B[0], B[1], B[2], B[3], B[0], B[1]]
    whole = Run(setup, ADAM, graph)
    for b in seq:
        whole.step(b)
    first = Run(setup, ADAM, graph)
    for b in seq[:3]:
        first.step(b)
    buf = io.BytesIO()
    torch.save(dict(state_dict=first.model.state_dict(), optimizer=first.opt.state_dict()), buf)
    buf.seek(0)
    checkpoint = torch.load(buf, map_location=torch.device('cpu'))
    second = Run(setup, ADAM, graph)
    for p in second.model.parameters():                     # nothing of the fresh module's own survives the load
        p.data.fill_(0.5)
    second.model.load_state_dict(checkpoint['state_dict'])
    second.opt.load_state_dict(checkpoint['optimizer'])
    for b in seq[3:]:
        second.step(b)
    _same(whole, second)
    assert set(_steps_of(second.opt).values()) == {6.0}
    if graph:
        assert whole.counters() == (1, 5, 1, 0)
        assert second.counters() == (1, 2, 1, 1)            # the load came after the stepper was built: it started over


# ------------------------------------------------------------------ 3. model.load_state_dict is in place
def test_model_load_state_dict_mid_run_is_in_place(setup):
    B = setup['batches']
    eager, graph = _pair(setup, ADAM)
    for r in (eager, graph):
        r.step(B[0])
        r.step(B[1])
        sd = {k: v.detach().clone() for k, v in r.model.state_dict().items()}
        where = [p.data_ptr() for p in r.model.parameters()]
        r.step(B[2])
        r.step(B[3])
        assert not po.bitwise_equal(next(r.model.parameters()), sd['first.0.0.weight'])
        r.model.load_state_dict(sd)
        assert where == [p.data_ptr() for p in r.model.parameters()]
        for k, v in r.model.state_dict().items():
            assert po.bitwise_equal(v, sd[k]), k
        r.step(B[0])
        r.step(B[1])
    assert graph.counters() == (1, 5, 1, 0)
    _same(eager, graph)
    assert all(int(v) == 4 for k, v in graph.model.state_dict().items() if k.endswith('num_batches_tracked'))


# ------------------------------------------------------------------ 4. two signatures alive (lockstep)
def test_two_signatures_alive(setup):
    A, O = setup['batches'], setup['ones']
    eager, graph = _pair(setup, ADAM)
    want = [(0, 0, 1), (1, 1, 1), (1, 1, 2), (2, 2, 2), (2, 3, 2), (2, 4, 2), (2, 5, 2)]
    for b, counters in zip([A[0], A[1], O[0], O[1], A[2], O[2], A[3]], want):
        eager.step(b)
        graph.step(b)
        assert graph.counters() == counters + (0,)
        _same(eager, graph)                                 # p.grad included: the graphs swap it between them


# ------------------------------------------------------------------ 5. p.grad under interference (lockstep)
def _optimizer_zero_grad(r, batch):
    r.opt.zero_grad()
    assert all(p.grad is None for p in r.model.parameters())


def _model_zero_grad(r, batch):
    r.model.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not bool(p.grad.any()) for p in r.model.parameters())


def _eager_epoch(r, batch):
    do_train(r.cfg, r.model, _loader([batch], False), r.factory, r.opt, 0, None, None, False)


@pytest.mark.parametrize('interfere', [_optimizer_zero_grad, _model_zero_grad, _eager_epoch],
                         ids=['optimizer.zero_grad', 'model.zero_grad', 'eager-epoch'])
def test_p_grad_under_interference(setup, interfere):
    B = setup['batches']
    eager, graph = _pair(setup, ADAM)
    for i in range(3):
        eager.step(B[i])
        graph.step(B[i])
        _same(eager, graph)
    for b in (B[3], B[0]):                                  # twice between two replays of the same graph
        interfere(eager, B[1])
        interfere(graph, B[1])
        eager.step(b)
        graph.step(b)
        _same(eager, graph)
    assert graph.counters() == (1, 4, 1, 0)


# ------------------------------------------------------------------ 6. validation between steps
def test_validation_between_steps(setup):
    B = setup['batches']
    eager, graph = _pair(setup, ADAM)
    for r in (eager, graph):
        r.val = []
        for i in range(3):
            r.step(B[i])
        for b, x in ((B[3], B[0][0]), (B[0], B[3][0])):
            r.model.eval()
            with torch.no_grad():
                r.val.append([o.clone() for o in r.model(x)])
            r.model.train()
            r.step(b)
    assert graph.counters() == (1, 4, 1, 0)
    _same(eager, graph)
    for ve, vg in zip(eager.val, graph.val):
        assert len(ve) == len(vg) == 2
        for a, b in zip(ve, vg):
            assert po.bitwise_equal(a, b)
    assert not po.bitwise_equal(graph.val[0][0], graph.val[1][0])
    for r in (eager, graph):                                # training steps only
        assert all(int(v) == 5 for k, v in r.model.state_dict().items() if k.endswith('num_batches_tracked'))
    x = B[1][0]
    oe = [o.clone() for o in eager.model.to_engine()(x)]
    og = [o.clone() for o in graph.model.to_engine()(x)]
    assert len(oe) == len(og) == 2
    for a, b in zip(oe, og):
        assert po.bitwise_equal(a, b)


# ------------------------------------------------------------------ 7. frozen parameters
def _frozen_first(m):
    for p in m.first.parameters():
        p.requires_grad_(False)
    return optim.Adam(m.parameters(), lr=1e-3)


def test_frozen_parameters(setup):
    B = setup['batches']
    eager, graph = _pair(setup, _frozen_first)
    for r in (eager, graph):
        for i in range(4):
            r.step(B[i])
    assert graph.counters() == (1, 3, 1, 0)
    _same(eager, graph, every_parameter=False)
    for r in (eager, graph):
        names = [k for k, _ in r.model.named_parameters()]
        frozen = [i for i, k in enumerate(names) if k.startswith('first.')]
        assert frozen == list(range(9))                     # three convolutions and three BatchNorm pairs, in front
        steps = _steps_of(r.opt)                            # no state for them; the others counted every step
        assert sorted(steps) == list(range(9, len(names))) and set(steps.values()) == {4.0}
        for k, p in r.model.named_parameters():
            if k.startswith('first.'):
                assert p.grad is None and po.bitwise_equal(p.detach().cpu(), torch.from_numpy(setup['case']['sd'][k])), k
            else:
                assert p.grad is not None, k


def test_freezing_after_a_capture_with_invalidate(setup):
    B = setup['batches']
    eager, graph = _pair(setup, ADAM)
    for r in (eager, graph):
        for i in range(3):
            r.step(B[i])
        held = {k: p.detach().clone() for k, p in r.model.named_parameters() if k.startswith('final_raw.')}
        assert len(held) == 8
        for p in r.model.final_raw.parameters():
            p.requires_grad_(False)
        if r.stepper:
            r.stepper.invalidate()                          # which tensors a step touches has changed: the caller says so
        for i in (3, 0, 1):
            r.step(B[i])
        steps = _steps_of(r.opt)
        for i, (k, p) in enumerate(r.model.named_parameters()):
            if k in held:
                assert p.grad is None and steps[i] == 3.0 and po.bitwise_equal(p.detach(), held[k]), k
            else:
                assert p.grad is not None and steps[i] == 6.0, k
    assert graph.counters() == (2, 4, 2, 1)
    _same(eager, graph, every_parameter=False)


# ------------------------------------------------------------------ 8. two groups and a scheduler
def _two_groups(m):
    backbone = list(m.first.parameters()) + list(m.stage.parameters())
    ids = set(id(p) for p in backbone)
    heads = [p for p in m.parameters() if id(p) not in ids]
    assert backbone and heads
    return optim.Adam([dict(params=backbone, lr=1e-3), dict(params=heads, lr=3e-3)])


def test_two_groups_follow_a_milestone_without_a_second_capture(setup):
    B = setup['batches']
    eager, graph = _pair(setup, _two_groups)
    for r in (eager, graph):
        sched = torch.optim.lr_scheduler.MultiStepLR(r.opt, milestones=[2], gamma=0.5)
        for i in range(4):
            r.step(B[i])
            sched.step()
        torch.cuda.synchronize()
        assert [g['lr'] for g in r.opt.param_groups] == [1e-3 * 0.5, 3e-3 * 0.5]
    assert graph.counters() == (1, 3, 1, 0)
    _same(eager, graph)
    for g, lr in zip(graph.opt.param_groups, (1e-3, 3e-3)):
        assert float(graph.opt._group_native(g)['lr']) == lr * 0.5
    plain = Run(setup, _two_groups, False)
    for i in range(4):
        plain.step(B[i])
    last = [p for p in plain.model.parameters()][-1], [p for p in eager.model.parameters()][-1]
    assert not po.bitwise_equal(*last)                      # the milestone reached the second group


# ------------------------------------------------------------------ 9. the reference's get_optimizer settings
@pytest.mark.parametrize('which', ['sgd', 'adam'])
def test_the_reference_settings(setup, which):
    B = setup['batches']
    cfg = make_cfg()
    cfg.TRAIN = config.CfgNode(OPTIMIZER=which, LR=1e-3, MOMENTUM=0.9, WD=1e-4, NESTEROV=True)
    eager, graph = _pair(setup, lambda m: optim.get_optimizer(cfg, m), cfg)
    g = graph.opt.param_groups[0]
    if which == 'sgd':
        assert isinstance(graph.opt, optim.SGD)
        assert (g['lr'], g['momentum'], g['weight_decay'], g['nesterov']) == (1e-3, 0.9, 1e-4, True)
    else:
        assert isinstance(graph.opt, optim.Adam) and (g['lr'], g['weight_decay']) == (1e-3, 0)
    for r in (eager, graph):
        for i in range(4):
            r.step(B[i])
    assert graph.counters() == (1, 3, 1, 0)
    _same(eager, graph)


# ------------------------------------------------------------------ 10. a by-value change
def _snapshot(r):
    """Every tensor a refused step could have touched, cloned: parameters, buffers, gradients, optimizer state, the device
    lr scalars and step arrays, the meters and the static batch buffers of every graph."""
    torch.cuda.synchronize()
    t = {('model', k): v for k, v in r.model.state_dict().items()}
    t.update({('grad', k): p.grad for k, p in r.model.named_parameters()})
    for i, st in r.opt.state_dict()['state'].items():
        t.update({('optimizer', i, name): v for name, v in st.items()})
    for j, group in enumerate(r.opt.param_groups):
        ns = r.opt._group_native(group)
        t[('lr', j)] = ns['lr']
        if ns['steps'] is not None:
            t[('steps', j)] = ns['steps']
    s = r.stepper
    t[('last',)], t[('sums',)] = s._last, s._sums
    for n, cap in enumerate(s._captured.values()):
        t.update({('static', n, m): v for m, v in enumerate(_flat(cap['static']))})
    return {k: v.detach().clone() for k, v in t.items()}


def test_a_by_value_change_is_refused_cleanly_and_undone_by_invalidate(setup):
    B = setup['batches']
    eager, graph = _pair(setup, ADAM)
    for r in (eager, graph):
        for i in range(3):
            r.step(B[i])
        r.opt.param_groups[0]['weight_decay'] = 1e-4
    before, sights = _snapshot(graph), dict(graph.stepper._sights)
    assert len(graph.stepper._captured) == 1
    with pytest.raises(RuntimeError, match='invalidate'):
        graph.stepper.step(*B[3])                           # another batch than the static buffers hold
    after = _snapshot(graph)
    assert sorted(before) == sorted(after)
    for k in before:
        assert po.bitwise_equal(before[k], after[k]), k
    assert graph.counters() == (1, 2, 1, 0) and graph.stepper._sights == sights
    with pytest.raises(RuntimeError, match='invalidate'):   # and so does the loop, eager or not
        graph.step(B[3])
    graph.stepper.invalidate()
    for i in (3, 0, 1):
        eager.step(B[i])
        graph.step(B[i])
    assert graph.counters() == (2, 4, 2, 1)
    _same(eager, graph)
    plain = Run(setup, ADAM, False)                         # the new value is in use: without it the bits differ
    for i in (0, 1, 2, 3, 0, 1):
        plain.step(B[i])
    assert not po.bitwise_equal(next(plain.model.parameters()), next(eager.model.parameters()))
    # a plain optimizer.step() under standing marks is refused as well, and works after forget_captures()
    for r in (eager, graph):
        r.opt.param_groups[0]['eps'] = 1e-6
    eager.opt.step()
    with pytest.raises(RuntimeError, match='captured'):
        graph.opt.step()
    generation = graph.opt.generation
    graph.opt.forget_captures()
    assert graph.opt.generation == generation + 1
    graph.opt.step()
    _same(eager, graph)
    assert set(_steps_of(graph.opt).values()) == {7.0}


# ------------------------------------------------------------------ 11. add_param_group after a capture (lockstep)
def _without_a_head(m):
    held = set(id(p) for p in m.final_raw[0].parameters())
    return optim.Adam([p for p in m.parameters() if id(p) not in held], lr=1e-3)


def test_add_param_group_after_a_capture(setup):
    B = setup['batches']
    eager, graph = _pair(setup, _without_a_head)
    for i in range(3):
        eager.step(B[i])
        graph.step(B[i])
        _same(eager, graph, every_parameter=False)
    assert graph.counters() == (1, 2, 1, 0)
    for r in (eager, graph):
        r.opt.add_param_group(dict(params=list(r.model.final_raw[0].parameters())))
        assert len(r.opt.state_dict()['state']) == len(list(r.model.parameters())) - 4
    # the next sight is eager and creates the new group's state; the one after captures; then a replay
    for b, counters in zip((B[3], B[0], B[1]), [(1, 2, 2, 1), (2, 3, 2, 1), (2, 4, 2, 1)]):
        eager.step(b)
        graph.step(b)
        assert graph.counters() == counters
        _same(eager, graph)
    steps = _steps_of(graph.opt)
    new = sorted(steps)[-4:]                                # the new group's parameters come last in state_dict()
    assert all(steps[i] == (3.0 if i in new else 6.0) for i in steps)


# ------------------------------------------------------------------ 12. a kept stepper over two epochs
def test_a_kept_stepper_over_two_epochs(setup):
    B = setup['batches']
    eager, graph = _pair(setup, ADAM)
    first = eager.epoch(B[:4]), graph.epoch(B[:4])
    assert first[0] == first[1] and graph.counters() == (1, 3, 1, 0)
    second = eager.epoch(B[1:4]), graph.epoch(B[1:4])
    assert second[0] == second[1] and second[0] != first[0]
    assert graph.counters() == (1, 6, 1, 0)                 # no capture and no eager step in the second epoch
    _same(eager, graph)
    # the meters started from zero: the running sums are the second epoch's three batches alone
    S = graph.cfg.LOSS.NUM_STAGES
    _, sums = graph.stepper.read()
    for k, key in enumerate(('heatmaps', 'push', 'pull')):
        for idx in range(S):
            if second[1][key][idx] is not None:
                assert sums[k * S + idx] / 6 == second[1][key][idx][1]
