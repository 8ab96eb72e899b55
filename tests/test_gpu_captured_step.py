"""``do_train(..., graph=True)`` / ``core.trainer.CapturedStep`` against the eager loop on the tiny architecture and batch
shape of tests/_train_net_case.py (N = 2, 64 x 64): from the same initial state the two perform the same sequence of updates,
so every parameter, every BatchNorm buffer (``num_batches_tracked`` included), every optimizer state tensor, every
``p.grad`` and the returned dict are the same bits -- the library's calls give the same bits launched or replayed
(DESIGN.md 4f), and torch's adds and means in between are elementwise."""
import pytest
import torch

import _poison as po
from _train_run import _assert_same, _loader, _module, setup  # noqa: F401  (setup: the module-scoped fixture)
from litepose_amd import optim
from litepose_amd.core.loss import MultiLossFactory
from litepose_amd.core.trainer import CapturedStep, do_train

pytestmark = pytest.mark.gpu


OPTIMIZERS = {
    'adam': lambda ps: optim.Adam(ps, lr=1e-3),
    'sgd': lambda ps: optim.SGD(ps, lr=1e-3, momentum=0.9),
}


def _train(setup, which, batches, graph, milestones=None, scribble=False):
    cfg = setup['cfg']
    m = _module(setup['case'])
    opt = OPTIMIZERS[which](m.parameters())
    factory = MultiLossFactory(cfg)
    stepper = CapturedStep(cfg, m, factory, opt) if graph else False
    if milestones is None:
        got = do_train(cfg, m, _loader(batches, scribble), factory, opt, 0, None, None, stepper)
    else:                                     # a scheduler stepped per batch: one do_train call per batch
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=0.5)
        for b in batches:
            got = do_train(cfg, m, _loader([b], scribble), factory, opt, 0, None, None, stepper)
            sched.step()
    torch.cuda.synchronize()
    return dict(model=m, opt=opt, got=got, stepper=stepper)


@pytest.mark.parametrize('which', ['adam', 'sgd'])
def test_four_equal_batches_capture_once_and_match_the_eager_loop(setup, which):
    four = setup['batches'][:4]
    eager = _train(setup, which, four, False)
    graph = _train(setup, which, four, True, scribble=True)
    s = graph['stepper']
    assert (s.captures, s.replays, s.eager_steps) == (1, 3, 1)
    _assert_same(graph, eager)
    assert all(int(v) == 4 for k, v in graph['model'].state_dict().items() if k.endswith('num_batches_tracked'))


def test_a_short_fifth_batch_runs_eagerly(setup):
    eager = _train(setup, 'adam', setup['batches'], False)
    graph = _train(setup, 'adam', setup['batches'], True, scribble=True)
    s = graph['stepper']
    assert (s.captures, s.replays, s.eager_steps) == (1, 3, 2)
    _assert_same(graph, eager)


def test_a_replay_after_an_eager_step_leaves_its_gradients_in_p_grad(setup):
    order = [setup['batches'][i] for i in (0, 1, 4, 2)]
    eager = _train(setup, 'adam', order, False)
    graph = _train(setup, 'adam', order, True)
    s = graph['stepper']
    assert (s.captures, s.replays, s.eager_steps) == (1, 2, 2)
    _assert_same(graph, eager)


def test_a_milestone_after_the_second_batch_needs_no_second_capture(setup):
    four = setup['batches'][:4]
    eager = _train(setup, 'adam', four, False, milestones=[2])
    graph = _train(setup, 'adam', four, True, milestones=[2])
    s = graph['stepper']
    assert (s.captures, s.replays, s.eager_steps) == (1, 3, 1)
    assert graph['opt'].param_groups[0]['lr'] == 5e-4
    _assert_same(graph, eager)
    plain = _train(setup, 'adam', four, False)
    assert not po.bitwise_equal(next(plain['model'].parameters()), next(eager['model'].parameters()))


def test_refusals(setup):
    cfg = setup['cfg']
    m = _module(setup['case'])
    factory = MultiLossFactory(cfg)
    with pytest.raises(TypeError, match='litepose_amd.optim'):
        CapturedStep(cfg, m, factory, torch.optim.Adam(m.parameters(), lr=1e-3))
    opt = optim.Adam(m.parameters(), lr=1e-3)
    m.eval()
    with pytest.raises(ValueError, match='training mode'):
        CapturedStep(cfg, m, factory, opt)
    m.train()
    with pytest.raises(ValueError, match='teacher'):
        do_train(cfg, m, iter(setup['batches'][:1]), factory, opt, 0, lambda x: None, None, True)
    with pytest.raises(TypeError):
        do_train(cfg, m, iter(setup['batches'][:1]), factory, torch.optim.SGD(m.parameters(), lr=1e-3), 0, None, None, True)
    for p in m.parameters():
        assert p.grad is None                                  # nothing ran
