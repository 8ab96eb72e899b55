"""``do_train(..., graph=True)`` / ``core.trainer.CapturedStep`` against the eager loop on the tiny architecture and batch
shape of tests/_train_net_case.py (N = 2, 64 x 64): from the same initial state the two perform the same sequence of updates,
so every parameter, every BatchNorm buffer (``num_batches_tracked`` included), every optimizer state tensor, every
``p.grad`` and the returned dict are the same bits -- the library's calls give the same bits launched or replayed
(DESIGN.md 4f), and torch's adds and means in between are elementwise."""
import random

import numpy as np
import pytest
import torch

import _poison as po
import _train_net_case as TC
from litepose_amd import config, optim
from litepose_amd.core import inference
from litepose_amd.core.loss import MultiLossFactory
from litepose_amd.core.trainer import CapturedStep, do_train
from litepose_amd.dataset import LabelledSet
from litepose_amd.models import pose_mobilenet as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def setup():
    cfg = config.get_cfg()
    cfg.DATASET.INPUT_SIZE, cfg.DATASET.OUTPUT_SIZE, cfg.DATASET.MAX_NUM_PEOPLE = 64, [16, 32], 6
    J = cfg.DATASET.NUM_JOINTS
    rng = np.random.RandomState(3)
    sizes = [(40, 56), (33, 47), (64, 64), (48, 36), (50, 50), (37, 61), (64, 40), (45, 45), (52, 38)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    joints = []
    for (h, w), people in zip(sizes, (2, 1, 3, 6, 2, 4, 1, 3, 2)):
        j = np.zeros((people, J, 3))
        j[:, :, 0], j[:, :, 1] = rng.uniform(0, w, (people, J)), rng.uniform(0, h, (people, J))
        j[:, :, 2] = rng.choice([0, 1, 2], (people, J))
        joints.append(j)
    ls = LabelledSet(images, joints, inference.flip_index_for(cfg)[:J], max_num_people=6, sigma=cfg.DATASET.SIGMA)
    # nine images in batches of two: four equal-shaped batches and a fifth with one image; materialised once and shared
    batches = list(ls.batches(64, [16, 32], 2, np.random.RandomState(8), random.Random(8)))
    assert [int(b[0].shape[0]) for b in batches] == [2, 2, 2, 2, 1]
    return dict(cfg=cfg, case=TC.load(), batches=batches)


def _module(case):
    m = pm.get_train_net(config.get_cfg(), TC.ARCH, backend='native')
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case['sd'].items()}, strict=False)
    return m.cuda().train()


def _clone(batch):
    return tuple([t.clone() for t in part] if isinstance(part, list) else part.clone() for part in batch)


def _loader(batches, scribble):
    """Fresh copies of the batches; ``scribble``: the previous batch's tensors are overwritten once the caller has come
    back for the next one."""
    prev = None
    for b in batches:
        if prev is not None and scribble:
            for part in prev:
                for t in (part if isinstance(part, list) else [part]):
                    t.fill_(7) if t.is_floating_point() else t.zero_()
        prev = _clone(b)
        yield prev


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


def _assert_same(a, b):
    sa, sb = a['model'].state_dict(), b['model'].state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert po.bitwise_equal(sa[k], sb[k]), ('state', k, po.first_difference(sa[k], sb[k]))
    for (k, p), (_, q) in zip(a['model'].named_parameters(), b['model'].named_parameters()):
        assert p.grad is not None and q.grad is not None and po.bitwise_equal(p.grad, q.grad), ('grad', k)
    oa, ob = a['opt'].state_dict(), b['opt'].state_dict()
    assert sorted(oa['state']) == sorted(ob['state']) and len(oa['state']) == len(list(a['model'].parameters()))
    for i in oa['state']:
        for name, v in oa['state'][i].items():
            assert po.bitwise_equal(v, ob['state'][i][name]), ('optimizer', i, name)
    assert a['got'] == b['got'], (a['got'], b['got'])
    assert a['got']['heatmaps'][0] is not None and a['got']['push'][0] is not None


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
