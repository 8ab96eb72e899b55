"""What tests/test_gpu_captured_step.py and tests/test_gpu_train_lifecycle.py share: the tiny architecture of
tests/_train_net_case.py (N = 2 and N = 1, 64 x 64, MAX_NUM_PEOPLE 6) as batches materialised once, a module loaded with the
golden weights, a loader that hands out fresh copies, and the bitwise comparison of two runs.  A plain module, not a
conftest: the tests import it by name (tests/ is on sys.path under pytest)."""
import random

import numpy as np
import pytest
import torch

import _poison as po
import _train_net_case as TC
from litepose_amd import config
from litepose_amd.core import inference
from litepose_amd.dataset import LabelledSet
from litepose_amd.models import pose_mobilenet as pm


def make_cfg():
    cfg = config.get_cfg()
    cfg.DATASET.INPUT_SIZE, cfg.DATASET.OUTPUT_SIZE, cfg.DATASET.MAX_NUM_PEOPLE = 64, [16, 32], 6
    return cfg


@pytest.fixture(scope='module')
def setup():
    cfg = make_cfg()
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
    # and three batches of one image each, for the runs that keep two batch signatures alive
    ones = list(ls.batches(64, [16, 32], 1, np.random.RandomState(9), random.Random(9)))[:3]
    assert [int(b[0].shape[0]) for b in ones] == [1, 1, 1]
    return dict(cfg=cfg, case=TC.load(), batches=batches, ones=ones)


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


def _assert_same(a, b, every_parameter=True):
    """Two runs (dicts of ``model``, ``opt``, ``got``) hold the same bits: every parameter and buffer, every ``p.grad``,
    every optimizer state tensor, the returned dicts.  ``every_parameter``: each parameter has a gradient and optimizer
    state; False for the runs with frozen or held-out parameters, where the two must still agree on which ones have."""
    sa, sb = a['model'].state_dict(), b['model'].state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert po.bitwise_equal(sa[k], sb[k]), ('state', k, po.first_difference(sa[k], sb[k]))
    for (k, p), (_, q) in zip(a['model'].named_parameters(), b['model'].named_parameters()):
        if every_parameter or p.grad is not None or q.grad is not None:
            assert p.grad is not None and q.grad is not None and po.bitwise_equal(p.grad, q.grad), ('grad', k)
    oa, ob = a['opt'].state_dict(), b['opt'].state_dict()
    assert sorted(oa['state']) == sorted(ob['state'])
    if every_parameter:
        assert len(oa['state']) == len(list(a['model'].parameters()))
    for i in oa['state']:
        assert sorted(oa['state'][i]) == sorted(ob['state'][i]), ('optimizer', i)
        for name, v in oa['state'][i].items():
            assert po.bitwise_equal(v, ob['state'][i][name]), ('optimizer', i, name)
    assert a['got'] == b['got'], (a['got'], b['got'])
    assert a['got']['heatmaps'][0] is not None and a['got']['push'][0] is not None
