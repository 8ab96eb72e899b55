"""The candidate loop of the architecture search on the device (litepose_amd.arch_search): AccuracyEvaluator against the
hand-written chain it stands for (CalibrationSet.batches -> SuperLitePose.calibrate on a copy -> PoseEngine.evaluate with a
KeypointEvaluator), what it leaves behind, and a small evolutionary search through it.  Random weights: the AP itself says
nothing about pose estimation here (it may be 0); the ranking logic is pinned on the CPU (tests/test_search_cpu.py), this
file pins the device chain."""
import copy
import gc
import random

import numpy as np
import pytest
import torch

import _poison as po
import _supernet_ref as sref

pytestmark = pytest.mark.gpu

SEED, CALIB_BATCH, EVAL_BATCH = 17, 4, 4
CALIB_SIZES = [(37, 53), (64, 48), (16, 16), (90, 31), (48, 48), (33, 70), (80, 60), (57, 57)]          # h, w
SEARCH_SIZES = [(60, 80), (80, 60), (64, 64), (45, 90), (60, 80), (72, 50), (64, 64), (96, 40)]
SEARCH_IDS = [40, 10, 30, 20, 80, 60, 70, 50]


def _archs():
    mixed = sref.mixed_arch()
    mixed['img_size'] = 96
    return [('half64', sref.fixed_sample(64, 0.5)), ('mixed96', mixed)]


def _supernet(cfg):
    from litepose_amd.models.pose_supermobilenet import SuperLitePose
    sd = sref.make_state_dict(seed=1234)
    for k in sd:                             # louder heads: noise peaks above the detection threshold
        if k.endswith('.conv.3.weight'):
            sd[k] = sd[k] * 8.0
    return SuperLitePose(cfg).load_state_dict(sd)


def _hand_chain(cfg, supernet, cal, images, ids, gt, arch):
    """What predict_acc stands for, written out."""
    from litepose_amd import coco_eval, config
    from litepose_amd.engine import PoseEngine
    from litepose_amd.models.pose_supermobilenet import SuperLitePose
    work = SuperLitePose(cfg).load_state_dict(supernet.state_dict())
    batches = cal.batches(arch['img_size'], CALIB_BATCH, np.random.RandomState(SEED), random.Random(SEED))
    sd = work.calibrate(arch, batches)
    eng = PoseEngine(config.apply_arch(cfg.clone(), arch), arch, sd)
    ev = coco_eval.KeypointEvaluator(gt)
    results = eng.evaluate(images, image_ids=ids, batch_size=EVAL_BATCH, evaluator=ev)
    stats = ev.summarize()
    eng.close()
    return sd, stats, results


@pytest.fixture(scope='module')
def world():
    from litepose_amd import coco_eval, config
    from litepose_amd.dataset.calibration import CalibrationSet
    cfg = config.get_cfg()
    rng = np.random.default_rng(3)
    calib = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in CALIB_SIZES]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SEARCH_SIZES]
    supernet = _supernet(cfg)
    cal = CalibrationSet(calib)
    # synthetic ground truth: two persons per image, joints spread over the image
    J = 14
    ann_ids, kpts, area, bbox = [], [], [], []
    for i, (h, w) in zip(SEARCH_IDS, SEARCH_SIZES):
        for p in range(2):
            k = np.zeros((J, 3))
            k[:, 0] = rng.uniform(0, w, J)
            k[:, 1] = rng.uniform(0, h, J)
            k[:, 2] = rng.integers(0, 3, J)
            ann_ids.append(i)
            kpts.append(k)
            area.append(float(w * h) / 2)
            bbox.append((0.0, 0.0, float(w), float(h)))
    gt = coco_eval.GroundTruth.from_arrays(SEARCH_IDS, ann_ids, np.stack(kpts), area, bbox)
    before = supernet.state_dict()
    hand = {name: _hand_chain(cfg, supernet, cal, images, SEARCH_IDS, gt, arch) for name, arch in _archs()}
    return dict(cfg=cfg, supernet=supernet, before=before, cal=cal, images=images, gt=gt, hand=hand)


def _evaluator(world, **kw):
    from litepose_amd import coco_eval
    from litepose_amd.arch_search import AccuracyEvaluator
    return AccuracyEvaluator(world['cfg'], world['supernet'], world['cal'], world['images'], SEARCH_IDS,
                             lambda: coco_eval.KeypointEvaluator(world['gt']), batch_size=CALIB_BATCH, seed=SEED,
                             eval_batch_size=EVAL_BATCH, **kw)


def _same_tensors(a, b):
    assert list(a) == list(b)
    for k in a:
        assert po.bitwise_equal(a[k], b[k]), k


def test_predict_acc_is_the_hand_written_chain(world):
    acc = _evaluator(world)
    for name, arch in _archs():
        sd, stats, results = world['hand'][name]
        print(name, 'AP', stats['AP'], 'detections', len(results))
        arch_in = copy.deepcopy(arch)
        ap = acc.predict_acc(arch)
        assert arch == arch_in                                     # the candidate is not edited
        assert ap == stats['AP'] and acc.last_stats == stats, name
        _same_tensors(acc.last_state_dict, sd)
        assert set(acc.last_timing) >= {'loader_s', 'calibrate_s', 'engine_s', 'evaluate_s', 'total_s'}
        # calibration moved the statistics: the chain is not comparing two untouched copies
        sub = world['supernet'].sub_state_dict(arch)
        moved = [k for k in sd if k.endswith('running_mean') and not torch.equal(sd[k], sub[k])]
        assert len(moved) > 10, name
    # the heads are loud enough for records to reach the evaluator in at least one candidate
    assert sum(len(world['hand'][n][2]) for n, _ in _archs()) > 0


def test_supernet_is_untouched_and_calls_are_deterministic(world):
    acc = _evaluator(world)
    name, arch = _archs()[0]
    a1 = acc.predict_acc(arch)
    sd1, st1 = acc.last_state_dict, acc.last_stats
    _same_tensors(world['supernet'].state_dict(), world['before'])
    # another candidate in between does not move what the first one starts from
    acc.predict_acc(_archs()[1][1])
    _same_tensors(world['supernet'].state_dict(), world['before'])
    a2 = acc.predict_acc(arch)
    assert a1 == a2 and st1 == acc.last_stats
    _same_tensors(sd1, acc.last_state_dict)
    assert sd1 is not acc.last_state_dict
    # another seed draws other augmentations: the statistics differ
    other = _evaluator(world)
    other.seed = SEED + 1
    other.predict_acc(arch)
    assert any(not torch.equal(sd1[k], other.last_state_dict[k]) for k in sd1 if k.endswith('running_var'))


class _Recording(object):
    """An accuracy predictor that notes the device memory around every candidate."""

    def __init__(self, inner):
        self.inner, self.after, self.peak = inner, [], []

    def predict_acc(self, arch):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ap = self.inner.predict_acc(arch)
        torch.cuda.synchronize()
        self.after.append(torch.cuda.memory_allocated())
        self.peak.append(torch.cuda.max_memory_allocated() - base)
        return ap


def test_smoke_search_releases_every_candidate(world):
    from litepose_amd.arch_search import EfficiencyEvaluator, EvolutionFinder
    rec = _Recording(_evaluator(world))
    eff = EfficiencyEvaluator(world['cfg'])
    finder = EvolutionFinder(world['cfg'], eff, rec, population_size=3, max_time_budget=1,
                             py_rng=random.Random(2), np_rng=np.random.RandomState(2))
    finder.set_efficiency_constraint(float('inf'))                 # admits every sample
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    gc.disable()                                                   # a collection must not be what frees a candidate
    try:
        best = finder.run_evolution_search()
    finally:
        gc.enable()
    members = [c for g in finder.history for c in g]
    assert len(members) == 6 == len(rec.after)
    assert any(best[1] is c[1] and best[0] == c[0] and best[2] == c[2] for c in members)
    assert best[0] == max(c[0] for c in finder.history[0])         # one generation: the best of the first population
    assert all(c[2] == eff.predict_eff(c[1]) for c in members)
    _same_tensors(world['supernet'].state_dict(), world['before'])
    # nothing accumulates: after any candidate no more is allocated than after the first plus one candidate's worth
    worth = max(rec.peak)
    print('allocated before', base, 'after each candidate', rec.after, 'peak of one candidate', rec.peak)
    assert worth > 0
    assert torch.cuda.memory_allocated() <= rec.after[0] + worth
    assert all(a <= rec.after[0] + worth for a in rec.after)
    # stronger than the bound above: a closed engine leaves nothing on the device, without waiting for a collection of
    # reference cycles.  1 MiB: far below the smallest buffer set of any candidate (their peaks are in the GiB)
    assert min(rec.peak) > 64 << 20
    assert all(a - base <= 1 << 20 for a in rec.after), (base, rec.after)
