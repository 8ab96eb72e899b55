#!/usr/bin/env python
"""Golden fixture of the architecture search's host side (tests/golden/golden_search.json).  Build container only (needs
the reference checkout).  Runs the REAL reference code:

  * lib/dataset/transforms/transforms.py (RandomAffineTransform, RandomHorizontalFlip) with stub ``cv2`` / ``torchvision``
    modules: the stub ``warpAffine`` records the matrix it is handed; for 3 seeds x 8 source sizes the fixture stores every
    ``mat_input`` and flip decision;
  * arch_manager.py + arch_search/evolution.py with the stub predictors of tests/_search_stubs.py: for 2 seeds the
    (accuracy, sample, efficiency) of every candidate in evaluation order and the returned best, population_size = 6,
    max_time_budget = 3.  The run itself shows that the constraint lets the reference's rejection loops end.
"""
import contextlib
import importlib.util
import io
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = '/root/reference'

import _search_stubs as stubs  # noqa: E402

SIZES = [(37, 53), (64, 48), (16, 16), (90, 31), (480, 640), (427, 640), (333, 500), (9, 301)]     # h, w (short side >= 7: below, the reference's own translate draw has an empty range)
AUG_CASES = [       # seed, input_size, then the keyword parameters of RandomAffineTransform / RandomHorizontalFlip
    dict(seed=0, input_size=256, max_rotation=30, min_scale=0.75, max_scale=1.5, scale_type='short', max_translate=40,
         flip_prob=0.5),
    dict(seed=1, input_size=448, max_rotation=30, min_scale=0.75, max_scale=1.5, scale_type='short', max_translate=40,
         flip_prob=0.5),
    dict(seed=2, input_size=96, max_rotation=45, min_scale=0.5, max_scale=1.25, scale_type='long', max_translate=0,
         flip_prob=0.3),
]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def transforms_golden():
    recorded = []

    def warp_affine(src, mat, dsize, *a, **k):
        recorded.append((src.ndim, np.array(mat, np.float64).copy(), tuple(dsize)))
        out = np.zeros((dsize[1], dsize[0]) + src.shape[2:], src.dtype)
        out[:, 0] = 1                      # a mark in the first column: it tells whether the flip mirrored the image
        return out

    cv2 = types.ModuleType('cv2')
    cv2.warpAffine = warp_affine
    tv = types.ModuleType('torchvision')
    tvt = types.ModuleType('torchvision.transforms')
    tvt.functional = types.ModuleType('torchvision.transforms.functional')
    tv.transforms = tvt
    saved = {k: sys.modules.get(k) for k in ('cv2', 'torchvision', 'torchvision.transforms',
                                             'torchvision.transforms.functional')}
    sys.modules.update({'cv2': cv2, 'torchvision': tv, 'torchvision.transforms': tvt,
                        'torchvision.transforms.functional': tvt.functional})
    try:
        T = _load('ref_dataset_transforms', os.path.join(REF, 'lib/dataset/transforms/transforms.py'))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    cases = []
    for case in AUG_CASES:
        S = case['input_size']
        outs = [S // 4, S // 2]
        aff = T.RandomAffineTransform(S, outs, case['max_rotation'], case['min_scale'], case['max_scale'],
                                      case['scale_type'], case['max_translate'])
        flip = T.RandomHorizontalFlip(list(range(14)), outs, case['flip_prob'])
        tf = T.Compose([aff, flip])
        np.random.seed(case['seed'])
        random.seed(case['seed'])
        mats, flips = [], []
        for h, w in SIZES:
            del recorded[:]
            image = np.zeros((h, w, 3), np.uint8)
            mask = [np.ones((o, o), np.float32) for o in outs]
            joints = [np.zeros((1, 14, 3)) for _ in outs]
            image, mask, joints = tf(image, mask, joints)
            ndim, mat, dsize = recorded[-1]
            assert ndim == 3 and dsize == (S, S) and len(recorded) == 3, recorded
            mats.append(mat.reshape(-1).tolist())
            flips.append(bool(image[0, 0, 0] == 0))
        cases.append(dict(case, sizes=SIZES, mat_input=mats, flip=flips))
    return cases


def evolution_golden():
    sys.path.insert(0, REF)              # evolution.py: ``from arch_manager import ArchManager``
    try:
        _load('arch_manager', os.path.join(REF, 'arch_manager.py'))
        evo = _load('ref_evolution', os.path.join(REF, 'arch_search/evolution.py'))
    finally:
        sys.path.remove(REF)
    NS = types.SimpleNamespace
    cfg = NS(MODEL=NS(EXTRA=NS(NUM_DECONV_FILTERS=[64, 48, 32])))
    runs = []
    for seed in stubs.EVOLUTION_SEEDS:
        acc = stubs.StubAccuracy()
        finder = evo.EvolutionFinder(cfg, stubs.StubEfficiency(), acc, population_size=stubs.POPULATION_SIZE,
                                     max_time_budget=stubs.MAX_TIME_BUDGET)
        finder.set_efficiency_constraint(stubs.CONSTRAINT)
        random.seed(seed)
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            best = finder.run_evolution_search()
        assert len(acc.calls) == stubs.POPULATION_SIZE * (1 + stubs.MAX_TIME_BUDGET)
        runs.append(dict(seed=seed, history=[list(c) for c in acc.calls], best=list(best)))
    return runs


def main():
    out = dict(transforms=transforms_golden(), evolution=evolution_golden(),
               population_size=stubs.POPULATION_SIZE, max_time_budget=stubs.MAX_TIME_BUDGET, constraint=stubs.CONSTRAINT)
    path = os.path.join(HERE, 'golden_search.json')
    with open(path, 'w') as f:
        json.dump(out, f)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
