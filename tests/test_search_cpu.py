"""The host side of the architecture search without a GPU (litepose_amd.arch_search, litepose_amd.dataset.calibration):
the augmentation draws and the evolutionary search against what the reference's own code produced
(tests/golden/golden_search.json, written by tests/golden/gen_golden_search.py), the multiply-accumulate count against a
brute-force count over the sub-network's weight shapes, every host refusal of lp_augment_batch_v with fake pointers that
are never dereferenced, and the command line."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import _search_stubs as stubs
import _supernet_ref as sref
from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_search.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------ dataset.calibration
def test_draw_transform_replays_the_reference(golden):
    from litepose_amd.dataset.calibration import draw_transform
    assert len(golden['transforms']) == 3
    for case in golden['transforms']:
        assert len(case['sizes']) == 8
        np_rng, py_rng = np.random.RandomState(case['seed']), random.Random(case['seed'])
        aug = {k: case[k] for k in ('max_rotation', 'min_scale', 'max_scale', 'scale_type', 'max_translate', 'flip_prob')}
        for (h, w), want, flip in zip(case['sizes'], case['mat_input'], case['flip']):
            mat, got_flip = draw_transform(h, w, case['input_size'], np_rng, py_rng, **aug)
            want = np.array(want).reshape(2, 3)
            assert mat.shape == (2, 3) and mat.dtype == np.float64
            err = np.abs(mat - want) / np.maximum(np.abs(want), 1e-300)
            assert err.max() <= 1e-12, (case['seed'], h, w, mat, want)
            assert got_flip is flip, (case['seed'], h, w)


def test_draw_transform_defaults_and_global_generators(golden):
    """The six defaults are supermobile.yaml's (the first golden case is drawn with them) and the generators default to
    the global ones."""
    from litepose_amd.dataset.calibration import AUG_DEFAULTS, draw_transform
    case = golden['transforms'][0]
    assert {k: case[k] for k in AUG_DEFAULTS} == AUG_DEFAULTS
    np_state, py_state = np.random.get_state(), random.getstate()
    try:
        np.random.seed(case['seed'])
        random.seed(case['seed'])
        for (h, w), want, flip in zip(case['sizes'], case['mat_input'], case['flip']):
            mat, got_flip = draw_transform(h, w, case['input_size'])
            assert np.allclose(mat.reshape(-1), want, rtol=1e-12, atol=0) and got_flip is flip
    finally:
        np.random.set_state(np_state)
        random.setstate(py_state)
    with pytest.raises(ValueError):
        draw_transform(32, 32, 64, np.random.RandomState(0), random.Random(0), scale_type='area')


def test_aug_desc_layout():
    from litepose_amd import _native as nv
    from litepose_amd.dataset import calibration as cal
    assert C.sizeof(nv.LpAugDesc) == 72 == cal.AUG_DESC_DTYPE.itemsize
    for f in ('src_offset', 'H', 'W', 'minv', 'flip', 'reserved'):
        assert getattr(nv.LpAugDesc, f).offset == cal.AUG_DESC_DTYPE.fields[f][1], f


# ------------------------------------------------------------------ arch_search.evolution
def _finder(seed, use_globals=False):
    from litepose_amd import config
    from litepose_amd.arch_search import EvolutionFinder
    acc = stubs.StubAccuracy()
    kw = {} if use_globals else dict(py_rng=random.Random(seed), np_rng=np.random.RandomState(seed))
    f = EvolutionFinder(config.get_cfg(), stubs.StubEfficiency(), acc, population_size=stubs.POPULATION_SIZE,
                        max_time_budget=stubs.MAX_TIME_BUDGET, **kw)
    f.set_efficiency_constraint(stubs.CONSTRAINT)
    return f, acc


def _as_json(x):
    return json.loads(json.dumps(x))


def test_evolution_reproduces_the_reference_history(golden, capsys):
    assert golden['population_size'] == stubs.POPULATION_SIZE == 6 and golden['max_time_budget'] == stubs.MAX_TIME_BUDGET == 3
    assert golden['constraint'] == stubs.CONSTRAINT and [r['seed'] for r in golden['evolution']] == list(stubs.EVOLUTION_SEEDS)
    for run in golden['evolution']:
        f, acc = _finder(run['seed'])
        best = f.run_evolution_search()
        assert _as_json([list(c) for c in acc.calls]) == run['history'], run['seed']
        assert _as_json(list(best)) == run['best'], run['seed']
        # the finder's own record: one list per generation, in evaluation order
        assert [len(g) for g in f.history] == [6] * 4
        assert _as_json([list(c) for g in f.history for c in g]) == run['history']
        assert all(c[2] <= stubs.CONSTRAINT for c in acc.calls)
    assert capsys.readouterr().out == ''                              # no prints unless verbose


def test_evolution_defaults(golden):
    """The reference's keyword defaults, and the global generators when none are injected."""
    from litepose_amd import config
    from litepose_amd.arch_search import EvolutionFinder
    f = EvolutionFinder(config.get_cfg(), None, None)
    assert (f.mutate_prob, f.population_size, f.max_time_budget, f.parent_ratio, f.mutation_ratio) == \
        (0.1, 40, 40, 0.25, 0.5)
    run = golden['evolution'][0]
    np_state, py_state = np.random.get_state(), random.getstate()
    try:
        random.seed(run['seed'])
        np.random.seed(run['seed'])
        f, acc = _finder(run['seed'], use_globals=True)
        best = f.run_evolution_search()
    finally:
        np.random.set_state(np_state)
        random.setstate(py_state)
    assert _as_json([list(c) for c in acc.calls]) == run['history'] and _as_json(list(best)) == run['best']


def test_evolution_rejection_loops_reject():
    """The constraint of the fixture is one the samplers really run into: a finder that accepts everything evaluates
    other candidates than the constrained one from the same seed."""
    f, acc = _finder(stubs.EVOLUTION_SEEDS[0])
    f.run_evolution_search()
    g, acc_free = _finder(stubs.EVOLUTION_SEEDS[0])
    g.set_efficiency_constraint(1e9)
    g.run_evolution_search()
    assert any(c[2] > stubs.CONSTRAINT for c in acc_free.calls)
    assert [c[1] for c in acc.calls] != [c[1] for c in acc_free.calls]


# ------------------------------------------------------------------ arch_search.eff_pred
def _brute_force_macs(sd, arch):
    """Every 4-D weight of the sub-network's state dict: out_pixels * Cout * Cin/groups * k * k, the plane sizes walked
    as the forward does (oracle/spec.derive names the strides)."""
    from oracle import spec
    d = spec.derive(arch)
    R = arch['img_size']

    def conv(key, out_hw, transposed=False):
        w = sd[key]                                  # Conv2d [Cout, Cin/groups, k, k]; ConvTranspose2d [Cin, Cout, k, k]
        cout, cin_g = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
        return out_hw * out_hw * cout * cin_g * w.shape[2] * w.shape[3]

    h = R // 2
    total = conv('first.0.0.weight', h) + conv('first.1.0.weight', h) + conv('first.2.weight', h)
    sizes = [h]
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            total += conv(p + '.inv.0.weight', h)
            h = h // blk['stride']
            total += conv(p + '.depth_conv.0.weight', h) + conv(p + '.point_conv.0.weight', h)
        sizes.append(h)
    h = sizes[-1]
    for i in range(3):
        h *= 2
        total += conv('deconv_refined.%d.weight' % i, h, True) + conv('deconv_raw.%d.weight' % i, h, True)
        if i > 0:
            for which in ('final_refined', 'final_raw'):
                total += conv('%s.%d.conv.0.weight' % (which, i - 1), h) + conv('%s.%d.conv.3.weight' % (which, i - 1), h)
    n4 = sum(1 for v in sd.values() if v.dim() == 4)
    return total, n4


def test_efficiency_equals_a_brute_force_count():
    from litepose_amd import config
    from litepose_amd.arch_search import EfficiencyEvaluator
    from litepose_amd.models.pose_supermobilenet import SuperLitePose
    cfg = config.get_cfg()
    sup = SuperLitePose(cfg)
    sup.load_state_dict(sref.make_state_dict(seed=7))
    eff = EfficiencyEvaluator(cfg)
    seen = set()
    for arch in (sref.fixed_sample(256, 0.5), sref.fixed_sample(512, 1.0), sref.mixed_arch()):
        want, n4 = _brute_force_macs(sup.sub_state_dict(arch), arch)
        assert len(eff.layers(arch)) == n4                         # every convolution, nothing else
        assert eff.macs(arch) == want
        assert eff.predict_eff(arch) == want / 1e9
        seen.add(want)
    assert len(seen) == 3
    # hand count of the stem at 256: 128 * 128 * (32 * 3 * 9 + 32 * 9 + 16 * 32)
    stem = sum(oh * ow * co * ci * k * k for n, oh, ow, co, ci, k in eff.layers(sref.fixed_sample(256, 0.5))[:3])
    assert stem == 128 * 128 * (32 * 27 + 32 * 9 + 16 * 32)


# ------------------------------------------------------------------ the C entry point
def test_augment_entry_point_validates_before_any_device_call():
    from litepose_amd import _native as nv
    lib = nv.lib()
    assert 'lp_augment_batch_v' in nv.EXPORTS
    BAD = -1                                     # LP_ERR_INVALID_ARG
    fake = C.c_void_p(0x1000)                    # never dereferenced: every call below is refused first
    mean = (C.c_float * 3)(0.485, 0.456, 0.406)
    std = (C.c_float * 3)(0.229, 0.224, 0.225)
    zstd = (C.c_float * 3)(0.229, 0.0, 0.225)
    av = lib.lp_augment_batch_v
    assert av(None, 100, fake, 1, 8, 8, mean, std, fake, fake, None) == BAD
    assert av(fake, 100, None, 1, 8, 8, mean, std, fake, fake, None) == BAD
    assert av(fake, 100, fake, 1, 8, 8, None, std, fake, fake, None) == BAD
    assert av(fake, 100, fake, 1, 8, 8, mean, None, fake, fake, None) == BAD
    assert av(fake, 100, fake, 1, 8, 8, mean, std, None, None, None) == BAD          # neither output
    assert b'no output' in lib.lp_last_error()
    assert av(fake, 0, fake, 1, 8, 8, mean, std, None, fake, None) == BAD            # empty source buffer
    for n in (0, -1, 65536):
        assert av(fake, 100, fake, n, 8, 8, mean, std, None, fake, None) == BAD, n
    for hd, wd in ((0, 8), (8, 0), (32768, 8), (8, 32768), (-3, 8)):
        assert av(fake, 100, fake, 1, hd, wd, mean, std, fake, None, None) == BAD, (hd, wd)
    assert av(fake, 100, fake, 1, 8, 8, mean, zstd, None, fake, None) == BAD


# ------------------------------------------------------------------ python -m litepose_amd.arch_search
def test_module_help_exits_zero():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'litepose_amd.arch_search', '--help'], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    for word in ('--cfg', '--supernet', '--calib-images', '--search-images', '--annotations', '--constraint'):
        assert word in r.stdout, word


def test_module_argument_parsing():
    from litepose_amd.arch_search.__main__ import parse_args
    a = parse_args(['--cfg', 'x.yaml', '--supernet', 's.pth', '--calib-images', 'c', '--search-images', 'i',
                    '--annotations', 'a.json', '--constraint', '1.5', 'TEST.FLIP_TEST', 'False'])
    assert (a.cfg, a.supernet, a.calib_images, a.search_images, a.annotations) == ('x.yaml', 's.pth', 'c', 'i', 'a.json')
    assert a.constraint == 1.5 and a.opts == ['TEST.FLIP_TEST', 'False']
    assert (a.population_size, a.max_time_budget, a.out) == (40, 40, os.path.join('arch_search', 'result'))
    with pytest.raises(SystemExit):
        parse_args(['--supernet', 's.pth'])                       # --cfg and the data paths are required
