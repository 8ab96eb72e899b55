"""The census of the training path's kernel forms, without a device: every form (tests/_train_forms.py) that a training step
of any zoo architecture reaches -- each at its own image size, with 14 and with 17 joints, at the batch sizes
tools/time_train_step.py measures -- is the form of a case of tests/test_gpu_train_forms.py, each of whose rows has the form
its table claims.  The forms come from the library's own host queries (lp_pw_tile_choice, the workspace sizes), so a
change of a launcher's selection that moves a real shape onto an untested form fails here, on a machine without a GPU.

A form that only a shape too large for a quick test has is named in UNSHRINKABLE with its reason (at most three)."""
import re

import pytest

import _train_forms as FM
import test_gpu_layer_grad as LG
import test_gpu_train_forms as GT
from litepose_amd import _native as nv
from litepose_amd import arch_zoo, config

BATCHES = (16, 64)
JOINTS = (14, 17)

UNSHRINKABLE = {
    # stride-2 forward with two tiles per wave needs N * C * tiles >= 65536, and an output plane of whole 16 x 16 tiles an
    # input plane of 32 x 32 at least: 65536 * 1024 floats, 256 MiB per tensor.  Both halves are covered apart: the
    # two-tile loop at (7, 2, 8, 8192, 4, 4), whole stride-2 tiles at (7, 2, 4, 9, 32, 32).
    ('dw', 7, 2, 'dwvec2', 'tiles<=4', 'whole', 'Cfull', 'slices'): 'N * C * tiles >= 65536 on whole 16 x 16 output tiles',
}


def _key(kind, text):
    return (kind,) + tuple(int(t) if re.fullmatch(r'\d+', t) else t for t in text.split())


def _case_forms():
    """-> [(case, claimed keys, the keys it has)] over every table of the GPU module"""
    rows = []
    for (n, c, h, w), claim in GT.BN_CASES:
        for res in (False, True):
            rows.append((('bn', n, c, h, w, res), [_key('bn', claim) + ('res' if res else 'plain',)], [FM.bn_form(n, c, h, w, res)]))
    for (ci, co, n, h, w), claims in GT.PW_CASES + GT.PW_ODD_CASES:
        has = [FM.pw_mm_form(n, ci, co, h, w, 'fwd'), FM.pw_mm_form(n, co, ci, h, w, 'dx'), FM.pw_dw_form(n, ci, co, h, w)]
        rows.append((('pw', ci, co, n, h, w), [_key(t.split()[0], t.split(None, 1)[1]) for t in claims], has))
    for (k, s, c, n, h, w), claim in GT.DW_CASES:
        rows.append((('dw', k, s, c, n, h, w), [_key('dw', claim)], [FM.dw_form(n, c, h, w, k, s)]))
    for (ca, cb, co, n, h, w), claim in GT.DECONV_CASES:
        rows.append((('deconv', ca, cb, co, n, h, w), [_key('deconv', claim)], [FM.deconv_form(n, ca, cb, co, h, w)]))
    for (n, h, w), claim in GT.STEM_CASES:
        rows.append((('stem', n, h, w), [_key('stem', claim)], [FM.stem_form(n, h, w)]))
    return rows


@pytest.fixture(scope='module')
def reached():
    """form key -> the first (architecture, joints, batch, layer call) that reaches it"""
    got = {}
    for name in arch_zoo.names():
        arch = arch_zoo.get(name)
        for joints in JOINTS:
            cfg = config.get_cfg()
            cfg.MODEL.NUM_JOINTS = joints
            shapes = FM.calls(cfg, arch, int(arch['img_size']))
            assert {s[0] for s in shapes} == {'pw', 'dw', 'bn', 'stem', 'deconv'}, name
            if joints == 17:
                assert any(s[0] == 'pw' and s[2] == 17 for s in shapes) and any(s[0] == 'pw' and s[2] == 34 for s in shapes)
            for n in BATCHES:
                for shape in shapes:
                    for key in FM.call_forms(shape, n):
                        got.setdefault(key, (name, joints, n, shape))
    return got


def test_the_zoo_is_walked(reached):
    assert len(arch_zoo.names()) == 7
    kinds = {k[0] for k in reached}
    assert kinds == {'bn', 'pw', 'pwdw', 'dw', 'deconv', 'stem'}
    # what the suite never ran before this census: more than one BatchNorm slice, NB 2 and 3, an odd K, Cin > 128
    assert not any(k[0] == 'bn' and k[2] == 'one' for k in reached), 'no zoo BatchNorm is single-slice at batch 16 or 64'
    assert {k[2] for k in reached if k[0] == 'pw'} == {1, 2, 3}
    assert any(k[0] == 'pw' and k[4] == 'Kodd' for k in reached) and any(k[0] == 'pwdw' and k[3] == 'z>0' for k in reached)


def test_every_form_the_zoo_reaches_has_a_case(reached):
    covered = set()
    for _, _, has in _case_forms():
        covered.update(has)
    missing = {k: v for k, v in reached.items() if k not in covered and k not in UNSHRINKABLE}
    assert not missing, '\n'.join('%s  first reached by %s' % kv for kv in missing.items())
    assert len(UNSHRINKABLE) <= 3
    for k in UNSHRINKABLE:
        assert k in reached and k not in covered, ('no longer an exception', k)


def test_each_case_has_the_form_it_claims():
    for case, claims, has in _case_forms():
        assert claims and all(c in has for c in claims), (case, claims, has)


def test_the_new_cases_reach_what_the_issue_names():
    has = set()
    for _, _, h in _case_forms():
        has.update(h)
    pw = [k for k in has if k[0] == 'pw']
    for what in ('fwd', 'dx'):
        assert {k[2] for k in pw if k[1] == what} == {1, 2, 3}, what
        assert {k[3] for k in pw if k[1] == what} == {1, 2, 4}, what
        assert any(k[4] == 'Kodd' for k in pw if k[1] == what) and any(k[6] == 'cbrag' for k in pw if k[1] == what)
    assert any(k[0] == 'pwdw' and k[2] == 'ragged' and k[3] == 'z>0' for k in has)
    bn = [k for k in has if k[0] == 'bn']
    assert {k[1] for k in bn} == {'vec', 'scalar'} and {k[2] for k in bn} == {'several', 'cap'}
    assert {k[4] for k in bn} == {'wide', 'even', 'rem'} and {k[3] for k in bn} == {'two', 'many'}
    assert {FM.bn_slices(n, c, h * w) for (n, c, h, w), _ in GT.BN_CASES} >= {2, 3, 4, 64}          # a cap below 64 among them
    inside = [c for c, _ in GT.BN_CASES if FM.bn_inside_plane(*c)]
    assert GT.BN_CASES[0][0] in inside and len(inside) >= 3
    for (n, c, h, w), _ in GT.BN_CASES:
        vec, units, S, chunk = FM.bn_geometry(n, c, h * w)
        assert S > 1 and chunk > 256, (n, c, h, w)            # partials to combine, more than one step per lane
    dw = [k for k in has if k[0] == 'dw']
    assert {(k[1], k[2]) for k in dw} == {(k_, s) for k_ in (3, 5, 7) for s in (1, 2)}
    assert {k[3] for k in dw} == {'pair16', 'pairvec', 'pairscalar', 'dwvec', 'dwscalar', 'dwvec2'}
    assert any(k[6] == 'Crag' for k in dw)


def test_the_parent_pointwise_cases_all_run_nb_1():
    """tests/test_gpu_layer_grad.py's PW_CH x PW_PLANES: careful arithmetic, one tile height -- not coverage of NB 2 / 3"""
    for ci, co in LG.PW_CH:
        assert ci % 2 == 0 and co % 2 == 0
        for n, h, w in LG.PW_PLANES:
            fwd, dx = FM.pw_tile(n, ci, co, h * w), FM.pw_tile(n, co, ci, h * w)
            assert fwd[0] == 1 and dx[0] == 1 and fwd[1] == dx[1] and fwd[1] in (1, 4), (ci, co, n, h, w, fwd, dx)
    for c in (3, 32):
        for n, h, w in ((2, 1, 1), (3, 5, 7), (2, 32, 32)):
            assert FM.bn_slices(n, c, h * w) == 1


def test_tile_choice_query():
    """declared in the header, bound by _native.py, host only: no pointer argument, refusals before any arithmetic"""
    with open(FM.ROOT + '/include/litepose_amd.h') as f:
        hdr = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    m = re.search(r'int\s+lp_pw_tile_choice\s*\(([^)]*)\)', hdr)
    assert m and '*' not in m.group(1) and m.group(1).count('int') == 6
    assert 'lp_pw_tile_choice' in nv.EXPORTS
    L = nv.lib()
    for bad in ((0, 8, 0, 8, 4, 0), (1, 0, 0, 8, 4, 0), (1, 8, -1, 8, 4, 0), (1, 8, 0, 0, 4, 0), (1, 8, 0, 8, 0, 0)):
        assert L.lp_pw_tile_choice(*bad) == -1, bad
    # PXV follows the plane alone; NB never exceeds the 32-channel blocks there are
    for hw, pxv in ((64, 4), (6, 2), (70, 2), (35, 1)):
        assert L.lp_pw_tile_choice(3, 8, 0, 8, hw, 0) % 16 == pxv
    for n in (1, 4, 64):
        for cout in (8, 32, 33, 64):
            v = L.lp_pw_tile_choice(n, 4, 0, cout, 128 * 128, 0)
            assert 1 <= v // 16 <= min(3, (cout + 31) // 32) and v % 16 == 4
    # two sources and a residual are part of the model's inputs: accepted, same range
    v = L.lp_pw_tile_choice(64, 48, 48, 96, 64 * 64, 1)
    assert v // 16 in (1, 2, 3) and v % 16 == 4
