"""The custom census without a GPU (tests/_custom_space.py, tests/test_gpu_custom_census.py): closure over the kernel
census's NOT_REACHED table, the rows' target shapes against oracle.spec.derive, the golden file against the oracle."""
import os

import numpy as np
import pytest
import torch

import _custom_space as cs
import _simplenet_ref as snr
from oracle import net_ref, spec, synth
from test_kernel_census_cpu import source_tags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_custom.npz')
OPTION_KEYS = {'mb16', 'mb16_run', 'mb16_min', 'mbt', 'mbt_s2', 'mbconv2', 'mbtb', 'mbtb_s2', 'mbtd', 'pw3d',
               'headb', 'dwt', 'stem'}


def _expected():
    return set().union(*[set(r[7]) | set(r[8]) for r in cs.ROWS])


def test_every_not_reached_tag_is_launched_by_a_row_or_unreachable():
    """Every tag the kernel census excuses is now either expected by a custom row (launched and compared on the device)
    or in UNREACHABLE with the launcher's reason -- never both, never neither."""
    import test_gpu_kernel_census as kc
    exp = _expected()
    neither = sorted(t for t in kc.NOT_REACHED if t not in exp and t not in cs.UNREACHABLE)
    both = sorted(t for t in kc.NOT_REACHED if t in exp and t in cs.UNREACHABLE)
    assert not neither, ('NOT_REACHED tags no custom row expects and UNREACHABLE does not list', neither)
    assert not both, ('expected by a custom row and listed as unreachable', both)
    assert set(cs.UNREACHABLE) <= set(kc.NOT_REACHED), sorted(set(cs.UNREACHABLE) - set(kc.NOT_REACHED))


def test_unreachable_and_expected_tags_exist_in_the_sources():
    tags = source_tags()
    assert set(cs.UNREACHABLE) <= tags, sorted(set(cs.UNREACHABLE) - tags)
    assert _expected() <= tags, sorted(_expected() - tags)
    assert cs.FUSED_K7 <= tags, sorted(cs.FUSED_K7 - tags)
    for t in [t[0] for v in cs.TARGET.values() for t in v if t[0]] + [t for v in cs.FORBID.values() for s in v.values() for t in s]:
        assert t in tags, t
    for tag, why in cs.UNREACHABLE.items():
        assert len(why) >= 30, (tag, why)


def test_rows_are_well_formed():
    ids = [r[0] for r in cs.ROWS]
    assert len(ids) == len(set(ids))
    assert set(cs.TARGET) == set(ids)
    assert set(cs.FORBID) <= set(ids) and set(cs.F16_ROWS) <= set(ids) and set(cs.INVARIANCE_ROWS) <= set(ids)
    for rid, arch, H, W, N, flip, options, e32, e16, why in cs.ROWS:
        assert arch in cs.ARCHS, rid
        assert H >= 16 and W >= 16 and H % 16 == 0 and W % 16 == 0, rid
        assert N >= 1 and flip in (0, 1, 2), rid
        assert set(cs.device_options(cs.row(rid))) <= OPTION_KEYS, (rid, options)
        assert {k for k in options if k.startswith('_')} <= {'_joints', '_plain', '_storages'}, (rid, options)
        assert isinstance(e32, (set, frozenset)) and isinstance(e16, (set, frozenset)) and len(why) >= 20, rid
        assert set(cs.storages_of(cs.row(rid))) <= {'f32', 'bf16', 'f16'}, rid
        # the default batch of the edge rows: three images and their mirror images, unless a gate needs more
        assert (N, flip) == (3, 2) or N * 2 >= 48 or ('f32', rid) in cs.REFUSED, rid


def test_refused_keys_name_rows_and_storages():
    ids = {r[0] for r in cs.ROWS}
    for (storage, rid), text in cs.REFUSED.items():
        assert storage in ('f32', 'bf16', 'f16') and rid in ids, (storage, rid)
        assert len(text) >= 10, (storage, rid, text)
    # fp32 refuses the three-stage net only
    assert [k for k in cs.REFUSED if k[0] == 'f32'] == [('f32', 'three_64')]


@pytest.mark.parametrize('rid', [r[0] for r in cs.ROWS])
def test_target_shapes_are_in_the_derived_architecture(rid):
    row = cs.row(rid)
    arch = cs.arch_of(row)
    if ('f32', rid) in cs.REFUSED:
        with pytest.raises(IndexError):                 # the reference's own bookkeeping has no such net (x_list[-5])
            spec.derive(arch)
        assert cs.TARGET[rid] == []
        return
    keys = cs.shape_keys(arch, cs.head_of(row))
    assert cs.TARGET[rid], rid
    for tgt in cs.TARGET[rid]:
        assert tuple(tgt[1:]) in keys, (rid, tgt, sorted(keys))
    # the stride pattern the two-source head needs (see the module docstring of _custom_space)
    strides = [st['stride'] for st in arch['backbone_setting']]
    assert strides[-4:] == [2, 2, 2, 1], (rid, strides)


def test_the_architectures_are_what_their_comments_say():
    d = spec.derive(cs.ARCHS['odd'])
    assert [(c['refined_in'], c['raw_in'], c['out']) for c in d['deconv']] == [(80, 48, 18), (18, 32, 17), (17, 24, 9)]
    assert [(h['refined_in'], h['raw_in']) for h in d['heads']] == [(17, 24), (9, 24)]
    d = spec.derive(cs.ARCHS['odd'], spec.HeadCfg(num_joints=17))
    assert [h['oup'] for h in d['heads']] == [34, 17]                 # two channel blocks in final.0
    d = spec.derive(cs.ARCHS['pair66'])
    assert (d['deconv'][1]['refined_in'] + d['deconv'][1]['raw_in'], d['deconv'][1]['out']) == (66, 40)
    d = spec.derive(cs.ARCHS['d4'])
    assert [(c['refined_in'] + c['raw_in']) % 4 for c in d['deconv']] == [0, 0, 0]
    assert [c['refined_in'] % 8 for c in d['deconv']] == [0, 4, 4]
    d = spec.derive(cs.ARCHS['mb24'])
    assert all((b['inp'], b['feat'], b['oup'], b['k']) == (24, 96, 24, 7) for b in d['stages'][0] + d['stages'][1])
    assert len(spec.derive(cs.ARCHS['five'])['stages']) == 5 and len(cs.ARCHS['three']['backbone_setting']) == 3
    ratios = {(b['feat'] // b['inp'], b['k']) for st in spec.derive(cs.ARCHS['ksize'])['stages'] for b in st}
    assert ratios >= {(6, 3), (6, 5), (3, 3), (1, 5), (8, 7)}, ratios


def _golden_rows():
    return [r for r in cs.ROWS if ('f32', r[0]) not in cs.REFUSED]


def test_golden_holds_every_row():
    g = np.load(GOLDEN)
    for r in _golden_rows():
        gid = cs.golden_id(r)
        H, W = r[2], r[3]
        oups = [h['oup'] for h in spec.derive(cs.arch_of(r), cs.head_of(r))['heads']]
        for k, div in ((0, 4), (1, 2)):
            key = '%s_out%d' % (gid, k)
            assert key + '_sample' in g.files and key + '_stats' in g.files, key
            assert tuple(g[key + '_shape']) == (1, oups[k], H // div, W // div), (r[0], tuple(g[key + '_shape']))
    # nothing but rows
    ids = {cs.golden_id(r) for r in _golden_rows()}
    assert {f.rsplit('_out', 1)[0] for f in g.files} == ids


@pytest.mark.parametrize('rid', sorted({cs.golden_id(r) for r in _golden_rows()}))
def test_oracle_reproduces_the_golden_samples(rid):
    """net_ref.forward (tests/_simplenet_ref.py for a plain head) on the generator's image against the samples of the
    real reference module within 1e-6 (bit-identical at equal thread count, as tests/test_supernet_cpu.py has it)."""
    g = np.load(GOLDEN)
    row = cs.row(rid)
    arch, head, plain = cs.arch_of(row), cs.head_of(row), bool(row[6].get('_plain'))
    sd = snr.make_state_dict(arch, head, seed=1234) if plain else synth.make_state_dict(arch, head, seed=1234)
    x = synth.make_images(1, row[2], seed=11, w=row[3])
    with torch.no_grad():
        outs = snr.forward(x, sd, arch, head) if plain else net_ref.forward(x, sd, arch, head)
    for k, o in enumerate(outs):
        key = '%s_out%d' % (rid, k)
        np.testing.assert_allclose(o.numpy().reshape(-1)[::13], g[key + '_sample'], rtol=0, atol=1e-6)
