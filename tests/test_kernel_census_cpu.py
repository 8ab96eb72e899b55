"""The kernel census without a GPU: every form the HIP sources can name (``last_kernel_tag = ...`` in
litepose_amd/csrc/) is expected by some row of tests/test_gpu_kernel_census.py's CASES or listed in its NOT_REACHED
with the reason; a NOT_REACHED entry for a tag that no longer exists fails too."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'litepose_amd', 'csrc')

_ASSIGN = re.compile(r'\blast_kernel_tag\s*=\s*([^;]*);')
_LITERAL = re.compile(r'"([^"]*)"')


def source_tags(csrc=CSRC):
    """Every non-empty string literal assigned to last_kernel_tag in the HIP / C++ sources (ternaries included)."""
    tags = set()
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith(('.hip', '.cpp', '.h')):
            continue
        with open(os.path.join(csrc, fn)) as f:
            src = f.read()
        for expr in _ASSIGN.findall(src):
            tags.update(t for t in _LITERAL.findall(expr) if t)
    return tags


def census_gaps(tags, cases, not_reached):
    """(tags neither expected nor excused, NOT_REACHED entries for tags that do not exist, tags both expected and excused)"""
    expected = set().union(*[set(c[8]) for c in cases])
    return (sorted(tags - expected - set(not_reached)), sorted(set(not_reached) - tags),
            sorted(expected & set(not_reached)))


def _census():
    import test_gpu_kernel_census as kc
    return kc.CASES, kc.NOT_REACHED


def test_sources_name_the_forms():
    tags = source_tags()
    # the dispatcher's families: a parser that finds far fewer has stopped reading the sources
    assert len(tags) >= 27, sorted(tags)
    for t in ('mb16_kernel', 'mbtd_kernel', 'mbconv_s2_kernel', 'dwb_kernel<7,2>', 'dw_pair16_kernel<7>'):
        assert t in tags, t


def test_every_tag_is_expected_by_a_case_or_excused():
    cases, not_reached = _census()
    missing, stale, both = census_gaps(source_tags(), cases, not_reached)
    assert not missing, ('kernel forms no CASES row expects and NOT_REACHED does not excuse', missing)
    assert not stale, ('NOT_REACHED names tags that are not in the sources', stale)
    assert not both, ('expected by a CASES row and listed as not reached', both)


def test_not_reached_reasons_name_the_gate():
    _, not_reached = _census()
    for tag, why in not_reached.items():
        assert len(why) >= 30, (tag, why)


def test_cases_table_is_well_formed():
    from litepose_amd import arch_zoo
    cases, _ = _census()
    ids = [c[0] for c in cases]
    assert len(ids) == len(set(ids))
    keys = {'mb16', 'mb16_run', 'mb16_min', 'mbt', 'mbt_s2', 'mbconv2', 'mbtb', 'mbtb_s2', 'mbtd', 'pw3d',
            'headb', 'dwt', 'stem'}
    for cid, arch, storage, H, W, N, flip, options, expect in cases:
        assert arch in arch_zoo.names(), cid
        assert storage in ('f32', 'bf16'), cid
        assert H >= 16 and W >= 16 and H % 16 == 0 and W % 16 == 0, cid
        assert N >= 1 and flip in (0, 1, 2), cid
        assert set(options) <= keys, (cid, options)            # diag_dwpw: the diagnostics flavour is out of scope
        assert isinstance(expect, (set, frozenset)), cid
    # every published arch at its native size in both storages
    native = {(c[1], c[2]) for c in cases if c[3] == c[4] == arch_zoo.get(c[1])['img_size'] and not c[7]}
    assert native >= {(a, s) for a in arch_zoo.names() for s in ('f32', 'bf16')}, native


@pytest.mark.parametrize('drop', ['row', 'fake_tag'])
def test_census_fails_when_coverage_is_lost(drop, tmp_path):
    """The check above has teeth: removing the only row that expects a tag, or a new tag in a copy of the sources,
    is reported."""
    cases, not_reached = _census()
    tags = source_tags()
    if drop == 'row':
        counts = {}
        for c in cases:
            for t in c[8]:
                counts.setdefault(t, []).append(c[0])
        only = sorted((ids[0], t) for t, ids in counts.items() if len(ids) == 1)
        assert only, 'no tag is expected by exactly one row'
        for cid, t in only:
            missing, _, _ = census_gaps(tags, [c for c in cases if c[0] != cid], not_reached)
            assert t in missing, (cid, t)
    else:
        for fn in os.listdir(CSRC):
            with open(os.path.join(CSRC, fn)) as f:
                (tmp_path / fn).write_text(f.read())
        with open(tmp_path / 'net_kernels.hip', 'a') as f:
            f.write('\nstatic void fake() { last_kernel_tag = "x_kernel"; }\n')
        missing, _, _ = census_gaps(source_tags(str(tmp_path)), cases, not_reached)
        assert missing == ['x_kernel'], missing
