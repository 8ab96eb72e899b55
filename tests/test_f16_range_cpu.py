"""The fp16 range-edge rows (tests/_f16_range.py) without a GPU: every 16-bit kernel form is the tag of a subnormal row or
excused, and every row's preconditions hold on the emulation alone, so that a GPU row (tests/test_gpu_f16_range.py) cannot
pass vacuously: the tensor the row is about really sits in the subnormal range (or past 65504), the derived bound is
tighter than a flush, and an emulated flush fails the row's own check."""
import pytest
import torch

import _f16_range as fr
import _f16_ref
from test_f16_cpu import FAMILIES_16
from test_kernel_census_cpu import source_tags

SUB_ROWS = [r[0] for r in fr.ROWS if r[9] == 'sub']
TOP_ROWS = [r[0] for r in fr.ROWS if r[9] == 'top']


def tags16():
    """The 16-bit kernel tags of the sources: the families tests/test_f16_cpu.py lists per format, and the fused stem
    (stem4_kernel carries one tag for its fp32, bf16 and fp16 forms)."""
    return {t for t in source_tags() if t.split('<')[0] in FAMILIES_16 + ('stem4_kernel',)}


def test_every_16bit_tag_has_a_subnormal_row_or_is_excused():
    tags = tags16()
    assert len(tags) >= 16, sorted(tags)
    have = {fr.row(rid)[6] for rid in SUB_ROWS}
    missing = sorted(tags - have - set(fr.UNREACHED))
    assert not missing, ('16-bit forms with no subnormal row and no excuse', missing)
    assert not sorted(set(fr.UNREACHED) - tags), 'UNREACHED names tags that are not in the sources'
    assert not sorted(set(fr.UNREACHED) & have), 'both a row and an excuse'
    assert not sorted(have - tags), ('rows for tags that are not in the sources', sorted(have - tags))
    for why in fr.UNREACHED.values():
        assert len(why) >= 30, why


def test_rows_are_well_formed():
    ids = [r[0] for r in fr.ROWS]
    assert len(ids) == len(set(ids))
    keys = {'mbtb', 'mbtb_s2', 'mbtd', 'headb', 'dwt', 'stem'}
    for rid, arch, H, W, N, options, tag, op, pos, edge in fr.ROWS:
        assert H % 16 == 0 and W % 16 == 0 and 1 <= N <= 2 and H * W <= 128 * 128, rid
        assert set(options) <= keys and edge in ('sub', 'top'), rid
        assert rid not in fr.WINDOWS or edge == 'sub', rid
        assert (rid in fr.GAINS) == (edge == 'top'), rid
    # every fused form at each of its positions; every one-op form at both (stemb_kernel reads the fp32 image: 'w' only)
    pos = {}
    for r in fr.ROWS:
        if r[9] == 'sub':
            pos.setdefault(r[6], set()).add(r[8])
    for t in ('mbtd_kernel', 'mbtb_kernel', 'mbtb_s2_kernel'):
        assert pos[t] == {'x', 'expand', 'dw', 'project'}, (t, pos[t])
    assert pos['stem4_kernel'] == {'conv', 'dw3', 'pw'} and pos['headb_kernel'] == {'in_refined', 'in_raw', 'pw'}
    for t in tags16() - {'mbtd_kernel', 'mbtb_kernel', 'mbtb_s2_kernel', 'stem4_kernel', 'headb_kernel', 'stemb_kernel'}:
        assert pos[t] == {'w', 'x'}, (t, pos.get(t))
    # 'top': every form that stores a linear tensor; pwb_kernel with and without the residual, and as stem.pw
    top = {(fr.row(rid)[6], fr.row(rid)[7]) for rid in TOP_ROWS}
    assert {t for t, _ in top} == {'pwb_kernel', 'mbtd_kernel', 'mbtb_kernel', 'mbtb_s2_kernel', 'stem4_kernel',
                                    'deconvb_kernel'}
    assert {o for t, o in top if t == 'pwb_kernel'} == {'stage.0.0.point_conv', 'stage.0.1.point_conv', 'stem.pw'}


def _emulate(rid):
    r = fr.row(rid)
    arch = fr.arch_of(r)
    sd, rc = fr.edge_state_dict(arch, r)
    x = fr.images(r)
    return r, arch, sd, x, fr.evaluate(r, sd, arch, x, rc['target'])


def _flush(t):
    """fp32 -> fp16 with every subnormal result zeroed -> fp32: the rounding of hardware that flushes."""
    h = _f16_ref.rh(t)
    return torch.where(h.abs() < fr.NORMAL_MIN, torch.zeros_like(h), h)


@pytest.mark.parametrize('rid', SUB_ROWS)
def test_subnormal_row_preconditions_hold_on_the_emulation(rid):
    r, arch, sd, x, res = _emulate(rid)
    nz, sub = fr.shares(res['target'])
    assert nz > 0.1 and sub > 0.1, (rid, nz, sub)
    assert float(res['bound'].max()) < fr.SUB_BOUND_MAX, (rid, float(res['bound'].max()))
    # the compared tensor itself carries the edge: a tenth of it is beyond the bound, and the emulation passes its check
    assert float((res['exp'].abs() > res['bound']).float().mean()) > 0.1, rid
    res['got'] = res['exp']
    assert fr.check_sub(res) == 0.0
    # teeth: the same plan with every 16-bit value (folded weights, stored and inner tensors) flushed fails the check
    vals = {'x': x}
    with torch.no_grad():
        for name, ins, fn in _f16_ref.plan(sd, arch, rnd=_flush):
            vals[name] = fn(*[vals[k] for k in ins])
            if name == r[7]:
                break
    res['got'] = vals[r[7]]
    with pytest.raises(AssertionError):
        fr.check_sub(res)


@pytest.mark.parametrize('rid', TOP_ROWS)
def test_top_row_preconditions_hold_on_the_emulation(rid):
    r, arch, sd, x, res = _emulate(rid)
    big, ninf = fr.top_shares(res['exp'])
    assert big >= 0.1 and ninf >= 100, (rid, big, ninf)
    assert not bool(torch.isnan(res['exp']).any())
    assert bool(torch.isfinite(res['raw']).all())          # the overflow is the store's: folded weights and sums are finite
    rounds_down = int(((res['raw'].abs() > fr.F16_MAX) & (res['raw'].abs() < fr.F16_INF_AT)).sum())
    res['got'] = res['exp']
    worst, undecided = fr.check_top(res)
    # at least 100 infinities the emulation DECIDES (a fused launch: the inner tensors' rounding, carried through the
    # scaled weights, leaves the values nearest the tie open); a launch that stores its own op decides all but a few
    decided = int((~torch.isfinite(res['exp']) & ((res['raw'].abs() - fr.F16_INF_AT).abs() > res['slack'])).sum())
    assert worst == 0.0 and decided >= 100, (rid, decided, undecided, ninf)
    assert fr.launch_inner(r) or undecided <= 0.01 * ninf + 2, (rid, undecided, ninf)
    print('%s: %.3f finite >= 2^14, %d inf, %d in (65504, 65520), %d undecided' % (rid, big, ninf, rounds_down, undecided))
    # teeth: a store that saturates instead of overflowing, and one that loses the sign of the infinity, fail
    for wrong in (torch.clamp(res['exp'], -fr.F16_MAX, fr.F16_MAX), res['exp'].abs()):
        if torch.equal(wrong, res['exp']):
            continue                                       # deconvb_kernel: ReLU leaves no -inf
        res['got'] = wrong
        with pytest.raises(AssertionError):
            fr.check_top(res)
