"""The rows of tests/test_gpu_resnet_census.py without a GPU: ``lp_net_create`` accepts each table, its key list and
shapes are the restatement's, the features derived from the row include what the row claims, the rows together cover
the literal REQUIRED list (deleting the only row that provides a feature fails here), and the float32 restatement
stays within a quarter of the device bounds of the float64 one."""
import ctypes as C

import pytest

import _resnet_ref as rr
import test_gpu_resnet_census as census

IDS = [r[0] for r in census.CASES]


def test_rows_are_well_formed():
    assert 12 <= len(census.CASES) <= 16 and len(set(IDS)) == len(IDS)
    for row in census.CASES:
        cid, table, filters, upk, joints, H, W, N, flip, expect = row
        m = max(16, census.deepest_divisor(table))
        assert H % m == 0 and W % m == 0 and H >= m and W >= m, cid
        assert upk in (3, 5, 7) and flip in (0, 2) and N in (1, 3, 5) and len(filters) == 3, cid


@pytest.mark.parametrize('cid', IDS)
def test_lp_net_create_accepts_the_row_and_its_keys_are_the_restatements(cid):
    from litepose_amd import _native as nv
    row = census.case(cid)
    a = census.arch_struct(row)
    h = C.c_void_p()
    lib = nv.lib()
    assert lib.lp_net_create(C.byref(h), C.byref(a)) == 0, lib.lp_last_error()
    try:
        shp = (C.c_int64 * 4)()
        nd = C.c_int()
        keys = []
        for i in range(lib.lp_net_num_keys(h)):
            k = lib.lp_net_key(h, i, shp, C.byref(nd)).decode()
            keys.append((k, tuple(int(shp[d]) for d in range(nd.value))))
    finally:
        lib.lp_net_destroy(h)
    assert keys == list(rr.state_dict_shapes(census.row_cfg(row), row[1]).items())
    # the test-local subclass goes the same way, and keeps the product's refusal of width_mult
    m = census.make_model(row)
    assert m.keys() == keys and m.final_channel == [2 * row[4], row[4]]
    assert m.size_multiple == max(16, census.deepest_divisor(row[1]))
    with pytest.raises(ValueError):
        type(m)(census.row_cfg(row), width_mult=0.5)


@pytest.mark.parametrize('cid', IDS)
def test_derived_features_include_what_the_row_claims(cid):
    row = census.case(cid)
    got = census.features(row)
    missing = [f for f in row[9] if f not in got]
    assert not missing, (cid, missing, sorted(got))
    assert set(row[9]) <= set(census.REQUIRED), sorted(set(row[9]) - set(census.REQUIRED))
    # the launch list: stem, two launches per block, three deconvs, two heads -- every plane exact
    ls = census.launches(row)
    nblocks = sum(n for _, _, _, n, _ in row[1][1])
    assert len(ls) == 2 + 2 * nblocks + 3 + 2
    assert [l[0] for l in ls][-4:] == ['deconv.1', 'final.0', 'deconv.2', 'final.1']


def _covered(cases):
    got = set()
    for row in cases:
        got |= census.features(row)
    return [f for f in census.REQUIRED if f not in got]


def test_rows_cover_the_required_list():
    assert len(set(census.REQUIRED)) == len(census.REQUIRED) >= 45
    assert not _covered(census.CASES), _covered(census.CASES)


def test_coverage_fails_when_a_sole_provider_is_deleted():
    """Every row that is the only provider of a REQUIRED feature: without it the coverage check above fails."""
    sole = 0
    for i, row in enumerate(census.CASES):
        rest = census.CASES[:i] + census.CASES[i + 1:]
        lost = _covered(rest)
        others = set()
        for r in rest:
            others |= census.features(r)
        only_here = [f for f in census.REQUIRED if f in census.features(row) and f not in others]
        assert sorted(lost) == sorted(only_here), row[0]
        sole += bool(only_here)
    assert sole >= 4                                          # deep32, the 16x1024 / 1024x16 inputs, width 0.5, ...


@pytest.mark.parametrize('cid', IDS)
def test_float32_restatement_is_within_a_quarter_of_the_bounds(cid):
    """CPU headroom (the table in test_gpu_resnet_census's docstring): the reference's own float32 rounding against
    float64 stays at or below a quarter of NET_ATOL / TAP_REL; a row that does not gets another head_gain / table, never
    another bound."""
    out, tap = census.cpu_headroom(census.case(cid))
    print('headroom %-14s outputs %.3f  taps %.3f' % (cid, out, tap))
    assert out <= 0.25 and tap <= 0.25, (cid, out, tap)
