"""The form table of mbt_kernel without a GPU (tests/_mbt_space.py, tests/test_gpu_mbt_forms.py): closure of the table
over the library's host query ``lp_mbt_form`` (launch_mbt's own gating, moved into one function), the inventory of the
forms that the nets of the other tables reach, and the default rule of option "mbt_strip" at its edge.

Inventory (test_inventory_of_existing_nets prints it; default options, a 256-CU device; "s2" keys are mbt_s2_kernel's,
listed for the record and outside this table):
  the seven published architectures at 256, 384, 448, 512 with 2 and with 128 images
      s2<1,1> s2<2,2>  strip<2,1,T>  tile<2,1,T> tile<3,2,T>
  the 128 rows of tests/_subnet_space.py
      s2<1,1> s2<1,2> s2<2,1> s2<2,2>  tile<2,1,T> tile<3,2,F> tile<3,2,T>
  the rows of tests/_custom_space.py, with their options
      s2<1,1> s2<2,1> s2<2,2>  tile<2,1,T>
tile<3,2,F> is the 48 -> 40 entry block of the last stage of a supernet draw on an input above 256 x 256 (a plane above
16 x 16); at full 64 filters, at 56, and on a ragged plane no net has it.  No existing net reaches another non-residual
stride-1 form of mbt_kernel (tile <1,1,F> <2,1,F> <2,2,F> <3,1,F>, strip <1,1,F> <2,1,F>), a 16-channel form (<1,1,*>,
which needs option "mbt" = 2), or a strip form other than <2,1,T>.  All of them are rows of tests/_mbt_space.py."""
import itertools

import pytest

import _custom_space as cs
import _mbt_space as ms
import _subnet_space as ss
from oracle import spec

ENGINE_OPTIONS = {'mbt': (0, 3), 'mbt_s2': (0, 1), 'mbt_strip': (0, 2)}     # engine.cpp lp_net::options()


def _lib():
    from litepose_amd import _native as nv
    return nv.lib()


def _form(shape, mode=1, mode_s2=1, mode_strip=1, cus=256):
    n, cin, cexp, cout, h, w, k, s, res = shape
    return ms.decode(_lib().lp_mbt_form(n, cin, cexp, cout, h, w, k, s, int(res), mode, mode_s2, mode_strip, cus))


def _table_keys():
    return {r[8] for r in ms.ROWS}


def test_query_is_exported_and_documented():
    import os
    import re
    from litepose_amd import _native as nv
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'litepose_amd.h')).read()
    assert re.search(r'int\s+lp_mbt_form\s*\(', hdr) and 'lp_mbt_form' in nv.EXPORTS
    for name, v in (('LP_MBT_NONE', 0), ('LP_MBT_TILE', 1), ('LP_MBT_STRIP', 2), ('LP_MBT_S2', 3)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, v), hdr), name
    assert 'BEFORE' in hdr[hdr.index('lp_mbt_form: host arithmetic'):hdr.index('#define LP_MBT_NONE')]   # the scratch check
    L = _lib()
    for bad in ((0, 32, 192, 32, 32, 32, 7, 1, 1, 1, 1, 1, 256), (1, 32, 192, 32, 0, 32, 7, 1, 1, 1, 1, 1, 256),
                (1, 0, 192, 32, 32, 32, 7, 1, 0, 1, 1, 1, 256)):
        assert L.lp_mbt_form(*bad) < 0, bad
    # the headline's stage 1 and its entry block
    assert _form((128, 32, 192, 32, 32, 32, 7, 1, True)) == ('strip', 2, 1, True)
    assert _form((2, 32, 192, 32, 32, 32, 7, 1, True)) == ('tile', 2, 1, True)
    assert _form((2, 16, 96, 32, 64, 64, 7, 2, False)) == ('s2', 1, 1, False)
    # gates: a single 16 x 16 plane, another depthwise size, a residual that changes the channels, Cin of 24, 16 filters by default
    assert _form((2, 32, 192, 32, 16, 16, 7, 1, True)) is None
    assert _form((2, 32, 192, 32, 32, 32, 5, 1, True)) is None
    assert _form((2, 32, 192, 48, 32, 32, 7, 1, True)) is None
    assert _form((2, 24, 96, 32, 64, 64, 7, 1, False)) is None
    assert _form((2, 16, 96, 16, 64, 64, 7, 1, True)) is None
    assert _form((2, 16, 96, 16, 64, 64, 7, 1, True), mode=2) == ('tile', 1, 1, True)
    assert _form((2, 16, 96, 48, 64, 64, 7, 1, False), mode=2) is None          # <1, 2> is not built


def test_rows_are_well_formed():
    ids = [r[0] for r in ms.ROWS]
    assert len(ids) == len(set(ids))
    assert set(ms.INVARIANCE_ROWS) <= set(ids) and set(ms.REFUSED) <= set(ids) and set(ms.CHUNKS) <= set(ids)
    for rid, arch, H, W, N, flip, options, launch, key in ms.ROWS:
        assert arch in ms.ARCHS, rid
        assert H >= 16 and W >= 16 and H % 16 == 0 and W % 16 == 0, rid
        assert N >= 1 and flip in (0, 2), rid
        assert set(options) <= set(ENGINE_OPTIONS), (rid, options)
        for k, v in options.items():
            assert ENGINE_OPTIONS[k][0] <= v <= ENGINE_OPTIONS[k][1], (rid, k, v)
        assert key[0] in ('tile', 'strip') and len(key) == 4, rid
        s, b = ms.block_of(ms.row(rid))
        d = spec.derive(ms.arch_of(ms.row(rid)))
        assert s == len(d['stages']) - 1 and b < len(d['stages'][s]), rid
        strides = [st['stride'] for st in ms.ARCHS[arch]['backbone_setting']]
        assert strides == [2, 2, 2, 1], (rid, strides)
    # what the issue asks for, by count: the strip heights with N = 3 and alternating flip give grids 3, 6, 9 and 18
    grids = set()
    for h in ms.HEIGHTS:
        for inst in ('s11F', 's21T', 's21F', 's11T'):
            r = ms.row('h%d_%s' % (h, inst))
            assert (r[2], r[3], r[4]) == (16 * h, 512, 3), r[0]
            grids.add(r[4] * (2 if r[5] == 2 else 1) * ((h + 15) // 16))
    assert grids >= {3, 6, 9, 18}, grids
    assert ms.HEIGHTS == (1, 2, 3, 13, 15, 16, 17, 19, 31, 33, 35)
    r = ms.row('g51_s21T')
    assert r[4] * ((r[2] // 16 + 15) // 16) == 51
    # chunk counts 1, 2, 3, 8 on both forms, from the derived Cexp
    seen = set()
    for rid, n in ms.CHUNKS.items():
        shape = ms.shape_of(ms.row(rid))
        assert shape[2] == 32 * n, (rid, shape)
        seen.add((ms.row(rid)[8][0], n))
    assert seen == {(f, n) for f in ('tile', 'strip') for n in (1, 2, 3, 8)}, seen
    # the epilogue below a whole M tile: strips at 8, 16, 24 filters, tiles at 24, 40, 48, 56
    couts = {(r[8][0], r[8][2], ms.shape_of(r)[3]) for r in ms.ROWS}
    assert couts >= {('strip', 1, 8), ('strip', 1, 16), ('strip', 1, 24), ('strip', 1, 32), ('tile', 1, 24), ('tile', 1, 32),
                     ('tile', 2, 40), ('tile', 2, 48), ('tile', 2, 56), ('tile', 2, 64)}, couts


@pytest.mark.parametrize('rid', [r[0] for r in ms.ROWS])
def test_row_key_is_what_the_query_returns(rid):
    r = ms.row(rid)
    o = r[6]
    shape = ms.shape_of(r)
    for cus in (1, 256, 1 << 20):                        # the rows force their form by option: no CU count changes it
        got = _form(shape, o.get('mbt', 1), o.get('mbt_s2', 1), o.get('mbt_strip', 1), cus)
        assert got == r[8], (rid, shape, got, r[8])
    assert shape[8] == r[8][3] and shape[6:8] == (7, 1), (rid, shape)
    if r[8][0] == 'strip':
        assert shape[5] == 32, (rid, shape)


def test_closure_every_form_the_query_can_return_is_a_row():
    """Every distinct (form, CK, NMT, RES) lp_mbt_form returns over the stride-1 shape space is the key of a row."""
    seen = {}
    for cin, cout8, res, w, h, mode, strip, cus in itertools.product(
            (16, 32, 48), range(1, 9), (False, True), (17, 32, 48), (1, 16, 17), range(4), range(3), (1, 256)):
        cout = 8 * cout8
        if res and cin != cout:
            continue                                     # not a legal block: a residual block keeps its channels
        key = _form((1, cin, 6 * cin, cout, h, w, 7, 1, res), mode, 1, strip, cus)
        if key is not None:
            seen.setdefault(key, (cin, cout, res, w, h, mode, strip, cus))
    assert all(k[0] in ('tile', 'strip') for k in seen), seen
    missing = {k: v for k, v in seen.items() if k not in _table_keys()}
    assert not missing, ('forms the query returns and no row of _mbt_space.py runs', missing)
    extra = _table_keys() - set(seen)
    assert not extra, ('rows whose key the query never returns', extra)
    # the variants the launcher builds, and nothing else
    assert set(seen) == {('tile', 1, 1, False), ('tile', 1, 1, True), ('tile', 2, 1, False), ('tile', 2, 1, True),
                         ('tile', 2, 2, False), ('tile', 3, 1, False), ('tile', 3, 2, False), ('tile', 3, 2, True),
                         ('strip', 1, 1, False), ('strip', 1, 1, True), ('strip', 2, 1, False), ('strip', 2, 1, True)}


def _net_keys(arch, H, W, N, head=None, options=None):
    o = options or {}
    d = spec.derive(arch, head)
    keys = set()
    for s, blocks in enumerate(d['stages']):
        for blk in blocks:
            h, w = ms.plane_of(arch, s, H, W)
            if blk['stride'] == 2:                       # plane_of: the block's output plane; a stride-2 block reads twice that
                h, w = 2 * h, 2 * w
            key = _form((N, blk['inp'], blk['feat'], blk['oup'], h, w, blk['k'], blk['stride'], bool(blk['residual'])),
                        o.get('mbt', 1), o.get('mbt_s2', 1), o.get('mbt_strip', 1), 256)
            if key is not None:
                keys.add(key)
    return keys


def _fmt(keys):
    return ' '.join('%s<%d,%d%s>' % (k[0], k[1], k[2], '' if k[0] == 's2' else ',' + 'FT'[k[3]]) for k in sorted(keys))


def test_inventory_of_existing_nets():
    """Which forms the nets of the other tables reach (printed; the module docstring has the list): each stride-1 one is
    a row here.  The rows of this table add every other."""
    from litepose_amd import arch_zoo
    zoo, sub, cus = set(), set(), set()
    assert len(arch_zoo.names()) == 7
    for name, size, n in itertools.product(arch_zoo.names(), (256, 384, 448, 512), (2, 128)):
        zoo |= _net_keys(arch_zoo.get(name), size, size, n)
    assert len(ss.ROWS) == 128
    for r in ss.ROWS:
        sub |= _net_keys(ss.row_arch(r), r[2], r[3], r[4] * (2 if r[5] == 2 else 1))
    for r in cs.ROWS:
        if ('f32', r[0]) in cs.REFUSED:
            continue
        cus |= _net_keys(cs.arch_of(r), r[2], r[3], r[4] * (2 if r[5] == 2 else 1), cs.head_of(r), cs.device_options(r))
    print('published architectures:', _fmt(zoo))
    print('_subnet_space.py:       ', _fmt(sub))
    print('_custom_space.py:       ', _fmt(cus))
    reached = {k for k in zoo | sub | cus if k[0] != 's2'}
    assert reached <= _table_keys(), reached - _table_keys()
    assert reached == {('strip', 2, 1, True), ('tile', 2, 1, True), ('tile', 3, 2, False), ('tile', 3, 2, True)}, _fmt(reached)
    print('reached only by _mbt_space.py:', _fmt(_table_keys() - reached))


def test_default_rule_at_its_edge():
    """"mbt_strip" = 1 takes strips when images x strips >= the CU count: strips at 256 against 256 CUs, tiles at 255."""
    blk = (32, 192, 32)
    for n, h in ((256, 16), (128, 32), (128, 17), (86, 33)):
        assert _form((n,) + blk + (h, 32, 7, 1, True), cus=256) == ('strip', 2, 1, True), (n, h)
    for n, h in ((255, 16), (127, 32), (127, 17), (85, 33)):
        assert _form((n,) + blk + (h, 32, 7, 1, True), cus=256) == ('tile', 2, 1, True), (n, h)
    assert _form((255, 32, 192, 32, 16, 32, 7, 1, True), cus=255) == ('strip', 2, 1, True)
    assert _form((256, 32, 192, 32, 16, 32, 7, 1, True), mode_strip=0, cus=1) == ('tile', 2, 1, True)
    assert _form((1, 32, 192, 32, 16, 32, 7, 1, True), mode_strip=2, cus=1 << 20) == ('strip', 2, 1, True)
    assert _form((256, 32, 192, 32, 16, 48, 7, 1, True), cus=1) == ('tile', 2, 1, True)             # 32 wide only
    # a shape whose strip variant is not built keeps the tiles
    assert _form((256, 32, 192, 64, 16, 32, 7, 1, False), mode_strip=2) == ('tile', 2, 2, False)
    assert _form((256, 48, 288, 48, 16, 32, 7, 1, True), mode_strip=2) == ('tile', 3, 2, True)
