"""The method of tests/_nonfinite.py, without a device.

  * the sites: the list holds what the kernels' tilings call for;
  * the two routes to a cone -- isnan / ~isfinite of torch's fp64 result on the injected input, and the op on the site's 0/1
    indicator with all-ones partners -- agree for every linear case, operand, site and value the GPU files run;
  * torch's BatchNorm facts the GPU tests take as the truth;
  * ``compare`` fails on a scrubbed NaN, on a NaN outside the cone, on a moved bit and on a wrong class."""
import pytest
import torch

import _nonfinite as NF

_id = lambda r: 'x'.join(str(v) for v in r)               # noqa: E731


# ------------------------------------------------------------------ sites
def test_sites_of_a_plane():
    got = dict(NF.sites((3, 6, 40, 24), [(16, 16)], ragged=True))
    n, c = 1, 3
    assert got['first'] == (0, 0, 0, 0) and got['last'] == (2, 5, 39, 23)
    assert {got['corner00'], got['corner0W'], got['cornerH0'], got['cornerHW']} == \
        {(n, c, 0, 0), (n, c, 0, 23), (n, c, 39, 0), (n, c, 39, 23)}
    assert got['edge'] == (n, c, 39, 12)
    assert got['last plane'][:2] == (2, 5)
    assert got['tile 16/16 lo'] == (n, c, 15, 15) and got['tile 16/16 hi'] == (n, c, 16, 16)
    assert got['ragged channel'][:2] == (n, 5)
    assert got['quad lo'] == (n, c, 20, 3) and got['quad hi'] == (n, c, 20, 20)
    # the deconv's 8 x 8 tiles; a plane no larger than the tile has no boundary
    assert dict(NF.sites((2, 4, 16, 16), [(8, 8)]))['tile 8/8 hi'] == (1, 2, 8, 8)
    assert not any(k.startswith('tile') for k, _ in NF.sites((2, 4, 8, 8), [(8, 8)]))
    # a plane wider than the tile in one direction only: the boundary is crossed in that direction
    assert dict(NF.sites((1, 4, 6, 40), [(16, 16)]))['tile 16/16 hi'] == (0, 2, 5, 16)
    idx = [i for _, i in NF.sites((1, 1, 4, 4))]
    assert len(idx) == len(set(idx))                       # a site is listed once
    assert [i for _, i in NF.sites((5,))] == [(0,), (4,), (2,)]


def test_the_plan_has_a_nan_at_every_site_and_both_infinities_at_the_ends():
    s = NF.sites((2, 3, 5, 7))
    p = NF.plan(s)
    assert [x for x, v in p if v == 'nan'] == s
    assert {(x[0], v) for x, v in p if v != 'nan'} == {('first', '+inf'), ('first', '-inf'), ('last', '+inf'), ('last', '-inf')}


def test_the_rows_are_rows_of_the_existing_tables_and_have_every_component():
    import _train_forms as FM
    import test_gpu_train_forms as GT
    pw = NF.rows('pw')
    keys = [k for r in pw for k in (FM.pw_mm_form(r[2], r[0], r[1], r[3], r[4], 'fwd'), FM.pw_mm_form(r[2], r[1], r[0], r[3], r[4], 'dx'))]
    for what in ('fwd', 'dx'):
        mine = [k for k in keys if k[1] == what]
        assert {k[2] for k in mine} == {1, 2, 3} and {k[3] for k in mine} == {1, 2, 4}
        assert {'Kodd', 'Mrag', 'cbrag'} <= {v for k in mine for v in k[4:]}
    wg = [FM.pw_dw_form(r[2], r[0], r[1], r[3], r[4]) for r in pw]
    assert {'z>0', 'ragged', 'scalar', 'vec'} <= {v for k in wg for v in k[1:]}
    dw = [FM.dw_form(r[3], r[2], r[4], r[5], r[0], r[1]) for r in NF.rows('dw')]
    fams = {'pair16', 'pairvec', 'pairscalar', 'dwvec', 'dwscalar'}
    assert {(k[1], k[3]) for k in dw} >= {(K, f) for K in (3, 5, 7) for f in fams}
    assert {'Crag', 'ragged', 'whole', 'slices', 'tiles>4', 'dwvec2'} <= {v for k in dw for v in k[3:]}
    bn = [FM.bn_form(*r, False) for r in NF.rows('bn')]
    assert {k[1] for k in bn} == {'vec', 'scalar'} and {k[2] for k in bn} == {'one', 'several', 'cap'}
    assert {k[4] for k in bn} == {'rem', 'even', 'wide'}
    dc = [FM.deconv_form(r[3], r[0], r[1], r[2], r[4], r[5]) for r in NF.rows('deconv')]
    assert {'odd', 'Mrag', 'COrag', 'two', 'one', 'slices', 'ragged'} <= {v for k in dc for v in k[1:]}
    st = [FM.stem_form(*r) for r in NF.rows('stem')]
    assert {k[1] for k in st} == {'slice', 'slices'} and 'ragged' in {k[2] for k in st}
    assert set(NF.rows('bn')) & {c for c, _ in GT.BN_CASES}
    for kind in ('pw', 'dw', 'bn', 'deconv', 'stem'):
        assert all(r[-2] * r[-1] >= NF.MIN_PLANE for r in NF.rows(kind))


# ------------------------------------------------------------------ the two routes
def _routes(kind, row, large=False):
    ref, kw = NF.LINEAR[kind], NF.linear_kw(kind, row)
    ins = NF.linear_inputs(kind, row)
    for operand in [k for k, v in ins.items() if v is not None]:
        cones = {}
        for (name, idx), vname in NF.plan(NF.linear_sites(kind, row, operand, ins[operand].shape), large):
            if idx not in cones:
                cones[idx] = NF.indicator_cone(ref, ins, operand, idx, **kw)
            bad = dict(ins)
            bad[operand] = NF.inject(ins[operand], idx, NF.VALUES[vname])
            out = ref(bad, **kw)
            for k, v in out.items():
                a, b = NF.cone(v, NF.VALUES[vname]), cones[idx][k]
                assert torch.equal(a, b), (kind, row, operand, name, vname, k, int(a.sum()), int(b.sum()))


# A reduction: the 1x1 rows above _nonfinite.LARGE (millions of cells, where the GPU file runs the short plan) are held on
# the device against the first route alone.  A 1x1 is the same sum per pixel whatever the plane and has no padding; every
# NB / PXV / ragged-channel site kind of those rows is among the rows held here (the last test of this section).
@pytest.mark.parametrize('row', [r for r in NF.rows('pw') if NF._numel('pw', r) <= NF.LARGE], ids=_id)
def test_the_two_routes_agree_pointwise(row):
    _routes('pw', row)


@pytest.mark.parametrize('row', NF.rows('dw'), ids=_id)
def test_the_two_routes_agree_depthwise(row):
    _routes('dw', row, NF._numel('dw', row) > NF.LARGE)


@pytest.mark.parametrize('row', NF.rows('deconv'), ids=_id)
def test_the_two_routes_agree_transposed_pair(row):
    _routes('deconv', row)


@pytest.mark.parametrize('row', NF.rows('stem'), ids=_id)
def test_the_two_routes_agree_stem(row):
    _routes('stem', row)


@pytest.mark.parametrize('row', NF.rows('conv'), ids=_id)
def test_the_two_routes_agree_dense_conv(row):
    _routes('conv', row)


def test_the_dense_conv_rows_cover_every_form():
    """every K meets every (stride, upsample) on every plane of that form; every channel set and both bias settings meet
    every K, every form and every plane; the leak's row and its control are among them"""
    rows = NF.rows('conv')
    assert len(rows) == len(set(rows))
    comps = lambda r: dict(ch=r[:3], plane=r[3:6], k=r[6], form=r[7:9], bias=r[9])     # noqa: E731
    for k in NF.CONV_KS:
        for form in NF.CONV_FORMS:
            assert {r[3:6] for r in rows if r[6] == k and r[7:9] == form} == set(NF.CONV_PLANES[form])
    met = {((a, ca[a]), (b, ca[b])) for ca in map(comps, rows) for a in ca for b in ca if a != b}
    values = dict(ch=NF.CONV_CH, k=NF.CONV_KS, form=NF.CONV_FORMS, bias=(True, False),
                  plane=[p for f in NF.CONV_FORMS for p in NF.CONV_PLANES[f]])
    for a in values:
        for b in values:
            for va in values[a]:
                for vb in values[b]:
                    if a == b or ('plane' in (a, b) and 'form' in (a, b)):
                        continue                             # a plane belongs to one form
                    assert ((a, va), (b, vb)) in met, (a, va, b, vb)
    assert (5, 0, 3, 2, 5, 7, 3, 1, 0, True) in rows
    assert any(r[3:9] == (2, 8, 16, 3, 1, 0) for r in rows)
    # what the channel sets are there for (csrc/dense_grad_kernels.hip: WgCut, 32-row blocks; convk3's 16-channel k-step)
    assert NF.CONV_CH[0][1] == 0 and NF.CONV_CH[1][1] > 0 and NF.CONV_CH[2][2] > 32 and NF.CONV_CH[2][2] % 32
    ca, cb, _ = NF.CONV_CH[1]
    for cg in (14, 10):
        assert (ca + cb + cg - 1) // cg >= 3 and ca % cg and (ca + cb) % 16
    # the planes: a partly filled tile, one full tile, 2 x 2 tiles with a ragged last row and column and a plane wider than 16
    s1 = NF.CONV_PLANES[(1, 0)]
    assert s1[0][1] < 8 and s1[0][2] < 16 and s1[1][1:] == (8, 16) and 8 < s1[2][1] < 16 < s1[2][2] < 32
    assert all(h % 2 == 0 and w % 2 == 0 for _, h, w in NF.CONV_PLANES[(2, 0)])
    assert NF.CONV_PLANES[(2, 0)][1][2] // 2 > 16 and 2 * NF.CONV_PLANES[(1, 1)][1][2] > 16


@pytest.mark.parametrize('kind,row', [('dw', (7, 2, 8, 1, 6, 10)), ('dw', (3, 1, 6, 2, 7, 7)), ('stem', (2, 10, 14)),
                                      ('deconv', (33, 7, 9, 2, 5, 7)), ('conv', (33, 7, 9, 2, 5, 7, 5, 1, 0, True)),
                                      ('conv', (5, 0, 3, 2, 6, 10, 3, 2, 0, False)), ('conv', (33, 7, 9, 2, 3, 5, 7, 1, 1, True))],
                         ids=['dw7s2', 'dw3s1', 'stem', 'deconv', 'conv5s1', 'conv3s2', 'conv7ups'])
def test_the_tap_wise_sums_are_torchs_convolutions_without_the_multiplied_padding(kind, row):
    """On finite data the restatement is torch's own convolution up to the order of the sums.  With a NaN in the first
    weight tap torch's conv2d poisons every border output the tap meets only as padding: wider than the cone."""
    ins, kw = NF.linear_inputs(kind, row), NF.linear_kw(kind, row)
    mine, theirs = NF.LINEAR[kind](ins, **kw), NF.torch_conv(kind, ins, **kw)
    for k in mine:
        assert torch.allclose(mine[k], theirs[k], rtol=1e-12, atol=1e-13), k
    # the weight gradient of a transposed convolution pads grad_y; a convolution's forward pads x
    operand, out = ('xa', 'gwa') if kind == 'deconv' else ('wa', 'y') if kind == 'conv' else ('w', 'y')
    bad = dict(ins)
    bad[operand] = NF.inject(ins[operand], (0, 0, 0, 0), NF.NAN)
    a, b = torch.isnan(NF.LINEAR[kind](bad, **kw)[out]), torch.isnan(NF.torch_conv(kind, bad, **kw)[out])
    assert bool((b | ~a).all()) and int(b.sum()) > int(a.sum())
    assert torch.equal(a, NF.indicator_cone(NF.LINEAR[kind], ins, operand, (0, 0, 0, 0), **kw)[out])


@pytest.mark.parametrize('row', NF.rows('conv'), ids=_id)
def test_the_mask_of_the_dense_data_gradient_is_the_dilated_formulations(row):
    """halo_products' mask for a site in a weight tap -- the tap's whole input channel -- is what torch marks when it forms
    the data gradient the way the library does (_nonfinite.dilated_data_gradient); on finite data that formulation is the
    data gradient.  It holds the cone, and at stride 2, where a tap meets the cells of one parity only, it is far wider."""
    ins, kw = NF.linear_inputs('conv', row), NF.linear_kw('conv', row)
    clean = NF.ref_conv(ins, **kw)
    for operand, key in (('wa', 'gxa'), ('wb', 'gxb')):
        if ins[operand] is None:
            continue
        g = NF.dilated_data_gradient(ins['dy'].double(), ins[operand].double(), kw['s'], kw['ups'])
        assert torch.allclose(g, clean[key], rtol=1e-12, atol=1e-13)
        shapes = {k: v.shape for k, v in clean.items()}
        for (name, idx), vname in NF.plan(NF.linear_sites('conv', row, operand, ins[operand].shape)):
            bad = NF.inject(ins[operand], idx, NF.VALUES[vname])
            theirs = NF.cone(NF.dilated_data_gradient(ins['dy'].double(), bad.double(), kw['s'], kw['ups']), NF.VALUES[vname])
            mine = NF.halo_products('conv', row, operand, idx, shapes)
            assert set(mine) == {key} and torch.equal(mine[key], theirs), (operand, name, vname)
            truth = NF.indicator_cone(NF.ref_conv, ins, operand, idx, **kw)[key]
            assert bool((theirs | ~truth).all())
            if kw['s'] == 2 and name == 'first':
                assert 4 * int(truth.sum()) <= int(theirs.sum())


# ------------------------------------------------------------------ the partly filled tile of the dense weight gradient
def _tiled_weight_gradient(x, dy, k, s, select):
    """A weight gradient that walks ALL 128 pixels of every 8 x 16 tile of the output plane: a pixel outside the plane has a
    zero grad_y, and its partner is the input cell it would read wherever that cell lies in the plane (zero outside it).
    select: the partner of such a pixel is selected away instead."""
    N, C, H, W = x.shape
    OH, OW = dy.shape[2:]
    TH, TW = -(-OH // 8) * 8, -(-OW // 16) * 16
    p = k // 2
    xp = torch.zeros((N, C, (TH - 1) * s + k, (TW - 1) * s + k), dtype=torch.float64)
    xp[:, :, p:p + H, p:p + W] = x[:, :, :xp.shape[2] - p, :xp.shape[3] - p]
    dyp = torch.zeros((N, dy.shape[1], TH, TW), dtype=torch.float64)
    dyp[:, :, :OH, :OW] = dy
    inside = torch.zeros((TH, TW), dtype=torch.bool)
    inside[:OH, :OW] = True
    gw = torch.zeros((dy.shape[1], C, k, k), dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            b = xp[:, :, ky:ky + (TH - 1) * s + 1:s, kx:kx + (TW - 1) * s + 1:s]
            if select:
                b = torch.where(inside, b, torch.zeros((), dtype=torch.float64))
            gw[:, :, ky, kx] = torch.einsum('nohw,nchw->oc', dyp, b)
    return gw.float()


@pytest.mark.parametrize('k,s,plane,leaks', [(3, 1, (2, 5, 7), True), (5, 1, (2, 5, 7), True), (3, 2, (2, 6, 10), True),
                                             (3, 1, (2, 8, 16), False)], ids=['k3', 'k5', 'k3s2', 'full-tile'])
def test_the_rows_see_a_partly_filled_tile_removed_by_a_multiplication(k, s, plane, leaks):
    """conv_wgrad_kernel before it selected: fed to ``compare`` in place of a device result, the scheme fails at the 'edge'
    site of xa on every plane that does not fill its 8 x 16 tiles, beyond torch's own mask, and passes on the full tile;
    with the select it passes everywhere.  On finite data the two are the same bits."""
    row = (5, 0, 3) + plane + (k, s, 0, True)
    ins, kw = NF.linear_inputs('conv', row), NF.linear_kw('conv', row)
    name, idx = [s_ for s_ in NF.linear_sites('conv', row, 'xa', ins['xa'].shape) if s_[0] == 'edge'][0]
    bad = dict(ins)
    bad['xa'] = NF.inject(ins['xa'], idx, NF.NAN)
    R, Rb, Wb = NF.ref_conv(ins, **kw)['gwa'], NF.ref_conv(bad, **kw)['gwa'], NF.torch_conv('conv', bad, **kw)['gwa']
    assert torch.equal(torch.isnan(Rb), torch.isnan(Wb))          # torch pads x, not grad_y: no allowance here
    run = lambda t, select: _tiled_weight_gradient(t['xa'], t['dy'], k, s, select)     # noqa: E731
    assert NF.bitwise(run(ins, False), run(ins, True))
    assert torch.allclose(run(ins, True).double(), R, rtol=1e-6, atol=1e-6)
    NF.compare('selected gwa', run(ins, True), run(bad, True), R, Rb, NF.NAN, True, Wb)
    if leaks:
        with pytest.raises(AssertionError, match='outside it poisoned'):
            NF.compare('multiplied gwa', run(ins, False), run(bad, False), R, Rb, NF.NAN, True, Wb)
        assert int(torch.isnan(run(bad, False)).sum()) > int(torch.isnan(Rb).sum())
    else:
        NF.compare('multiplied gwa', run(ins, False), run(bad, False), R, Rb, NF.NAN, True, Wb)


def test_every_kernel_size_and_stride_is_among_the_rows_held_here():
    assert {(r[0], r[1]) for r in NF.rows('dw')} == {(k, s) for k in (3, 5, 7) for s in (1, 2)}
    small = [r for r in NF.rows('pw') if NF._numel('pw', r) <= NF.LARGE]
    names = lambda rs: {n.split()[0] for r in rs for op in ('x', 'dy') for (n, _), _v in     # noqa: E731
                        NF.plan(NF.linear_sites('pw', r, op, (r[2], r[0] if op == 'x' else r[1], r[3], r[4])), NF._numel('pw', r) > NF.LARGE)}
    assert names(NF.rows('pw')) <= names(small)
    assert 'next' in names(small)                            # the first channel of the last image


# ------------------------------------------------------------------ torch's BatchNorm facts
@pytest.mark.parametrize('vname', ['nan', '+inf', '-inf'])
def test_batch_norm_in_training_mode_loses_the_whole_channel(vname):
    ins = NF.bn_inputs((3, 4, 5, 7), True)
    clean = NF.ref_bn(ins, 'relu6', True)
    bad = dict(ins)
    bad['x'] = NF.inject(ins['x'], (1, 2, 3, 4), NF.VALUES[vname])
    out = NF.ref_bn(bad, 'relu6', True)
    ch = torch.zeros(4, dtype=torch.bool)
    ch[2] = True
    for k in ('y', 'gx'):
        assert torch.equal(torch.isnan(out[k]), ch.view(1, 4, 1, 1).expand_as(out[k])), k
    for k in ('invstd', 'rv', 'gg'):
        assert torch.equal(torch.isnan(out[k]), ch), k
    for k in ('mean', 'rm'):
        assert torch.equal(~torch.isfinite(out[k]), ch), k
        assert bool(torch.isnan(out[k][2])) == (vname == 'nan')
    for k in out:                                             # every other channel: the same bits
        sel = ~ch.view(1, 4, 1, 1).expand_as(out[k]) if out[k].dim() == 4 else ~ch
        assert torch.equal(out[k][sel], clean[k][sel]), k
    # the bias gradient is the sum of what the activation's gate lets through, and a NaN z passes torch's gate: finite
    assert bool(torch.isfinite(out['gb']).all())


def test_relu6_keeps_a_nan_and_eval_mode_touches_one_cell():
    z = torch.tensor([NF.NAN, -1.0, 7.0, NF.PINF, NF.NINF], dtype=torch.float64)
    assert torch.isnan(NF.ACT['relu6'](z)).tolist() == [True, False, False, False, False]
    assert torch.isnan(NF.ACT['relu'](z)).tolist() == [True, False, False, False, False]
    ins = NF.bn_inputs((3, 4, 5, 7), False)
    clean = NF.ref_bn(ins, 'relu6', False)['y']
    for act in (None, 'relu', 'relu6'):
        bad = dict(ins)
        bad['x'] = NF.inject(ins['x'], (1, 2, 3, 4), NF.NAN)
        y = NF.ref_bn(bad, act, False)['y']
        assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[1, 2, 3, 4]))
    bad['x'] = NF.inject(ins['x'], (1, 2, 3, 4), NF.PINF)
    y = NF.ref_bn(bad, 'relu6', False)['y']
    assert bool(torch.isfinite(y).all()) and float(y[1, 2, 3, 4]) in (0.0, 6.0)
    y[1, 2, 3, 4] = clean[1, 2, 3, 4]
    assert torch.equal(y, clean)


def test_a_nan_gradient_under_a_closed_gate_goes_nowhere():
    ins = NF.bn_inputs((3, 4, 5, 7), False)
    clean = NF.ref_bn(ins, 'relu', True)
    closed = torch.nonzero(clean['y'] == 0)
    assert closed.shape[0] > 0
    idx = tuple(int(v) for v in closed[0])
    bad = dict(ins)
    bad['dy'] = NF.inject(ins['dy'], idx, NF.NAN)
    out = NF.ref_bn(bad, 'relu', True)
    for k in out:
        assert torch.equal(out[k], clean[k]), k


# ------------------------------------------------------------------ compare() sees what it claims to see
def _pair():
    ins = NF.linear_inputs('dw', (3, 1, 6, 2, 7, 7))
    bad = dict(ins)
    bad['x'] = NF.inject(ins['x'], (1, 3, 0, 6), NF.NAN)
    R, Rb = NF.ref_dw(ins, 3, 1), NF.ref_dw(bad, 3, 1)
    return {k: v.float() for k, v in R.items()}, {k: v.float() for k, v in Rb.items()}, R, Rb


def test_compare_passes_the_truth_itself():
    O, Ob, R, Rb = _pair()
    sizes = NF.compare_all('dw', O, Ob, R, Rb, NF.NAN, True)
    assert sizes['y'] == 4 and sizes['gx'] == 0 and sizes['gw'] == 4      # a corner cell: 2 x 2 outputs, 2 x 2 taps


def test_compare_fails_on_a_scrubbed_nan():
    O, Ob, R, Rb = _pair()
    Ob['y'] = torch.nan_to_num(Ob['y'], nan=0.0)
    with pytest.raises(AssertionError, match='scrubbed'):
        NF.compare_all('dw', O, Ob, R, Rb, NF.NAN, True)


def test_compare_fails_on_a_padding_cell_removed_by_a_multiplication():
    """the depthwise forward of a kernel that reads the clamped neighbour of a padding cell and multiplies it by zero: exact
    on finite data, a NaN at every output whose window hangs over the edge next to the site"""
    O, Ob, R, Rb = _pair()
    assert torch.equal(O['y'].double(), R['y'].float().double())
    leak = Ob['y'].clone()
    leak[1, 3, 2, 6] = leak[1, 3, 2, 6] + 0.0 * NF.NAN
    Ob['y'] = leak
    with pytest.raises(AssertionError, match='outside it poisoned'):
        NF.compare_all('dw', O, Ob, R, Rb, NF.NAN, True)


def test_compare_takes_either_side_where_torch_multiplies_padding_and_nothing_beyond():
    ins = NF.linear_inputs('dw', (3, 1, 6, 2, 7, 7))
    bad = dict(ins)
    bad['w'] = NF.inject(ins['w'], (2, 0, 0, 0), NF.NAN)
    R, Rb, Wb = NF.ref_dw(ins, 3, 1), NF.ref_dw(bad, 3, 1), NF.torch_conv('dw', bad, k=3, s=1)
    O = {k: v.float() for k, v in R.items()}
    NF.compare_all('dw', O, {k: v.float() for k, v in Rb.items()}, R, Rb, NF.NAN, True, Wb)     # the kernel that selects
    NF.compare_all('dw', O, {k: v.float() for k, v in Wb.items()}, R, Rb, NF.NAN, True, Wb)     # the one that multiplies
    with pytest.raises(AssertionError, match='outside it poisoned'):
        NF.compare_all('dw', O, {k: v.float() for k, v in Wb.items()}, R, Rb, NF.NAN, True)
    leak = {k: v.float() for k, v in Wb.items()}
    leak['y'][0, 3, 3, 3] = NF.NAN                            # another channel
    with pytest.raises(AssertionError, match='outside it poisoned'):
        NF.compare_all('dw', O, leak, R, Rb, NF.NAN, True, Wb)


def test_compare_fails_on_a_moved_bit_and_on_a_wrong_class():
    O, Ob, R, Rb = _pair()
    Ob['y'][0, 0, 0, 0] = torch.nextafter(Ob['y'][0, 0, 0, 0], torch.tensor(9.0))
    with pytest.raises(AssertionError, match='moved'):
        NF.compare_all('dw', O, Ob, R, Rb, NF.NAN, True)
    ins = NF.linear_inputs('dw', (3, 1, 6, 2, 7, 7))
    bad = dict(ins)
    bad['x'] = NF.inject(ins['x'], (1, 3, 0, 6), NF.PINF)
    R, Rb = NF.ref_dw(ins, 3, 1), NF.ref_dw(bad, 3, 1)
    O, Ob = {k: v.float() for k, v in R.items()}, {k: v.float() for k, v in Rb.items()}
    NF.compare_all('dw', O, Ob, R, Rb, NF.PINF, True)
    wrong = {k: v.clone() for k, v in Ob.items()}
    wrong['y'][torch.isinf(wrong['y'])] = NF.NAN              # what a bf16 split makes of an infinity
    NF.compare_all('dw', O, wrong, R, Rb, NF.PINF, False)
    with pytest.raises(AssertionError, match='NaN where'):
        NF.compare_all('dw', O, wrong, R, Rb, NF.PINF, True)
    wrong = {k: v.clone() for k, v in Ob.items()}
    wrong['y'] = torch.where(torch.isinf(wrong['y']), -wrong['y'], wrong['y'])
    with pytest.raises(AssertionError, match='wrong sign'):
        NF.compare_all('dw', O, wrong, R, Rb, NF.PINF, True)
