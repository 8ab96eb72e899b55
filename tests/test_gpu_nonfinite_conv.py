"""NaN / Inf propagation and containment in the dense K x K convolution (lp_conv_forward / lp_conv_backward,
litepose_amd.nn.functional.conv_forward / conv_backward / dense_conv) by the method of tests/_nonfinite.py, as
tests/test_gpu_nonfinite_layers.py does it for the other training layers: one element of xa, wa, xb, wb, the bias or grad_y
is set to NaN (at every site) or to an infinity (at the first and the last element); the non-finite outputs have to be the
site's cone, and every output that does not depend on the site keeps the bits of the clean run.

The truth is _nonfinite.ref_conv, the op of tests/_dense_conv_check.py summed tap by tap in fp64; torch's own conv2d
(_nonfinite.torch_conv) multiplies its padding, and between the two masks a kernel may go either way.  The rows and what each
is there for: _nonfinite.CONV_PLANES and its neighbours.  The sites: the corners, the edge, the 8 x 16 tile of the weight
gradient and convk3_kernel's tile in each operand's own coordinates, the ragged channel, the corner taps of the weights.

y, grad_xa, grad_xb come from convk3_kernel on the bf16x3 split, where inf - bf16(inf) is a NaN: non-finiteness only.
grad_wa, grad_wb (fp32 MFMA products, fp64 slice sum) and grad_bias (fp64) also have the class and the sign of the truth.

What the rows found:
  conv_wgrad_kernel   FIXED.  It walks all 128 pixels of every 8 x 16 tile; a pixel outside the plane had a zero grad_y
                      but a real input cell as its partner, so a NaN in the last rows or columns of x reached taps whose sum
                      never holds that cell -- beyond torch's mask as well.  On the parent's kernel all 18 rows whose output
                      plane does not fill its tiles failed on grad_wa, at the 'last' site of xa, the first that lies in the
                      last row (5x0x3x2x5x7x3x1x0: a cone of 12 taps, 15 more poisoned; 3x0x40x2x5x7x7x1x0: 640 and 1320),
                      and the three 8 x 16 controls passed.  The kernel now selects, and all 21 rows pass; on finite data
                      its results are the parent's bits (the ragged-slice cases of tests/test_gpu_dense_conv.py, compared
                      once).
  the data gradient   KEPT, a known deviation: convk3_kernel's stride-1 launch over grad_y -- at stride 2 over grad_y spread
                      over the input plane -- with the flipped, transposed weights multiplies the zeros of its halo and of
                      the dilation, so a non-finite weight tap poisons its whole input channel of grad_x, where the truth and
                      torch reach the cells of the tap's parity inside the border only (_nonfinite.HALO_KERNELS,
                      halo_products).  One strict expected failure per (stride, upsample) below; the allowance is counted, and
                      the last test fails if anything else passes through it.
  a non-finite grad_y at stride 2 and everything through pool2_kernel stay inside the cone: no allowance, the rows pass.

Wall time on MI355X: 16 s for the 26 tests and 4 expected failures of this file, 1428 injected runs; the slowest row,
33x7x9x1x11x21x7x1x0, 2.2 s, nearly all of it the fp64 truth on the CPU."""
import time

import pytest
import torch

import _nonfinite as NF
from litepose_amd.nn import functional as F

pytestmark = pytest.mark.gpu
_id = lambda r: 'x'.join(str(int(v)) for v in r)          # noqa: E731
EXACT = {'y': False, 'gxa': False, 'gxb': False, 'gwa': True, 'gwb': True, 'gb': True}


def _cuda(ins):
    return {k: (None if v is None else v.cuda()) for k, v in ins.items()}


# ------------------------------------------------------------------ the device side
def dev_direct(d, k, s, ups):
    y = F.conv_forward(d['xa'], d['wa'], d['xb'], d['wb'], d['bias'], s, bool(ups))
    gxa, gwa, gxb, gwb, gb = F.conv_backward(d['dy'], d['xa'], d['wa'], d['xb'], d['wb'], s, bool(ups), (True,) * 5)
    out = dict(y=y, gxa=gxa, gwa=gwa, gb=gb)
    if d['xb'] is not None:
        out.update(gxb=gxb, gwb=gwb)
    return out


def dev_autograd(d, k, s, ups):
    """F.dense_conv + autograd: every input that is there requires a gradient; without a bias there is no grad_bias"""
    names = [n for n in ('xa', 'wa', 'xb', 'wb', 'bias') if d[n] is not None]
    leaves = {n: d[n].detach().clone().requires_grad_() for n in names}
    y = F.dense_conv(leaves['xa'], leaves['wa'], leaves.get('xb'), leaves.get('wb'), leaves.get('bias'), stride=s,
                     upsample=bool(ups))
    g = dict(zip(names, torch.autograd.grad(y, [leaves[n] for n in names], d['dy'])))
    out = dict(y=y.detach(), gxa=g['xa'], gwa=g['wa'])
    if 'xb' in g:
        out.update(gxb=g['xb'], gwb=g['wb'])
    if 'bias' in g:
        out['gb'] = g['bias']
    return out


# ------------------------------------------------------------------ the truth of a row, once per (operand, site, value)
_truths = {}


def _truth(row):
    if row not in _truths:
        kw, ins = NF.linear_kw('conv', row), NF.linear_inputs('conv', row)
        R = NF.ref_conv(ins, **kw)
        shapes = {k: v.shape for k, v in R.items()}
        runs = []
        for operand in [k for k, v in ins.items() if v is not None]:
            for (name, idx), vname in NF.plan(NF.linear_sites('conv', row, operand, ins[operand].shape)):
                bad = dict(ins)
                bad[operand] = NF.inject(ins[operand], idx, NF.VALUES[vname])
                runs.append((operand, name, idx, vname, bad, NF.ref_conv(bad, **kw), NF.torch_conv('conv', bad, **kw),
                             NF.halo_products('conv', row, operand, idx, shapes)))
        _truths[row] = (ins, R, runs)
    return _truths[row]


def _one(what, O, Ob, R, Rb, Wb, halo, vname):
    assert set(O) == set(Ob) and set(O) <= set(R), (what, sorted(O), sorted(R))
    return {k: NF.compare('%s %s' % (what, k), O[k], Ob[k], R[k], Rb[k], NF.VALUES[vname], EXACT[k], Wb[k], halo.get(k))
            for k in O}


def _row(row, dev):
    t0 = time.time()
    kw = NF.linear_kw('conv', row)
    ins, R, runs = _truth(row)
    O = dev(_cuda(ins), **kw)
    for operand, name, idx, vname, bad, Rb, Wb, halo in runs:
        sizes = _one('conv %s %s at %s %s %s:' % (_id(row), operand, name, idx, vname), O, dev(_cuda(bad), **kw), R, Rb, Wb,
                     halo, vname)
        if name == 'last' and vname == 'nan':
            assert sum(sizes.values()) > 0, (row, operand)
    print('conv %s: %d injected runs, %.2f s' % (_id(row), len(runs), time.time() - t0))


# ------------------------------------------------------------------ the known deviation, one strict expected failure each
# (row, operand): a NaN in the first weight tap, against the cone and torch's own mask WITHOUT the allowance of
# _nonfinite.halo_products: stride 1 (the tap meets the halo below the last row and right of the last column), through the
# upsample (K = 7: the 2x2 sums spread what the tap reaches, and with K = 3 on these planes they already reach every source
# cell, so that row has nothing beyond its cone), and stride 2 (it meets the dilation's zeros as well) with one source and
# with two.  A data gradient that is changed to select makes its case pass, which strict turns into a failure: the allowance
# in HALO_KERNELS is then to go.
KNOWN_LEAKS = [((5, 0, 3, 2, 5, 7, 3, 1, 0, True), 'wa'), ((5, 0, 3, 2, 3, 5, 7, 1, 1, True), 'wa'),
               ((5, 0, 3, 2, 6, 10, 5, 2, 0, False), 'wa'), ((33, 7, 9, 1, 18, 36, 5, 2, 0, True), 'wb')]


@pytest.mark.parametrize('row, operand', KNOWN_LEAKS, ids=['%s-%s' % (_id(r), o) for r, o in KNOWN_LEAKS])
@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason='the data gradient is convk3_kernel at stride 1 over the (stride 2: zero-dilated) grad_y: the zeros of '
                          'the halo and of the dilation are multiplied, and a non-finite weight tap poisons its whole input '
                          'channel of grad_x (csrc/dense_grad_kernels.hip, csrc/convk_kernels.hip; DESIGN.md 4f)')
def test_the_data_gradient_multiplies_its_halo_and_its_dilation(row, operand):
    assert row in NF.rows('conv') and ('conv', operand) in NF.HALO_KERNELS
    kw = NF.linear_kw('conv', row)
    ins, R, runs = _truth(row)
    _, name, idx, vname, bad, Rb, Wb, halo = [r for r in runs if r[0] == operand and r[1] == 'first' and r[3] == 'nan'][0]
    key = NF.HALO_KERNELS[('conv', operand)][0]
    O, Ob = dev_direct(_cuda(ins), **kw), dev_direct(_cuda(bad), **kw)
    for k in O:                                              # every other output holds without the allowance
        if k != key:
            NF.compare('conv %s %s first: %s' % (_id(row), operand, k), O[k], Ob[k], R[k], Rb[k], NF.NAN, EXACT[k], Wb[k])
    NF.compare('conv %s %s first: %s' % (_id(row), operand, key), O[key], Ob[key], R[key], Rb[key], NF.NAN, False, Wb[key])


@pytest.mark.parametrize('row', NF.rows('conv'), ids=_id)
def test_dense_conv(row):
    _row(row, dev_direct)


@pytest.mark.parametrize('row', [r for r in NF.rows('conv') if r[6] == 3 and r[3:6] in ((2, 5, 7), (2, 3, 5), (2, 6, 10))], ids=_id)
def test_dense_conv_through_autograd(row):
    """one row per (stride, upsample) once more through F.dense_conv and autograd"""
    _row(row, dev_autograd)


def test_one_autograd_row_per_form():
    got = [r[7:9] for r in NF.rows('conv') if r[6] == 3 and r[3:6] in ((2, 5, 7), (2, 3, 5), (2, 6, 10))]
    assert sorted(got) == sorted(NF.CONV_FORMS)


# ------------------------------------------------------------------ what the allowance let through
def test_nothing_leaks_but_the_known_data_gradient():
    """runs after the row tests of this file: every output of a dense convolution they let through beyond the cone and
    torch's mask is a data gradient with the site in its own weights"""
    mine = {what: count for what, count in NF.LEAKS.items() if what.split()[0] == 'conv'}
    assert mine, 'the row tests of this file have not run, or the data gradient now selects: remove its allowance'
    for what, count in mine.items():
        operand = what.split()[2]
        assert ('conv', operand) in NF.HALO_KERNELS and what.split()[-1] == NF.HALO_KERNELS[('conv', operand)][0], (what, count)
    # every stride-2 row leaks at its first tap: the dilation
    for row in [r for r in NF.rows('conv') if r[7] == 2]:
        assert any(w.startswith('conv %s wa at first' % _id(row)) for w in mine), row
    print('%d injected runs poisoned %d outputs of a data gradient through a multiplied halo or dilation'
          % (len(mine), sum(mine.values())))
