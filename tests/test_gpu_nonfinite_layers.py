"""NaN / Inf propagation and containment in every call of litepose_amd.nn.functional, forward and backward, by the method of
tests/_nonfinite.py: one element of one operand is set to NaN (at every site) or to an infinity (at the first and the last
element), and the non-finite outputs have to be exactly the site's cone -- what torch's fp64 result on the same inputs marks
-- while every output that does not depend on the site keeps the bits of the clean run.

The operands are taken in turn: x, the weight, grad_y, and for BatchNorm gamma, beta and the residual.  The rows are rows of
the existing tables, for each component of a form key the smallest that has it (_nonfinite.rows).  A row of more than
_nonfinite.LARGE elements runs the short plan.

BatchNorm, the depthwise kernels: plain fp32 / fp64 arithmetic, so with an infinity the class and the sign are the truth's
too.  1x1, stem, transposed pair: operands are taken apart into bf16 pieces, an infinity may come out as a NaN, and only
non-finiteness is compared.

What the tests found in the parent's kernels (each failed there and passes now):
  bn_fwd_kernel, bn_apply_kernel   ``var > 0 ? var : 0`` made a NaN variance 0: stat, running_var and y of a channel holding a
                                   NaN or an Inf stayed finite; fminf(fmaxf(z, lo), hi) made a NaN z 0 (ReLU, ReLU6) or -inf
  pw2_kernel, dw_kernel,           the same clamp with lo = -inf, hi = +inf under ACT_NONE: a NaN sum left every training 1x1
  dw_pair_kernel, dw_pair16_kernel and depthwise as -inf (all 15 + 18 rows)
  bn_bwd_*_kernel (bn_pass)        ``z > 0`` closed the gate at a NaN z, where torch's backward (``z <= 0 ? 0 : g``) passes it:
                                   dbeta of a NaN channel was 0 instead of the sum of dy
  dw_wgrad_kernel, stem_wgrad_kernel,   LEAKS, found and KEPT: a zero-filled halo of the partner operand is multiplied, so a NaN next
  deconv_wgrad_kernel,                  to the border poisons outputs that do not depend on it and that torch leaves finite
  deconv_raw_kernel                     (_nonfinite.HALO_KERNELS, halo_products).  One strict expected failure each below; the
                                        allowance is counted, and the last test fails if anything else passes through it
  and two things that are no errors: torch's conv2d / conv_transpose2d multiply their own zero padding (a NaN weight tap
  poisons border outputs it meets only as padding): between the cone and torch's mask a kernel may go either way
  (_nonfinite.torch_conv); torch's batch_norm associates an infinite gamma differently from its own definition
  (_nonfinite.ref_bn follows the definition, as the kernel does).

Synchronised BatchNorm (F.bn_sync_*, the ranks simulated as tests/test_gpu_sync_bn.py does) has rows of its own below, against
ref_bn over the concatenated batch: its kernels share bn_moments, bn_fwd_slice and bn_pass with the plain ones, and the rows
passed on the first run.  The dense K x K convolution: tests/test_gpu_nonfinite_conv.py.

Sensitivity, on MI355X: scratch builds with one wrong edit each (not committed), against this file and against the files the
suite had for the same kernels (tests/test_gpu_layer_grad.py and tests/test_gpu_train_forms.py, -k of the layer kind).
  edit                                                   the files before      this file
  dw_kernel: the staged tile's padding removed by        152 pass              7 of 18 test_depthwise rows fail: every stride-2
    ``v * (ok ? 1 : 0)`` instead of the select                                 row (the 'quad' sites: a clamped 16-byte load at
                                                                               the edge re-reads columns 0..3 / W-4..W-1)
  bn_bwd_stats / bn_bwd_apply: ``g = dy * (pass ? 1 : 0)``  77 pass            12 of 37 BatchNorm tests fail: every training-mode
    instead of ``pass ? dy : 0``                                               row with ReLU or ReLU6 (a NaN or Inf grad_y at a
                                                                               closed cell reaches dx, dgamma, dbeta)
  pw2_kernel: the odd-K tail's half == 1 lanes load the   106 pass             4 of 15 test_pointwise rows fail: every row with
    next row too (channel 0 of the next image; not for                         an odd K in the forward or the data gradient
    the last image, where it would leave the buffer),                          (16 / 32 -> 17, 33 -> 7), at the 'next image'
    against the zero weight of the pack                                        site: y or dX of the image before goes NaN

Wall time on MI355X: this file and tests/test_gpu_nonfinite_train.py together 29 s for 98 tests and 5 expected failures (the
slowest, 7x2x8x8192x4x4, 2.3 s)."""
import time

import pytest
import torch

import _nonfinite as NF
from litepose_amd.nn import functional as F

pytestmark = pytest.mark.gpu
_id = lambda r: 'x'.join(str(v) for v in r)               # noqa: E731


def _cuda(ins):
    return {k: (None if v is None else v.cuda()) for k, v in ins.items()}


# ------------------------------------------------------------------ the device side of each op
def dev_pw(d):
    gx, gw = F.pw_backward(d['dy'], d['x'], d['w'])
    return dict(y=F.pw_forward(d['x'], d['w']), gx=gx, gw=gw)


def dev_dw(d, k, s):
    gx, gw = F.dw_backward(d['dy'], d['x'], d['w'], s)
    return dict(y=F.dw_forward(d['x'], d['w'], s), gx=gx, gw=gw)


def dev_stem(d):
    return dict(y=F.stem_forward(d['x'], d['w']), gw=F.stem_backward(d['dy'], d['x']))


def dev_deconv(d):
    y = F.deconv_forward(d['xa'], d['wa'], d['xb'], d['wb'])
    gxa, gxb, gwa, gwb = F.deconv_backward(d['dy'], d['xa'], d['wa'], d['xb'], d['wb'])
    out = dict(y=y, gxa=gxa, gwa=gwa)
    if d['xb'] is not None:
        out.update(gxb=gxb, gwb=gwb)
    return out


def dev_bn(d, act, training):
    running = torch.stack([d['rm'], d['rv']]).contiguous()
    y, stat = F.bn_forward(d['x'], d['gamma'], d['beta'], running, act, d['res'], training, NF.MOM, NF.EPS)
    if not training:
        assert stat is None and NF.bitwise(running, torch.stack([d['rm'], d['rv']]))
        return dict(y=y)
    gx, gg, gb = F.bn_backward(d['dy'], d['x'], d['gamma'], d['beta'], stat, act)
    return dict(y=y, mean=stat[0], invstd=stat[1], rm=running[0], rv=running[1], gx=gx, gg=gg, gb=gb)


DEV = {'pw': dev_pw, 'dw': dev_dw, 'stem': dev_stem, 'deconv': dev_deconv}


def _linear(kind, row, exact):
    t0 = time.time()
    ref, dev, kw = NF.LINEAR[kind], DEV[kind], NF.linear_kw(kind, row)
    ins = NF.linear_inputs(kind, row)
    large = NF._numel(kind, row) > NF.LARGE
    R, O = ref(ins, **kw), dev(_cuda(ins), **kw)
    runs = 0
    for operand in [k for k, v in ins.items() if v is not None]:
        for (name, idx), vname in NF.plan(NF.linear_sites(kind, row, operand, ins[operand].shape), large):
            bad = dict(ins)
            bad[operand] = NF.inject(ins[operand], idx, NF.VALUES[vname])
            wide = None if kind == 'pw' else NF.torch_conv(kind, bad, **kw)        # a 1x1 has no padding
            halo = NF.halo_products(kind, row, operand, idx, {k: v.shape for k, v in R.items()})
            sizes = NF.compare_all('%s %s %s at %s %s %s:' % (kind, _id(row), operand, name, idx, vname), O,
                                   dev(_cuda(bad), **kw), R, ref(bad, **kw), NF.VALUES[vname], exact, wide, halo)
            runs += 1
            if name == 'last' and vname == 'nan' and operand != 'w':       # a dead weight tap has an empty cone
                assert sum(sizes.values()) > 0, (kind, row, operand)
    print('%s %s: %d injected runs, %.2f s' % (kind, _id(row), runs, time.time() - t0))


# ------------------------------------------------------------------ the known leaks, one strict expected failure each
# (kind, row, operand, site name): the smallest row of the kind; against the cone and torch's own mask, WITHOUT the allowance
# of _nonfinite.halo_products.  A kernel that is changed to select makes its case pass, which strict turns into a failure:
# the allowance for it in HALO_KERNELS is then to be removed.
KNOWN_LEAKS = [('dw', (3, 1, 8, 1, 6, 10), 'x', 'last'), ('dw', (7, 2, 4, 9, 4, 4), 'x', 'last'), ('stem', (2, 10, 14), 'x', 'last'),
               ('deconv', (5, 0, 3, 2, 5, 7), 'wa', 'first'), ('deconv', (5, 0, 3, 2, 5, 7), 'dy', 'last')]


@pytest.mark.parametrize('kind, row, operand, site', KNOWN_LEAKS, ids=['%s-%s-%s' % (k[0], _id(k[1]), k[2]) for k in KNOWN_LEAKS])
@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason='a zero-filled halo is multiplied, not selected: dw_wgrad_kernel (layer_kernels.hip), stem_wgrad_kernel '
                          'and deconv_wgrad_kernel (conv_grad_kernels.hip), deconv_raw_kernel (calib_kernels.hip) poison outputs '
                          'that do not depend on the site and that torch leaves finite')
def test_a_halo_is_multiplied_not_selected(kind, row, operand, site):
    assert row in NF.rows(kind) and (kind, operand) in NF.HALO_KERNELS
    ref, dev, kw = NF.LINEAR[kind], DEV[kind], NF.linear_kw(kind, row)
    ins = NF.linear_inputs(kind, row)
    idx = dict(NF.linear_sites(kind, row, operand, ins[operand].shape))[site]
    bad = dict(ins)
    bad[operand] = NF.inject(ins[operand], idx, NF.NAN)
    NF.compare_all('%s %s %s at %s:' % (kind, _id(row), operand, site), dev(_cuda(ins), **kw), dev(_cuda(bad), **kw),
                   ref(ins, **kw), ref(bad, **kw), NF.NAN, False, NF.torch_conv(kind, bad, **kw))


@pytest.mark.parametrize('row', NF.rows('pw'), ids=_id)
def test_pointwise(row):
    _linear('pw', row, exact=False)


@pytest.mark.parametrize('row', NF.rows('dw'), ids=_id)
def test_depthwise(row):
    _linear('dw', row, exact=True)


@pytest.mark.parametrize('row', NF.rows('deconv'), ids=_id)
def test_deconv_pair(row):
    _linear('deconv', row, exact=False)


@pytest.mark.parametrize('row', NF.rows('stem'), ids=_id)
def test_stem(row):
    _linear('stem', row, exact=False)


# ------------------------------------------------------------------ BatchNorm
def _closed_cell(R, c):
    """a cell of channel c the activation closed in the clean truth (y is exactly the bound there), or None"""
    y = R['y'][:, c]
    hit = torch.nonzero((y == 0) | (y == 6))
    return None if not hit.shape[0] else (int(hit[0, 0]), c, int(hit[0, 1]), int(hit[0, 2]))


def _bn(row, act, with_res, training):
    t0 = time.time()
    ins = NF.bn_inputs(row, with_res)
    n, c, h, w = row
    large = NF._numel('bn', row) > NF.LARGE
    R, O = NF.ref_bn(ins, act, training), dev_bn(_cuda(ins), act, training)
    todo = []
    for operand in ('x', 'gamma', 'beta', 'res', 'dy', 'rm', 'rv'):
        if ins[operand] is None or (operand == 'dy' and not training) or (operand in ('rm', 'rv') and large):
            continue
        s = NF.sites(ins[operand].shape, [(16, 16)], ragged=bool(c % 4)) if ins[operand].dim() == 4 else NF.sites((c,))
        todo += [(operand, site, v) for site, v in NF.plan(s, large)]
    if training and act is not None and not with_res:
        # a non-finite upstream gradient at a cell the activation closed: torch selects, so it goes nowhere
        cell = _closed_cell(R, c // 2)
        if cell is not None:
            todo += [('dy', ('closed', cell), v) for v in ('nan', '+inf')]
    for operand, (name, idx), vname in todo:
        bad = dict(ins)
        bad[operand] = NF.inject(ins[operand], idx, NF.VALUES[vname])
        if operand == 'rv' and vname == '-inf':
            continue                                         # a negative variance is no input of a BatchNorm
        # an infinity in gamma, beta, a running value or grad_y: inf * 0 and inf - inf depend on how the affine map and the
        # backward's bracket are associated (torch's own batch_norm and its definition differ there), so only
        # non-finiteness is compared; an infinity in x or the residual has one answer
        exact = vname == 'nan' or operand in ('x', 'res')
        NF.compare_all('bn %s %s %s %s at %s %s %s:' % (_id(row), act, 'train' if training else 'eval', operand, name, idx,
                                                        vname), O, dev_bn(_cuda(bad), act, training), R,
                       NF.ref_bn(bad, act, training), NF.VALUES[vname], exact)
    print('bn %s %s %s: %d injected runs, %.2f s' % (_id(row), act, 'train' if training else 'eval', len(todo), time.time() - t0))


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('row', NF.rows('bn'), ids=_id)
def test_batch_norm_relu6(row, with_res, training):
    _bn(row, 'relu6', with_res, training)


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('act', [None, 'relu'], ids=['none', 'relu'])
@pytest.mark.parametrize('row', NF.rows('bn')[:3], ids=_id)
def test_batch_norm_every_activation(row, act, training):
    _bn(row, act, True, training)
    _bn(row, act, False, training)


def test_batch_norm_act_through_autograd_keeps_a_nan_for_good():
    """the module-level function: after a batch with one NaN the running pair of that channel is NaN, and a clean batch
    after it leaves it NaN, as torch's BatchNorm2d does"""
    ins = NF.bn_inputs((3, 4, 5, 7), False)
    d = _cuda(ins)
    bad = NF.inject(d['x'], (1, 2, 3, 4), NF.NAN)
    bn = torch.nn.BatchNorm2d(4, eps=NF.EPS, momentum=NF.MOM).double()
    bn.running_mean.copy_(ins['rm']), bn.running_var.copy_(ins['rv'])
    for x in (bad, d['x']):
        F.batch_norm_act(x, d['gamma'], d['beta'], d['rm'], d['rv'], 'relu6', None, True, NF.MOM, NF.EPS)
        bn(x.cpu().double())
        for mine, theirs in ((d['rm'], bn.running_mean), (d['rv'], bn.running_var)):
            assert torch.isnan(mine).cpu().tolist() == torch.isnan(theirs).tolist() == [False, False, True, False]


# ------------------------------------------------------------------ synchronised BatchNorm
# The ranks are simulated in one process exactly as tests/test_gpu_sync_bn.py does it: every shard's row, the rows stacked in
# rank order, the second half of each pass per shard, every shard its own allocation.  The truth is ref_bn over the
# concatenated batch in training mode.  Rows of that file's table, named directly (MIN_PLANE is a rule of ``pick``):
# (per-rank N, C, H, W, act, residual)
SYNC_CASES = [((3, 1, 2), 5, 3, 5, 'relu6', True),          # uneven ranks, the scalar walk
              ((2, 2), 16, 16, 16, 'relu6', True),
              ((2, 3), 8, 33, 33, 'relu6', True),           # several slices per channel
              ((3, 1, 2), 5, 3, 5, None, False)]
SYNC_IDS = ['%s-c%d-%dx%d-%s-%s' % ('+'.join(map(str, c[0])), c[1], c[2], c[3], c[4] or 'none', 'res' if c[5] else 'plain')
            for c in SYNC_CASES]


def dev_bn_sync(d, ns, act):
    """-> the outputs of dev_bn over the concatenated batch -- y and grad_x concatenated in rank order, the kept and the
    running pair of rank 0 (every rank's are the same bits: asserted here, NaNs included), grad_gamma / grad_beta the fp64
    sum of the ranks' shares -- and the ranks' shares themselves"""
    c = d['x'].shape[1]
    xs, dys = [v.clone() for v in d['x'].split(list(ns))], [v.clone() for v in d['dy'].split(list(ns))]
    ress = [v.clone() for v in d['res'].split(list(ns))] if d['res'] is not None else [None] * len(ns)
    running0 = torch.stack([d['rm'], d['rv']]).contiguous()
    rows = torch.stack([F.bn_sync_stats(v) for v in xs])
    ys, stats, runs = [], [], []
    for v, r in zip(xs, ress):
        running = running0.clone()
        y, stat = F.bn_sync_forward(v, d['gamma'], d['beta'], running, rows, act, r, NF.MOM, NF.EPS)
        ys.append(y), stats.append(stat), runs.append(running)
    brows = torch.stack([F.bn_sync_backward_stats(g, v, d['gamma'], d['beta'], s, act) for g, v, s in zip(dys, xs, stats)])
    grads = [F.bn_sync_backward(g, v, d['gamma'], d['beta'], s, brows, rank, act)
             for rank, (g, v, s) in enumerate(zip(dys, xs, stats))]
    for stat, running in zip(stats[1:], runs[1:]):
        assert NF.bitwise(stat, stats[0]) and NF.bitwise(running, runs[0]), 'the ranks hold different statistics'
    out = dict(y=torch.cat(ys), mean=stats[0][:c], invstd=stats[0][c:2 * c], rm=runs[0][0], rv=runs[0][1],
               gx=torch.cat([g[0] for g in grads]), gg=sum(g[1].double() for g in grads), gb=sum(g[2].double() for g in grads))
    return out, [(g[1], g[2]) for g in grads]


def _sync_todo(ins, ns):
    n, c, h, w = ins['x'].shape
    mid = len(ns) // 2                                        # a rank that is neither the first nor, with three, the last
    xs = [('first', (0, 0, 0, 0)), ('last', (n - 1, c - 1, h - 1, w - 1)), ('rank %d' % mid, (sum(ns[:mid]), c // 2, h // 2, w // 2))]
    todo = [('x', site, v) for site, v in NF.plan(xs)]
    for operand in ('gamma', 'beta', 'res', 'dy'):
        if ins[operand] is not None:
            todo += [(operand, site, v) for site, v in NF.plan(NF.sites(ins[operand].shape)[:2])]
    return todo


@pytest.mark.parametrize('case', SYNC_CASES, ids=SYNC_IDS)
def test_sync_batch_norm(case):
    """A NaN in one rank's x: the channel's y and grad_x are NaN on every rank, mean, invstd and the running pair are NaN
    with the same bits on every rank, every rank's grad_gamma of the channel is NaN, and every other channel keeps the clean
    call's bits.  grad_beta follows the truth: the sum of what the gate lets through, and torch's gate passes a NaN z, so
    every rank's share stays the finite sum of its grad_y (tests/test_nonfinite_cpu.py pins that of torch)."""
    t0 = time.time()
    ns, c, h, w, act, with_res = case
    ins = NF.bn_inputs((sum(ns), c, h, w), with_res)
    R, (O, _) = NF.ref_bn(ins, act, True), dev_bn_sync(_cuda(ins), ns, act)
    todo = _sync_todo(ins, ns)
    for operand, (name, idx), vname in todo:
        bad = dict(ins)
        bad[operand] = NF.inject(ins[operand], idx, NF.VALUES[vname])
        Rb = NF.ref_bn(bad, act, True)
        Ob, shares = dev_bn_sync(_cuda(bad), ns, act)
        what = 'sync bn %s %s %s at %s %s %s:' % (SYNC_IDS[SYNC_CASES.index(case)], act, operand, name, idx, vname)
        NF.compare_all(what, O, Ob, R, Rb, NF.VALUES[vname], vname == 'nan' or operand in ('x', 'res'))
        if operand == 'x':
            ch = idx[1]
            assert bool(torch.isnan(Rb['gg'][ch])) and bool(torch.isfinite(Rb['gb'][ch]))
            for rank, (gg, gb) in enumerate(shares):
                assert bool(torch.isnan(gg[ch])) and bool(torch.isfinite(gb[ch])), (what, rank)
                assert bool(torch.isfinite(gg[:ch]).all()) and bool(torch.isfinite(gg[ch + 1:]).all()), (what, rank)
    print('sync bn %s: %d injected runs, %.2f s' % (SYNC_IDS[SYNC_CASES.index(case)], len(todo), time.time() - t0))


@pytest.mark.parametrize('act, with_res', [('relu6', True), (None, False)], ids=['relu6-res', 'none-plain'])
def test_sync_batch_norm_of_one_rank_has_the_masks_of_the_plain_calls(act, with_res):
    row = (6, 5, 3, 5)
    ins = NF.bn_inputs(row, with_res)
    for operand, (name, idx), vname in _sync_todo(ins, (6,)):
        bad = dict(ins)
        bad[operand] = NF.inject(ins[operand], idx, NF.VALUES[vname])
        d = _cuda(bad)
        plain, (sync, _) = dev_bn(d, act, True), dev_bn_sync(d, (6,), act)
        for k in plain:
            a, b = plain[k].double(), sync[k].double()
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), (operand, name, vname, k)
            fin = torch.isfinite(a)
            assert torch.equal(a[fin], b[fin]), (operand, name, vname, k)


# ------------------------------------------------------------------ what the allowance let through
def test_nothing_leaks_but_the_known_halos():
    """runs after the row tests of this file: every output they let through beyond the cone and torch's mask belongs to a
    kernel and an operand HALO_KERNELS names"""
    assert NF.LEAKS, 'the row tests of this file have not run, or the halo kernels now select: remove their allowance'
    for what, count in NF.LEAKS.items():
        kind, _, operand = what.split()[:3]
        assert (kind, operand) in NF.HALO_KERNELS and what.split()[-1] in NF.HALO_KERNELS[(kind, operand)][0], (what, count)
    print('%d injected runs poisoned %d outputs through a multiplied halo' % (len(NF.LEAKS), sum(NF.LEAKS.values())))
