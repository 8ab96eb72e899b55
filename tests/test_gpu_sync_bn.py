"""The synchronised BatchNorm calls (lp_bn_sync_*, litepose_amd.nn.functional.bn_sync_*) in ONE process: the ranks are
simulated -- every shard's row is computed, the rows are stacked in rank order (what the all-gather would hand every
rank) and the second half of each pass runs per shard.

  * oracle: the concatenated y, the running pair, grad_x and the rank-summed grad_gamma / grad_beta against fp64 torch
    BatchNorm over the concatenated batch on the CPU, held to the per-layer BatchNorm rule of tests/test_gpu_layer_grad.py
    (its docstring derives the constants: y 5 (6 with a residual), everything else 3, times 2^-24 times the sum of the
    absolute values of the expression's terms); the rank sum of grad_gamma / grad_beta is taken in fp64 here, so the W
    single roundings of the ranks' shares together stay within the one rounding the rule counts
  * rank identity: mean, invstd, the total count and the running pair are the same bits on every simulated rank
  * W = 1: the same bits as lp_bn_forward / lp_bn_backward on the same inputs
  * against lp_bn_forward on the concatenated batch on the same GPU: both are within the rule of the truth, so they differ
    by at most twice the rule; the number of elements whose bits differ is printed (no bitwise claim: the sums associate
    differently)
  * two calls and a graph replay of one rank's forward + backward, rows pre-gathered, give the same bits"""
import pytest
import torch
import torch.nn.functional as TF

import _poison as po
import test_gpu_layer_grad as LG
from litepose_amd import _native as nv
from litepose_amd.nn import functional as F

pytestmark = pytest.mark.gpu
U, EPS, MOM, EDGE, ACT = LG.U, LG.EPS, LG.MOM, LG.EDGE, LG.ACT

# (per-rank N, C, H, W, act, residual)
CASES = [
    ((1, 1), 1, 1, 1, 'relu6', False),                      # total count 2
    ((1, 1), 1, 1, 1, None, True),
    ((1, 1), 24, 2, 2, 'relu6', True),                      # the deepest plane of the golden training case
    ((1, 1), 24, 2, 2, 'relu', False),
    ((3, 1, 2), 5, 3, 5, 'relu6', True),                    # uneven ranks, the scalar walk
    ((3, 1, 2), 5, 3, 5, None, False),
] + [((2, 2), 16, 16, 16, act, res) for act in (None, 'relu', 'relu6') for res in (False, True)] + [
    ((2, 3), 8, 64, 64, 'relu6', True),                     # several slices per channel, 16-byte walk
    ((2, 3), 8, 33, 33, 'relu', False),                     # several slices per channel, scalar walk
]
IDS = ['%s-c%d-%dx%d-%s-%s' % ('+'.join(map(str, c[0])), c[1], c[2], c[3], c[4] or 'none', 'res' if c[5] else 'plain')
       for c in CASES]
_runs = {}


def _slices(n, c, hw):
    """slices per channel of bn_cut: the workspace is one (sum, sumsq) fp64 pair per workgroup"""
    return nv.lib().lp_bn_workspace_bytes(n, c, hw) // (16 * c)


def _inputs(ns, c, h, w):
    seed = 9000 + 131 * c + 17 * sum(ns) + h * w + len(ns)
    n = sum(ns)
    x = LG._rand((n, c, h, w), seed, 1.5, 0.75)
    o = 0
    for r, k in enumerate(ns):                              # every rank its own level: a rank's statistics are not the batch's
        x[o:o + k] += 0.5 * r
        o += k
    gamma, beta = LG._rand((c,), seed + 1, 0.5, 1.0), LG._rand((c,), seed + 2, 1.0, 1.5)
    if c >= 3:                                              # the kink channels and the constant channel of _bn_inputs
        gamma[0], beta[0] = 0.0, 0.0
        gamma[1], beta[1] = 0.0, 6.0
        x[:, 2] = 1.25
    rm, rv = LG._rand((c,), seed + 3, 0.3), LG._rand((c,), seed + 4, 0.1, 1.0).abs()
    return x, gamma, beta, rm, rv, LG._rand((n, c, h, w), seed + 5), LG._rand((n, c, h, w), seed + 6)


def _truth(x, gamma, beta, rm, rv, res, dy, act, with_res):
    """fp64 torch over the whole batch and the bounds of the rule, as test_batch_norm_act forms them"""
    n, c, h, w = x.shape
    cnt = n * h * w
    X, G, B = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    R = res.double() if with_res else None
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    z = TF.batch_norm(X, rm64, rv64, G, B, True, MOM, EPS)
    y = ACT[act](z) + (R if with_res else 0)
    gx, gg, gb = torch.autograd.grad(y, (X, G, B), dy.double())
    generic = torch.ones(c, dtype=torch.bool)
    if c >= 3:
        generic[:2] = False
    if act is not None:                                     # precondition of the case, not of the code under test
        zz = z.detach()[:, generic]
        far = zz.abs() if act == 'relu' else torch.minimum(zz.abs(), (zz - 6).abs())
        assert float(far.min()) >= EDGE, 'the case has a generic cell on a kink: pick another seed'
    mean = x.double().mean((0, 2, 3))
    var = x.double().var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    bc = lambda t: t.view(1, -1, 1, 1)                      # noqa: E731
    ax = (x.double().abs() + bc(mean.abs())) * bc(invstd)
    terms_y = ax * bc(gamma.double().abs()) + bc(beta.double().abs()) + (res.double().abs() if with_res else 0)
    zd = z.detach()
    g = dy.double() * ((zd > 0) & ((zd < 6) if act == 'relu6' else True) if act else 1.0)
    a1, a2 = g.abs().mean((0, 2, 3)), (g.abs() * ax).mean((0, 2, 3))
    k = bc(gamma.double().abs() * invstd)
    unb = var * (cnt / (cnt - 1.0))
    return dict(y=y.detach(), gx=gx, gg=gg, gb=gb, rm=rm64, rv=rv64, mean=mean, invstd=invstd,
                b_y=(6 if with_res else 5) * U * terms_y,
                b_rm=3 * U * ((1 - MOM) * rm.double().abs() + MOM * mean.abs()),
                b_rv=3 * U * ((1 - MOM) * rv.double().abs() + MOM * unb),
                b_gx=3 * U * k * (g.abs() + bc(a1) + ax * bc(a2)), b_gg=3 * U * a2 * cnt, b_gb=3 * U * a1 * cnt,
                b_mean=3 * 2.0 ** -53 * x.double().abs().mean((0, 2, 3)) * cnt)


def _run(case):
    """everything a case needs, once: inputs, the truth, and the simulated ranks' results on the device"""
    if case in _runs:
        return _runs[case]
    ns, c, h, w, act, with_res = case
    x, gamma, beta, rm, rv, res, dy = _inputs(ns, c, h, w)
    t = _truth(x, gamma, beta, rm, rv, res, dy, act, with_res)
    gd, bd = gamma.cuda(), beta.cuda()
    # every shard its own allocation, as a rank has it (a view into the batch need not be 16-byte aligned)
    xs, ress, dys = ([v.cuda() for v in whole.split(list(ns))] for whole in (x, res, dy))
    if not with_res:
        ress = [None] * len(ns)
    running0 = torch.stack([rm, rv]).cuda()
    rows = torch.stack([F.bn_sync_stats(v) for v in xs])
    ys, stats, runs = [], [], []
    for v, r in zip(xs, ress):
        running = running0.clone()
        y, stat = F.bn_sync_forward(v, gd, bd, running, rows, act, r, MOM, EPS)
        ys.append(y), stats.append(stat), runs.append(running)
    brows = torch.stack([F.bn_sync_backward_stats(d, v, gd, bd, s, act) for d, v, s in zip(dys, xs, stats)])
    grads = [F.bn_sync_backward(d, v, gd, bd, s, brows, rank, act)
             for rank, (d, v, s) in enumerate(zip(dys, xs, stats))]
    torch.cuda.synchronize()
    _runs[case] = dict(t=t, x=x, gd=gd, bd=bd, xs=xs, ress=ress, dys=dys, running0=running0, rows=rows, ys=ys, stats=stats,
                       runs=runs, brows=brows, grads=grads)
    return _runs[case]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_against_fp64_batch_norm_over_the_concatenated_batch(case):
    ns, c, h, w, act, with_res = case
    r = _run(case)
    t = r['t']
    cnt = sum(ns) * h * w
    assert r['rows'].shape == (len(ns), 2 * c + 2) and r['brows'].shape == (len(ns), 2 * c)
    for k, row in zip(ns, r['rows'].cpu()):
        assert float(row[2 * c]) == k * h * w and float(row[2 * c + 1]) == 0.0
    LG._held(torch.cat(r['ys']), t['y'], t['b_y'], 'sync y')
    LG._held(r['stats'][0][:c], t['mean'], t['b_mean'], 'sync mean (fp64)')
    assert torch.allclose(r['stats'][0][c:2 * c].cpu(), t['invstd'], rtol=1e-9, atol=0)
    assert float(r['stats'][0][2 * c].cpu()) == cnt
    LG._held(r['runs'][0][0], t['rm'], t['b_rm'], 'sync running_mean')
    LG._held(r['runs'][0][1], t['rv'], t['b_rv'], 'sync running_var')
    LG._held(torch.cat([g[0] for g in r['grads']]), t['gx'], t['b_gx'], 'sync dx')
    LG._held(sum(g[1].double().cpu() for g in r['grads']), t['gg'], t['b_gg'], 'sync dgamma, summed over the ranks')
    LG._held(sum(g[2].double().cpu() for g in r['grads']), t['gb'], t['b_gb'], 'sync dbeta, summed over the ranks')
    if c >= 3 and act is not None:
        assert not any(bool(g[0][:, 0].any()) for g in r['grads']), 'gradient through z = 0 must be zero'
    if c >= 3 and act == 'relu6':
        assert not any(bool(g[0][:, 1].any()) for g in r['grads']), 'gradient through z = 6 must be zero'
    if len(ns) > 1 and c * h * w > 1:
        # the power of the case: a rank's own statistics are not the batch's
        own = r['xs'][1].double().mean((0, 2, 3)).cpu()
        generic = slice(3, None) if c >= 3 else slice(None)
        assert bool(((own - t['mean'])[generic].abs() > 1e-3).all())


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_every_rank_holds_the_same_statistics(case):
    r = _run(case)
    ns, c = case[0], case[1]
    for stat, running in zip(r['stats'][1:], r['runs'][1:]):
        assert po.bitwise_equal(stat, r['stats'][0])
        assert po.bitwise_equal(running, r['runs'][0])
    tail = r['stats'][0][2 * c:].cpu()
    assert float(tail[0]) == sum(ns) * case[2] * case[3] and po.bitwise_equal(tail[1:], torch.zeros(1, dtype=torch.float64))
    assert not po.bitwise_equal(r['runs'][0], r['running0'])


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_one_rank_gives_the_bits_of_the_plain_calls(case):
    ns, c, h, w, act, with_res = case
    r = _run(case)
    x, res, dy, gd, bd = r['xs'][0], r['ress'][0], r['dys'][0], r['gd'], r['bd']
    plain_running = r['running0'].clone()
    y0, stat0 = F.bn_forward(x, gd, bd, plain_running, act, res, True, MOM, EPS)
    gx0, gg0, gb0 = F.bn_backward(dy, x, gd, bd, stat0, act)
    running = r['running0'].clone()
    rows = F.bn_sync_stats(x)[None]
    y, stat = F.bn_sync_forward(x, gd, bd, running, rows, act, res, MOM, EPS)
    brows = F.bn_sync_backward_stats(dy, x, gd, bd, stat, act)[None]
    gx, gg, gb = F.bn_sync_backward(dy, x, gd, bd, stat, brows, 0, act)
    assert po.bitwise_equal(y, y0)
    assert po.bitwise_equal(stat[:2 * c].view(2, c), stat0)
    assert float(stat[2 * c].cpu()) == ns[0] * h * w
    assert po.bitwise_equal(running, plain_running)
    assert po.bitwise_equal(gx, gx0) and po.bitwise_equal(gg, gg0) and po.bitwise_equal(gb, gb0)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_against_the_plain_forward_on_the_full_batch(case):
    ns, c, h, w, act, with_res = case
    r = _run(case)
    full_x = torch.cat(r['xs'])
    full_res = torch.cat(r['ress']) if with_res else None
    running = r['running0'].clone()
    y0, stat0 = F.bn_forward(full_x, r['gd'], r['bd'], running, act, full_res, True, MOM, EPS)
    y = torch.cat(r['ys'])
    differ = int((po.as_bits(y) != po.as_bits(y0)).sum())
    print('sync y against lp_bn_forward on the full batch: %d of %d elements differ bitwise; running pair %s'
          % (differ, y.numel(), 'equal' if po.bitwise_equal(running, r['runs'][0]) else 'differs'))
    # both are within the rule of the truth
    err = (y.double() - y0.double()).abs().cpu()
    assert bool((err <= 2 * r['t']['b_y']).all())


@pytest.mark.parametrize('case', [CASES[2], CASES[4], CASES[-2], CASES[-1]], ids=[IDS[2], IDS[4], IDS[-2], IDS[-1]])
def test_two_calls_and_a_graph_replay_give_the_same_bits(case):
    ns, c, h, w, act, with_res = case
    r = _run(case)
    rank = len(ns) - 1
    x, res, dy, gd, bd = r['xs'][rank], r['ress'][rank], r['dys'][rank], r['gd'], r['bd']
    rows, brows = r['rows'], r['brows']                      # pre-gathered: a collective is not part of the capture

    def fn():
        running = r['running0'].clone()
        row = F.bn_sync_stats(x)
        y, stat = F.bn_sync_forward(x, gd, bd, running, rows, act, res, MOM, EPS)
        brow = F.bn_sync_backward_stats(dy, x, gd, bd, stat, act)
        return (row, y, stat, running, brow) + F.bn_sync_backward(dy, x, gd, bd, stat, brows, rank, act)

    outs = LG._twice_and_replayed(fn, 'sync forward + backward')
    assert po.bitwise_equal(outs[0], rows[rank]) and po.bitwise_equal(outs[4], brows[rank])
    assert po.bitwise_equal(outs[1], r['ys'][rank]) and po.bitwise_equal(outs[5], r['grads'][rank][0])


def test_the_sliced_cases_have_more_than_one_slice_per_channel():
    for ns, c, h, w, _, _ in CASES[-2:]:
        assert all(_slices(n, c, h * w) > 1 for n in ns), (ns, c, h, w)
        assert sum(ns) * c * h * w * 4 <= 4 << 20
    assert _slices(3, 5, 15) == 1 and _slices(2, 16, 256) == 1
