"""``lp_optim_adam`` / ``lp_optim_sgd`` and ``litepose_amd.optim`` on the device.

One step is held against the header's formulas evaluated in fp64 on the widened fp32 inputs, element by element, with
bounds of the form c * 2^-24 * sum |terms|, c = the fp32 roundings the kernel puts on that result + 2 (the 2 covers second
order and the fp64 bias corrections).  A hyperparameter rounded to fp32 counts as a rounding.  The counts (wd = 0 / wd != 0):

  Adam  g' = g + wd p          0 / 3 on the wd p term (wd, product, sum), 1 on g
        m = b1 m + (1-b1) g'   3 / 6: a term carries its coefficient, its product and the sum, after g' on the way
                               terms |b1 m| + (1-b1) G, G = |g| + |wd p|
        v = b2 v + (1-b2) g'^2 4 / 10: coefficient, two products, the sum; g' enters twice (2 * 3)
                               terms b2 v + (1-b2) G^2
        p = p - s m / d        s = lr / (1 - b1^t), d = sqrt(v) / sqrt(1 - b2^t) + eps, A = s m / d:
                               1 (the difference) on |p| + |A|; on |A| 3 (s, the quotient, the product) + d's relative
                               error = 4 (sqrt, its divisor, the quotient, the sum with eps) + half of v's relative error
                               (v's count * terms / v); m's count on s * (m's terms) / d
  SGD   buf = mu buf + g'      3 / 4: mu, product, sum on mu buf; g' and the sum on the rest; terms |mu buf| + G
        p = p - lr d           d = buf: buf's count + 3 (lr, product, difference) on lr * (buf's terms), 1 on |p|
                               nesterov, d = g' + mu buf: buf's count + 6 on lr * (G + mu * (buf's terms))
                               mu = 0, d = g': 3 / 6 on lr * G
Two cases are exact: g = 0 on fresh state with wd = 0 leaves p as it is, and SGD with mu = 0, wd = 0 is p - lr * g as two
separately rounded fp32 operations.

Drift: 20 steps on fixed random gradients; per tensor e = |p - p64| / |p64| against the fp64 trajectory may be at most 4
times the e of torch.optim.Adam / SGD in fp32 on the same inputs -- torch's own fp32 error is the yardstick, 4 the factor
tests/test_gpu_train_net.py gives the module over the reference.  The measured ratios are printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _poison as po
from litepose_amd import _native as nv, optim

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
E = 4096                                         # LP_OPTIM_BLOCK_ELEMS
LENGTHS = [1, 3, 27 * 32, E - 1, E, E + 1, 3 * E + 517]


def _arr(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _numel(ts):
    return (C.c_int64 * len(ts))(*[t.numel() for t in ts])


def _layout(lengths, misaligned=()):
    """Offsets of the tensors inside one flat buffer: 16-byte aligned starts with a gap in between, except the tensors
    named in ``misaligned``, which start one element later (4- but not 16-byte aligned)."""
    offs, o = [], 4
    for i, n in enumerate(lengths):
        offs.append(o + (1 if i in misaligned else 0))
        o = (offs[-1] + n + 3) // 4 * 4 + 4
    return offs, o


def _views(flat, offs, lengths):
    return [flat[o:o + n] for o, n in zip(offs, lengths)]


def _rand(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _lr(v):
    return torch.tensor(v, dtype=torch.float64, device='cuda')


def _mask(total, offs, lengths, per_tensor=None):
    m = np.zeros(total, bool)
    t = np.zeros(total)
    for i, (o, n) in enumerate(zip(offs, lengths)):
        m[o:o + n] = True
        if per_tensor is not None:
            t[o:o + n] = per_tensor[i]
    return m, t


def adam_reference(p, g, m, v, t, lr, b1, b2, eps, wd):
    """fp64 results and the bounds of the module docstring; ``t``: per element, the step count AFTER this step."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    G = np.abs(g) + np.abs(wd * p)
    g1 = g + wd * p
    cm, cv = (3, 4) if wd == 0 else (6, 10)
    mt = np.abs(b1 * m) + (1 - b1) * G
    vt = b2 * v + (1 - b2) * G * G
    m1 = b1 * m + (1 - b1) * g1
    v1 = b2 * v + (1 - b2) * g1 * g1
    s = lr / (1 - b1 ** t)
    d = np.sqrt(v1) / np.sqrt(1 - b2 ** t) + eps
    A = s * m1 / d
    p1 = p - A
    rel_v = np.where(v1 > 0, cv * vt / np.where(v1 > 0, v1, 1.0), 0.0)
    bp = U * (3 * (np.abs(p) + np.abs(A)) + np.abs(A) * (3 + 4 + 0.5 * rel_v) + s * cm * mt / d)
    return (p1, m1, v1), (bp, (cm + 2) * U * mt, (cv + 2) * U * vt)


def sgd_reference(p, g, buf, lr, mu, wd, nesterov):
    p, g, buf = (np.asarray(a, np.float64) for a in (p, g, buf))
    G = np.abs(g) + np.abs(wd * p)
    g1 = g + wd * p
    cg = 0 if wd == 0 else 3
    if mu == 0:
        return (p - lr * g1, buf), ((cg + 3 + 2) * U * (np.abs(p) + lr * G), np.zeros_like(p))
    cb = 3 if wd == 0 else 4
    bt = np.abs(mu * buf) + G
    b1 = mu * buf + g1
    if nesterov:
        return (p - lr * (g1 + mu * b1), b1), ((cb + 6 + 2) * U * (np.abs(p) + lr * (G + mu * bt)), (cb + 2) * U * bt)
    return (p - lr * b1, b1), ((cb + 3 + 2) * U * (np.abs(p) + lr * bt), (cb + 2) * U * bt)


def _within(got, want, bound, mask, what):
    got = got.cpu().double().numpy()
    err = np.abs(got - want)
    assert np.all(err[mask] <= bound[mask]), (what, float((err[mask] / np.maximum(bound[mask], 1e-300)).max()))
    return float((err[mask] / np.maximum(bound[mask], 1e-300)).max()) if mask.any() else 0.0


def _adam_call(P, G, M, V, steps, lr, b1, b2, eps, wd):
    rc = nv.lib().lp_optim_adam(len(P), _arr(P), _arr(G), _arr(M), _arr(V), _numel(P), nv.dptr(steps), nv.dptr(lr), b1, b2,
                                eps, wd, nv.stream_ptr())
    assert rc == 0, nv.lib().lp_last_error()


def _sgd_call(P, G, B, lr, mu, wd, nesterov):
    rc = nv.lib().lp_optim_sgd(len(P), _arr(P), _arr(G), _arr(B) if B is not None else None, _numel(P), nv.dptr(lr), mu, wd,
                               int(nesterov), nv.stream_ptr())
    assert rc == 0, nv.lib().lp_last_error()


# ------------------------------------------------------------------ one step against the formulas
@pytest.mark.parametrize('wd', [0.0, 0.01], ids=['wd0', 'wd'])
def test_adam_step_against_fp64(wd):
    lengths = LENGTHS + [E + 9, 5]
    mis = {len(LENGTHS), 2}                                   # E + 9 and 27 * 32 at 4-byte aligned pointers, next to aligned ones
    offs, total = _layout(lengths, mis)
    p, g, m = _rand(total, 1), _rand(total, 2, 0.1), _rand(total, 3, 0.05)
    v = _rand(total, 4, 0.01).abs()
    steps0 = [0, 7, 1, 2, 0, 999, 3, 12, 0]
    steps = torch.tensor(steps0, dtype=torch.float32, device='cuda')
    before = [a.clone() for a in (p, g, m, v)]
    P, G, M, V = (_views(a, offs, lengths) for a in (p, g, m, v))
    assert P[2].data_ptr() % 16 == 4 and P[0].data_ptr() % 16 == 0
    lr, b1, b2, eps = 3e-3, 0.9, 0.999, 1e-8
    _adam_call(P, G, M, V, steps, _lr(lr), b1, b2, eps, wd)
    mask, t = _mask(total, offs, lengths, [s + 1 for s in steps0])
    t[~mask] = 1
    (p1, m1, v1), (bp, bm, bv) = adam_reference(*[a.cpu().numpy() for a in before], t, lr, b1, b2, eps, wd)
    r = [_within(p, p1, bp, mask, 'p'), _within(m, m1, bm, mask, 'm'), _within(v, v1, bv, mask, 'v')]
    print('adam wd=%g: largest error / bound  p %.3f  m %.3f  v %.3f' % (wd, r[0], r[1], r[2]))
    for a, b in zip((p, m, v), (before[0], before[2], before[3])):            # the gaps between the tensors
        assert torch.equal(a.cpu()[torch.from_numpy(~mask)], b.cpu()[torch.from_numpy(~mask)])
    assert torch.equal(g, before[1])
    assert steps.tolist() == [s + 1.0 for s in steps0]


@pytest.mark.parametrize('mu,wd,nesterov', [(0.0, 0.0, False), (0.9, 0.0, False), (0.9, 1e-3, True), (0.0, 1e-3, False),
                                            (0.5, 1e-3, False)], ids=['plain', 'mom', 'nesterov-wd', 'wd', 'mom-wd'])
def test_sgd_step_against_fp64(mu, wd, nesterov):
    lengths = LENGTHS + [E + 9, 5]
    mis = {len(LENGTHS), 2}
    offs, total = _layout(lengths, mis)
    p, g, b = _rand(total, 5), _rand(total, 6, 0.1), _rand(total, 7, 0.3)
    before = [a.clone() for a in (p, g, b)]
    P, G, B = (_views(a, offs, lengths) for a in (p, g, b))
    lr = 0.0375
    _sgd_call(P, G, B if mu else None, _lr(lr), mu, wd, nesterov)
    mask, _ = _mask(total, offs, lengths)
    (p1, b1), (bp, bb) = sgd_reference(*[a.cpu().numpy() for a in before], lr, mu, wd, nesterov)
    r = [_within(p, p1, bp, mask, 'p'), _within(b, b1, bb, mask, 'buf')]
    print('sgd mu=%g wd=%g nesterov=%d: largest error / bound  p %.3f  buf %.3f' % (mu, wd, nesterov, r[0], r[1]))
    keep = torch.from_numpy(~mask)
    assert torch.equal(p.cpu()[keep], before[0].cpu()[keep]) and torch.equal(g, before[1])
    if mu == 0:
        assert torch.equal(b, before[2])
    else:
        assert torch.equal(b.cpu()[keep], before[2].cpu()[keep])
    if mu == 0 and wd == 0:                                   # p - lr * g, the product and the difference rounded separately
        lrf = torch.tensor(lr, dtype=torch.float32)
        want = before[0].cpu() - lrf * before[1].cpu()
        m = torch.from_numpy(mask)
        assert po.bitwise_equal(p.cpu()[m], want[m])
        assert po.bitwise_equal(p.cpu()[m], (before[0] - lr * before[1]).cpu()[m])     # as torch's SGD evaluates it


def test_zero_gradient_on_fresh_state_leaves_p():
    offs, total = _layout(LENGTHS, {1})
    p = _rand(total, 8)
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    steps = torch.zeros(len(LENGTHS), device='cuda')
    want = p.clone()
    P, G, M, V = (_views(a, offs, LENGTHS) for a in (p, g, m, v))
    _adam_call(P, G, M, V, steps, _lr(1e-3), 0.9, 0.999, 1e-8, 0.0)
    assert po.bitwise_equal(p, want) and not bool(m.any()) and not bool(v.any())
    _sgd_call(P, G, M, _lr(0.1), 0.9, 0.0, False)
    assert po.bitwise_equal(p, want)


def test_700_tiny_tensors_take_more_than_one_chunk():
    rng = np.random.RandomState(0)
    lengths = [int(n) for n in rng.randint(1, 41, 700)]
    offs, o = [], 0
    for n in lengths:                                         # packed back to back: every alignment occurs
        offs.append(o)
        o += n
    total = o
    p, g, m = _rand(total, 11), _rand(total, 12, 0.1), _rand(total, 13, 0.05)
    v = _rand(total, 14, 0.01).abs()
    steps0 = [int(s) for s in rng.randint(0, 50, 700)]
    steps = torch.tensor(steps0, dtype=torch.float32, device='cuda')
    before = [a.clone() for a in (p, g, m, v)]
    P, G, M, V = (_views(a, offs, lengths) for a in (p, g, m, v))
    ne = (C.c_int64 * 700)(*lengths)
    assert nv.lib().lp_optim_launches(700, ne) == 11          # 64 tensors per chunk
    _adam_call(P, G, M, V, steps, _lr(1e-3), 0.9, 0.999, 1e-8, 0.0)
    mask, t = _mask(total, offs, lengths, [s + 1 for s in steps0])
    (p1, m1, v1), (bp, bm, bv) = adam_reference(*[a.cpu().numpy() for a in before], t, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    _within(p, p1, bp, mask, 'p'), _within(m, m1, bm, mask, 'm'), _within(v, v1, bv, mask, 'v')
    assert steps.tolist() == [s + 1.0 for s in steps0]
    b = before[2].clone()
    pb = before[0].clone()
    _sgd_call(_views(pb, offs, lengths), G, _views(b, offs, lengths), _lr(0.05), 0.9, 0.0, False)
    (p2, b2), (bp2, bb2) = sgd_reference(before[0].cpu().numpy(), before[1].cpu().numpy(), before[2].cpu().numpy(), 0.05, 0.9,
                                         0.0, False)
    _within(pb, p2, bp2, mask, 'sgd p'), _within(b, b2, bb2, mask, 'sgd buf')


# ------------------------------------------------------------------ the optimizer classes
def _params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in shapes]


def _grads(params, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        x = torch.randn(p.shape, generator=g).cuda() * 0.1
        p.grad = None if i in skip else x


def test_a_parameter_without_a_gradient_is_skipped():
    shapes = [(7, 5), (33,), (E + 3,), (2, 3)]
    a, b = _params(shapes, 20), _params(shapes, 20)
    mine, ref = optim.Adam(a, lr=1e-2, weight_decay=1e-3), torch.optim.Adam(b, lr=1e-2, weight_decay=1e-3)
    for r, skip in enumerate([(), (1,), (1,), ()]):
        _grads(a, 30 + r, skip), _grads(b, 30 + r, skip)
        before = a[1].detach().clone()
        mine.step(), ref.step()
        if skip:
            assert po.bitwise_equal(a[1].detach(), before)
    assert mine._steps(mine.param_groups[0]).tolist() == [4.0, 2.0, 4.0, 4.0]
    assert [float(ref.state[q]['step']) for q in b] == [4.0, 2.0, 4.0, 4.0]
    for p, q in zip(a, b):                    # the same trajectory as torch's (a sanity check; the bounds are the fp64 tests')
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6)
    # a parameter that never had a gradient has no state, as in torch
    c = _params(shapes, 21)
    o = optim.SGD(c, lr=0.1, momentum=0.9)
    _grads(c, 40, (2,))
    o.step()
    assert c[2] not in o.state or not o.state[c[2]]


def test_two_groups_with_their_own_lr():
    shapes = [(9, 4), (17,)]
    for cls, ref_cls, kw in ((optim.Adam, torch.optim.Adam, {}), (optim.SGD, torch.optim.SGD, dict(momentum=0.9))):
        a, b = _params(shapes, 50), _params(shapes, 50)
        mine = cls([dict(params=[a[0]], lr=0.5), dict(params=[a[1]])], lr=1e-3, **kw)
        ref = ref_cls([dict(params=[b[0]], lr=0.5), dict(params=[b[1]])], lr=1e-3, **kw)
        start = [p.detach().clone() for p in a]
        for r in range(2):
            _grads(a, 60 + r), _grads(b, 60 + r)
            mine.step(), ref.step()
        for p, q in zip(a, b):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), cls
        moved = [float((p.detach() - s).abs().max()) for p, s in zip(a, start)]
        assert moved[0] > 20 * moved[1] if cls is optim.Adam else moved[0] > moved[1]


# ------------------------------------------------------------------ drift over 20 steps
DRIFT_SHAPES = [(3, 5), (27 * 32,), (E + 1,), (64, 33)]


def _trajectory(make, dtype, rounds=20):
    g = torch.Generator().manual_seed(70)
    params = [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype).cuda()) for s in DRIFT_SHAPES]
    opt = make(params)
    gg = torch.Generator().manual_seed(71)
    for _ in range(rounds):
        for p in params:
            p.grad = (torch.randn(p.shape, generator=gg) * 0.1).to(dtype).cuda()
        opt.step()
    return [p.detach().double().cpu() for p in params], opt


def _drift(name, mine, ref):
    p64, _ = _trajectory(ref, torch.float64)
    p32, _ = _trajectory(ref, torch.float32)
    got, _ = _trajectory(mine, torch.float32)
    for i, (a, b, c) in enumerate(zip(got, p32, p64)):
        e_mine = float((a - c).norm() / c.norm())
        e_ref = float((b - c).norm() / c.norm())
        print('%s drift, tensor %s: e = %.3e, torch fp32 e = %.3e, ratio %.3f' % (name, DRIFT_SHAPES[i], e_mine, e_ref,
                                                                                 e_mine / e_ref))
        assert e_mine <= 4 * e_ref, (name, i, e_mine / e_ref)


def test_adam_drift_against_torch_fp32():
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    _drift('adam', lambda ps: optim.Adam(ps, **kw), lambda ps: torch.optim.Adam(ps, **kw))


def test_sgd_drift_against_torch_fp32():
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    _drift('sgd', lambda ps: optim.SGD(ps, **kw), lambda ps: torch.optim.SGD(ps, **kw))


def test_interchange_with_torch_adam_mid_run():
    """Five steps of torch.optim.Adam, its state_dict loaded into the library's, five more steps of each: the two stay
    within the drift bound of each other's fp64 trajectory."""
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    mk = lambda dtype: [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(80 + i)).to(dtype).cuda())  # noqa: E731
                        for i, s in enumerate(DRIFT_SHAPES)]

    def run(params, opt, rounds, seed):
        gg = torch.Generator().manual_seed(seed)
        for _ in range(rounds):
            for p in params:
                p.grad = (torch.randn(p.shape, generator=gg) * 0.1).to(p.dtype).cuda()
            opt.step()

    p64, p32 = mk(torch.float64), mk(torch.float32)
    o64, o32 = torch.optim.Adam(p64, **kw), torch.optim.Adam(p32, **kw)
    run(p64, o64, 5, 90), run(p32, o32, 5, 90)
    mine_p = [torch.nn.Parameter(p.detach().clone()) for p in p32]
    mine = optim.Adam(mine_p, lr=1.0)
    mine.load_state_dict(o32.state_dict())
    assert mine._steps(mine.param_groups[0]).tolist() == [5.0] * len(DRIFT_SHAPES)
    run(p64, o64, 5, 91), run(p32, o32, 5, 91), run(mine_p, mine, 5, 91)
    assert mine._steps(mine.param_groups[0]).tolist() == [10.0] * len(DRIFT_SHAPES)
    for i, (a, b, c) in enumerate(zip(mine_p, p32, p64)):
        c = c.detach().double()
        e_mine, e_ref = float((a.detach().double() - c).norm() / c.norm()), float((b.detach().double() - c).norm() / c.norm())
        print('interchange, tensor %s: e = %.3e, torch fp32 e = %.3e, ratio %.3f' % (DRIFT_SHAPES[i], e_mine, e_ref,
                                                                                   e_mine / e_ref))
        assert e_mine <= 4 * e_ref, (i, e_mine / e_ref)


# ------------------------------------------------------------------ determinism and capture
def _fresh(cls, seed=100, **kw):
    params = _params([(5, 7), (E + 5,), (3,)], seed)
    return params, cls(params, **kw)


@pytest.mark.parametrize('which', ['adam', 'sgd'])
def test_two_runs_and_a_replayed_capture_give_the_same_bits(which):
    cls, kw = (optim.Adam, dict(lr=1e-2, weight_decay=1e-3)) if which == 'adam' else (optim.SGD, dict(lr=0.05, momentum=0.9))

    def eager(rounds, lrs=None):
        params, opt = _fresh(cls, **kw)
        _grads(params, 110)
        for r in range(rounds):
            if lrs:
                opt.param_groups[0]['lr'] = lrs[r]
            opt.step()
        return [p.detach().clone() for p in params], opt.state_dict()

    a, sa = eager(4)
    b, sb = eager(4)
    assert all(po.bitwise_equal(x, y) for x, y in zip(a, b))

    def same_state(s, t):
        for k in s['state']:
            for name, v in s['state'][k].items():
                assert po.bitwise_equal(v, t['state'][k][name]), (k, name)

    same_state(sa, sb)
    # one eager step creates the state; the second is captured and replayed three times = four eager steps
    params, opt = _fresh(cls, **kw)
    _grads(params, 110)
    opt.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for _ in range(3):
        opt.sync_hyperparameters()
        graph.replay()
    assert all(po.bitwise_equal(x.detach(), y) for x, y in zip(params, a))
    same_state(opt.state_dict(), sa)
    # a new lr between replays takes effect without a new capture
    lrs = [kw['lr'], kw['lr'], 0.5 * kw['lr'], 0.125 * kw['lr']]
    c, sc = eager(4, lrs)
    params, opt = _fresh(cls, **kw)
    _grads(params, 110)
    opt.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for r in range(1, 4):
        opt.param_groups[0]['lr'] = lrs[r]
        opt.sync_hyperparameters()
        graph.replay()
    assert all(po.bitwise_equal(x.detach(), y) for x, y in zip(params, c))
    assert not all(po.bitwise_equal(x, y) for x, y in zip(a, c))
    same_state(opt.state_dict(), sc)
    # a hyperparameter that travels by value cannot change under a captured step
    opt.param_groups[0]['weight_decay'] = 0.5
    with pytest.raises(RuntimeError, match='captured'):
        opt.sync_hyperparameters()
