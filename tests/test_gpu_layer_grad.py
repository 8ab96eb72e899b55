"""The training-mode layers (lp_bn_* / lp_pw_* / lp_dw_*, litepose_amd.nn.functional) against torch in fp64 on the CPU, on
the widened fp32 inputs: F.conv2d / F.batch_norm with the activation and the residual, plus autograd.

Tolerances are derived, not tuned:
  * a result that is a sum of n fp32 products, whatever its order:  |d - f| <= (n + 1) 2^-24 sum|terms|, sum|terms| computed
    here in fp64 (the same op on the absolute values).  1x1: forward n = Cin, data gradient n = Cout, weight gradient
    n = N HW; depthwise: forward and data gradient n = K^2, weight gradient n = N OH OW
  * BatchNorm: sums are fp64, so a result is held to c 2^-24 times the sum of the absolute values of its expression's terms,
    c = the fp32 roundings of the kernel's own expression (layer_kernels.hip) plus two:
      y       3 (subtract, multiply, fused multiply-add; 4 with the residual add) + 2 (mean and invstd rounded to fp32)
      dx, dgamma, dbeta, the running pair
              1 (fp64 on the fp32 inputs and the kept fp64 pair, rounded once) + 2
  * where f is exactly zero, d is zero (the gradient under a saturated activation, weight taps that only meet padding)
For every backward call two calls give identical bits, and so does a replay from a captured graph."""
import os
import re

import pytest
import torch
import torch.nn.functional as TF

import _poison as po
from conftest import ROOT
from litepose_amd import _native as nv
from litepose_amd.nn import functional as F

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _macro(name):
    with open(os.path.join(ROOT, 'include', 'litepose_amd.h')) as f:
        return int(re.search(r'#define\s+%s\s+(\d+)' % name, f.read()).group(1))


PW_SLICE, DW_SLICE = _macro('LP_PW_WGRAD_SLICE'), _macro('LP_DW_WGRAD_SLICE')


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).float()


def _held(d, f, bound, what):
    d, f, bound = d.detach().cpu().double(), f.detach().double(), bound.detach().double()
    assert d.shape == f.shape, (what, d.shape, f.shape)
    err = (d - f).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('%s: max |d - f| / bound = %.3f' % (what, worst))
    assert bool((err <= bound).all()), (what, worst)
    assert not bool(d[f == 0].any()), what + ': nonzero where the truth is exactly zero'


def _twice_and_replayed(fn, what):
    """fn() -> tuple of output tensors (None allowed): two eager calls and a graph replay into poisoned outputs agree
    bitwise; returns the first call's outputs."""
    a = [t.clone() for t in fn() if t is not None]
    b = [t for t in fn() if t is not None]
    assert all(po.bitwise_equal(x, y) for x, y in zip(a, b)), what + ': two calls differ'
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # launches in a row on one stream, no branches
        outs = [t for t in fn() if t is not None]
    for pat in ('N', 'H'):
        for t in outs:
            po.fill(t, pat)
        graph.replay()
        torch.cuda.synchronize()
        assert all(po.bitwise_equal(x, y) for x, y in zip(a, outs)), what + ': graph replay differs (%s)' % pat
    return a


# ------------------------------------------------------------------ 1x1
PW_CH = [(6, 14), (16, 96), (40, 28), (96, 24)]
PW_PLANES = [(3, 1, 1), (3, 37, 41), (2, 64, 64)]
_pw_truth = {}


def _pw_case(cin, cout, n, h, w):
    """inputs and the fp64 truth with its sum|terms|, computed once per shape"""
    key = (cin, cout, n, h, w)
    if key not in _pw_truth:
        seed = hash(key) % 100000
        x, wt, dy = _rand((n, cin, h, w), seed), _rand((cout, cin, 1, 1), seed + 1, 0.3), _rand((n, cout, h, w), seed + 2)
        res = []
        for ab in (False, True):
            xs, ws, ds = (t.double().abs() if ab else t.double() for t in (x, wt, dy))
            xs.requires_grad_(), ws.requires_grad_()
            y = TF.conv2d(xs, ws)
            gx, gw = torch.autograd.grad(y, (xs, ws), ds)
            res.append((y.detach(), gx, gw))
        _pw_truth[key] = (x, wt, dy, res[0], res[1])
    return _pw_truth[key]


def _pw_check(cin, cout, n, h, w, mode):
    x, wt, dy, (y, gx, gw), (ya, gxa, gwa) = _pw_case(cin, cout, n, h, w)
    xd, wd, dyd = x.cuda(), wt.cuda(), dy.cuda()
    if mode == 'both':
        _held(F.pw_forward(xd, wd), y, (cin + 1) * U * ya, 'pw forward')
    need_x, need_w = mode in ('both', 'dx'), mode in ('both', 'dw')
    outs = _twice_and_replayed(lambda: F.pw_backward(dyd, xd, wd, need_x, need_w), 'pw backward ' + mode)
    if need_x:
        _held(outs[0], gx, (cout + 1) * U * gxa, 'pw dX')
    if need_w:
        _held(outs[-1].reshape(gw.shape), gw, (n * h * w + 1) * U * gwa, 'pw dW')


@pytest.mark.parametrize('mode', ['both', 'dx', 'dw'])
@pytest.mark.parametrize('plane', PW_PLANES, ids=lambda p: '%dx%dx%d' % p)
@pytest.mark.parametrize('ch', PW_CH, ids=lambda c: '%dto%d' % c)
def test_pointwise(ch, plane, mode):
    _pw_check(ch[0], ch[1], *plane, mode)


@pytest.mark.parametrize('plane', [(1, 1, 2 * PW_SLICE + 36), (3, 1, (2 * PW_SLICE + 75) // 3)], ids=['vec', 'scalar'])
def test_pointwise_weight_gradient_over_ragged_slices(plane):
    """at least three slices of LP_PW_WGRAD_SLICE pixels, the last one shorter; 16-byte and scalar loads"""
    n, h, w = plane
    assert (n * h * w + PW_SLICE - 1) // PW_SLICE >= 3 and (n * h * w) % PW_SLICE
    assert ((h * w) % 4 == 0) == (n == 1)
    _pw_check(40, 28, n, h, w, 'both')


def test_pointwise_through_autograd():
    x, wt, dy, (y, gx, gw), (ya, gxa, gwa) = _pw_case(16, 96, 3, 37, 41)
    xd, wd = x.cuda().requires_grad_(), wt.cuda().requires_grad_()
    out = F.pointwise(xd, wd)
    out.backward(dy.cuda())
    _held(out, y, 17 * U * ya, 'pointwise()')
    _held(xd.grad, gx, 97 * U * gxa, 'pointwise() dX')
    _held(wd.grad, gw, (3 * 37 * 41 + 1) * U * gwa, 'pointwise() dW')
    xd2 = x.cuda()                                          # an input without grad: only the weight gradient is computed
    F.pointwise(xd2, wd).backward(dy.cuda())


# ------------------------------------------------------------------ depthwise
DW_PLANES = [(2, 2), (6, 10), (16, 16), (40, 24)]
_dw_truth = {}


def _dw_case(k, s, c, n, h, w):
    key = (k, s, c, n, h, w)
    if key not in _dw_truth:
        seed = hash(key) % 100000
        oh, ow = (h - 1) // s + 1, (w - 1) // s + 1
        x, wt, dy = _rand((n, c, h, w), seed), _rand((c, 1, k, k), seed + 1, 0.3), _rand((n, c, oh, ow), seed + 2)
        res = []
        for ab in (False, True):
            xs, ws, ds = (t.double().abs() if ab else t.double() for t in (x, wt, dy))
            xs.requires_grad_(), ws.requires_grad_()
            y = TF.conv2d(xs, ws, None, s, k // 2, 1, c)
            gx, gw = torch.autograd.grad(y, (xs, ws), ds)
            res.append((y.detach(), gx, gw))
        _dw_truth[key] = (x, wt, dy, res[0], res[1])
    return _dw_truth[key]


def _dw_check(k, s, c, n, h, w, modes=('both', 'dx', 'dw')):
    x, wt, dy, (y, gx, gw), (ya, gxa, gwa) = _dw_case(k, s, c, n, h, w)
    xd, wd, dyd = x.cuda(), wt.cuda(), dy.cuda()
    _held(F.dw_forward(xd, wd, s), y, (k * k + 1) * U * ya, 'dw forward')
    for mode in modes:
        need_x, need_w = mode in ('both', 'dx'), mode in ('both', 'dw')
        outs = _twice_and_replayed(lambda: F.dw_backward(dyd, xd, wd, s, need_x, need_w), 'dw backward ' + mode)
        if need_x:
            _held(outs[0], gx, (k * k + 1) * U * gxa, 'dw dX')
        if need_w:
            _held(outs[-1], gw, (n * y.shape[2] * y.shape[3] + 1) * U * gwa, 'dw dW')
    return gw


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('plane', DW_PLANES, ids=lambda p: '%dx%d' % p)
@pytest.mark.parametrize('c', [8, 24])
@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('k', [3, 5, 7])
def test_depthwise(k, s, c, plane, n):
    gw = _dw_check(k, s, c, n, *plane, modes=('both',) if (c, n) != (8, 3) else ('both', 'dx', 'dw'))
    if plane == (2, 2) and k == 7:
        assert not bool(gw[:, 0, 0, 0].any())               # a tap that only ever meets padding: the truth is exactly zero


@pytest.mark.parametrize('k,s,side', [(3, 1, 16), (5, 2, 32), (7, 1, 16)])
def test_depthwise_weight_gradient_over_ragged_slices(k, s, side):
    """three slices of LP_DW_WGRAD_SLICE units (one 16x16 output tile per image here), the last one shorter"""
    n = 2 * DW_SLICE + 3
    _dw_check(k, s, 8, n, side, side, modes=('dw',))


def test_depthwise_stride_2_refuses_odd_planes():
    L = nv.lib()
    x = torch.zeros(1, 8, 6, 7, device='cuda')
    w = torch.zeros(8, 3, 3, device='cuda')
    y = torch.zeros(1, 8, 3, 4, device='cuda')
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    for h, wd in ((6, 7), (7, 6), (5, 5)):
        assert L.lp_dw_forward(nv.dptr(x), nv.dptr(w), nv.dptr(y), 1, 8, h, wd, 3, 2, nv.dptr(ws), ws.numel(),
                               nv.stream_ptr()) == -1
        assert L.lp_dw_backward(nv.dptr(y), nv.dptr(x), nv.dptr(w), nv.dptr(x), nv.dptr(w), 1, 8, h, wd, 3, 2, nv.dptr(ws),
                                ws.numel(), nv.stream_ptr()) == -1
        assert L.lp_dw_backward_workspace_bytes(1, 8, h, wd, 3, 2, 1) == 0
    assert L.lp_dw_forward(nv.dptr(x), nv.dptr(w), nv.dptr(y), 1, 8, 6, 7, 3, 1, None, 0, nv.stream_ptr()) == -6
    with pytest.raises(nv.LitePoseNativeError):
        F.depthwise(x, w, 2)


def test_depthwise_through_autograd():
    x, wt, dy, (y, gx, gw), (ya, gxa, gwa) = _dw_case(5, 2, 24, 3, 40, 24)
    xd, wd = x.cuda().requires_grad_(), wt.cuda().requires_grad_()
    out = F.depthwise(xd, wd, 2)
    out.backward(dy.cuda())
    _held(out, y, 26 * U * ya, 'depthwise()')
    _held(xd.grad, gx, 26 * U * gxa, 'depthwise() dX')
    _held(wd.grad, gw, (3 * 20 * 12 + 1) * U * gwa, 'depthwise() dW')


# ------------------------------------------------------------------ BatchNorm
ACT = {None: lambda z: z, 'relu': torch.relu, 'relu6': TF.relu6}
EPS, MOM = 1e-5, 0.1
EDGE = 1e-5          # the generic cells of a case lie at least this far from the activation's kinks (asserted: the case's own precondition)


def _bn_inputs(c, n, h, w):
    seed = 7000 + 131 * c + 17 * n + h * w
    x = _rand((n, c, h, w), seed, 1.5, 0.75)
    gamma = _rand((c,), seed + 1, 0.5, 1.0)
    beta = _rand((c,), seed + 2, 1.0, 1.5)
    # channel 0: z sits on the lower kink (gamma = 0, beta = 0); channel 1: on ReLU6's upper kink (gamma = 0, beta = 6);
    # channel 2: every value equal (variance 0, invstd = 1 / sqrt(eps))
    gamma[0], beta[0] = 0.0, 0.0
    gamma[1], beta[1] = 0.0, 6.0
    x[:, 2] = 1.25
    rm, rv = _rand((c,), seed + 3, 0.3), _rand((c,), seed + 4, 0.1, 1.0).abs()
    return x, gamma, beta, rm, rv, _rand((n, c, h, w), seed + 5), _rand((n, c, h, w), seed + 6)


@pytest.mark.parametrize('plane', [(2, 1, 1), (3, 5, 7), (2, 32, 32)], ids=lambda p: '%dx%dx%d' % p)
@pytest.mark.parametrize('c', [3, 32])
@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('act', [None, 'relu', 'relu6'], ids=['none', 'relu', 'relu6'])
def test_batch_norm_act(act, with_res, c, plane):
    n, h, w = plane
    x, gamma, beta, rm, rv, res, dy = _bn_inputs(c, n, h, w)
    cnt = n * h * w
    # ---- fp64 truth
    X, G, B = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    R = res.double().requires_grad_() if with_res else None
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    z = TF.batch_norm(X, rm64, rv64, G, B, True, MOM, EPS)
    y = ACT[act](z) + (R if with_res else 0)
    gx, gg, gb = torch.autograd.grad(y, (X, G, B), dy.double(), retain_graph=with_res)
    generic = torch.ones(c, dtype=torch.bool)
    generic[:2] = False
    if act is not None:                                      # precondition of the case, not of the code under test
        zz = z.detach()[:, generic]
        far = zz.abs() if act == 'relu' else torch.minimum(zz.abs(), (zz - 6).abs())
        assert not far.numel() or float(far.min()) >= EDGE, 'the case has a generic cell on a kink: pick another seed'
    mean = x.double().mean((0, 2, 3))
    var = x.double().var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    bc = lambda t: t.view(1, -1, 1, 1)                       # noqa: E731
    # ---- device
    xd, gd, bd, rd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), res.cuda() if with_res else None, dy.cuda()
    running = torch.stack([rm, rv]).cuda()
    yd, stat = F.bn_forward(xd, gd, bd, running, act, rd, True, MOM, EPS)
    ax = (x.double().abs() + bc(mean.abs())) * bc(invstd)    # the terms of xhat
    terms_y = ax * bc(gamma.double().abs()) + bc(beta.double().abs()) + (res.double().abs() if with_res else 0)
    _held(yd, y, (6 if with_res else 5) * U * terms_y, 'bn y')
    _held(stat[0], mean, 3 * 2.0 ** -53 * x.double().abs().mean((0, 2, 3)) * cnt, 'bn mean (fp64)')
    assert torch.allclose(stat[1].cpu(), invstd, rtol=1e-9, atol=0)
    _held(running[0], rm64, 3 * U * ((1 - MOM) * rm.double().abs() + MOM * mean.abs()), 'running_mean')
    unb = var * (cnt / (cnt - 1.0))
    _held(running[1], rv64, 3 * U * ((1 - MOM) * rv.double().abs() + MOM * unb), 'running_var')
    outs = _twice_and_replayed(lambda: F.bn_backward(dyd, xd, gd, bd, stat, act), 'bn backward')
    # g = dy * act'(z) of the truth; the kinks' channels pass nothing
    g = dy.double() * ((z.detach() > 0) & ((z.detach() < 6) if act == 'relu6' else True) if act else 1.0)
    a1 = g.abs().mean((0, 2, 3))
    a2 = (g.abs() * ax).mean((0, 2, 3))
    k = bc(gamma.double().abs() * invstd)
    _held(outs[0], gx, 3 * U * k * (g.abs() + bc(a1) + ax * bc(a2)), 'bn dx')
    _held(outs[1], gg, 3 * U * a2 * cnt, 'bn dgamma')
    _held(outs[2], gb, 3 * U * a1 * cnt, 'bn dbeta')
    if act is not None:
        assert not bool(outs[0][:, 0].any()), 'gradient through z = 0 must be zero'
    if act == 'relu6':
        assert not bool(outs[0][:, 1].any()), 'gradient through z = 6 must be zero'
    assert float(stat[1][2].cpu()) == pytest.approx(EPS ** -0.5, rel=1e-9)
    # ---- eval mode: the running pair is the statistics; nothing but y is written
    before = running.clone()
    ye, none = F.bn_forward(xd, gd, bd, running, act, rd, False, MOM, EPS)
    assert none is None and po.bitwise_equal(before, running)
    rm2, rv2 = before[0].cpu().double(), before[1].cpu().double()
    ze = TF.batch_norm(x.double(), rm2, rv2, gamma.double(), beta.double(), False, MOM, EPS)
    inv2 = 1.0 / torch.sqrt(rv2 + EPS)
    terms_e = (x.double().abs() + bc(rm2.abs())) * bc(inv2 * gamma.double().abs()) + bc(beta.double().abs()) + \
        (res.double().abs() if with_res else 0)
    _held(ye, ACT[act](ze) + (res.double() if with_res else 0), (6 if with_res else 5) * U * terms_e, 'bn y (eval)')


def test_batch_norm_act_through_autograd():
    """batch_norm_act() is the pair of calls checked above: the same bits, the residual's gradient is the upstream itself,
    the running pair moves in place; an eval-mode forward works and its backward is refused."""
    x, gamma, beta, rm, rv, res, dy = _bn_inputs(32, 2, 32, 32)
    running = torch.stack([rm, rv]).cuda()
    y0, stat = F.bn_forward(x.cuda(), gamma.cuda(), beta.cuda(), running, 'relu6', res.cuda(), True, MOM, EPS)
    gx0, gg0, gb0 = F.bn_backward(dy.cuda(), x.cuda(), gamma.cuda(), beta.cuda(), stat, 'relu6')
    xd, gd, bd, rd = (t.cuda().requires_grad_() for t in (x, gamma, beta, res))
    rmd, rvd = rm.cuda(), rv.cuda()
    out = F.batch_norm_act(xd, gd, bd, rmd, rvd, 'relu6', rd, True, MOM, EPS)
    out.backward(dy.cuda())
    assert po.bitwise_equal(out.detach(), y0)
    assert po.bitwise_equal(rd.grad, dy.cuda())
    assert po.bitwise_equal(xd.grad, gx0) and po.bitwise_equal(gd.grad, gg0) and po.bitwise_equal(bd.grad, gb0)
    assert po.bitwise_equal(rmd, running[0]) and po.bitwise_equal(rvd, running[1])
    assert not po.bitwise_equal(rmd, rm.cuda()) and not po.bitwise_equal(rvd, rv.cuda())
    oe = F.batch_norm_act(xd, gd, bd, rmd, rvd, 'relu6', rd, False, MOM, EPS)
    assert oe.shape == out.shape and bool(torch.isfinite(oe).all())
    with pytest.raises(NotImplementedError):
        oe.sum().backward()
