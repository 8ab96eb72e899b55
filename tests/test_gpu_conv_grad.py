"""The stem and transposed-convolution calls (lp_stem_* / lp_deconv_*, litepose_amd.nn.functional) against torch in fp64 on
the CPU, on the widened fp32 inputs: F.conv2d / F.conv_transpose2d plus autograd (tests/_conv_grad_check.py), by the method
of tests/test_gpu_layer_grad.py.

A result that is a sum of n fp32 products, whatever its order, is held to |d - f| <= (n + 1) 2^-24 sum|terms|, sum|terms|
being the same op on the absolute values in fp64:
    stem forward n = 27, stem dW n = N (H/2) (W/2); deconv forward n = 4 (Ca + Cb) (the terms that reach one output cell),
    deconv dX n = 16 Cout, deconv dW n = N h w
Where the truth is exactly zero the result is zero: a 1x1 deconv plane leaves 12 of the 16 taps of every dW at zero, a 2x2
stem image 5 of the 9.  Two calls and a graph replay into poisoned outputs agree bitwise."""
import pytest
import torch

import _conv_grad_check as K
from litepose_amd.nn import functional as F
from test_gpu_layer_grad import U, _held, _twice_and_replayed

pytestmark = pytest.mark.gpu

DECONV_CH = [(16, 16, 8), (80, 48, 16), (24, 16, 24), (5, 0, 3), (33, 7, 9)]
DECONV_PLANES = [(3, 1, 1), (2, 5, 7), (2, 16, 16)]
STEM_PLANES = [(3, 2, 2), (2, 10, 14), (2, 64, 64)]
DECONV_SLICE, STEM_SLICE = K.macro('LP_DECONV_WGRAD_SLICE'), K.macro('LP_STEM_WGRAD_SLICE')


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _deconv_check(ca, cb, cout, n, h, w, mode):
    xa, wa, xb, wb, dy, (y, gxa, gxb, gwa, gwb), (ya, axa, axb, awa, awb) = K.deconv_case(ca, cb, cout, n, h, w)
    xad, wad, xbd, wbd, dyd = _cuda(xa, wa, xb, wb, dy)
    if mode == 'both':
        _held(F.deconv_forward(xad, wad, xbd, wbd), y, (4 * (ca + cb) + 1) * U * ya, 'deconv forward')
    need_x, need_w = mode in ('both', 'dx'), mode in ('both', 'dw')
    outs = _twice_and_replayed(lambda: F.deconv_backward(dyd, xad, wad, xbd, wbd, need_x, need_w), 'deconv backward ' + mode)
    assert len(outs) == (need_x + need_w) * (2 if cb else 1)
    if need_x:
        _held(outs[0], gxa, (16 * cout + 1) * U * axa, 'deconv dXa')
        if cb:
            _held(outs[1], gxb, (16 * cout + 1) * U * axb, 'deconv dXb')
    if need_w:
        got = outs[-2:] if cb else outs[-1:]
        _held(got[0], gwa, (n * h * w + 1) * U * awa, 'deconv dWa')
        if cb:
            _held(got[1], gwb, (n * h * w + 1) * U * awb, 'deconv dWb')
        return got
    return None


@pytest.mark.parametrize('mode', ['both', 'dx', 'dw'])
@pytest.mark.parametrize('plane', DECONV_PLANES, ids=lambda p: '%dx%dx%d' % p)
@pytest.mark.parametrize('ch', DECONV_CH, ids=lambda c: '%d+%dto%d' % c)
def test_deconv_pair(ch, plane, mode):
    got = _deconv_check(*ch, *plane, mode)
    if got is not None and plane[1:] == (1, 1):
        # cell (0, 0) reaches outputs (ky - 1, kx - 1) of a 2x2 plane: only ky, kx in {1, 2} meet it
        for g in got:
            dead = g.clone()
            dead[:, :, 1:3, 1:3] = 0
            assert not bool(dead.any()) and bool(g[:, :, 1:3, 1:3].all())


@pytest.mark.parametrize('plane', [(2 * DECONV_SLICE // K.DECONV_TILE + 3, 8, 8), (1, 8, 8 * (2 * DECONV_SLICE // K.DECONV_TILE + 5)),
                                   (2 * DECONV_SLICE // K.DECONV_TILE + 3, 3, 5)], ids=['images', 'row', 'partial-tiles'])
def test_deconv_weight_gradient_over_ragged_slices(plane):
    """at least three slices of LP_DECONV_WGRAD_SLICE cells (8x8 tiles), the last one shorter: across images, along one
    plane, and with tiles the plane only partly fills.  The kernel has one load form."""
    n, h, w = plane
    tiles = n * ((h + 7) // 8) * ((w + 7) // 8)
    per = DECONV_SLICE // K.DECONV_TILE
    assert K.deconv_slices(n, h, w) >= 3 and tiles % per
    _deconv_check(33, 7, 9, n, h, w, 'dw')


def _stem_check(n, H, W, forward=True):
    x, w, dy, (y, gw), (ya, awa) = K.stem_case(n, H, W)
    xd, wd, dyd = _cuda(x, w, dy)
    if forward:
        _held(F.stem_forward(xd, wd), y, 28 * U * ya, 'stem forward')
    outs = _twice_and_replayed(lambda: (F.stem_backward(dyd, xd),), 'stem backward')
    _held(outs[0], gw, (n * (H // 2) * (W // 2) + 1) * U * awa, 'stem dW')
    return outs[0]


@pytest.mark.parametrize('plane', STEM_PLANES, ids=lambda p: '%dx%dx%d' % p)
def test_stem(plane):
    gw = _stem_check(*plane)
    if plane[1:] == (2, 2):
        # the one output pixel reads rows / columns -1, 0, 1: the taps with ky = 0 or kx = 0 only meet padding
        assert not bool(gw[:, :, 0, :].any()) and not bool(gw[:, :, :, 0].any()) and bool(gw[:, :, 1:, 1:].all())


@pytest.mark.parametrize('plane', [(2 * STEM_SLICE // K.STEM_TILE + 3, 16, 32), (1, 16, 32 * (2 * STEM_SLICE // K.STEM_TILE + 5)),
                                   (2 * STEM_SLICE // K.STEM_TILE + 3, 6, 10)], ids=['images', 'row', 'partial-tiles'])
def test_stem_weight_gradient_over_ragged_slices(plane):
    """at least three slices of LP_STEM_WGRAD_SLICE pixels (8x16 tiles), the last one shorter.  One load form."""
    n, H, W = plane
    tiles = n * ((H // 2 + 7) // 8) * ((W // 2 + 15) // 16)
    assert K.stem_slices(n, H, W) >= 3 and tiles % (STEM_SLICE // K.STEM_TILE)
    _stem_check(n, H, W, forward=False)


def test_deconv_pair_through_autograd():
    ca, cb, cout, n, h, w = 33, 7, 9, 2, 5, 7
    xa, wa, xb, wb, dy, (y, gxa, gxb, gwa, gwb), (ya, axa, axb, awa, awb) = K.deconv_case(ca, cb, cout, n, h, w)
    ins = [t.cuda().requires_grad_() for t in (xa, wa, xb, wb)]
    out = F.deconv_pair(*ins)
    out.backward(dy.cuda())
    _held(out, y, (4 * (ca + cb) + 1) * U * ya, 'deconv_pair()')
    for t, f, a, cnt, what in ((ins[0], gxa, axa, 16 * cout, 'dXa'), (ins[2], gxb, axb, 16 * cout, 'dXb'),
                               (ins[1], gwa, awa, n * h * w, 'dWa'), (ins[3], gwb, awb, n * h * w, 'dWb')):
        _held(t.grad, f, (cnt + 1) * U * a, 'deconv_pair() ' + what)
    full = [t.grad.clone() for t in ins]
    # subsets of needs_input_grad: what is asked for is the same bits, what is not stays None
    for wanted in ((0,), (3,), (1, 3), (0, 2), (1, 2)):
        sub = [t.detach().clone().requires_grad_(i in wanted) for i, t in enumerate(ins)]
        F.deconv_pair(*sub).backward(dy.cuda())
        for i, t in enumerate(sub):
            assert (t.grad is None) == (i not in wanted), (wanted, i)
            assert t.grad is None or torch.equal(t.grad, full[i]), (wanted, i)
    # the one-source form
    xa, wa, _, _, dy, (y, gxa, _, gwa, _), (ya, axa, _, awa, _) = K.deconv_case(5, 0, 3, 2, 5, 7)
    xd, wd = xa.cuda().requires_grad_(), wa.cuda().requires_grad_()
    out = F.deconv_pair(xd, wd)
    out.backward(dy.cuda())
    _held(out, y, 21 * U * ya, 'deconv_pair() one source')
    _held(xd.grad, gxa, 49 * U * axa, 'deconv_pair() one source dX')
    _held(wd.grad, gwa, (2 * 5 * 7 + 1) * U * awa, 'deconv_pair() one source dW')
    with pytest.raises(ValueError):
        F.deconv_pair(xd, wd, xd)
    with pytest.raises(ValueError):
        F.deconv_pair(xd, wd.double())


def test_stem_conv_through_autograd():
    x, w, dy, (y, gw), (ya, awa) = K.stem_case(2, 10, 14)
    xd, wd = x.cuda(), w.cuda().requires_grad_()
    out = F.stem_conv(xd, wd)
    out.backward(dy.cuda())
    _held(out, y, 28 * U * ya, 'stem_conv()')
    _held(wd.grad, gw, (2 * 5 * 7 + 1) * U * awa, 'stem_conv() dW')
    assert torch.equal(wd.grad, F.stem_backward(dy.cuda(), xd))
    out = F.stem_conv(xd, wd.detach())                      # nothing requires a gradient: a plain forward
    assert not out.requires_grad
    with pytest.raises(ValueError):
        F.stem_conv(xd.clone().requires_grad_(), wd)        # no data gradient in the library
    with pytest.raises(ValueError):
        F.stem_conv(xd[:, :, :9], wd)                       # odd H
