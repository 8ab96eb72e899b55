"""The dense K x K convolution calls (lp_conv_*, litepose_amd.nn.functional.dense_conv) against torch in fp64 on the CPU, on
the widened fp32 inputs: F.interpolate + F.conv2d plus autograd (tests/_dense_conv_check.py), by the method of
tests/test_gpu_conv_grad.py.

A result that is a sum of n products is held to |d - f| <= (n + c) 2^-24 sum|terms|, sum|terms| being the same op on the
absolute values in fp64:
    forward n = K^2 (Ca + Cb) (+ 1 with a bias); dX n = K^2 Cout, times 4 through the upsample; dW and dbias n = N OH OW
c = 1 for a result built from single-rounded fp32 products: dW (v_mfma_f32_32x32x2_f32) and dbias (fp64 sums, one rounding).
c = 4 for a result computed on the bf16x3 split, the forward and dX (both run convk3_kernel): with x = hi + mid + lo in
8-bit pieces the products the split drops (mid*lo, lo*mid, lo*lo) are at most (2 + 2^-8) 2^-24 |x w| per term.
Where the truth is exactly zero the result is zero.  Two calls and a graph replay into poisoned outputs agree bitwise."""
import pytest
import torch

import _dense_conv_check as K
from litepose_amd.nn import functional as F
from test_gpu_layer_grad import U, _held, _twice_and_replayed

pytestmark = pytest.mark.gpu

FORMS = [(k, s, ups) for k in (3, 5, 7) for s, ups in ((1, 0), (1, 1), (2, 0))]
CH = [(3, 0, 32), (16, 0, 64), (80, 48, 16), (24, 32, 28), (5, 0, 3), (33, 7, 9)]
PLANES_S1 = [(3, 1, 1), (2, 5, 7), (2, 16, 16)]
PLANES_S2 = [(3, 2, 2), (2, 6, 10), (2, 16, 16)]
MODES = ['both', 'dx', 'dw']
SLICE = K.macro('LP_CONV_WGRAD_SLICE')
C_SPLIT, C_F32 = 4, 1


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _need(mode, cb, bias):
    nx, nw = mode in ('both', 'dx'), mode in ('both', 'dw')
    return (nx, nw, nx and cb > 0, nw and cb > 0, bias and nw)


def _check(ch, plane, form, mode, bias):
    ca, cb, cout = ch
    n, h, w = plane
    k, s, ups = form
    (xa, wa, xb, wb, b, dy), (y, gxa, gwa, gxb, gwb, gb), (ya, axa, awa, axb, awb, ab) = K.dense_case(ca, cb, cout, n, h, w, k, s, ups, bias)
    xad, wad, xbd, wbd, bd, dyd = _cuda(xa, wa, xb, wb, b, dy)
    oh, ow = K.out_plane(h, w, s, ups)
    if mode == 'both':
        _held(F.conv_forward(xad, wad, xbd, wbd, bd, s, bool(ups)), y, (k * k * (ca + cb) + int(bias) + C_SPLIT) * U * ya,
              'conv forward')
    need = _need(mode, cb, bias)
    outs = _twice_and_replayed(lambda: F.conv_backward(dyd, xad, wad, xbd, wbd, s, bool(ups), need), 'conv backward ' + mode)
    assert len(outs) == sum(need)
    got = dict(zip([nm for nm, v in zip(('xa', 'wa', 'xb', 'wb', 'b'), need) if v], outs))
    nx = k * k * cout * (4 if ups else 1) + C_SPLIT
    nw = n * oh * ow + C_F32
    for nm, f, a, cnt in (('xa', gxa, axa, nx), ('xb', gxb, axb, nx), ('wa', gwa, awa, nw), ('wb', gwb, awb, nw),
                          ('b', gb, ab, nw)):
        if nm in got:
            _held(got[nm], f, cnt * U * a, 'conv d' + nm)
    return got


def _ids(v):
    return 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _cases():
    out = []
    for fi, form in enumerate(FORMS):
        planes = PLANES_S2 if form[1] == 2 else PLANES_S1
        for ci, ch in enumerate(CH):
            # every form meets every channel set on the 16 x 16 plane with every output, and on a small plane in one mode
            out.append((ch, planes[2], form, 'both', ci % 2 == 0))
            out.append((ch, planes[(ci + fi) % 2], form, MODES[(ci + 2 * fi + ci // 3) % 3], (ci + fi) % 2 == 1))
    return out


@pytest.mark.parametrize('ch,plane,form,mode,bias', _cases(), ids=_ids)
def test_dense_conv(ch, plane, form, mode, bias):
    _check(ch, plane, form, mode, bias)


def test_the_case_list_covers_every_form():
    """every K x S x ups form meets a one-source shape, a two-source shape, a ragged channel count, every plane and mode"""
    for form in FORMS:
        mine = [c for c in _cases() if c[2] == form]
        assert any(c[0][1] == 0 for c in mine) and any(c[0][1] > 0 for c in mine)
        assert any(c[0][0] % 8 or c[0][2] % 8 for c in mine)
        assert {c[1] for c in mine} == set(PLANES_S2 if form[1] == 2 else PLANES_S1)
        assert {c[3] for c in mine} == set(MODES) and {c[4] for c in mine} == {True, False}


@pytest.mark.parametrize('ups', [0, 1])
def test_taps_that_only_meet_padding_are_exactly_zero_on_a_1x1_plane(ups):
    """K = 7 on a 1x1 plane: only the centre tap meets the cell; through the upsample the 2x2 plane is met by taps 2..4"""
    got = _check((33, 7, 9), (3, 1, 1), (7, 1, ups), 'dw', False)
    lo, hi = (2, 5) if ups else (3, 4)
    for g in (got['wa'], got['wb']):
        dead = g.clone()
        dead[:, :, lo:hi, lo:hi] = 0
        assert not bool(dead.any()) and bool(g[:, :, lo:hi, lo:hi].all())


@pytest.mark.parametrize('k', [3, 5, 7])
def test_taps_that_only_meet_padding_are_exactly_zero_at_stride_2(k):
    """a 2x2 plane at stride 2 has one output pixel, which reads rows / columns -K/2 .. K/2: taps K/2 and K/2 + 1 meet the plane"""
    got = _check((5, 0, 3), (3, 2, 2), (k, 2, 0), 'dw', False)
    g, p = got['wa'], k // 2
    dead = g.clone()
    dead[:, :, p:p + 2, p:p + 2] = 0
    assert not bool(dead.any()) and bool(g[:, :, p:p + 2, p:p + 2].all())


PER = SLICE // K.CONV_TILE


@pytest.mark.parametrize('form,plane', [((3, 1, 0), (2 * PER + 3, 8, 16)), ((3, 1, 0), (1, 8, 16 * (2 * PER + 5))),
                                        ((3, 1, 0), (2 * PER + 3, 3, 5)), ((7, 2, 0), (2 * PER + 3, 16, 32)),
                                        ((5, 1, 1), (2 * PER + 3, 4, 8))],
                         ids=['images', 'row', 'partial-tiles', 'images-s2', 'images-ups'])
def test_weight_gradient_over_ragged_slices(form, plane):
    """at least three slices of LP_CONV_WGRAD_SLICE pixels (8x16 tiles), the last one shorter: across images, along one
    plane, and with tiles the plane only partly fills.  The kernel has one load form per (K, S)."""
    n, h, w = plane
    oh, ow = K.out_plane(h, w, form[1], form[2])
    tiles = n * ((oh + 7) // 8) * ((ow + 15) // 16)
    assert K.conv_slices(n, oh, ow) >= 3 and tiles % PER
    _check((33, 7, 9), plane, form, 'dw', True)


def test_dense_conv_through_autograd():
    ca, cb, cout, n, h, w, k = 33, 7, 9, 2, 5, 7, 5
    (xa, wa, xb, wb, b, dy), (y, gxa, gwa, gxb, gwb, gb), (ya, axa, awa, axb, awb, ab) = K.dense_case(ca, cb, cout, n, h, w, k, 1, 1, True)
    ins = [t.cuda().requires_grad_() for t in (xa, wa, xb, wb, b)]
    dyd = dy.cuda()
    out = F.dense_conv(*ins, stride=1, upsample=True)
    torch.autograd.backward(out, dyd)
    _held(out, y, (k * k * (ca + cb) + 1 + C_SPLIT) * U * ya, 'dense_conv()')
    direct = F.conv_backward(dyd, *[t.detach() for t in ins[:4]], 1, True, (True,) * 5)
    for t, d in zip(ins, direct):
        assert torch.equal(t.grad, d)                       # autograd is the direct call, bitwise
    assert torch.equal(out, F.conv_forward(*[t.detach() for t in ins], 1, True))
    nx, nw = 4 * k * k * cout + C_SPLIT, n * 4 * h * w + C_F32
    for t, f, a, cnt, what in ((ins[0], gxa, axa, nx, 'dXa'), (ins[2], gxb, axb, nx, 'dXb'), (ins[1], gwa, awa, nw, 'dWa'),
                               (ins[3], gwb, awb, nw, 'dWb'), (ins[4], gb, ab, nw, 'dbias')):
        _held(t.grad, f, cnt * U * a, 'dense_conv() ' + what)
    full = [t.grad.clone() for t in ins]
    # subsets of needs_input_grad: what is asked for is the same bits, what is not stays None
    for wanted in ((0,), (3,), (4,), (1, 3), (0, 2), (1, 2, 4)):
        sub = [t.detach().clone().requires_grad_(i in wanted) for i, t in enumerate(ins)]
        torch.autograd.backward(F.dense_conv(*sub, stride=1, upsample=True), dyd)
        for i, t in enumerate(sub):
            assert (t.grad is None) == (i not in wanted), (wanted, i)
            assert t.grad is None or torch.equal(t.grad, full[i]), (wanted, i)
    # the one-source form at stride 2, no bias
    (xa, wa, _, _, _, dy), (y, gxa, gwa, _, _, _), (ya, axa, awa, _, _, _) = K.dense_case(5, 0, 3, 2, 6, 10, 3, 2, 0, False)
    xd, wd = xa.cuda().requires_grad_(), wa.cuda().requires_grad_()
    out = F.dense_conv(xd, wd, stride=2)
    out.backward(dy.cuda())
    _held(out, y, (45 + C_SPLIT) * U * ya, 'dense_conv() one source')
    _held(xd.grad, gxa, (27 + C_SPLIT) * U * axa, 'dense_conv() one source dX')
    _held(wd.grad, gwa, (2 * 3 * 5 + C_F32) * U * awa, 'dense_conv() one source dW')
    assert not F.dense_conv(xd.detach(), wd.detach(), stride=2).requires_grad
    with pytest.raises(ValueError):
        F.dense_conv(xd, wd, xd)
    with pytest.raises(ValueError):
        F.dense_conv(xd, wd.double())
