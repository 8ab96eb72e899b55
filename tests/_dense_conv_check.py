"""Shared by the tests of the dense K x K convolution calls (lp_conv_*, litepose_amd.nn.functional.dense_conv): the header's
macro, the inputs of a shape and their fp64 truth -- torch's interpolate + conv2d plus autograd on the widened fp32 inputs on
the CPU, and the same op on the absolute values, which gives sum|terms| of every result.  A truth is computed once per shape
and never changed."""
import torch
import torch.nn.functional as TF

from _conv_grad_check import LP_ERR_INVALID_ARG, LP_ERR_UNSUPPORTED, LP_ERR_WORKSPACE, macro, rand  # noqa: F401

CONV_TILE = 8 * 16               # output pixels of a tile of the weight gradient (litepose_amd.h)


def out_plane(h, w, s, ups):
    return ((h << ups) - 1) // s + 1, ((w << ups) - 1) // s + 1


def conv_slices(n, oh, ow):
    pixels = n * ((oh + 7) // 8) * ((ow + 15) // 16) * CONV_TILE
    s = macro('LP_CONV_WGRAD_SLICE')
    return (pixels + s - 1) // s


def reference(xa, wa, xb, wb, bias, s, ups):
    """the op itself on whatever dtype the tensors share"""
    k = wa.shape[-1]
    up = (lambda t: TF.interpolate(t, scale_factor=2, mode='nearest')) if ups else (lambda t: t)
    y = TF.conv2d(up(xa), wa, bias, s, k // 2)
    if xb is not None:
        y = y + TF.conv2d(up(xb), wb, None, s, k // 2)
    return y


_cases = {}


def dense_case(ca, cb, cout, n, h, w, k, s, ups, with_bias):
    """-> (xa, wa, xb, wb, bias, dy) (xb, wb None with cb = 0, bias None without), truth, truth of the absolute values; a
    truth is (y, gxa, gwa, gxb, gwb, gbias) in fp64, None where the input is"""
    key = (ca, cb, cout, n, h, w, k, s, ups, with_bias)
    if key not in _cases:
        seed = 7000 + 1000 * ca + 100 * cb + 10 * cout + n * h * w + 13 * k + 5 * s + ups
        xa, wa = rand((n, ca, h, w), seed), rand((cout, ca, k, k), seed + 1, 0.3)
        xb, wb = (rand((n, cb, h, w), seed + 2), rand((cout, cb, k, k), seed + 3, 0.3)) if cb else (None, None)
        bias = rand((cout,), seed + 5) if with_bias else None
        oh, ow = out_plane(h, w, s, ups)
        dy = rand((n, cout, oh, ow), seed + 4)
        res = []
        for ab in (False, True):
            ins = [None if t is None else (t.double().abs() if ab else t.double()).requires_grad_()
                   for t in (xa, wa, xb, wb, bias)]
            y = reference(*ins, s, ups)
            live = [t for t in ins if t is not None]
            g = iter(torch.autograd.grad(y, live, dy.double().abs() if ab else dy.double()))
            res.append((y.detach(),) + tuple(None if t is None else next(g) for t in ins))
        _cases[key] = ((xa, wa, xb, wb, bias, dy), res[0], res[1])
    return _cases[key]
