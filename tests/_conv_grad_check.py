"""Shared by the tests of the stem and transposed-convolution calls (lp_stem_* / lp_deconv_*): the header's macros, the
inputs of a shape and their fp64 truth -- torch's conv2d / conv_transpose2d plus autograd on the widened fp32 inputs on the
CPU, and the same op on the absolute values, which gives sum|terms| of every result.  A truth is computed once per shape."""
import os
import re

import torch
import torch.nn.functional as TF

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'litepose_amd.h')
LP_ERR_INVALID_ARG, LP_ERR_UNSUPPORTED, LP_ERR_WORKSPACE = -1, -8, -6
DECONV_TILE = 8 * 8              # input cells of a tile of the deconv weight gradient (litepose_amd.h)
STEM_TILE = 8 * 16               # output pixels of a tile of the stem weight gradient


def macro(name):
    with open(HEADER) as f:
        return int(re.search(r'#define\s+%s\s+(\d+)' % name, f.read()).group(1))


def deconv_slices(n, h, w):
    cells = n * ((h + 7) // 8) * ((w + 7) // 8) * DECONV_TILE
    s = macro('LP_DECONV_WGRAD_SLICE')
    return (cells + s - 1) // s


def stem_slices(n, H, W):
    pixels = n * ((H // 2 + 7) // 8) * ((W // 2 + 15) // 16) * STEM_TILE
    s = macro('LP_STEM_WGRAD_SLICE')
    return (pixels + s - 1) // s


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).float()


_deconv, _stem = {}, {}


def deconv_case(ca, cb, cout, n, h, w):
    """-> xa, wa, xb, wb, dy (xb, wb None with cb = 0), truth, truth of the absolute values; a truth is (y, gxa, gxb, gwa,
    gwb) in fp64 (gxb, gwb None with cb = 0)"""
    key = (ca, cb, cout, n, h, w)
    if key not in _deconv:
        seed = 1000 * ca + 100 * cb + 10 * cout + n * h * w
        xa, wa = rand((n, ca, h, w), seed), rand((ca, cout, 4, 4), seed + 1, 0.3)
        xb, wb = (rand((n, cb, h, w), seed + 2), rand((cb, cout, 4, 4), seed + 3, 0.3)) if cb else (None, None)
        dy = rand((n, cout, 2 * h, 2 * w), seed + 4)
        res = []
        for ab in (False, True):
            ins = [None if t is None else (t.double().abs() if ab else t.double()).requires_grad_() for t in (xa, xb, wa, wb)]
            y = TF.conv_transpose2d(ins[0], ins[2], None, 2, 1)
            if cb:
                y = y + TF.conv_transpose2d(ins[1], ins[3], None, 2, 1)
            g = torch.autograd.grad(y, [t for t in ins if t is not None], dy.double().abs() if ab else dy.double())
            g = list(g) if cb else [g[0], None, g[1], None]
            res.append((y.detach(), g[0], g[1], g[2], g[3]))
        _deconv[key] = (xa, wa, xb, wb, dy, res[0], res[1])
    return _deconv[key]


def stem_case(n, H, W):
    """-> x, w, dy, (y, gw), the same of the absolute values"""
    key = (n, H, W)
    if key not in _stem:
        seed = 5000 + n * H * W
        x, w, dy = rand((n, 3, H, W), seed), rand((32, 3, 3, 3), seed + 1, 0.3), rand((n, 32, H // 2, W // 2), seed + 2)
        res = []
        for ab in (False, True):
            xs, ws, ds = (t.double().abs() if ab else t.double() for t in (x, w, dy))
            ws.requires_grad_()
            y = TF.conv2d(xs, ws, None, 2, 1)
            res.append((y.detach(), torch.autograd.grad(y, ws, ds)[0]))
        _stem[key] = (x, w, dy, res[0], res[1])
    return _stem[key]
