"""Shared by the tests of NaN / Inf propagation and containment (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite_*.py).

One library call is run twice: clean, giving outputs O, and with ONE element of one operand -- the site -- set to NaN, +inf or
-inf, giving O'.  The truth is the same op in torch, fp64, on the CPU, on the widened inputs, forward plus autograd, clean (R)
and with the injected value (R').  The CONE of the site is the set of outputs that depend on it: isnan(R') for a NaN,
~isfinite(R') for an Inf.  ``compare`` requires

  * isnan(O') == cone (NaN injected), ~isfinite(O') == cone (Inf injected), tensor by tensor;
  * ``exact`` (the kernels with plain fp32 / fp64 arithmetic): with an Inf the class and the sign are those of R' too.  The
    two-value kernels (1x1, stem, transposed pair) take their operands apart into bf16 pieces, where inf - bf16(inf) is a
    NaN: there only non-finiteness is compared;
  * where R' is R -- the output does not depend on the site -- O' is BITWISE O.  Every sum of these kernels has one order
    fixed by the shapes, so such an element cannot move by one bit, and an exact zero stays an exact zero.  An output the
    site reaches without making it non-finite (relu6(+inf) = 6, a sum the activation's gate closes) has R' != R: it has to
    be finite, which the first rule already says, and nothing more is asked of it.

What the rules see that a bound on finite data cannot: a kernel that scrubs a NaN (maxNum / minNum clamps, ``v > 0 ? v : 0``)
has a smaller mask than the cone; a kernel that removes padding, a ragged tail or a neighbour's element by MULTIPLYING a
wrongly read value by zero has a larger one, since 0 * NaN is NaN.

Two allowances, both on the side of MORE non-finite outputs and both only for outputs whose sum holds a product of the site
with a zero that stands for padding: torch's own convolutions multiply their padding, so between the cone (summed tap by tap
over the cells a tap really meets) and torch's mask a kernel may go either way (``torch_conv``); and four kernels multiply a
zero-filled halo where torch does not, as does the dense convolution's data gradient, which also multiplies the zeros of a
dilated grad_y at stride 2 -- known deviations, named in HALO_KERNELS, counted in LEAKS and held as strict expected failures
in tests/test_gpu_nonfinite_layers.py and tests/test_gpu_nonfinite_conv.py (``halo_products``).

For the linear ops the cone is derived a second way (``indicator_cone``): the same op on the 0/1 indicator of the site with
all-ones partners, exact integer arithmetic in fp64; tests/test_nonfinite_cpu.py holds the two routes to each other for every
case, operand, site and value the GPU files use.

Cases are rows of the existing tables (tests/test_gpu_train_forms.py, test_gpu_layer_grad.py, test_gpu_conv_grad.py): for
each component of a form key (tests/_train_forms.py) the smallest row that has it (``pick``).  The dense K x K convolution
has a table of its own (``CONV_PLANES`` and its neighbours), and the synchronised BatchNorm rows are named in
tests/test_gpu_nonfinite_layers.py."""
import math

import torch
import torch.nn.functional as TF

NAN, PINF, NINF = float('nan'), float('inf'), float('-inf')
VALUES = {'nan': NAN, '+inf': PINF, '-inf': NINF}
EPS, MOM = 1e-5, 0.1
ACT = {None: lambda z: z, 'relu': torch.relu, 'relu6': TF.relu6}


# ------------------------------------------------------------------ sites
def sites(shape, tiles=(), ragged=False):
    """The fixed list of sites of a tensor: [(name, index tuple)].  ``tiles``: (th, tw) pairs, the kernel's tile in this
    tensor's own coordinates; ``ragged``: the channel count is no multiple of the kernel's channel block."""
    shape = tuple(int(v) for v in shape)
    out = [('first', (0,) * len(shape)), ('last', tuple(v - 1 for v in shape))]
    if len(shape) == 4:
        N, C, H, W = shape
        n, c = N // 2, C // 2
        out += [('corner00', (n, c, 0, 0)), ('corner0W', (n, c, 0, W - 1)), ('cornerH0', (n, c, H - 1, 0)),
                ('cornerHW', (n, c, H - 1, W - 1)), ('edge', (n, c, H - 1, W // 2)), ('last plane', (N - 1, C - 1, H // 2, W // 2)),
                # the first channel of the last image: the row after the last channel of the image before it, which a
                # kernel that runs past a ragged channel tail (against a zero weight) reads
                ('next image', (N - 1, 0, H // 2, W // 2))]
        for th, tw in tiles:
            if H > th or W > tw:
                out += [('tile %d/%d lo' % (th, tw), (n, c, min(th - 1, H - 1), min(tw - 1, W - 1))),
                        ('tile %d/%d hi' % (th, tw), (n, c, min(th, H - 1), min(tw, W - 1)))]
        if W >= 8:                   # one 16-byte load in from either side: what a clamped vector load at the edge re-reads
            out += [('quad lo', (n, c, H // 2, 3)), ('quad hi', (n, c, H // 2, W - 4))]
        if ragged:
            out.append(('ragged channel', (n, C - 1, H // 2, W // 2)))
    elif len(shape) == 2:
        out.append(('middle', (shape[0] // 2, shape[1] - 1)))
    elif len(shape) == 1:
        out.append(('middle', (shape[0] // 2,)))
    seen, uniq = set(), []
    for name, idx in out:
        if idx not in seen:
            seen.add(idx)
            uniq.append((name, idx))
    return uniq


def inject(t, idx, value):
    t = t.clone()
    t[idx] = value
    return t


LARGE = 300000                       # elements of a row's largest tensor above which a row runs the short plan


def plan(site_list, large=False):
    """(site, value name) pairs of one operand: a NaN at every site, both infinities at the first and the last one.  A
    LARGE row keeps the first and the last element, the tile boundary, the quad sites, the ragged channel and the next image."""
    if large:
        site_list = [s for s in site_list if s[0] in ('first', 'last', 'ragged channel', 'next image') or s[0].startswith(('tile', 'quad'))]
    out = [(s, 'nan') for s in site_list]
    for s in site_list[:2]:                 # 'first' and 'last'
        out += [(s, '+inf'), (s, '-inf')]
    return out


# ------------------------------------------------------------------ the fp64 truth of each op: dict of fp32 inputs -> dict
def _w(t, grad=True):
    return None if t is None else t.detach().double().requires_grad_(grad)


def _grads(y, ins, dy):
    return torch.autograd.grad(y, ins, dy.detach().double(), allow_unused=True)


def ref_pw(ins):
    x, w = _w(ins['x']), _w(ins['w'])
    y = TF.conv2d(x, w.reshape(w.shape[0], -1, 1, 1))
    gx, gw = _grads(y, (x, w), ins['dy'])
    return dict(y=y.detach(), gx=gx, gw=gw)


def _valid(k, size, out, s, pad):
    """tap k of a convolution of stride s and padding pad: the outputs o whose input cell o * s - pad + k lies in
    [0, size) -> (o0, o1, i0), o1 exclusive, i0 the first input cell; None when the tap only ever meets padding"""
    o0 = max(0, -((k - pad) // s))
    o1 = min(out - 1, (size - 1 + pad - k) // s)
    return (o0, o1 + 1, o0 * s - pad + k) if o1 >= o0 else None


def _taps(K, H, W, OH, OW, s, pad):
    """(ky, kx, output slices, input slices) of the taps that meet the plane at all"""
    for ky in range(K):
        r = _valid(ky, H, OH, s, pad)
        for kx in range(K):
            c = _valid(kx, W, OW, s, pad)
            if r and c:
                yield (ky, kx, (slice(r[0], r[1]), slice(c[0], c[1])),
                       (slice(r[2], r[2] + (r[1] - r[0] - 1) * s + 1, s), slice(c[2], c[2] + (c[1] - c[0] - 1) * s + 1, s)))


# The convolutions with padding are summed tap by tap over the cells a tap really meets.  torch's conv2d and
# conv_transpose2d materialise the padding as zeros and MULTIPLY it: a NaN weight tap, or a NaN cell next to the border
# in a weight gradient, then poisons outputs that do not depend on it (0 * NaN), and the mask is wider than the cone
# (tests/test_nonfinite_cpu.py pins this).  On finite data the two are the same sums in another order.
def ref_dw(ins, k, s):
    x, w = _w(ins['x']), _w(ins['w'])
    N, C, H, W = x.shape
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    y = torch.zeros((N, C, OH, OW), dtype=torch.float64)
    for ky, kx, (orow, ocol), (irow, icol) in _taps(k, H, W, OH, OW, s, k // 2):
        y[:, :, orow, ocol] += x[:, :, irow, icol] * w[:, 0, ky, kx].view(1, C, 1, 1)
    gx, gw = _grads(y, (x, w), ins['dy'])
    return dict(y=y.detach(), gx=gx, gw=gw)


def ref_stem(ins):
    x, w = _w(ins['x'], False), _w(ins['w'])
    N, _, H, W = x.shape
    y = torch.zeros((N, 32, H // 2, W // 2), dtype=torch.float64)
    for ky, kx, (orow, ocol), (irow, icol) in _taps(3, H, W, H // 2, W // 2, 2, 1):
        y[:, :, orow, ocol] += torch.einsum('oc,nchw->nohw', w[:, :, ky, kx], x[:, :, irow, icol])
    # the weight gradient does not read w: the library's call does not even take it
    return dict(y=y.detach(), gw=_grads(y, (w,), ins['dy'])[0])


def _deconv_one(x, w, y):
    """y[2 i - 1 + ky][2 j - 1 + kx] += sum over c of x[c][i][j] w[c][o][ky][kx]: an output cell 2 i - 1 + k of stride 1 is
    what ``_valid`` calls the input cell of output i at stride 2, padding 1"""
    h, wd = x.shape[2:]
    for ky, kx, (irow, icol), (orow, ocol) in _taps(4, 2 * h, 2 * wd, h, wd, 2, 1):
        y[:, :, orow, ocol] += torch.einsum('nchw,co->nohw', x[:, :, irow, icol], w[:, :, ky, kx])


def ref_deconv(ins):
    two = ins.get('xb') is not None
    xa, wa, xb, wb = _w(ins['xa']), _w(ins['wa']), _w(ins.get('xb')), _w(ins.get('wb'))
    y = torch.zeros((xa.shape[0], wa.shape[1], 2 * xa.shape[2], 2 * xa.shape[3]), dtype=torch.float64)
    _deconv_one(xa, wa, y)
    if two:
        _deconv_one(xb, wb, y)
    g = _grads(y, (xa, wa, xb, wb) if two else (xa, wa), ins['dy'])
    out = dict(y=y.detach(), gxa=g[0], gwa=g[1])
    if two:
        out.update(gxb=g[2], gwb=g[3])
    return out


def _up(t, ups):
    return TF.interpolate(t, scale_factor=2, mode='nearest') if ups else t


def _conv_operands(ins):
    """the fp64 leaves of a dense convolution; without a bias a zero one stands in, so that its gradient -- the sum of
    grad_y, which the library hands out with or without a bias -- comes from the same autograd call"""
    xa, wa, xb, wb = _w(ins['xa']), _w(ins['wa']), _w(ins.get('xb')), _w(ins.get('wb'))
    b = _w(ins['bias']) if ins.get('bias') is not None else torch.zeros(wa.shape[0], dtype=torch.float64, requires_grad=True)
    return xa, wa, xb, wb, b


def _conv_outputs(y, leaves, ins):
    xa, wa, xb, wb, b = leaves
    two = xb is not None
    g = _grads(y, (xa, wa, xb, wb, b) if two else (xa, wa, b), ins['dy'])
    out = dict(y=y.detach(), gxa=g[0], gwa=g[1], gb=g[-1])
    if two:
        out.update(gxb=g[2], gwb=g[3])
    return out


def ref_conv(ins, k, s, ups):
    """The dense K x K convolution of tests/_dense_conv_check.py (``reference``: nearest x2 upsample when ups, conv2d of
    stride s and padding k // 2 over one or two sources, bias), summed tap by tap over the cells a tap really meets, as the
    other convolutions here are: torch's own conv2d -- ``reference`` itself, which is this op's ``torch_conv`` -- multiplies
    its padding in the forward and in the weight gradient (tests/test_nonfinite_cpu.py holds the two to each other on finite
    data and pins the difference).  -> y, gxa, gwa, gb (the sum of grad_y, with or without a bias), gxb, gwb with two sources"""
    leaves = xa, wa, xb, wb, b = _conv_operands(ins)
    H, W = xa.shape[2] << ups, xa.shape[3] << ups
    OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
    ua, ub = _up(xa, ups), (None if xb is None else _up(xb, ups))
    y = b.view(1, -1, 1, 1).expand(xa.shape[0], wa.shape[0], OH, OW).clone()
    for ky, kx, (orow, ocol), (irow, icol) in _taps(k, H, W, OH, OW, s, k // 2):
        t = torch.einsum('oc,nchw->nohw', wa[:, :, ky, kx], ua[:, :, irow, icol])
        if ub is not None:
            t = t + torch.einsum('oc,nchw->nohw', wb[:, :, ky, kx], ub[:, :, irow, icol])
        y[:, :, orow, ocol] += t
    return _conv_outputs(y, leaves, ins)


def torch_conv(kind, ins, **kw):
    """The same ops by torch's own convolutions plus autograd: what the tap-wise sums restate, WITH the multiplied padding.
    Its non-finite mask is the widest a kernel may have: one that materialises its halo as zeros and multiplies it, as torch
    does, poisons these outputs as torch does; one that selects does not.  Both are accepted (``compare``, ``Wb``)."""
    two = ins.get('xb') is not None
    if kind == 'conv':
        from _dense_conv_check import reference
        leaves = _conv_operands(ins)
        return _conv_outputs(reference(*leaves, kw['s'], kw['ups']), leaves, ins)
    if kind == 'deconv':
        xa, wa, xb, wb = _w(ins['xa']), _w(ins['wa']), _w(ins.get('xb')), _w(ins.get('wb'))
        y = TF.conv_transpose2d(xa, wa, None, 2, 1)
        if two:
            y = y + TF.conv_transpose2d(xb, wb, None, 2, 1)
        g = _grads(y, (xa, wa, xb, wb) if two else (xa, wa), ins['dy'])
        out = dict(y=y.detach(), gxa=g[0], gwa=g[1])
        if two:
            out.update(gxb=g[2], gwb=g[3])
        return out
    x, w = _w(ins['x'], kind == 'dw'), _w(ins['w'])
    if kind == 'dw':
        y = TF.conv2d(x, w, None, kw['s'], kw['k'] // 2, 1, x.shape[1])
        gx, gw = _grads(y, (x, w), ins['dy'])
        return dict(y=y.detach(), gx=gx, gw=gw)
    y = TF.conv2d(x, w, None, 2, 1)
    return dict(y=y.detach(), gw=_grads(y, (w,), ins['dy'])[0])


def ref_bn(ins, act, training):
    """BatchNorm by its definition, z = (x - mean) * invstd * gamma + beta, in torch, fp64, with autograd through the
    batch statistics.  torch's own batch_norm evaluates x * (gamma * invstd) + (beta - mean * gamma * invstd): the same
    value on finite data, but inf - inf where gamma is an infinity, which the definition (and the kernel, which follows it)
    does not have.  training: y, mean, invstd (the kept pair), rm, rv (the running pair after the step), gx, gg, gb;
    eval: y"""
    x, g, b = _w(ins['x']), _w(ins['gamma']), _w(ins['beta'])
    rm, rv = ins['rm'].double(), ins['rv'].double()
    res = ins.get('res')
    bc = lambda t: t.view(1, -1, 1, 1)                       # noqa: E731
    if training:
        cnt = x.shape[0] * x.shape[2] * x.shape[3]
        mean = x.mean((0, 2, 3))
        var = ((x - bc(mean)) ** 2).mean((0, 2, 3))
        rm = (1 - MOM) * rm + MOM * mean.detach()
        rv = (1 - MOM) * rv + MOM * (var.detach() * (cnt / (cnt - 1.0)) if cnt > 1 else var.detach())
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + EPS)
    z = (x - bc(mean)) * bc(invstd) * bc(g) + bc(b)
    y = ACT[act](z) + (res.double() if res is not None else 0)
    if not training:
        return dict(y=y.detach())
    gx, gg, gb = _grads(y, (x, g, b), ins['dy'])
    return dict(y=y.detach(), mean=mean.detach(), invstd=invstd.detach(), rm=rm, rv=rv, gx=gx, gg=gg, gb=gb)


# The kernels that stage a zero-filled halo of the partner operand and multiply it: (kind, operand) -> (output, kernel).
# Their outputs in ``halo_products`` go non-finite although they do not depend on the site and although torch's own
# convolution leaves them finite.  Kept as they are (a select per MFMA operand in four kernels is a change of its own);
# tests/test_gpu_nonfinite_layers.py holds each as a strict expected failure and counts what it lets through elsewhere.
HALO_KERNELS = {
    ('dw', 'x'): ('gw', 'dw_wgrad_kernel, csrc/layer_kernels.hip'),
    ('stem', 'x'): ('gw', 'stem_wgrad_kernel, csrc/conv_grad_kernels.hip'),
    ('deconv', 'wa'): ('y', 'deconv_raw_kernel, csrc/calib_kernels.hip'),
    ('deconv', 'wb'): ('y', 'deconv_raw_kernel, csrc/calib_kernels.hip'),
    ('deconv', 'dy'): ('gwa, gwb', 'deconv_wgrad_kernel, csrc/conv_grad_kernels.hip'),
    # the dense convolution's data gradient is convk3_kernel's stride-1 launch over grad_y (stride 2: over grad_y spread
    # over the input plane by dilate2_kernel) with the flipped, transposed weights: a weight tap meets the staged halo at
    # the border and, at stride 2, the dilation's zeros at the cells of the other parities
    ('conv', 'wa'): ('gxa', 'convk3_kernel over dilate2_kernel, csrc/convk_kernels.hip, csrc/dense_grad_kernels.hip'),
    ('conv', 'wb'): ('gxb', 'convk3_kernel over dilate2_kernel, csrc/convk_kernels.hip, csrc/dense_grad_kernels.hip'),
}
LEAKS = {}                           # what -> outputs poisoned beyond cone and torch's mask, filled by ``compare``


def halo_products(kind, row, operand, idx, shapes):
    """Outputs whose sum, in a kernel that stages a zero-filled halo of the PARTNER operand and multiplies it, holds a
    product of the site with such a zero -- beyond what torch's own convolutions already show (torch_conv).  0 * NaN is a
    NaN: a kernel may poison these outputs or not, as it may where torch does.  Four cases, read off the tilings:
      dense convolution data gradient, site in a weight tap: the whole input channel of the tap (below);
      depthwise and stem weight gradient, site in x: every tap whose stride parity the cell matches, whether or not the
        output cell it pairs with lies in the plane (grad_y's halo);
      transposed pair forward, site in a weight tap: the outputs that tap reaches from the one-cell halo of the input;
      transposed pair weight gradient, site in grad_y: the taps that pair the cell with an input cell of that halo.
    -> {output name: bool mask}"""
    out = {}
    if kind in ('dw', 'stem') and operand == 'x':
        k, s = (row[0], row[1]) if kind == 'dw' else (3, 2)
        m = torch.zeros(shapes['gw'], dtype=torch.bool)
        ky = [t for t in range(k) if (idx[2] + k // 2 - t) % s == 0]
        kx = [t for t in range(k) if (idx[3] + k // 2 - t) % s == 0]
        for a in ky:
            for b in kx:
                if kind == 'dw':
                    m[idx[1], 0, a, b] = True
                else:
                    m[:, idx[1], a, b] = True
        out['gw'] = m
    if kind == 'deconv' and operand in ('wa', 'wb'):
        m = torch.zeros(shapes['y'], dtype=torch.bool)
        H, W = shapes['y'][2:]
        rows = [2 * i - 1 + idx[2] for i in range(-1, H // 2 + 1) if 0 <= 2 * i - 1 + idx[2] < H]
        cols = [2 * j - 1 + idx[3] for j in range(-1, W // 2 + 1) if 0 <= 2 * j - 1 + idx[3] < W]
        for r in rows:
            m[:, idx[1], r, cols] = True
        out['y'] = m
    if kind == 'deconv' and operand == 'dy':
        for key in ('gwa', 'gwb'):
            if key in shapes:
                m = torch.zeros(shapes[key], dtype=torch.bool)
                for a in [t for t in range(4) if (idx[2] + 1 - t) % 2 == 0]:
                    for b in [t for t in range(4) if (idx[3] + 1 - t) % 2 == 0]:
                        m[:, idx[1], a, b] = True
                out[key] = m
    if kind == 'conv' and operand in ('wa', 'wb'):
        # dense convolution data gradient, site in a weight tap [co][ci][ky][kx]: a stride-1 convolution applies every tap
        # at every cell of its output, to a cell of the plane, of the halo or -- at stride 2 -- to a zero of the dilation;
        # so the tap is a factor of one product in every cell of input channel ci, in every image, and the 2x2 sums behind
        # the upsample keep that.  (dilated_data_gradient below is that formulation in torch.)
        key = 'gxa' if operand == 'wa' else 'gxb'
        m = torch.zeros(shapes[key], dtype=torch.bool)
        m[:, idx[1]] = True
        out[key] = m
    return out


def dilated_data_gradient(dy, w, s, ups):
    """The data gradient of a dense convolution the way lp_conv_backward forms it, in torch on whatever dtype the tensors
    share: grad_y spread over the input plane (stride 2: at the even cells, zeros elsewhere), a stride-1 conv2d with the
    flipped, transposed weights and padding K / 2, then the 2x2 sums behind a nearest x2 upsample."""
    z = dy
    if s == 2:
        z = torch.zeros(dy.shape[:2] + (2 * dy.shape[2], 2 * dy.shape[3]), dtype=dy.dtype)
        z[:, :, ::2, ::2] = dy
    g = TF.conv2d(z, w.flip(2, 3).transpose(0, 1), None, 1, w.shape[-1] // 2)
    return 4 * TF.avg_pool2d(g, 2) if ups else g


LINEAR = {'pw': ref_pw, 'dw': ref_dw, 'stem': ref_stem, 'deconv': ref_deconv, 'conv': ref_conv}


def indicator_cone(ref, ins, operand, idx, **kw):
    """The cone of the site by the second route: the op on the indicator of the site in ``operand`` with all-ones partners,
    against the op with that operand all zeros.  Integers in fp64: exact.  -> dict of bool masks"""
    ones = {k: (None if v is None else torch.ones_like(v)) for k, v in ins.items()}
    ind, zero = dict(ones), dict(ones)
    zero[operand] = torch.zeros_like(ins[operand])
    ind[operand] = inject(zero[operand], idx, 1.0)
    a, b = ref(ind, **kw), ref(zero, **kw)
    return {k: (torch.zeros(0, dtype=torch.bool) if a[k] is None else a[k] != b[k]) for k in a}


def cone(rb, value):
    return torch.isnan(rb) if math.isnan(value) else ~torch.isfinite(rb)


# ------------------------------------------------------------------ the comparison
def bitwise(a, b):
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return a.view(torch.uint8).eq(b.view(torch.uint8)).all().item() if a.numel() else True


def compare(what, O, Ob, R, Rb, value, exact, Wb=None, halo=None):
    """One output tensor.  O, Ob: the clean and the injected run of the code under test (any device); R, Rb: the fp64 truth,
    clean and injected (CPU); Wb: torch's own convolution on the injected input, whose mask may be wider than the cone by the
    outputs whose sum holds a product of the site with a padding zero -- there a kernel may go either way (torch_conv);
    halo: more outputs of that kind (halo_products).
    Returns the size of the cone."""
    assert O.shape == Ob.shape == R.shape == Rb.shape, (what, O.shape, Ob.shape, R.shape, Rb.shape)
    dev = Ob.device
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(O).all()), what + ': the clean run is not finite'
    want = cone(Rb, value).to(dev)
    may = want if Wb is None else want | cone(Wb, value).to(dev)
    if halo is not None:
        beyond = int((cone(Ob, value) & halo.to(dev) & ~may).sum())
        if beyond:
            LEAKS[what] = beyond
        may = may | halo.to(dev)
    got = cone(Ob, value)
    if bool((want & ~got).any()) or bool((got & ~may).any()):
        lost, leaked = int((want & ~got).sum()), int((got & ~may).sum())
        where = torch.nonzero((want & ~got) | (got & ~may))[:4].tolist()
        raise AssertionError('%s: cone of %d outputs, %d of them scrubbed, %d outputs outside it poisoned; first at %s'
                             % (what, int(want.sum()), lost, leaked, where))
    if exact and not math.isnan(value):
        rb = Rb.to(dev)
        assert torch.equal(torch.isnan(Ob) & want, torch.isnan(rb)), what + ': NaN where the truth is an infinity, or the reverse'
        inf = torch.isinf(rb)
        assert torch.equal(Ob[inf] > 0, rb[inf] > 0), what + ': an infinity of the wrong sign'
    same = (Rb == R).to(dev) & ~got
    a, b = Ob[same], O[same]
    if not bitwise(a, b):
        bad = torch.nonzero(same & (Ob.view(torch.int32) != O.view(torch.int32) if Ob.dtype == torch.float32
                                    else Ob.view(torch.int64) != O.view(torch.int64)))
        raise AssertionError('%s: %d outputs that do not depend on the site moved; first at %s'
                             % (what, bad.shape[0], bad[:4].tolist()))
    zero = same & (O == 0)
    assert not bool(Ob[zero].any()), what + ': an exact zero outside the cone did not stay zero'
    return int(want.sum())


def compare_all(what, O, Ob, R, Rb, value, exact, Wb=None, halo=None):
    assert set(O) == set(Ob) == set(R) == set(Rb), (what, sorted(O), sorted(R))
    return {k: compare('%s %s' % (what, k), O[k], Ob[k], R[k], Rb[k], value, exact, None if Wb is None else Wb[k],
                       None if halo is None else halo.get(k)) for k in O if O[k] is not None}


# ------------------------------------------------------------------ inputs
def rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).float()


def linear_inputs(kind, row):
    """fp32 inputs of moderate size (no fp32 overflow where fp64 has none) without an exact zero"""
    if kind == 'pw':
        ci, co, n, h, w = row
        ins = dict(x=rand((n, ci, h, w), 11), w=rand((co, ci), 12, 0.3), dy=rand((n, co, h, w), 13))
    elif kind == 'dw':
        k, s, c, n, h, w = row
        ins = dict(x=rand((n, c, h, w), 21), w=rand((c, 1, k, k), 22, 0.3), dy=rand((n, c, (h - 1) // s + 1, (w - 1) // s + 1), 23))
    elif kind == 'stem':
        n, H, W = row
        ins = dict(x=rand((n, 3, H, W), 31), w=rand((32, 3, 3, 3), 32, 0.3), dy=rand((n, 32, H // 2, W // 2), 33))
    elif kind == 'conv':
        ca, cb, co, n, h, w, k, s, ups, bias = row
        ins = dict(xa=rand((n, ca, h, w), 61), wa=rand((co, ca, k, k), 62, 0.3),
                   dy=rand((n, co, ((h << ups) - 1) // s + 1, ((w << ups) - 1) // s + 1), 65))
        ins['xb'], ins['wb'] = (rand((n, cb, h, w), 63), rand((co, cb, k, k), 64, 0.3)) if cb else (None, None)
        ins['bias'] = rand((co,), 66) if bias else None
    else:
        ca, cb, co, n, h, w = row
        ins = dict(xa=rand((n, ca, h, w), 41), wa=rand((ca, co, 4, 4), 42, 0.3), dy=rand((n, co, 2 * h, 2 * w), 45))
        ins['xb'], ins['wb'] = (rand((n, cb, h, w), 43), rand((cb, co, 4, 4), 44, 0.3)) if cb else (None, None)
    for v in ins.values():
        assert v is None or bool(v.ne(0).all())
    return ins


def linear_kw(kind, row):
    if kind == 'conv':
        return dict(k=row[6], s=row[7], ups=row[8])
    return dict(k=row[0], s=row[1]) if kind == 'dw' else {}


def convk3_tile(ow, s):
    """convk3_kernel's output tile (rows, columns) on a plane ow wide: 32 columns, or 16 on planes at most 16 wide; a wave
    owns two pixel groups of 32 cells at stride 1 and one at stride 2 (ck_geo, csrc/convk_kernels.hip)"""
    tw = 16 if ow <= 16 else 32
    return (4 * (2 if s == 1 else 1) * (32 // tw), tw)


def linear_sites(kind, row, operand, shape):
    """the sites of ``operand``: tiles in the operand's own coordinates, ragged channel counts flagged"""
    if kind == 'pw':
        ci, co = row[:2]
        if operand == 'w':
            return sites(shape)
        return sites(shape, [(16, 16)], ragged=bool((ci if operand == 'x' else co) % 32))
    if kind == 'dw':
        k, s, c = row[:3]
        if operand == 'w':
            return sites(shape, ragged=bool(c % 4))
        t = [(16, 16)] + ([(32, 32)] if s == 2 and operand == 'x' else [])
        return sites(shape, t, ragged=bool(c % 4))
    if kind == 'stem':
        return sites(shape) if operand == 'w' else sites(shape, [(16, 32)] if operand == 'x' else [(8, 16)])
    if kind == 'conv':
        ca, cb, co, n, h, w, k, s, ups, _ = row
        if operand == 'bias':
            return sites(shape)
        if operand in ('wa', 'wb'):      # [Cout][C][K][K]: the corner and edge taps are the ones that meet padding
            return sites(shape, ragged=bool(shape[1] % 16))
        ow = ((w << ups) - 1) // s + 1
        if operand == 'dy':
            # the weight gradient's 8 x 16 pixels, and the tile of the data gradient's stride-1 launch over the (dilated)
            # plane, in grad_y's coordinates
            th, tw = convk3_tile(w << ups, 1)
            return sites(shape, [(8, 16), (th // s, tw // s)], ragged=bool(co % 32))
        # the weight gradient's tile and the forward's, in the source's coordinates
        th, tw = convk3_tile(ow, s)
        return sites(shape, [(8 * s >> ups, 16 * s >> ups), (th * s >> ups, tw * s >> ups)], ragged=bool(shape[1] % 16))
    ca, cb, co = row[:3]
    if operand in ('wa', 'wb'):
        return sites(shape, ragged=bool(co % 8))
    if operand == 'dy':
        return sites(shape, [(16, 16)], ragged=bool(co % 8))
    return sites(shape, [(8, 8)], ragged=bool((ca + cb) % 32))


def bn_inputs(row, with_res):
    n, c, h, w = row
    ins = dict(x=rand((n, c, h, w), 51, 1.5, 0.75), gamma=rand((c,), 52, 0.5, 1.0), beta=rand((c,), 53, 1.0, 1.5),
               rm=rand((c,), 54, 0.3), rv=rand((c,), 55, 0.1, 1.0).abs(), dy=rand((n, c, h, w), 57))
    ins['res'] = rand((n, c, h, w), 56) if with_res else None
    return ins


# ------------------------------------------------------------------ the rows
def _numel(kind, row):
    if kind == 'pw':
        ci, co, n, h, w = row
        return n * max(ci, co) * h * w
    if kind == 'dw':
        k, s, c, n, h, w = row
        return n * c * h * w
    if kind == 'bn':
        n, c, h, w = row
        return n * c * h * w
    if kind == 'stem':
        n, H, W = row
        return n * 8 * H * W
    if kind == 'conv':
        ca, cb, co, n, h, w, k, s, ups, _ = row
        return n * max(ca + cb, co) * (h << ups) * (w << ups)
    ca, cb, co, n, h, w = row
    return n * max(ca + cb, 4 * co) * h * w


MIN_PLANE = 16                       # below 4 x 4 cells the corners, the edge midpoint and the centre of a plane coincide


def pick(kind, rows, forms):
    """For each component (position, value) of the form keys ``forms(row)`` gives, the smallest of ``rows`` that has it; the
    union, smallest first.  Ties go to the earlier row.  Planes of fewer than MIN_PLANE cells are left out."""
    rows = sorted((r for r in dict.fromkeys(rows) if r[-2] * r[-1] >= MIN_PLANE), key=lambda r: _numel(kind, r))
    chosen, seen = [], set()
    for r in rows:
        comps = {(key[:2] if key[0] == 'pw' else key[0], i, v) for key in forms(r) for i, v in enumerate(key)}
        if comps - seen:
            seen |= comps
            chosen.append(r)
    return chosen


_rows = {}

# The dense K x K convolution: rows (ca, cb, cout, n, h, w, k, s, ups, bias), the smallest shapes that select each thing that
# can go wrong.  What each component is there for:
#   forms     every K of {3, 5, 7} (one weight-gradient load form and column cut each) with every (stride, upsample)
#   channels  (5, 0, 3)   one source
#             (33, 7, 9)  two sources, ragged against the 16-channel k-step and the 32-row block; Ct = 40 crosses several
#                         channel groups of the weight gradient (14 / 10 / 10 per workgroup), the source boundary inside one
#             (3, 0, 40)  two 32-row blocks of Cout, the second ragged
#   planes    stride 1: (2, 5, 7) one partly filled 8 x 16 tile of the weight gradient -- pixels of the tile outside the plane;
#             (2, 8, 16) exactly one full tile, the control: the same sites, and no pixel outside the plane exists;
#             (1, 11, 21) 2 x 2 tiles, the last row and column partly filled, and convk3's 32-wide form
#             stride 2: (2, 6, 10) -> 3 x 5, (1, 18, 36) -> 9 x 18, the 32-wide form of the data gradient
#             through the upsample: (2, 3, 5) -> 6 x 10, (1, 6, 11) -> 12 x 22
# Not the full product: every K meets every (stride, upsample) on every plane of that form, and the channel sets and the bias
# rotate so that every component meets every component of another kind (tests/test_nonfinite_cpu.py asserts it).
CONV_KS = (3, 5, 7)
CONV_FORMS = ((1, 0), (1, 1), (2, 0))
CONV_CH = ((5, 0, 3), (33, 7, 9), (3, 0, 40))
CONV_PLANES = {(1, 0): ((2, 5, 7), (2, 8, 16), (1, 11, 21)), (1, 1): ((2, 3, 5), (1, 6, 11)), (2, 0): ((2, 6, 10), (1, 18, 36))}


def conv_rows():
    out = []
    for ki, k in enumerate(CONV_KS):
        for fi, form in enumerate(CONV_FORMS):
            for pi, plane in enumerate(CONV_PLANES[form]):
                out.append(CONV_CH[(ki + fi + pi) % 3] + plane + (k,) + form + ((ki + pi) % 2 == 0,))
    return out


def rows(kind):
    """the cases of ``kind``: 'pw', 'dw', 'bn', 'deconv', 'stem' are rows of the existing tables, chosen by ``pick``; 'conv'
    is the table above"""
    if kind in _rows:
        return _rows[kind]
    if kind == 'conv':
        _rows[kind] = conv_rows()
        return _rows[kind]
    import _train_forms as FM
    import test_gpu_conv_grad as CG
    import test_gpu_layer_grad as LG
    import test_gpu_train_forms as GT
    if kind == 'pw':
        cand = [(ci, co) + p for ci, co in LG.PW_CH for p in LG.PW_PLANES] + [c for c, _ in GT.PW_CASES + GT.PW_ODD_CASES]
        got = pick(kind, cand, lambda r: [FM.pw_mm_form(r[2], r[0], r[1], r[3], r[4], 'fwd'),
                                          FM.pw_mm_form(r[2], r[1], r[0], r[3], r[4], 'dx'),
                                          FM.pw_dw_form(r[2], r[0], r[1], r[3], r[4])])
    elif kind == 'dw':
        cand = [(k, s, c, n) + p for k in (3, 5, 7) for s in (1, 2) for c in (8, 24) for p in LG.DW_PLANES for n in (1, 3)]
        cand += [c for c, _ in GT.DW_CASES]

        def dw_key(r):                   # K, stride and forward family as ONE component: every K meets every family
            f = FM.dw_form(r[3], r[2], r[4], r[5], r[0], r[1])
            return [('dw', f[1:4]) + f[4:]]
        got = pick(kind, cand, dw_key)
    elif kind == 'bn':
        cand = [(n, c, h, w) for c in (3, 32) for n, h, w in ((2, 1, 1), (3, 5, 7), (2, 32, 32))] + [c for c, _ in GT.BN_CASES]
        got = pick(kind, cand, lambda r: [FM.bn_form(*r, False)[:6]])
    elif kind == 'deconv':
        cand = [ch + p for ch in CG.DECONV_CH for p in CG.DECONV_PLANES] + [c for c, _ in GT.DECONV_CASES]
        got = pick(kind, cand, lambda r: [FM.deconv_form(r[3], r[0], r[1], r[2], r[4], r[5])])
    else:
        cand = list(CG.STEM_PLANES) + [c for c, _ in GT.STEM_CASES]
        got = pick(kind, cand, lambda r: [FM.stem_form(*r)])
    _rows[kind] = got
    return got
