"""The fp32 network as UNITS in float64, each with a per-element error magnitude: the fp32 analogue of
``net_ref.bf16_plan``.  A unit is what the fp32 engine stores on both sides of: its inputs are taps of the device
(``lp_net_tap``: 'first', 'stage.S.B', 'deconv.I') or the image, its output is a tap or one of the two network outputs.

  stem        image -> 'first'                conv3x3 s2 + BN + relu6, dw3 + BN + relu6, 1x1 + BN
  stage.S.B   previous tap -> 'stage.S.B'     expand, depthwise, project (+ the residual where the block has one)
  deconv.I    (refined, raw) -> 'deconv.I'    the two transposed convolutions, summed, + BN + relu
  final.I     (refined, raw) -> output I      per branch dw5 + BN + relu, then 1x1; the branches summed

``fn(*inputs)`` of a unit returns ``(ref, B, ref32)`` for fp32 inputs (the DEVICE's own taps, so that the drift of the
layers in front is out of the comparison):
  * ``ref``: the unit in float64.  BatchNorm is folded in float64 and the folded weight rounded ONCE to fp32, as the
    device plan does; what is left between ``ref`` and the device is the kernel's arithmetic alone.
  * ``B >= 0``: the first-order error magnitude per element, in float64.  One convolution: ``A = conv(|x|, |w|) + |b|``.
    Through a chain clamp and relu are 1-Lipschitz, so the magnitude of a stage travels through the absolute weights
    of the later ones: ``E1 = A1``, ``E2 = A2 + |W2| E1``, ``E3 = A3 + |W3| E2`` and ``B = E3 + |ref|`` (the last term:
    the residual add and the store).  A unit that is a single convolution (deconv.I, a dense k x k convolution of
    pose_resnet) has ``B = A``.
  * ``ref32``: the same unit in plain fp32 torch in the reference's op order (conv -> BN -> act, unfused): the
    reference's own arithmetic, the yardstick of R.

With ``e = |got - ref|`` and ``u = 2^-24``, per unit and per compared image:
  P (per element)   e <= C_MAX[kind] * u * B everywhere;
  R (whole tap)     rms(e / B) <= M * rms(|ref32 - ref| / B).
``C_MAX`` and ``M`` come from tests/test_fp32_units_cpu.py: a pessimistic emulation of the correct kernel arithmetic
and mutants of it, on the CPU.  They are never set from a device measurement.

For a head FORM that is not the default (pose_simplenet: one source per deconv and head) ``units(..., heads=False)``
gives the stem and block units only: the deconv and output-head units are SKIPPED there.  Another HeadCfg of the default
form (17 joints) changes channel counts only and keeps all units."""
import torch
import torch.nn.functional as F

from oracle import net_ref, spec

U = 2.0 ** -24

# ---- the constants, from tests/test_fp32_units_cpu.py (its docstring has the table they come from)
# M: half of the smallest R ratio of any product-class mutant; the pessimistic emulation stays at or below M / 2.
#    Weakest mutant: R = 26.3 (the activation split into two pieces, at the project of 64 -> 384 -> 24); the emulation: at
#    most 5.9 (a single convolution of 1024 products), 3.1 among the blocks (120 -> 720 -> 120, 160 -> 960 -> 160).
#    The dense k x k convolutions of pose_resnet are a class of their own: their sums are up to 9408 products long, the
#    fully sequential emulation drifts to R = 11.3 there while the weakest mutant of the class has R = 42.9.  M_KIND holds
#    half of that; the emulation passes it (0.54 of it) without the factor 2 to spare that the other classes have.
M = 13.0
M_KIND = {'dense': 21.0}
# C_MAX: twice the largest per-element e / (u B) of the pessimistic emulation, per unit kind: 10.7 for a single
# convolution (B = A) and 8.3 for a dense k x k one; 0.37 / 1.01 / 0.45 for a block / head / stem, whose chained B is 20
# to 40 times A.  'block_small': the blocks of the small-magnitude row (project BatchNorm weight x 2^-8), where B is
# close to |ref| and the rounding of the final add alone is up to 0.5: 0.84.
C_MAX = {'conv': 22.0, 'dense': 17.0, 'block': 0.75, 'block_small': 1.7, 'head': 2.1, 'stem': 0.95}


def m_of(kind):
    return M_KIND.get(kind, M)


# ------------------------------------------------------------------ pieces, any dtype
def fold(sd, wkey, bn, transposed=False):
    """(weight, bias) as float64 tensors holding the fp32 values the device plan packs: folded in float64, rounded
    once to fp32.  ``bn`` None: the plain weight, no bias."""
    w = sd[wkey].double()
    if bn is None:
        return w.float().double(), None
    s = sd[bn + '.weight'].double() / torch.sqrt(sd[bn + '.running_var'].double() + net_ref.BN_EPS)
    sh = sd[bn + '.bias'].double() - sd[bn + '.running_mean'].double() * s
    w = w * (s.view(1, -1, 1, 1) if transposed else s.view(-1, 1, 1, 1))
    return w.float().double(), sh.float().double()


def pw(x, w, b=None):
    """1x1 convolution as a matrix product; w (Cout, Cin, 1, 1)."""
    n, c, h, wd = x.shape
    y = torch.matmul(w.view(w.shape[0], c), x.reshape(n, c, h * wd)).view(n, w.shape[0], h, wd)
    return y if b is None else y + b.view(1, -1, 1, 1)


def dw(x, w, b, stride, pad):
    """Depthwise k x k convolution as k*k shifted multiply-adds (row-major tap order); w (C, 1, k, k)."""
    k = w.shape[-1]
    n, c, h, wd = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    y = torch.zeros((n, c, ho, wo), dtype=x.dtype)
    for i in range(k):
        for j in range(k):
            y += w[:, 0, i, j].view(1, -1, 1, 1) * xp[:, :, i:i + stride * (ho - 1) + 1:stride,
                                                      j:j + stride * (wo - 1) + 1:stride]
    return y if b is None else y + b.view(1, -1, 1, 1)


def _relu6(x):
    return torch.clamp(x, 0.0, 6.0)


class Unit(object):
    """name, kind (key of C_MAX), ins (tap names, 'x' = the image), out (tap name or ('out', I)), fn."""

    def __init__(self, name, kind, ins, out, fn):
        self.name, self.kind, self.ins, self.out, self.fn = name, kind, ins, out, fn


# ------------------------------------------------------------------ the four unit bodies
def block_fn(sd, p, blk):
    w1, b1 = fold(sd, p + '.inv.0.weight', p + '.inv.1')
    wd, bd = fold(sd, p + '.depth_conv.0.weight', p + '.depth_conv.1')
    w3, b3 = fold(sd, p + '.point_conv.0.weight', p + '.point_conv.1')
    s, pad = blk['stride'], blk['k'] // 2

    def fn(x):
        x64 = x.double()
        y1 = pw(x64, w1, b1)
        e1 = pw(x64.abs(), w1.abs(), b1.abs())
        y1 = _relu6(y1)
        y2 = dw(y1, wd, bd, s, pad)
        e2 = dw(y1 + e1, wd.abs(), bd.abs(), s, pad)             # A2 + |Wd| E1: y1 >= 0
        del e1, y1
        y2 = _relu6(y2)
        ref = pw(y2, w3, b3)
        e3 = pw(y2 + e2, w3.abs(), b3.abs())                     # A3 + |W3| E2: y2 >= 0
        if blk['residual']:
            ref = ref + x64
        with torch.no_grad():
            ref32 = net_ref.inv_bottleneck(x, sd, p, blk)
        return ref, e3 + ref.abs(), ref32
    return fn


def stem_fn(sd):
    w0, b0 = fold(sd, 'first.0.0.weight', 'first.0.1')
    w1, b1 = fold(sd, 'first.1.0.weight', 'first.1.1')
    w2, b2 = fold(sd, 'first.2.weight', 'first.3')

    def fn(x):
        x64 = x.double()
        y0 = _relu6(F.conv2d(x64, w0, b0, 2, 1))
        e0 = F.conv2d(x64.abs(), w0.abs(), b0.abs(), 2, 1)
        y1 = _relu6(dw(y0, w1, b1, 1, 1))
        e1 = dw(y0 + e0, w1.abs(), b1.abs(), 1, 1)
        ref = pw(y1, w2, b2)
        e2 = pw(y1 + e1, w2.abs(), b2.abs())
        with torch.no_grad():
            ref32 = net_ref.stem(x, sd)
        return ref, e2 + ref.abs(), ref32
    return fn


def deconv_fn(sd, i):
    bn = 'deconv_bnrelu.%d.0' % i
    wr, sh = fold(sd, 'deconv_refined.%d.weight' % i, bn, transposed=True)
    ww, _ = fold(sd, 'deconv_raw.%d.weight' % i, bn, transposed=True)

    def fn(a, b):
        a64, b64 = a.double(), b.double()
        ref = F.relu(F.conv_transpose2d(a64, wr, None, 2, 1) + F.conv_transpose2d(b64, ww, None, 2, 1)
                     + sh.view(1, -1, 1, 1))
        B = F.conv_transpose2d(a64.abs(), wr.abs(), None, 2, 1) + F.conv_transpose2d(b64.abs(), ww.abs(), None, 2, 1) \
            + sh.abs().view(1, -1, 1, 1)
        with torch.no_grad():
            r = F.conv_transpose2d(a, sd['deconv_refined.%d.weight' % i], None, 2, 1)
            w = F.conv_transpose2d(b, sd['deconv_raw.%d.weight' % i], None, 2, 1)
            ref32 = F.relu(net_ref._bn(r + w, sd, bn))
        return ref, B, ref32
    return fn


def head_fn(sd, i):
    pr, pq = 'final_refined.%d.conv' % i, 'final_raw.%d.conv' % i
    wa, ba = fold(sd, pr + '.0.weight', pr + '.1')
    wb, bb = fold(sd, pq + '.0.weight', pq + '.1')
    w3a, _ = fold(sd, pr + '.3.weight', None)
    w3b, _ = fold(sd, pq + '.3.weight', None)

    def fn(a, b):
        ref, E = 0.0, 0.0
        for x, wdw, bdw, w3 in ((a, wa, ba, w3a), (b, wb, bb, w3b)):
            x64 = x.double()
            y = F.relu(dw(x64, wdw, bdw, 1, 2))
            e = dw(x64.abs(), wdw.abs(), bdw.abs(), 1, 2)
            ref = ref + pw(y, w3)
            E = E + pw(y + e, w3.abs())
        with torch.no_grad():
            ref32 = net_ref.sep_conv(a, sd, pr) + net_ref.sep_conv(b, sd, pq)
        return ref, E + ref.abs(), ref32
    return fn


def conv_unit(x, w, b, stride=1, pad=0):
    """A single dense convolution (+ bias) in float64 on fp32 values: (ref before any activation, B = conv(|x|, |w|) +
    |b|).  ``w`` and ``b`` are the folded fp32 values the device holds."""
    x64, w64 = x.double(), w.double()
    b64 = None if b is None else b.double()
    ref = F.conv2d(x64, w64, b64, stride, pad)
    B = F.conv2d(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), stride, pad)
    return ref, B


def units(sd, arch, head=None, heads=True):
    """The units of the fp32 network in launch order.  ``heads`` False: the stem and the blocks only."""
    d = spec.derive(arch, head)
    out = [Unit('stem', 'stem', ['x'], 'first', stem_fn(sd))]
    prev = 'first'
    ends = ['first']
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            out.append(Unit(p, 'block', [prev], p, block_fn(sd, p, blk)))
            prev = p
        ends.append(prev)
    if not heads:
        return out
    refined, raw = ends[-1], ends[-2]
    for i in range(len(d['deconv'])):
        out.append(Unit('deconv.%d' % i, 'conv', [refined, raw], 'deconv.%d' % i, deconv_fn(sd, i)))
        refined, raw = 'deconv.%d' % i, ends[-i - 3]
        if i > 0:
            out.append(Unit('final.%d' % (i - 1), 'head', [refined, raw], ('out', i - 1), head_fn(sd, i - 1)))
    return out


# ------------------------------------------------------------------ the two criteria
def measure(got, ref, B, ref32):
    """(P: max e / (u B), R: rms(e / B) / rms(|ref32 - ref| / B)) of one image; B == 0 demands e == 0."""
    e = (got.double() - ref).abs()
    y = (ref32.double() - ref).abs()
    zero = B <= 0
    assert not bool((e[zero] > 0).any()), 'an element with B == 0 differs from the reference'
    Bs = torch.where(zero, torch.ones_like(B), B)
    q = e / Bs
    p = float(q.max()) / U
    r = float(torch.sqrt((q * q).mean())) / max(float(torch.sqrt(((y / Bs) ** 2).mean())), 1e-300)
    return p, r


def check(got, ref, B, ref32, kind, what, assert_r=True):
    """P and R of one image as fractions of their bounds (both asserted): (P / C_MAX[kind], R / M)."""
    p, r = measure(got, ref, B, ref32)
    pf, rf = p / C_MAX[kind], r / m_of(kind)
    assert pf <= 1.0, ('P: an element beyond c_max u B', what, kind, p, C_MAX[kind])
    if assert_r:
        assert rf <= 1.0, ('R: the tap beyond m times the fp32 reference', what, kind, r, m_of(kind))
    return pf, rf


def check_device(m, sd, arch, xin, outs, images, head=None, heads=True, kinds=None):
    """Every unit on the device's own taps of the last forward, for the images ``images`` of the device batch ``xin``
    (N', 3, H, W; the mirrored half already flipped).  ``kinds``: {unit kind: the C_MAX class to use instead}.  Returns
    {unit name: (worst P fraction, worst R fraction)}."""
    NB = xin.shape[0]
    us = units(sd, arch, head, heads)
    flat = {}
    for un in us:
        if not isinstance(un.out, tuple):
            flat[un.out] = m.tap(un.out).view(NB, -1)
    rows = {}
    for n in images:
        dev = {'x': xin[n:n + 1].cpu().float()}
        for un in us:
            ref, B, ref32 = un.fn(*[dev[k] for k in un.ins])
            if isinstance(un.out, tuple):
                got = outs[un.out[1]][n:n + 1].cpu()
            else:
                got = flat[un.out][n:n + 1].cpu().view(ref.shape)
                dev[un.out] = got
            assert got.shape == ref.shape, (un.name, got.shape, ref.shape)
            pf, rf = check(got, ref, B, ref32, (kinds or {}).get(un.kind, un.kind), (un.name, 'image', n))
            old = rows.get(un.name, (0.0, 0.0))
            rows[un.name] = (max(old[0], pf), max(old[1], rf))
    return rows
