"""fp16-storage emulation of the network (LP_STORAGE_F16): oracle/net_ref.py's bf16_plan / forward_bf16 restated with
IEEE-half rounding.  The same op list, op names, BN folding (double, then fp32) and rounding places: folded conv weights
rounded once, fp32 accumulation / bias / activation / residual, every stored tensor rounded once (round-to-nearest-even,
subnormals kept, overflow to +-inf: ``tensor.to(torch.float16)``), the two head outputs fp32 and not rounded.

``rh`` is the rounding; ``plan(sd, arch, rnd=rh)`` takes another one so the tests can run the identical plan in bf16 and
compare the two formats on one footing.  ``plan(sd, arch, absolute=True)`` is the same op list computing, per output
element, the sum of the MAGNITUDES of the terms the op adds (|weights| against |inputs|, |bias|, |residual|; no activation,
no rounding): the scale of the fp32 accumulation error, which at fp16 resolution is visible where the terms cancel
(an output of 1e-3 from terms that sum to 45 in magnitude: two fp32 summation orders differ by a few 1e-6 there)."""
import torch
import torch.nn.functional as F

from oracle import net_ref, spec


def rh(x):
    """fp32 -> fp16 (RNE, subnormals kept) -> fp32."""
    return x.to(torch.float16).to(torch.float32)


def _fold(sd, wkey, bn, rnd, transposed=False, absolute=False):
    w = sd[wkey].double()
    if bn is None:
        w = rnd(w.float())
        return (w.abs() if absolute else w), None
    s = sd[bn + '.weight'].double() / torch.sqrt(sd[bn + '.running_var'].double() + net_ref.BN_EPS)
    sh = sd[bn + '.bias'].double() - sd[bn + '.running_mean'].double() * s
    w = rnd((w * (s.view(1, -1, 1, 1) if transposed else s.view(-1, 1, 1, 1))).float())
    return (w.abs(), sh.float().abs()) if absolute else (w, sh.float())


def plan(sd, arch, head=None, rnd=rh, absolute=False):
    """``(name, inputs, fn)`` in launch order, as net_ref.bf16_plan: ``fn`` maps the named inputs ('x' = the fp32
    image, otherwise an earlier op's name) to the op's output after the store rounding ``rnd`` (``absolute``: to the
    magnitude sum of its terms, see the module docstring)."""
    d = spec.derive(arch, head)
    ops = []
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)

    def conv(name, src, wkey, bn, stride=1, pad=0, groups=1, act=None, res=None):
        w, b = _fold(sd, wkey, bn, rnd, absolute=absolute)

        def fn(x, r=None):
            y = F.conv2d(ab(x), w, b, stride, pad, 1, groups)
            if absolute:
                return y if r is None else y + r.abs()
            if act == 'relu6':
                y = torch.clamp(y, 0.0, 6.0)
            elif act == 'relu':
                y = F.relu(y)
            if r is not None:
                y = y + r
            return rnd(y)
        ops.append((name, [src] + ([res] if res is not None else []), fn))
        return name

    x = conv('stem.conv3x3s2', 'x', 'first.0.0.weight', 'first.0.1', 2, 1, 1, 'relu6')
    x = conv('stem.dw3', x, 'first.1.0.weight', 'first.1.1', 1, 1, 32, 'relu6')
    x = conv('stem.pw', x, 'first.2.weight', 'first.3')
    x_list = [x]
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            e = conv(p + '.inv', x, p + '.inv.0.weight', p + '.inv.1', act='relu6')
            e = conv(p + '.depth_conv', e, p + '.depth_conv.0.weight', p + '.depth_conv.1', blk['stride'],
                     blk['k'] // 2, blk['feat'], 'relu6')
            x = conv(p + '.point_conv', e, p + '.point_conv.0.weight', p + '.point_conv.1',
                     res=x if blk['residual'] else None)
        x_list.append(x)
    refined, raw = x_list[-1], x_list[-2]
    for i in range(len(d['deconv'])):
        bn = 'deconv_bnrelu.%d.0' % i
        wr, sh = _fold(sd, 'deconv_refined.%d.weight' % i, bn, rnd, transposed=True, absolute=absolute)
        ww, _ = _fold(sd, 'deconv_raw.%d.weight' % i, bn, rnd, transposed=True, absolute=absolute)

        def dfn(a, b, wr=wr, ww=ww, sh=sh):
            y = F.conv_transpose2d(ab(a), wr, None, 2, 1) + F.conv_transpose2d(ab(b), ww, None, 2, 1) + sh.view(1, -1, 1, 1)
            return y if absolute else rnd(F.relu(y))
        ops.append(('deconv.%d' % i, [refined, raw], dfn))
        refined = 'deconv.%d' % i
        raw = x_list[-i - 3]
        if i > 0:
            pr, pw = 'final_refined.%d.conv' % (i - 1), 'final_raw.%d.conv' % (i - 1)
            ca = d['heads'][i - 1]['refined_in']
            cb = d['heads'][i - 1]['raw_in']
            a = conv('final_refined.%d.dw5' % (i - 1), refined, pr + '.0.weight', pr + '.1', 1, 2, ca, 'relu')
            bq = conv('final_raw.%d.dw5' % (i - 1), raw, pw + '.0.weight', pw + '.1', 1, 2, cb, 'relu')
            w3a, _ = _fold(sd, pr + '.3.weight', None, rnd, absolute=absolute)
            w3b, _ = _fold(sd, pw + '.3.weight', None, rnd, absolute=absolute)

            def hfn(a, b, w3a=w3a, w3b=w3b):                # fp32 out: the AE stage reads fp32 maps
                return F.conv2d(ab(a), w3a) + F.conv2d(ab(b), w3b)
            ops.append(('final.%d.pw' % (i - 1), [a, bq], hfn))
    return ops


def forward(x, sd, arch, head=None, taps=None, rnd=rh):
    """fp16-storage emulation of net_ref.forward (same return value; ``taps`` as net_ref.forward_bf16)."""
    vals = {'x': x}
    outs = []
    for name, ins, fn in plan(sd, arch, head, rnd):
        y = fn(*[vals[k] for k in ins])
        vals[name] = y
        if name.startswith('final.') and name.endswith('.pw'):
            outs.append(y)
    if taps is not None:
        for k, v in vals.items():
            if k == 'x':
                continue
            taps[k] = v
            if k == 'stem.pw':
                taps['first'] = v
            elif k.endswith('.point_conv'):
                taps[k[:-len('.point_conv')]] = v
    return outs
