"""CPU restatement of pose_simplenet (reference lib/models/pose_simplenet.py): LitePose without the Fusion Deconv Head.
TEST INFRASTRUCTURE, pinned bit for bit against the real module by tests/golden/gen_golden_simplenet.py.

The stem and the InvBottleneck stages are oracle/net_ref.py's; the head differs (pose_simplenet.py:128-136):
  * deconv i   = ReLU(BN(ConvTranspose2d(refined)))      -- no deconv_raw term
  * output i-1 = final_refined[i-1](refined) (SepConv2d)  -- no final_raw term
``state_dict_shapes`` is oracle/spec.py's key scheme without ``deconv_raw.*`` / ``final_raw.*`` (the reference module's
registration order), ``make_state_dict`` the seeded synthetic weights of oracle/synth.py restricted to those keys.
``plan`` is the 16-bit storage emulation of the device path (tests/_f16_ref.py's op list and rounding places, plain head):
``rnd`` = net_ref._rb for bf16, _f16_ref.rh for fp16; ``absolute=True`` gives each element's term-magnitude sum."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import net_ref, spec, synth


def _is_raw(key):
    return key.startswith('deconv_raw.') or key.startswith('final_raw.')


def state_dict_shapes(arch, head=None):
    return OrderedDict((k, v) for k, v in spec.state_dict_shapes(arch, head).items() if not _is_raw(k))


def make_state_dict(arch, head=None, seed=1234, head_gain=1.0):
    sd = synth.make_state_dict(arch, head, seed=seed, head_gain=head_gain)
    return OrderedDict((k, sd[k]) for k in state_dict_shapes(arch, head))


def forward(x, sd, arch, head=None, taps=None):
    """[out0 (N, oup0, H/4, W/4), out1 (N, oup1, H/2, W/2)]; ``taps`` receives 'first', 'stage.S.B', 'deconv.I'."""
    d = spec.derive(arch, head)
    x = net_ref.stem(x, sd)
    if taps is not None:
        taps['first'] = x
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            x = net_ref.inv_bottleneck(x, sd, 'stage.%d.%d' % (s, b), blk, taps)
            if taps is not None:
                taps['stage.%d.%d' % (s, b)] = x
    outs = []
    refined = x
    for i in range(len(d['deconv'])):
        r = F.conv_transpose2d(refined, sd['deconv_refined.%d.weight' % i], None, 2, 1)
        refined = F.relu(net_ref._bn(r, sd, 'deconv_bnrelu.%d.0' % i))
        if taps is not None:
            taps['deconv.%d' % i] = refined
        if i > 0:
            outs.append(net_ref.sep_conv(refined, sd, 'final_refined.%d.conv' % (i - 1)))
    return outs


def _fold(sd, wkey, bn, rnd, transposed=False, absolute=False):
    w = sd[wkey].double()
    if bn is None:
        w = rnd(w.float())
        return (w.abs() if absolute else w), None
    s = sd[bn + '.weight'].double() / torch.sqrt(sd[bn + '.running_var'].double() + net_ref.BN_EPS)
    sh = sd[bn + '.bias'].double() - sd[bn + '.running_mean'].double() * s
    w = rnd((w * (s.view(1, -1, 1, 1) if transposed else s.view(-1, 1, 1, 1))).float())
    return (w.abs(), sh.float().abs()) if absolute else (w, sh.float())


def plan(sd, arch, rnd=net_ref._rb, head=None, absolute=False):
    """``(name, inputs, fn)`` in launch order under the device op names (lp_net_tap accepts them): ``fn`` maps the named
    inputs ('x' = the fp32 image) to the op's output after the store rounding ``rnd``; the two head 1x1s are fp32 and
    not rounded.  Folded weights: BN folded in double, then fp32, then ``rnd`` once."""
    d = spec.derive(arch, head)
    ops = []
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)

    def conv(name, src, wkey, bn, stride=1, pad=0, groups=1, act=None, res=None, store=True):
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
            return rnd(y) if store else y
        ops.append((name, [src] + ([res] if res is not None else []), fn))
        return name

    x = conv('stem.conv3x3s2', 'x', 'first.0.0.weight', 'first.0.1', 2, 1, 1, 'relu6')
    x = conv('stem.dw3', x, 'first.1.0.weight', 'first.1.1', 1, 1, 32, 'relu6')
    x = conv('stem.pw', x, 'first.2.weight', 'first.3')
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            e = conv(p + '.inv', x, p + '.inv.0.weight', p + '.inv.1', act='relu6')
            e = conv(p + '.depth_conv', e, p + '.depth_conv.0.weight', p + '.depth_conv.1', blk['stride'],
                     blk['k'] // 2, blk['feat'], 'relu6')
            x = conv(p + '.point_conv', e, p + '.point_conv.0.weight', p + '.point_conv.1',
                     res=x if blk['residual'] else None)
    refined = x
    for i in range(len(d['deconv'])):
        wr, sh = _fold(sd, 'deconv_refined.%d.weight' % i, 'deconv_bnrelu.%d.0' % i, rnd, transposed=True,
                       absolute=absolute)

        def dfn(a, wr=wr, sh=sh):
            y = F.conv_transpose2d(ab(a), wr, None, 2, 1) + sh.view(1, -1, 1, 1)
            return y if absolute else rnd(F.relu(y))
        ops.append(('deconv.%d' % i, [refined], dfn))
        refined = 'deconv.%d' % i
        if i > 0:
            pr = 'final_refined.%d.conv' % (i - 1)
            a = conv('final_refined.%d.dw5' % (i - 1), refined, pr + '.0.weight', pr + '.1', 1, 2,
                     d['heads'][i - 1]['refined_in'], 'relu')
            conv('final.%d.pw' % (i - 1), a, pr + '.3.weight', None, store=False)
    return ops


def is_head(name):
    return name.startswith('final.') and name.endswith('.pw')
