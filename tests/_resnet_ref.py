"""CPU restatement of pose_resnet (reference lib/models/pose_resnet.py: LitePose built from dense FusedMBConv blocks).
TEST INFRASTRUCTURE, pinned bit for bit against the real module by tests/golden/gen_golden_resnet.py.

The network (pose_resnet.py:21-131, layers.py:18-24,58-88):
  * stem       conv 7x7 s2 p3 3->32 + BN + ReLU6, conv 7x7 s1 p3 32->16 + BN + ReLU6
  * stages     FusedMBConv blocks, table [r, k, c, n, s] below: conv k x k (stride s on the first block of a stage,
               pad k//2) inp -> make_divisible(round(inp * r), 8) + BN + ReLU6, conv 1x1 -> c + BN, + x iff s == 1 and inp == c
  * deconv i   ReLU(BN(UpConv_refined(refined) + UpConv_raw(raw))), UpConv = nearest x2 then conv k x k pad k//2, no bias
  * output i-1 final_refined[i-1](refined) + final_raw[i-1](raw): one biased 3x3 conv each, no BN, no activation
There is no arch JSON: the table is fixed, the deconv widths / kernels come from cfg.MODEL.EXTRA.
Every function takes an optional ``table = (input_channel, [[r, k, c, n, s], ...])`` in place of the module's constants
(None: the constants): the same generic code on another table, for the tables ``lp_net_create`` accepts and the
reference module cannot express (tests/test_gpu_resnet_census.py; tests/golden/gen_golden_resnet.py pins the tables
``width_mult`` can express to the real module).  ``forward`` runs on whatever dtype ``x`` and ``sd`` share: with
float64 tensors it is the high-precision reference.
``make_state_dict`` follows oracle/synth.py's recipe (randomised BN statistics; std = sqrt(2 / fan_in), x0.35 on
point_conv, x0.5 on the UpConv convs, x0.05 * head_gain on the head convs)."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
INPUT_CHANNEL = 16
BACKBONE = [[4, 7, 16, 4, 2], [4, 7, 32, 6, 2], [4, 5, 48, 8, 2], [4, 3, 80, 8, 1]]      # r, k, c, n, s


def _make_divisible(v, divisor=8):
    nv = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if nv < 0.9 * v:
        nv += divisor
    return nv


def derive(cfg, table=None):
    """Channel bookkeeping: c0, stages [[{inp, feat, oup, k, stride, residual}]], channel, deconv, heads."""
    input_channel, backbone = (INPUT_CHANNEL, BACKBONE) if table is None else table
    c0 = _make_divisible(input_channel)
    channel, stages, inp = [c0], [], c0
    for r, k, c, n, s in backbone:
        c = _make_divisible(c)
        blocks = []
        for b in range(n):
            st = s if b == 0 else 1
            blocks.append(dict(inp=inp, feat=_make_divisible(round(inp * r)), oup=c, k=k, stride=st,
                               residual=(st == 1 and inp == c)))
            inp = c
        stages.append(blocks)
        channel.append(c)
    extra = cfg.MODEL.EXTRA
    nd = int(extra.NUM_DECONV_LAYERS)
    filters = [int(f) for f in extra.NUM_DECONV_FILTERS]
    kernels = [int(k) for k in extra.NUM_DECONV_KERNELS]
    deconv, inplanes = [], channel[-1]
    for i in range(nd):
        deconv.append(dict(refined_in=inplanes, raw_in=channel[-i - 2], out=filters[i], k=kernels[i]))
        inplanes = filters[i]
    dim_tag = cfg.MODEL.NUM_JOINTS if cfg.MODEL.TAG_PER_JOINT else 1
    heads = []
    for i in range(1, nd):
        oup = (cfg.MODEL.NUM_JOINTS if cfg.LOSS.WITH_HEATMAPS_LOSS[i - 1] else 0) + \
              (dim_tag if cfg.LOSS.WITH_AE_LOSS[i - 1] else 0)
        heads.append(dict(refined_in=filters[i], raw_in=channel[-i - 3], oup=int(oup)))
    return dict(c0=c0, stages=stages, channel=channel, deconv=deconv, heads=heads)


def _bn_keys(out, p, c):
    out[p + '.weight'] = (c,)
    out[p + '.bias'] = (c,)
    out[p + '.running_mean'] = (c,)
    out[p + '.running_var'] = (c,)
    out[p + '.num_batches_tracked'] = ()


def state_dict_shapes(cfg, table=None):
    """The module's state_dict() keys in registration order -> shapes."""
    d = derive(cfg, table)
    o = OrderedDict()
    o['first.0.0.weight'] = (32, 3, 7, 7)
    _bn_keys(o, 'first.0.1', 32)
    o['first.1.0.weight'] = (d['c0'], 32, 7, 7)
    _bn_keys(o, 'first.1.1', d['c0'])
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            o[p + '.inv.0.weight'] = (blk['feat'], blk['inp'], blk['k'], blk['k'])
            _bn_keys(o, p + '.inv.1', blk['feat'])
            o[p + '.point_conv.0.weight'] = (blk['oup'], blk['feat'], 1, 1)
            _bn_keys(o, p + '.point_conv.1', blk['oup'])
    for which, src in (('deconv_refined', 'refined_in'), ('deconv_raw', 'raw_in')):
        for i, dc in enumerate(d['deconv']):
            o['%s.%d.conv.weight' % (which, i)] = (dc['out'], dc[src], dc['k'], dc['k'])
    for i, dc in enumerate(d['deconv']):
        _bn_keys(o, 'deconv_bnrelu.%d.0' % i, dc['out'])
    for which, src in (('final_refined', 'refined_in'), ('final_raw', 'raw_in')):
        for i, h in enumerate(d['heads']):
            o['%s.%d.weight' % (which, i)] = (h['oup'], h[src], 3, 3)
            o['%s.%d.bias' % (which, i)] = (h['oup'],)
    return o


def make_state_dict(cfg, seed=1234, head_gain=1.0, table=None):
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for k, shp in state_dict_shapes(cfg, table).items():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith('running_var') or (k.endswith('.weight') and len(shp) == 1):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k.endswith('running_mean') or k.endswith('.bias'):
            sd[k] = torch.randn(shp, generator=g) * 0.1
        else:
            std = math.sqrt(2.0 / (shp[1] * shp[2] * shp[3]))
            if '.point_conv.' in k:
                std *= 0.35
            elif k.startswith('deconv'):
                std *= 0.5
            elif k.startswith('final'):
                std *= 0.05 * head_gain
            sd[k] = torch.randn(shp, generator=g) * std
    return sd


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'],
                        False, 0.0, BN_EPS)


def _convbnrelu6(x, sd, conv, bn, stride):
    w = sd[conv + '.weight']
    return F.relu6(_bn(F.conv2d(x, w, None, stride, w.shape[2] // 2), sd, bn))


def _upconv(x, w):
    return F.conv2d(F.interpolate(x, scale_factor=2), w, None, 1, w.shape[2] // 2)


def forward(x, sd, cfg, taps=None, table=None):
    """[out0 (N, oup0, H/4, W/4), out1 (N, oup1, H/2, W/2)] (a table whose deepest plane is 1/32: H/8 and H/4); ``taps``
    receives 'first', 'stage.S.B.inv', 'stage.S.B', 'deconv.I'."""
    d = derive(cfg, table)
    x = _convbnrelu6(x, sd, 'first.0.0', 'first.0.1', 2)
    if taps is not None:
        taps['first.0'] = x                               # a launch name, not a block tap: tap_names leaves it out
    x = _convbnrelu6(x, sd, 'first.1.0', 'first.1.1', 1)
    if taps is not None:
        taps['first'] = x
    x_list = [x]
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            e = _convbnrelu6(x, sd, p + '.inv.0', p + '.inv.1', blk['stride'])
            if taps is not None:
                taps[p + '.inv'] = e
            y = _bn(F.conv2d(e, sd[p + '.point_conv.0.weight']), sd, p + '.point_conv.1')
            x = y + x if blk['residual'] else y
            if taps is not None:
                taps[p] = x
        x_list.append(x)
    outs = []
    refined, raw = x_list[-1], x_list[-2]
    for i in range(len(d['deconv'])):
        r = _upconv(refined, sd['deconv_refined.%d.conv.weight' % i])
        w = _upconv(raw, sd['deconv_raw.%d.conv.weight' % i])
        refined = F.relu(_bn(r + w, sd, 'deconv_bnrelu.%d.0' % i))
        raw = x_list[-i - 3]
        if taps is not None:
            taps['deconv.%d' % i] = refined
        if i > 0:
            fr = F.conv2d(refined, sd['final_refined.%d.weight' % (i - 1)], sd['final_refined.%d.bias' % (i - 1)], 1, 1)
            fw = F.conv2d(raw, sd['final_raw.%d.weight' % (i - 1)], sd['final_raw.%d.bias' % (i - 1)], 1, 1)
            outs.append(fr + fw)
    return outs


def tap_names(cfg, table=None):
    d = derive(cfg, table)
    names = ['first']
    for s, blocks in enumerate(d['stages']):
        for b in range(len(blocks)):
            names += ['stage.%d.%d.inv' % (s, b), 'stage.%d.%d' % (s, b)]
    return names + ['deconv.%d' % i for i in range(len(d['deconv']))]


# ------------------------------------------------------------------ tables and cfgs other than the module's constants
def width_table(width_mult):
    """The table ``LitePose(cfg, width_mult=w)`` builds (pose_resnet.py:33,42): every channel count scaled, then rounded
    to a multiple of 8 -- as integers, the form ``lp_arch`` takes."""
    return (_make_divisible(INPUT_CHANNEL * width_mult),
            [[r, k, _make_divisible(c * width_mult), n, s] for r, k, c, n, s in BACKBONE])


def variant_cfg(cfg, filters=None, kernel=None, joints=None):
    """A copy of ``cfg`` with other NUM_DECONV_FILTERS / one NUM_DECONV_KERNELS for every layer / NUM_JOINTS."""
    c = cfg.clone()
    c.defrost()
    if filters is not None:
        c.MODEL.EXTRA.NUM_DECONV_FILTERS = [int(f) for f in filters]
    if kernel is not None:
        c.MODEL.EXTRA.NUM_DECONV_KERNELS = [int(kernel)] * int(c.MODEL.EXTRA.NUM_DECONV_LAYERS)
    if joints is not None:
        c.MODEL.NUM_JOINTS = int(joints)
        c.DATASET.NUM_JOINTS = int(joints)
    return c


# name -> (width_mult, NUM_DECONV_FILTERS or None, (H, W)): what the REAL module can express beyond resnet.yaml; its
# samples are tests/golden/golden_resnet_variants.npz (gen_golden_resnet.py), replayed by tests/test_resnet_cpu.py
VARIANTS = OrderedDict([
    ('w0.5', (0.5, None, (96, 160))),
    ('w1.5', (1.5, None, (64, 96))),
    ('f20_12_10', (1.0, [20, 12, 10], (96, 160))),
    ('w0.5_f20_12_10', (0.5, [20, 12, 10], (64, 64))),
])
VARIANT_SEED = 1234
