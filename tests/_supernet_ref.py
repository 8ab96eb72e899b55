"""CPU restatement of the weight-sharing supernet (reference lib/models/pose_supermobilenet.py, layers/super_layers.py,
arch_manager.py) and of its BatchNorm calibration (calibrate_test.py:44-122).  TEST INFRASTRUCTURE, pinned against the
real module by tests/golden/gen_golden_supernet.py.

  * ``state_dict_shapes`` / ``make_state_dict``: the supernet's keys in registration order and a seeded synthetic
    checkpoint (oracle/synth.py's recipe; BatchNorm statistics that are not 0 / 1, ``Linear5x5`` / ``Linear3x3`` that
    are not the identity)
  * ``sub_state_dict``: the slices of super_layers.py as a strict pose_mobilenet state dict.  BatchNorm tensors are
    VIEWS of the supernet's (the reference normalises with ``running_mean[:c]``), so a training-mode forward moves the
    supernet's own statistics; conv weights are views or, for k = 5 / 3, the window transform
  * ``train_forward``: the training-mode forward on such a dict, torch functional, in the dtype of its tensors -- float64
    tensors make it the high-precision reference
  * ``sample_index`` / ``bn_layers``: which channels of which BatchNorm the golden stores
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import net_ref, spec

BN_EPS = 1e-5
INPUT_CHANNEL = 24
SETTING = [[6, 32, 6, 2], [6, 64, 8, 2], [6, 96, 10, 2], [6, 160, 10, 1]]          # t, c, n, s of the supernet
ARCH_SETTING = [[32, 4, 2], [64, 6, 2], [96, 8, 2], [160, 8, 1]]                  # c, n, s of ArchManager
FILTERS = [64, 48, 32]                                                            # mobile.yaml NUM_DECONV_FILTERS


def super_derive(filters=FILTERS, head=None):
    head = head or spec.HeadCfg()
    channel, stages, inp = [INPUT_CHANNEL], [], INPUT_CHANNEL
    for t, c, n, s in SETTING:
        blocks = []
        for b in range(n):
            blocks.append(dict(inp=inp, feat=round(inp * 6), oup=c, stride=s if b == 0 else 1))
            inp = c
        stages.append(blocks)
        channel.append(c)
    deconv, inplanes = [], channel[-1]
    for i in range(3):
        deconv.append(dict(refined_in=inplanes, raw_in=channel[-i - 2], out=filters[i]))
        inplanes = filters[i]
    dim_tag = head.num_joints if head.tag_per_joint else 1
    heads = []
    for i in range(1, 3):
        oup = (head.num_joints if head.with_heatmaps_loss[i - 1] else 0) + (dim_tag if head.with_ae_loss[i - 1] else 0)
        heads.append(dict(refined_in=filters[i], raw_in=channel[-i - 3], oup=oup))
    return dict(channel=channel, stages=stages, deconv=deconv, heads=heads)


def _bn_keys(o, p, c):
    for k in ('weight', 'bias', 'running_mean', 'running_var'):
        o[p + '.' + k] = (c,)
    o[p + '.num_batches_tracked'] = ()


def state_dict_shapes(filters=FILTERS, head=None):
    d = super_derive(filters, head)
    o = OrderedDict()
    o['first.0.0.weight'] = (32, 3, 3, 3)
    _bn_keys(o, 'first.0.1', 32)
    o['first.1.0.weight'] = (32, 1, 3, 3)
    _bn_keys(o, 'first.1.1', 32)
    o['first.2.weight'] = (INPUT_CHANNEL, 32, 1, 1)
    _bn_keys(o, 'first.3', INPUT_CHANNEL)
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            o[p + '.inv.0.weight'] = (blk['feat'], blk['inp'], 1, 1)
            _bn_keys(o, p + '.inv.1', blk['feat'])
            o[p + '.depth_conv.0.weight'] = (blk['feat'], 1, 7, 7)
            _bn_keys(o, p + '.depth_conv.1', blk['feat'])
            o[p + '.point_conv.0.weight'] = (blk['oup'], blk['feat'], 1, 1)
            _bn_keys(o, p + '.point_conv.1', blk['oup'])
            o[p + '.Linear5x5.weight'] = (25, 25)
            o[p + '.Linear5x5.bias'] = (25,)
            o[p + '.Linear3x3.weight'] = (9, 9)
            o[p + '.Linear3x3.bias'] = (9,)
    for which, src in (('deconv_refined', 'refined_in'), ('deconv_raw', 'raw_in')):
        for i, dc in enumerate(d['deconv']):
            o['%s.%d.weight' % (which, i)] = (dc[src], dc['out'], 4, 4)
    for i, dc in enumerate(d['deconv']):
        _bn_keys(o, 'deconv_bnrelu.%d.0' % i, dc['out'])
    for which, src in (('final_refined', 'refined_in'), ('final_raw', 'raw_in')):
        for i, h in enumerate(d['heads']):
            p = '%s.%d.conv' % (which, i)
            o[p + '.0.weight'] = (h[src], 1, 5, 5)
            _bn_keys(o, p + '.1', h[src])
            o[p + '.3.weight'] = (h['oup'], h[src], 1, 1)
    return o


def make_state_dict(seed=1234, filters=FILTERS, head=None):
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for k, shp in state_dict_shapes(filters, head).items():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif '.Linear' in k:
            if k.endswith('.weight'):
                sd[k] = torch.eye(shp[0]) + 0.1 * torch.randn(shp, generator=g)
            else:
                sd[k] = 0.02 * torch.randn(shp, generator=g)
        elif k.endswith('running_var') or (k.endswith('.weight') and len(shp) == 1):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k.endswith('running_mean') or k.endswith('.bias'):
            sd[k] = torch.randn(shp, generator=g) * 0.1
        else:
            fan_in = shp[0] * 4 if k.startswith('deconv') else shp[1] * shp[2] * shp[3]
            std = math.sqrt(2.0 / fan_in)
            if '.point_conv.' in k:
                std *= 0.35
            elif k.startswith('deconv'):
                std *= 0.5
            elif k.endswith('conv.3.weight'):
                std *= 0.05
            sd[k] = torch.randn(shp, generator=g) * std
    return sd


# ------------------------------------------------------------------ architectures (arch_manager.py)
def fixed_sample(reso=256, ratio=0.5, filters=FILTERS):
    md = spec.make_divisible
    return {'img_size': reso, 'input_channel': md(INPUT_CHANNEL * ratio, 8),
            'deconv_setting': [md(f * ratio, 8) for f in filters],
            'backbone_setting': [{'num_blocks': n, 'stride': s, 'channel': md(c * ratio, 8),
                                  'block_setting': [[6, 7] for _ in range(n)]} for c, n, s in ARCH_SETTING]}


def mixed_arch():
    """Mixed channel ratios, fewer blocks, and 5x5 / 3x3 blocks (the reference forward honours any block_setting)."""
    ks = [7, 5, 3]
    chans, blocks = [24, 32, 72, 120], [3, 5, 6, 7]
    bs = []
    for i, (c, n) in enumerate(zip(chans, blocks)):
        bs.append({'num_blocks': n, 'stride': ARCH_SETTING[i][2], 'channel': c,
                   'block_setting': [[6 if (i + j) % 3 else 4, ks[(i + j) % 3]] for j in range(n)]})
    return {'img_size': 256, 'input_channel': 16, 'deconv_setting': [48, 24, 32], 'backbone_setting': bs}


def golden_archs():
    """(name, cfg_arch) in fixture order: the order is part of the fixture (view semantics)."""
    return [('half', fixed_sample(ratio=0.5)), ('full', fixed_sample(ratio=1.0)), ('mixed', mixed_arch())]


# ------------------------------------------------------------------ slicing (super_layers.py)
def _bn_slice(out, sd, p, c):
    for k in ('weight', 'bias', 'running_mean', 'running_var'):
        out[p + '.' + k] = sd[p + '.' + k][:c]
    out[p + '.num_batches_tracked'] = sd[p + '.num_batches_tracked']


def window(sd, p, mid, k):
    """The depthwise filter of block ``p`` for kernel size k: centre crop, then Linear5x5 / Linear3x3 on the flat window."""
    l, r = 3 - k // 2, 3 + k // 2 + 1
    w = sd[p + '.depth_conv.0.weight'][:mid, :, l:r, l:r]
    if k == 5:
        w = F.linear(w.reshape(mid, 1, -1), sd[p + '.Linear5x5.weight'], sd[p + '.Linear5x5.bias']).reshape(mid, 1, 5, 5)
    elif k == 3:
        w = F.linear(w.reshape(mid, 1, -1), sd[p + '.Linear3x3.weight'], sd[p + '.Linear3x3.bias']).reshape(mid, 1, 3, 3)
    return w


def sub_state_dict(sd, arch):
    d = spec.derive(arch)
    out = OrderedDict()
    out['first.0.0.weight'] = sd['first.0.0.weight']
    _bn_slice(out, sd, 'first.0.1', 32)
    out['first.1.0.weight'] = sd['first.1.0.weight']
    _bn_slice(out, sd, 'first.1.1', 32)
    out['first.2.weight'] = sd['first.2.weight'][:d['c0'], :32]
    _bn_slice(out, sd, 'first.3', d['c0'])
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            t, k = arch['backbone_setting'][s]['block_setting'][b]
            mid = round(blk['inp'] * t)
            assert mid == blk['feat'], 'round(in * t) must be what pose_mobilenet builds'
            out[p + '.inv.0.weight'] = sd[p + '.inv.0.weight'][:mid, :blk['inp']]
            _bn_slice(out, sd, p + '.inv.1', mid)
            out[p + '.depth_conv.0.weight'] = window(sd, p, mid, k)
            _bn_slice(out, sd, p + '.depth_conv.1', mid)
            out[p + '.point_conv.0.weight'] = sd[p + '.point_conv.0.weight'][:blk['oup'], :mid]
            _bn_slice(out, sd, p + '.point_conv.1', blk['oup'])
    for which, src in (('deconv_refined', 'refined_in'), ('deconv_raw', 'raw_in')):
        for i, dc in enumerate(d['deconv']):
            out['%s.%d.weight' % (which, i)] = sd['%s.%d.weight' % (which, i)][:dc[src], :dc['out']]
    for i, dc in enumerate(d['deconv']):
        _bn_slice(out, sd, 'deconv_bnrelu.%d.0' % i, dc['out'])
    for which, src in (('final_refined', 'refined_in'), ('final_raw', 'raw_in')):
        for i, h in enumerate(d['heads']):
            p = '%s.%d.conv' % (which, i)
            out[p + '.0.weight'] = sd[p + '.0.weight'][:h[src]]
            _bn_slice(out, sd, p + '.1', h[src])
            out[p + '.3.weight'] = sd[p + '.3.weight'][:h['oup'], :h[src]]
    assert list(out) == list(spec.state_dict_shapes(arch)), 'sub-network key order'
    return out


def to_double(sd):
    return OrderedDict((k, v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items())


# ------------------------------------------------------------------ training-mode forward
def bn_layers(arch):
    """Every BatchNorm of the sub-network in forward order: (state_dict prefix, channels)."""
    d = spec.derive(arch)
    L = [('first.0.1', 32), ('first.1.1', 32), ('first.3', d['c0'])]
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            L += [(p + '.inv.1', blk['feat']), (p + '.depth_conv.1', blk['feat']), (p + '.point_conv.1', blk['oup'])]
    for i, dc in enumerate(d['deconv']):
        L.append(('deconv_bnrelu.%d.0' % i, dc['out']))
        if i > 0:
            L.append(('final_refined.%d.conv.1' % (i - 1), d['heads'][i - 1]['refined_in']))
            L.append(('final_raw.%d.conv.1' % (i - 1), d['heads'][i - 1]['raw_in']))
    return L


def _tbn(x, sd, p, momentum):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'],
                        True, momentum, BN_EPS)


def train_forward(x, sd, arch, momentum=0.1):
    """One calibration step: the forward of pose_supermobilenet.py:133-165 in training mode on the sliced dict ``sd``;
    ``running_mean`` / ``running_var`` of ``sd`` move in place (through to the supernet when they are views)."""
    d = spec.derive(arch)
    relu6 = lambda t: torch.clamp(t, 0.0, 6.0)  # noqa: E731
    x = relu6(_tbn(F.conv2d(x, sd['first.0.0.weight'], None, 2, 1), sd, 'first.0.1', momentum))
    x = relu6(_tbn(F.conv2d(x, sd['first.1.0.weight'], None, 1, 1, 1, 32), sd, 'first.1.1', momentum))
    x = _tbn(F.conv2d(x, sd['first.2.weight']), sd, 'first.3', momentum)
    x_list = [x]
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            o = relu6(_tbn(F.conv2d(x, sd[p + '.inv.0.weight']), sd, p + '.inv.1', momentum))
            o = relu6(_tbn(F.conv2d(o, sd[p + '.depth_conv.0.weight'], None, blk['stride'], blk['k'] // 2, 1,
                                    blk['feat']), sd, p + '.depth_conv.1', momentum))
            o = _tbn(F.conv2d(o, sd[p + '.point_conv.0.weight']), sd, p + '.point_conv.1', momentum)
            x = o + x if blk['residual'] else o
        x_list.append(x)
    outs = []
    refined, raw = x_list[-1], x_list[-2]
    for i in range(len(d['deconv'])):
        r = F.conv_transpose2d(refined, sd['deconv_refined.%d.weight' % i], None, 2, 1)
        w = F.conv_transpose2d(raw, sd['deconv_raw.%d.weight' % i], None, 2, 1)
        refined = F.relu(_tbn(r + w, sd, 'deconv_bnrelu.%d.0' % i, momentum))
        raw = x_list[-i - 3]
        if i > 0:
            fo = []
            for which, src in (('final_refined', refined), ('final_raw', raw)):
                p = '%s.%d.conv' % (which, i - 1)
                t = F.relu(_tbn(F.conv2d(src, sd[p + '.0.weight'], None, 1, 2, 1, src.shape[1]), sd, p + '.1', momentum))
                fo.append(F.conv2d(t, sd[p + '.3.weight']))
            outs.append(fo[0] + fo[1])
    return outs


def eval_forward(x, sd, arch):
    """Eval-mode outputs of the sub-network: the oracle network on the sliced dict."""
    return net_ref.forward(x, sd, arch)


# ------------------------------------------------------------------ what the golden stores
def sample_index(c, cap=32):
    """Channels of a BatchNorm whose running pair the golden stores: all up to ``cap``, else ``cap`` evenly spread ones
    (first and last included); the golden also stores the fp64 sum over ALL channels."""
    if c <= cap:
        return np.arange(c)
    return np.unique(np.round(np.linspace(0, c - 1, cap)).astype(np.int64))


def pairs_of(sd, arch):
    """{prefix: (running_mean, running_var)} as float64 numpy copies, for every BatchNorm."""
    return OrderedDict((p, (sd[p + '.running_mean'].detach().double().numpy().copy(),
                            sd[p + '.running_var'].detach().double().numpy().copy())) for p, _ in bn_layers(arch))


def pack_pairs(pairs, arch):
    """The stored form of ``pairs_of``: sampled values [2][sum of samples] and whole-layer sums [2][layers]."""
    vals, sums = [[], []], [[], []]
    for p, c in bn_layers(arch):
        idx = sample_index(c)
        for q in range(2):
            vals[q].append(pairs[p][q][idx])
            sums[q].append(pairs[p][q].sum())
    return np.stack([np.concatenate(v) for v in vals]), np.array(sums)


CASES = [(64, 64), (96, 160)]          # H, W; N = 4, three steps each
N_IMAGES, STEPS, SEED = 4, 3, 1234


def step_images(H, W, arch_i, step):
    from oracle import synth
    return synth.make_images(N_IMAGES, H, seed=100 + 10 * arch_i + step, w=W)
