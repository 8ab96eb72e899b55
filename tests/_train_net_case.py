"""The case of tests/golden/golden_train_net.npz, shared by its generator and the tests that read it: a tiny LitePose
(four stages, kernels 3 / 5 / 7, expansions 1 / 2 / 3, one stride-1 stage with a residual entry block, 8- and 16-channel
stages and 24- / 48-channel expansions, three deconvs, heads of 28 and 14 channels), N = 2 images of 64 x 64, one step
of the reference module in train() mode in fp32 and in fp64.

The file packs per-key tensors into flat vectors in ``state_dict`` order (an .npz entry per tensor would cost more than
the tensors): ``split`` cuts them again."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_train_net.npz')

N, RES, J = 2, 64, 14
ARCH = {
    'img_size': RES, 'input_channel': 8, 'deconv_setting': [8, 8, 8],
    'backbone_setting': [
        {'num_blocks': 2, 'stride': 2, 'channel': 8, 'block_setting': [[2, 3], [3, 5]]},
        {'num_blocks': 2, 'stride': 2, 'channel': 16, 'block_setting': [[3, 7], [2, 3]]},
        {'num_blocks': 1, 'stride': 2, 'channel': 16, 'block_setting': [[2, 5]]},
        {'num_blocks': 2, 'stride': 1, 'channel': 16, 'block_setting': [[1, 7], [3, 3]]},
    ],
}
HEADS = (28, 14)
OUT_RES = (16, 32)


def kind(key):
    """The layer kind of a parameter: the pools of the whole-module comparison."""
    if key.startswith('first.0.0.'):
        return 'stem'
    if key.startswith(('deconv_refined.', 'deconv_raw.')):
        return 'deconv'
    if key.endswith('.bias'):
        return 'beta'
    return None                      # a weight: gamma, 1x1 or depthwise by its shape (kind_of)


def kind_of(key, shape):
    k = kind(key)
    if k is not None:
        return k
    if len(shape) == 1:
        return 'gamma'
    return 'pw' if shape[2] == 1 else 'dw'


def split(flat, keys, shapes):
    out, o = {}, 0
    for k, s in zip(keys, shapes):
        n = int(np.prod(s)) if len(s) else 1
        out[k] = flat[o:o + n].reshape(s)
        o += n
    assert o == flat.size, (o, flat.size)
    return out


def load():
    """-> dict: x, up0, up1, sd (key -> fp32), params / buffers (key lists), out{s}_32 / _64, grad_32 / grad_64 (key ->),
    run_32 / run_64 (running_mean / running_var keys -> after the step)."""
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    keys = [str(k) for k in g['keys']]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(g['shapes'], g['ndims'])]
    shp = dict(zip(keys, shapes))
    c = dict(x=g['x'], up0=g['up0'], up1=g['up1'], keys=keys, shapes=shp)
    sd = split(g['sd'], [k for k in keys if not k.endswith('num_batches_tracked')],
               [shp[k] for k in keys if not k.endswith('num_batches_tracked')])
    c['sd'] = sd
    c['params'] = [k for k in sd if not k.endswith(('running_mean', 'running_var'))]
    c['buffers'] = [k for k in sd if k.endswith(('running_mean', 'running_var'))]
    for tag in ('32', '64'):
        c['grad_' + tag] = split(g['grad_' + tag], c['params'], [shp[k] for k in c['params']])
        c['run_' + tag] = split(g['run_' + tag], c['buffers'], [shp[k] for k in c['buffers']])
        for s in range(2):
            c['out%d_%s' % (s, tag)] = g['out%d_%s' % (s, tag)]
    return c
