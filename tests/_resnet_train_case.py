"""The case of tests/golden/golden_resnet_train*.npz, shared by its generator and the tests that read it: one training step
of the reference's pose_resnet LitePose at ``width_mult = 0.25`` (channels 8 / 8 / 16 / 24, about 0.55 M parameters) with
the settings of tests/golden/resnet.yaml, N = 2 images of 64 x 64, in train() mode in fp32 and in fp64.

The weights are not stored: ``state()`` recomputes ``_resnet_ref.make_state_dict(cfg, SEED, table=width_table(0.25))``.
Per-key tensors are packed into flat vectors in ``state_dict`` order; ``load`` cuts them again.  The fp64 gradients are
stored rounded to fp32 (GRAD_STORED_F32: an elementwise rounding moves a tensor by at most 2^-24 of itself in the 2-norm,
which the comparisons add to a gradient's allowed relative error) and split over three files, so that each stays under the
repository's limit for a committed file; ``e32`` -- the relative error of the reference's own fp32 gradient per parameter --
was computed at generation against the unrounded fp64."""
import os

import numpy as np
import torch

import _resnet_ref as rr
from _train_net_case import split

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = os.path.join(GOLDEN_DIR, 'golden_resnet_train.npz')
GOLDEN_GRADS = [os.path.join(GOLDEN_DIR, 'golden_resnet_train_g%d.npz' % i) for i in range(3)]
YAML = os.path.join(GOLDEN_DIR, 'resnet.yaml')

N, RES, WIDTH, SEED = 2, 64, 0.25, 4321
HEADS = (28, 14)
OUT_RES = (16, 32)
GRAD_STORED_F32 = True
GRAD_ROUNDING = 2.0 ** -24 if GRAD_STORED_F32 else 0.0
KINDS = ('beta', 'conv_bias', 'dense', 'gamma', 'out_conv', 'pw')


def cfg():
    from litepose_amd import config
    return config.update_config(config.get_cfg('crowd_pose'), YAML)


def table():
    return rr.width_table(WIDTH)


def state(c=None):
    """the state dict BEFORE the step (fp32 tensors, num_batches_tracked zero)"""
    return rr.make_state_dict(c or cfg(), SEED, table=table())


def kind_of(key, shape):
    """The layer kind of a parameter: the pools of the whole-module comparison."""
    if key.startswith(('final_refined.', 'final_raw.')):
        return 'conv_bias' if key.endswith('.bias') else 'out_conv'
    if len(shape) == 1:
        return 'gamma' if key.endswith('.weight') else 'beta'
    return 'pw' if shape[2] == 1 else 'dense'


def load():
    """-> dict: x, up0, up1, params / buffers (key lists), shapes, out{s}_32 / _64, grad_64 (key -> fp32-rounded fp64
    gradient), e32 (key -> the reference's own fp32 relative error), run_32 / run_64 (running pairs after the step)."""
    g = {}
    for path in [GOLDEN] + GOLDEN_GRADS:
        with np.load(path) as z:
            g.update({k: z[k] for k in z.files})
    shp = rr.state_dict_shapes(cfg(), table())
    keys = list(shp)
    c = dict(x=g['x'], up0=g['up0'], up1=g['up1'], keys=keys, shapes=shp)
    c['buffers'] = [k for k in keys if k.endswith(('running_mean', 'running_var'))]
    c['params'] = [k for k in keys if k not in c['buffers'] and not k.endswith('num_batches_tracked')]
    assert [str(k) for k in g['params']] == c['params']
    flat = np.concatenate([g['grad_64_part%d' % i] for i in range(len(GOLDEN_GRADS))])
    c['grad_64'] = split(flat, c['params'], [shp[k] for k in c['params']])
    c['e32'] = dict(zip(c['params'], (float(v) for v in g['e32'])))
    for tag in ('32', '64'):
        c['run_' + tag] = split(g['run_' + tag], c['buffers'], [shp[k] for k in c['buffers']])
        for s in range(2):
            c['out%d_%s' % (s, tag)] = g['out%d_%s' % (s, tag)]
    return c


def tensors(d, dtype=torch.float32):
    return {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
