"""Helpers of the supernet-training tests (tests/test_supertrain_cpu.py, tests/test_gpu_supertrain.py) and of their
fixture generator tests/golden/gen_golden_supertrain.py, which drives the REAL reference (pose_supermobilenet.SuperLitePose,
core/trainer.do_train, arch_manager.ArchManager) and writes tests/golden/golden_supertrain.npz.  TEST INFRASTRUCTURE.

  * ``slices(arch)``: for every parameter of the supernet the index of the part the sub-network ``arch`` touches (None:
    untouched, its gradient stays None)
  * ``sample(key, arch)``: the flat indices, inside that part, of the gradient elements the golden stores
  * ``kind_of``: the layer kinds the 4-times rule of tests/test_gpu_train_net.py pools by, plus ``linear``
  * ``resize_ref``: trainer.py:49-59 restated in torch, asserted against the real ``do_train`` while generating
  * ``make_batch``: the seeded batch of the resize fixture
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import _supernet_ref as sr
from oracle import spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_supertrain.npz')
N, RES, SEED_SAMPLE, SAMPLES, STRIDE = 2, 64, 7, 32, 13
FRACTIONS = [(4, 8), (5, 8), (6, 8), (7, 8), (8, 8)]          # the five training sizes as fractions of the input size


def step_archs(golden):
    """The two architectures of the training-step fixture: the random-width one (every block k = 7) that the reference's
    ArchManager.random_sample() drew for the golden, and the mixed one with k in {3, 5, 7}."""
    return [('random', json.loads(str(golden['arch_random']))), ('mixed', sr.mixed_arch())]


def slices(arch):
    """{parameter key: index tuple of the touched part, or None} over every parameter of the supernet."""
    shapes = sr.state_dict_shapes()
    d = spec.derive(arch)
    out = OrderedDict((k, None) for k in shapes if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked')))

    def bn(p, c):
        out[p + '.weight'] = out[p + '.bias'] = (slice(0, c),)

    full = (slice(None),)
    out['first.0.0.weight'] = out['first.1.0.weight'] = full
    bn('first.0.1', 32)
    bn('first.1.1', 32)
    out['first.2.weight'] = (slice(0, d['c0']), slice(0, 32))
    bn('first.3', d['c0'])
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            t, k = arch['backbone_setting'][s]['block_setting'][b]
            mid = round(blk['inp'] * t)
            out[p + '.inv.0.weight'] = (slice(0, mid), slice(0, blk['inp']))
            bn(p + '.inv.1', mid)
            l, r = 3 - k // 2, 3 + k // 2 + 1
            out[p + '.depth_conv.0.weight'] = (slice(0, mid), slice(None), slice(l, r), slice(l, r))
            bn(p + '.depth_conv.1', mid)
            out[p + '.point_conv.0.weight'] = (slice(0, blk['oup']), slice(0, mid))
            bn(p + '.point_conv.1', blk['oup'])
            if k != 7:
                out[p + '.Linear%dx%d.weight' % (k, k)] = out[p + '.Linear%dx%d.bias' % (k, k)] = full
    for which, src in (('deconv_refined', 'refined_in'), ('deconv_raw', 'raw_in')):
        for i, dc in enumerate(d['deconv']):
            out['%s.%d.weight' % (which, i)] = (slice(0, dc[src]), slice(0, dc['out']))
    for i, dc in enumerate(d['deconv']):
        bn('deconv_bnrelu.%d.0' % i, dc['out'])
    for which, src in (('final_refined', 'refined_in'), ('final_raw', 'raw_in')):
        for i, h in enumerate(d['heads']):
            p = '%s.%d.conv' % (which, i)
            out[p + '.0.weight'] = (slice(0, h[src]),)
            bn(p + '.1', h[src])
            out[p + '.3.weight'] = (slice(0, h['oup']), slice(0, h[src]))
    return out


def inside_mask(shape, index):
    m = np.zeros(shape, bool)
    m[index] = True
    return m


def sample(shape, index):
    """Flat indices (into the full tensor) of the stored gradient elements: up to SAMPLES evenly spread over the touched
    part, first and last included."""
    flat = np.flatnonzero(inside_mask(shape, index).reshape(-1))
    if flat.size <= SAMPLES:
        return flat
    return flat[np.unique(np.round(np.linspace(0, flat.size - 1, SAMPLES)).astype(np.int64))]


def kind_of(key, shape):
    if '.Linear' in key:
        return 'linear'
    if key == 'first.0.0.weight':
        return 'stem'
    if key.startswith('deconv_r'):
        return 'deconv'
    if len(shape) == 1:
        return 'gamma' if key.endswith('weight') else 'beta'
    return 'dw' if shape[1] == 1 and shape[2] > 1 else 'pw'


def grid(a, bits):
    return (np.round(np.asarray(a) * (1 << bits)) / (1 << bits)).astype(np.float32)


def step_inputs(heads):
    """x [N,3,RES,RES] and the upstream gradients of the two outputs, on a 2^-6 grid."""
    rng = np.random.RandomState(20250311)
    x = grid(rng.standard_normal((N, 3, RES, RES)), 6)
    ups = [grid(rng.standard_normal((N, c, RES // 4 << s, RES // 4 << s)), 6) for s, c in enumerate(heads)]
    return x, ups


# ------------------------------------------------------------------ trainer.py:49-59
def nearest_index(out, inn):
    """The integer rule of lp_train_resize: source cell of every output cell of a line."""
    return np.minimum(np.arange(out) * inn // out, inn - 1)


def remap_joint(j, size, base):
    """Element 0 of a joint under the resize, in integers (j >= 0)."""
    j = np.asarray(j, np.int64)
    return (j // base * size // base) * size + (j % base) * size // base


def resize_ref(images, heatmaps, masks, joints, size, base):
    """Lines 49-59 in torch, ``base`` in place of the hard-coded 512; joints as int64 tensors, new tensors returned."""
    oup = size // 4
    images = F.interpolate(images, size=(size, size))
    heatmaps, masks, joints = list(heatmaps), list(masks), [j.clone() for j in joints]
    for cnt in range(len(heatmaps)):
        heatmaps[cnt] = F.interpolate(heatmaps[cnt], size=(oup, oup))
        masks[cnt] = F.interpolate(masks[cnt].unsqueeze(1), size=(oup, oup)).squeeze(1)
        x = torch.trunc((joints[cnt][:, :, :, 0] % base * size) / base)
        y = torch.trunc((joints[cnt][:, :, :, 0] // base * size) / base)
        joints[cnt][:, :, :, 0] = y * size + x
        oup *= 2
    return images, heatmaps, masks, joints


def make_batch(base, n=2, J=3, M=2, seed=5):
    """A seeded batch: images [n,3,base,base], heatmaps [n,J,R,R], masks [n,R,R] (fp32, 2^-6 grid), joints int64 [n,M,J,2]
    with element 0 a flat cell index of the stage's plane and element 1 a 0/1 flag."""
    rng = np.random.RandomState(seed)
    images = torch.from_numpy(grid(rng.standard_normal((n, 3, base, base)), 6))
    heatmaps, masks, joints = [], [], []
    for s in range(2):
        R = base // 4 << s
        heatmaps.append(torch.from_numpy(grid(rng.uniform(0, 1, (n, J, R, R)), 6)))
        masks.append(torch.from_numpy((rng.uniform(0, 1, (n, R, R)) > 0.3).astype(np.float32)))
        j = np.zeros((n, M, J, 2), np.int64)
        j[..., 0] = rng.randint(0, R * R, (n, M, J))
        j[..., 1] = rng.randint(0, 2, (n, M, J))
        j[0, 0, 0, 0], j[0, 0, 1, 0] = R * R - 1, 0
        joints.append(torch.from_numpy(j))
    return images, heatmaps, masks, joints


def load():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}
