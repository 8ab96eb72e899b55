"""The batch of the loss-gradient tests: the four images of tests/golden/golden_targets.npz plus the one image that
tests/golden/golden_loss_grad.npz adds (two persons share a cell of one joint), as numpy arrays.  A plain module
(tests/ is on sys.path under pytest); numpy only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TARGETS = os.path.join(HERE, 'golden', 'golden_targets.npz')
GOLDEN = os.path.join(HERE, 'golden', 'golden_loss_grad.npz')
CFGS = [dict(heat=(True, True), ae=(True, False)), dict(heat=(False, True), ae=(True, True))]
FACTORS = (1.0, 0.001, 0.001)                  # heat, push, pull: the factors of the fixture, on both stages
OUTS = (16, 32)
N = 5


def extend(t, extra):
    """The inputs of golden_targets.npz (dict ``t``) with the extra image (dict ``extra``: x_out_16, x_out_32, x_out_32_tags,
    x_jt_16, x_jt_32, x_heat_from, x_mask_from) appended -> dict of [5, ...] arrays under the names of golden_targets."""
    b = {}
    for k in ('out_16', 'out_32', 'out_32_tags', 'jt_16', 'jt_32'):
        b[k] = np.concatenate([t[k], extra['x_' + k][None]])
    for R in OUTS:
        h, m = int(extra['x_heat_from']), int(extra['x_mask_from'])
        b['heat_%d' % R] = np.concatenate([t['heat_%d' % R], t['heat_%d' % R][h:h + 1]])
        b['mask_t_%d' % R] = np.concatenate([t['mask_t_%d' % R], t['mask_t_%d' % R][m:m + 1]])
    b['J'], b['M'] = int(t['J']), int(t['M'])
    return b


def load():
    """-> (batch, golden): the five-image inputs and the stored gradients and upstream weights."""
    with np.load(TARGETS) as z:
        t = {k: z[k] for k in z.files}
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    return extend(t, g), g


def stage(b, c, s):
    """(out, J, tag_offset, heat or None, mask, joints) of stage s under loss configuration c, numpy."""
    R = OUTS[s]
    out = b['out_16'] if s == 0 else (b['out_32'] if c == 0 else b['out_32_tags'])
    J = b['J']
    heat = b['heat_%d' % R] if CFGS[c]['heat'][s] else None
    off = (J if CFGS[c]['heat'][s] else 0) if CFGS[c]['ae'][s] else -1
    return out, J, off, heat, b['mask_t_%d' % R], b['jt_%d' % R]
