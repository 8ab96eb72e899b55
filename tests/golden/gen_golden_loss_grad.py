#!/usr/bin/env python
"""Golden fixture of the gradient of the training loss (tests/golden/golden_loss_grad.npz).  Build container only (needs
the reference checkout).  Runs autograd through the REAL lib/core/loss.py (MultiLossFactory, both AE_LOSS_TYPEs) on the CPU.

Data only.  The inputs are those of tests/golden/golden_targets.npz (N = 4 images with 0, 1, 2 and 4 persons, R = 16 / 32,
both loss configurations) plus ONE image stored here: seeded normal outputs, the heatmaps of image 3, the mask of image 1
(the zero block) and the joints of image 3 with the first slot of one person moved onto the first cell of another
(x_shared_R names the two), so that two persons share a cell of one joint.  Per image an upstream weight per term (w_heat, w_push, w_pull, float32 [5]; all differ, each has
one zero).  Stored per configuration c, stage s and loss type:

  gheat{c}_{s}_ref / _f64      [5,J,R,R]  d(sum_n w_heat[n] * heat_loss[n]) / d out[:, :J]: autograd (fp32) and
                                          tests/_loss_grad_ref.heat_grad (fp64); the same for 'exp' and 'max', asserted
  gtag{c}_{lt}_{s}_ref / _f64  [5,K,R,R]  d(w_push[n] * push_n + w_pull[n] * pull_n) / d out[n, off:], one image per call of
                                          the real factory (a batch of one: its mean is the image's term)

Asserted here: every push pair's |mu_p - mu_q| lies at least 1e-3 from 0 and from 1 (the kinks of 'max'), the gradient
outside the two terms is exactly zero, and the shared cell is really shared."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _loss_grad_case as GC  # noqa: E402
import _loss_grad_ref as GR  # noqa: E402
from gen_golden_targets import FACTORS, LOSS_CFGS, _load, REF  # noqa: E402

W_HEAT = np.array([0.75, 1.5, 0.0, 0.3125, 1.25], np.float32)
W_PUSH = np.array([1.0, 0.0, 2.5, 0.625, 1.75], np.float32)
W_PULL = np.array([0.5, 1.25, 0.875, 0.0, 2.0], np.float32)


def extra_image(t):
    rng = np.random.RandomState(11)
    J = int(t['J'])
    x = dict(x_out_16=rng.standard_normal((2 * J, 16, 16)).astype(np.float32),
             x_out_32=rng.standard_normal((J, 32, 32)).astype(np.float32),
             x_out_32_tags=rng.standard_normal((2 * J, 32, 32)).astype(np.float32), x_heat_from=3, x_mask_from=1)
    for R in GC.OUTS:
        jt = t['jt_%d' % R][3].copy()
        a, b = [p for p in range(jt.shape[0]) if jt[p, 0, 1] == 1][:2]     # the first two persons with a visible joint
        assert jt[a, 0, 0] != jt[b, 0, 0]
        jt[b, 0, 0] = jt[a, 0, 0]                      # b's first visible joint lands on a's cell
        x['x_jt_%d' % R], x['x_shared_%d' % R] = jt, np.array([a, b])
    return x


def main():
    L = _load('ref_core_loss', os.path.join(REF, 'lib/core/loss.py'))
    with np.load(GC.TARGETS) as z:
        t = {k: z[k] for k in z.files}
    out = extra_image(t)
    b = GC.extend(t, out)
    J, M = b['J'], b['M']
    out.update(w_heat=W_HEAT, w_push=W_PUSH, w_pull=W_PULL)
    NS = types.SimpleNamespace
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    for c, lc in enumerate(LOSS_CFGS):
        assert lc == dict(WITH_HEATMAPS_LOSS=GC.CFGS[c]['heat'], WITH_AE_LOSS=GC.CFGS[c]['ae'])
        heat_seen = {}
        for lt in ('exp', 'max'):
            cfg = NS(MODEL=NS(NUM_JOINTS=J), DATASET=NS(MAX_NUM_PEOPLE=M, OUTPUT_SIZE=list(GC.OUTS)),
                     LOSS=NS(NUM_STAGES=2, AE_LOSS_TYPE=lt, **dict(FACTORS, **lc)))
            fac = L.MultiLossFactory(cfg)
            stages = [GC.stage(b, c, s) for s in range(2)]
            grads = [np.zeros(st[0].shape, np.float32) for st in stages]
            for n in range(GC.N):
                outs = [tt(st[0][n:n + 1]).requires_grad_() for st in stages]
                hl, pu, pl = fac(outs, [tt(b['heat_%d' % R][n:n + 1]) for R in GC.OUTS],
                                 [tt(b['mask_t_%d' % R][n:n + 1]) for R in GC.OUTS],
                                 [tt(b['jt_%d' % R][n:n + 1]).long() for R in GC.OUTS])
                loss = 0
                for s in range(2):
                    if hl[s] is not None:
                        loss = loss + float(W_HEAT[n]) * hl[s][0]
                    if pu[s] is not None:
                        loss = loss + float(W_PUSH[n]) * pu[s] + float(W_PULL[n]) * pl[s]
                loss.backward()
                for s in range(2):
                    grads[s][n] = outs[s].grad.numpy()[0]
            for s, (o, _, off, heat, mask, jts) in enumerate(stages):
                hi = J if heat is not None else 0
                assert not grads[s][:, hi:(off if off >= 0 else None)].any()       # outside both terms
                if heat is not None:
                    f64 = np.stack([GR.heat_grad(o[n, :J], heat[n], mask[n], FACTORS['HEATMAPS_LOSS_FACTOR'][s], W_HEAT[n])
                                    for n in range(GC.N)])
                    ref = grads[s][:, :J].copy()
                    if (c, s) in heat_seen:
                        assert np.array_equal(heat_seen[c, s], ref)
                    heat_seen[c, s] = ref
                    out['gheat%d_%d_ref' % (c, s)], out['gheat%d_%d_f64' % (c, s)] = ref, f64
                if off >= 0:
                    for n in range(GC.N):
                        for gap in GR.push_gaps(o[n, off:], jts[n]):
                            assert gap >= 1e-3 and abs(gap - 1.0) >= 1e-3, (c, s, n, gap)
                    f64 = np.stack([GR.tag_grad(o[n, off:], jts[n], lt, FACTORS['PUSH_LOSS_FACTOR'][s],
                                                FACTORS['PULL_LOSS_FACTOR'][s], W_PUSH[n], W_PULL[n]) for n in range(GC.N)])
                    out['gtag%d_%s_%d_ref' % (c, lt, s)], out['gtag%d_%s_%d_f64' % (c, lt, s)] = grads[s][:, off:].copy(), f64
                    pa, pb = out['x_shared_%d' % GC.OUTS[s]]
                    shared = int(jts[4][pa, 0, 0])
                    assert int(jts[4][pb, 0, 0]) == shared and f64[4].reshape(-1)[shared] != 0
    path = GC.GOLDEN
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print('wrote %s (%d bytes)' % (path, size))


if __name__ == '__main__':
    main()
