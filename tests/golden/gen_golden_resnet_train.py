#!/usr/bin/env python
"""Golden fixture of one training step of pose_resnet (tests/golden/golden_resnet_train.npz + golden_resnet_train_g{0,1,2}.npz).
Build container only (needs the reference checkout, like gen_golden_resnet.py).  Runs the REAL
lib/models/pose_resnet.LitePose(cfg, width_mult=0.25) on the CPU in train() mode with the settings of
tests/golden/resnet.yaml: forward on N = 2 images of 64 x 64, backward of sum_s (out_s * up_s).sum() with fixed upstream
gradients, once in fp32 and once more with the same module in fp64 (.double(), the same widened values).

Data only (tests/_resnet_train_case.py reads it).  The weights are NOT stored: they are
``_resnet_ref.make_state_dict(cfg, SEED, table=width_table(0.25))``, which the tests recompute.

  x [2,3,64,64], up0 [2,28,16,16], up1 [2,14,32,32]   fp32, on a 2^-6 grid (they compress)
  params                                              the parameter names, in state_dict order
  out{s}_32 / out{s}_64                               the stage outputs
  run_32 / run_64                                     running_mean / running_var AFTER the step, flat, in state_dict order
  e32                                                 per parameter |g32 - g64|_2 / |g64|_2 of the reference's own fp32
                                                      gradient, against the unrounded fp64
  grad_64_part{0,1,2}                                  every parameter's fp64 gradient ROUNDED TO fp32, flat, in state_dict
                                                      order, cut in three files: 0.55 M values do not fit one committed file

Asserted here: the module's keys and shapes are _resnet_ref.state_dict_shapes', every parameter has a gradient that is not
all zeros, every running tensor moved."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402  (puts the repo root on sys.path, loads oracle.*)
import _resnet_ref as rr  # noqa: E402
import _resnet_train_case as RC  # noqa: E402


def grid(a, bits):
    return (np.round(a * (1 << bits)) / (1 << bits)).astype(np.float32)


def step(model, sd, x, ups, dtype):
    model.load_state_dict(sd, strict=True)
    model.to(dtype).train()
    model.zero_grad()
    outs = model(torch.from_numpy(x).to(dtype))
    loss = sum((o * torch.from_numpy(u).to(dtype)).sum() for o, u in zip(outs, ups))
    loss.backward()
    grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
    run = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()
           if k.endswith(('running_mean', 'running_var'))}
    return [o.detach().numpy().copy() for o in outs], grads, run


def main():
    torch.set_num_threads(1)
    gg.load_reference()
    pr = gg._load('ref_pose_resnet', os.path.join(gg.REF, 'lib/models/pose_resnet.py'))
    cfg = RC.cfg()
    torch.manual_seed(0)
    model = pr.LitePose(cfg, width_mult=RC.WIDTH)
    shapes = rr.state_dict_shapes(cfg, RC.table())
    msd = model.state_dict()
    assert list(msd.keys()) == list(shapes.keys()), 'state_dict key scheme/order mismatch'
    assert all(tuple(msd[k].shape) == v for k, v in shapes.items())
    sd = RC.state(cfg)
    rng = np.random.RandomState(20241021)
    x = grid(rng.standard_normal((RC.N, 3, RC.RES, RC.RES)), 6)
    ups = [grid(rng.standard_normal((RC.N, c, r, r)), 6) for c, r in zip(RC.HEADS, RC.OUT_RES)]
    params = [k for k, _ in model.named_parameters()]
    buffers = [k for k in shapes if k.endswith(('running_mean', 'running_var'))]
    assert params == [k for k in shapes if k not in buffers and not k.endswith('num_batches_tracked')]
    out = dict(x=x, up0=ups[0], up1=ups[1], params=np.array(params))
    res = {}
    for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
        outs, grads, run = step(model, sd, x, ups, dtype)
        for s, o in enumerate(outs):
            assert o.shape == (RC.N, RC.HEADS[s], RC.OUT_RES[s], RC.OUT_RES[s])
            out['out%d_%s' % (s, tag)] = o
        for k in params:
            assert grads[k].any(), k
        for k in buffers:
            assert not np.array_equal(run[k].astype(np.float32), sd[k].numpy()), k
        out['run_' + tag] = np.concatenate([run[k].reshape(-1) for k in buffers])
        res[tag] = grads
    assert res['64'][params[0]].dtype == np.float64 and res['32'][params[0]].dtype == np.float32
    out['e32'] = np.array([np.linalg.norm(res['32'][k].astype(np.float64) - res['64'][k]) / np.linalg.norm(res['64'][k])
                           for k in params])
    np.savez_compressed(RC.GOLDEN, **out)
    flat = np.concatenate([res['64'][k].reshape(-1) for k in params]).astype(np.float32)
    sizes = [os.path.getsize(RC.GOLDEN)]
    for i, part in enumerate(np.array_split(flat, len(RC.GOLDEN_GRADS))):
        np.savez_compressed(RC.GOLDEN_GRADS[i], **{'grad_64_part%d' % i: part})
        sizes.append(os.path.getsize(RC.GOLDEN_GRADS[i]))
    assert all(s < (1 << 20) - (64 << 10) for s in sizes), sizes
    pools = {}
    for k, e in zip(params, out['e32']):
        kind = RC.kind_of(k, shapes[k])
        pools[kind] = max(pools.get(kind, 0.0), float(e))
    print('wrote %s (+ %d gradient files), %s bytes, %d parameters' % (RC.GOLDEN, len(RC.GOLDEN_GRADS), sizes, flat.size))
    print('largest reference e32 per kind:', {k: '%.2e' % v for k, v in sorted(pools.items())})


if __name__ == '__main__':
    main()
