#!/usr/bin/env python
"""Golden fixture of one training step of the network (tests/golden/golden_train_net.npz).  Build container only (needs
the reference checkout).  Runs the REAL lib/models/pose_mobilenet.LitePose on the CPU in train() mode on the tiny
architecture of tests/_train_net_case.py: forward on N = 2 images of 64 x 64, backward of sum_s (out_s * up_s).sum() with
fixed upstream gradients, once in fp32 and once more with the same module in fp64 (.double(), the same widened values).

Data only, packed into flat vectors in state_dict order (tests/_train_net_case.split):

  x [2,3,64,64], up0 [2,28,16,16], up1 [2,14,32,32]   fp32, on a 2^-6 grid (they compress)
  keys / shapes / ndims                               the state_dict's names and shapes
  sd                                                  every tensor but num_batches_tracked, fp32, on a 2^-8 grid:
                                                      seeded weights, gamma in [0.5, 1.5], beta in [-0.5, 0.5], running_mean
                                                      in [-0.5, 0.5], running_var in [0.5, 1.5] -- the state BEFORE the step
  out{s}_32 / out{s}_64                               the stage outputs
  grad_32 / grad_64                                   the gradient of every parameter
  run_32 / run_64                                     running_mean / running_var AFTER the step

Asserted here: every parameter has a gradient that is not all zeros, and every running tensor moved."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = '/root/reference'

import _train_net_case as TC  # noqa: E402


def _load(name, path):
    s = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(s)
    sys.modules[name] = m
    s.loader.exec_module(m)
    return m


def make_cfg():
    NS = types.SimpleNamespace
    return NS(LOSS=NS(NUM_STAGES=2, WITH_HEATMAPS_LOSS=[True, True], WITH_AE_LOSS=[True, False]),
              MODEL=NS(NAME='pose_mobilenet', NUM_JOINTS=TC.J, TAG_PER_JOINT=True, INIT_WEIGHTS=False, PRETRAINED='',
                       EXTRA=NS(NUM_DECONV_LAYERS=3, NUM_DECONV_KERNELS=[4, 4, 4])))


def grid(a, bits):
    return (np.round(a * (1 << bits)) / (1 << bits)).astype(np.float32)


def make_state(model, rng):
    sd = {}
    for k, v in model.state_dict().items():
        shp = tuple(v.shape)
        if k.endswith('num_batches_tracked'):
            continue
        if k.endswith('running_var'):
            a = rng.uniform(0.5, 1.5, shp)
        elif k.endswith('running_mean'):
            a = rng.uniform(-0.5, 0.5, shp)
        elif len(shp) == 1:
            a = rng.uniform(0.5, 1.5, shp) if k.endswith('weight') else rng.uniform(-0.5, 0.5, shp)
        else:
            fan_in = int(np.prod(shp[1:])) if 'deconv' not in k else shp[0] * 4
            a = rng.standard_normal(shp) * (2.0 / fan_in) ** 0.5
        sd[k] = grid(a, 8)
        if len(shp) == 1 and k.endswith(('weight', 'running_var')):
            assert sd[k].min() >= 0.5
    return sd


def step(model, sd, x, ups, dtype):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
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
    warnings.simplefilter('ignore')
    sys.path[:0] = [REF, os.path.join(REF, 'lib')]
    pm = _load('ref_pose_mobilenet', os.path.join(REF, 'lib/models/pose_mobilenet.py'))
    torch.manual_seed(0)
    model = pm.LitePose(make_cfg(), cfg_arch=TC.ARCH)
    rng = np.random.RandomState(20240607)
    sd = make_state(model, rng)
    x = grid(rng.standard_normal((TC.N, 3, TC.RES, TC.RES)), 6)
    ups = [grid(rng.standard_normal((TC.N, c, r, r)), 6) for c, r in zip(TC.HEADS, TC.OUT_RES)]
    keys = list(model.state_dict().keys())
    shapes = [tuple(v.shape) for v in model.state_dict().values()]
    out = dict(x=x, up0=ups[0], up1=ups[1], keys=np.array(keys), ndims=np.array([len(s) for s in shapes], np.int32),
               shapes=np.array([list(s) + [0] * (4 - len(s)) for s in shapes], np.int32),
               sd=np.concatenate([sd[k].reshape(-1) for k in keys if k in sd]))
    params = [k for k, _ in model.named_parameters()]
    buffers = [k for k in keys if k.endswith(('running_mean', 'running_var'))]
    assert params == [k for k in keys if k in sd and k not in buffers]
    for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
        outs, grads, run = step(model, sd, x, ups, dtype)
        for s, o in enumerate(outs):
            assert o.shape == (TC.N, TC.HEADS[s], TC.OUT_RES[s], TC.OUT_RES[s])
            out['out%d_%s' % (s, tag)] = o
        for k in params:
            assert grads[k].any(), k
        for k in buffers:
            assert not np.array_equal(run[k].astype(np.float32), sd[k]), k
        out['grad_' + tag] = np.concatenate([grads[k].reshape(-1) for k in params])
        out['run_' + tag] = np.concatenate([run[k].reshape(-1) for k in buffers])
        assert out['grad_' + tag].dtype == (np.float32 if tag == '32' else np.float64)
    np.savez_compressed(TC.GOLDEN, **out)
    size = os.path.getsize(TC.GOLDEN)
    assert size < (1 << 20), size
    print('wrote %s (%d bytes), %d parameters' % (TC.GOLDEN, size, out['grad_32'].size))


if __name__ == '__main__':
    main()
