"""``get_train_net(..., backend='native')`` on the device against one training step of the real reference module
(tests/golden/golden_train_net.npz): forward on the golden input, backward with the golden upstream gradients.

No bound can be derived through forty layers, so the yardstick is the reference's own fp32.  For each parameter tensor
e = |g - g64|_2 / |g64|_2; the tensors are pooled by layer kind (1x1 weight, depthwise weight, gamma, beta, stem, deconv);
the module's e for a tensor may not exceed FOUR times the largest e the reference's fp32 CPU gradient shows for any tensor
of that kind.  Why four: two fp32 evaluations in different summation orders have errors of the same size, pooling by
kind removes tensors where the reference got lucky, four leaves room for that spread and no more.  The same rule holds the
two outputs (one pool).  A running tensor is held by the per-layer BatchNorm rule -- 3 * 2^-24 times the terms
(1 - m) |running| + |m * batch statistic| -- plus four times the largest relative error the reference's fp32 forward shows
for a running tensor of its kind (means, variances).

Measured on MI355X (largest ratio e / (largest reference e of the kind); the bound is 4): see DESIGN.md 4f.

Then: do_train with SGD on a small LabelledSet, one step against p - lr * g bitwise, and to_engine()."""
import random

import numpy as np
import pytest
import torch

import _poison as po
import _train_net_case as TC
from litepose_amd import config
from litepose_amd.models import pose_mobilenet as pm

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LR = 0.25            # a power of two: lr * g is exact, p - lr * g rounds once however the optimizer evaluates it


@pytest.fixture(scope='module')
def case():
    return TC.load()


def _module(case, backend='native'):
    m = pm.get_train_net(config.get_cfg(), TC.ARCH, backend=backend)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case['sd'].items()}, strict=False)
    return m.cuda()


def _forward_backward(case, m):
    m.train()
    m.zero_grad()
    outs = m(torch.from_numpy(case['x']).cuda())
    torch.autograd.backward(outs, [torch.from_numpy(case['up%d' % s]).cuda() for s in range(2)])
    return outs


@pytest.fixture(scope='module')
def step(case):
    m = _module(case)
    outs = _forward_backward(case, m)
    return dict(outs=[o.detach().clone() for o in outs], grads={k: p.grad.detach().clone() for k, p in m.named_parameters()},
                sd={k: v.detach().clone() for k, v in m.state_dict().items()})


def _rel(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_outputs_and_gradients_against_the_reference_step(case, step):
    pools, mine = {}, {}
    for k in case['params']:
        kind = TC.kind_of(k, case['shapes'][k])
        ref = _rel(case['grad_32'][k], case['grad_64'][k])
        pools[kind] = max(pools.get(kind, 0.0), ref)
        mine[k] = (kind, _rel(step['grads'][k], case['grad_64'][k]))
    assert sorted(pools) == ['beta', 'deconv', 'dw', 'gamma', 'pw', 'stem']
    worst = {}
    for k, (kind, e) in mine.items():
        worst[kind] = max(worst.get(kind, 0.0), e / pools[kind])
    pool_out = max(_rel(case['out%d_32' % s], case['out%d_64' % s]) for s in range(2))
    worst['output'] = max(_rel(step['outs'][s], case['out%d_64' % s]) for s in range(2)) / pool_out
    for kind in sorted(worst):
        print('%-7s largest e / (largest reference e of the kind) = %.3f' % (kind, worst[kind]))
    for k, (kind, e) in mine.items():
        assert e <= 4 * pools[kind], (k, kind, e / pools[kind])
    assert worst['output'] <= 4


def test_running_pairs_against_the_reference_step(case, step):
    m = 0.1
    pools = {}
    for k in case['buffers']:
        kind = k.rsplit('.', 1)[1]
        pools[kind] = max(pools.get(kind, 0.0), _rel(case['run_32'][k], case['run_64'][k]))
    worst = 0.0
    for k in case['buffers']:
        f = np.asarray(case['run_64'][k], np.float64)
        r0 = (1 - m) * case['sd'][k].astype(np.float64)
        terms = np.abs(r0) + np.abs(f - r0)
        bound = 3 * U * np.linalg.norm(terms) + 4 * pools[k.rsplit('.', 1)[1]] * np.linalg.norm(f)
        err = np.linalg.norm(step['sd'][k].cpu().double().numpy() - f)
        worst = max(worst, err / bound)
        assert err <= bound, (k, err / bound)
        assert not np.array_equal(step['sd'][k].cpu().numpy(), case['sd'][k]), k
    print('running pairs: largest error / bound = %.3f' % worst)
    assert all(int(v) == 1 for k, v in step['sd'].items() if k.endswith('num_batches_tracked'))


TORCH_KINDS = ('stem', 'deconv')      # weights whose gradient is torch's own convolution backward: no fixed order promised


def test_two_steps_give_the_same_bits(case, step):
    """Everything the library's kernels compute is the same from run to run: the outputs, and the gradient of every 1x1
    and depthwise weight, gamma and beta.  (The stem's and the deconvs' weight gradients are torch's.)"""
    m = _module(case)
    outs = _forward_backward(case, m)
    assert all(po.bitwise_equal(a, b) for a, b in zip(outs, step['outs']))
    differ = [k for k, p in m.named_parameters() if not po.bitwise_equal(p.grad, step['grads'][k])]
    assert all(TC.kind_of(k, case['shapes'][k]) in TORCH_KINDS for k in differ), differ


def test_one_sgd_step_is_p_minus_lr_g(case, step):
    m = _module(case)
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    _forward_backward(case, m)
    opt.step()
    for k, p in m.named_parameters():
        g = step['grads'][k]
        if TC.kind_of(k, case['shapes'][k]) in TORCH_KINDS:
            g = p.grad                                       # torch's own backward: this run's gradient
        assert po.bitwise_equal(p.detach(), before[k] - LR * g), k


def test_do_train_trains_every_parameter(case):
    from litepose_amd.core import inference
    from litepose_amd.core.loss import MultiLossFactory
    from litepose_amd.core.trainer import do_train
    from litepose_amd.dataset import LabelledSet
    cfg = config.get_cfg()
    cfg.DATASET.INPUT_SIZE, cfg.DATASET.OUTPUT_SIZE, cfg.DATASET.MAX_NUM_PEOPLE = 64, [16, 32], 6
    J = cfg.DATASET.NUM_JOINTS
    rng = np.random.RandomState(3)
    sizes = [(40, 56), (33, 47), (64, 64), (48, 36)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    joints = []
    for (h, w), people in zip(sizes, (2, 1, 3, 6)):
        j = np.zeros((people, J, 3))
        j[:, :, 0], j[:, :, 1] = rng.uniform(0, w, (people, J)), rng.uniform(0, h, (people, J))
        j[:, :, 2] = rng.choice([0, 1, 2], (people, J))
        joints.append(j)
    ls = LabelledSet(images, joints, inference.flip_index_for(cfg)[:J], max_num_people=6, sigma=cfg.DATASET.SIGMA)
    m = _module(case)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    got = do_train(cfg, m, ls.batches(64, [16, 32], 2, np.random.RandomState(8), random.Random(8)), MultiLossFactory(cfg), opt)
    assert m.training
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), k
    for k, v in m.state_dict().items():
        if k.endswith(('running_mean', 'running_var')):
            assert not torch.equal(v, before[k]), k
        elif k.endswith('num_batches_tracked'):
            assert int(v) == 2, k
    for key, vals in got.items():
        for v in vals:
            assert v is None or (np.isfinite(v[0]) and np.isfinite(v[1])), (key, vals)
    assert got['heatmaps'][0] is not None and got['heatmaps'][1] is not None and got['push'][0] is not None


def test_to_engine_agrees_with_the_eval_mode_forward(case):
    m = _module(case).eval()
    x = torch.from_numpy(case['x']).cuda()
    with torch.no_grad():
        want = m(x)
        torch_way = _module(case, 'torch').eval()(x)
    eng = m.to_engine()
    assert isinstance(eng, pm.LitePose) and eng.storage == 'f32'
    got = eng(x)
    for s in range(2):
        tol = 2e-5 * max(1.0, float(want[s].abs().max()))               # the network tolerance of tests/test_gpu_supernet.py
        assert float((got[s] - want[s]).abs().max()) <= tol, s
        assert float((torch_way[s] - want[s]).abs().max()) <= tol, s
    # a state_dict of the engine loads back into the module, strictly
    back = pm.get_train_net(config.get_cfg(), TC.ARCH)
    back.load_state_dict(eng.state_dict())
    for k, v in m.state_dict().items():
        if not k.endswith('num_batches_tracked'):
            assert torch.equal(back.state_dict()[k], v.cpu()), k
