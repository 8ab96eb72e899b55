"""``pose_resnet.get_train_net(..., backend='native')`` on the device against one training step of the real reference
module (tests/golden/golden_resnet_train*.npz, width_mult 0.25): forward on the golden input, backward with the golden
upstream gradients, held by the rule of tests/test_gpu_train_net.py.

No bound can be derived through forty layers, so the yardstick is the reference's own fp32.  For each parameter tensor
e = |g - g64|_2 / |g64|_2; the tensors are pooled by layer kind (dense K x K weight, 1x1 weight, output-conv weight, gamma,
beta, conv bias); the module's e for a tensor may not exceed FOUR times the largest stored e32 of that kind (that file's
argument for four applies unchanged), plus 2^-24 because the fp64 gradients are stored rounded to fp32.  The same rule
holds the two outputs (one pool).  A running tensor is held by the per-layer BatchNorm rule of that file.

Measured on MI355X (largest ratio e / (largest reference e of the kind); the bound is 4): see DESIGN.md 4f.

Then: no torch convolution runs (also with an image that requires a gradient), two runs give the same bits for EVERY
parameter, one SGD step is p - lr * g bitwise, do_train eager and captured end with the same bits, and to_engine()."""
import random

import numpy as np
import pytest
import torch

import _poison as po
import _resnet_ref as rr
import _resnet_train_case as RC
from litepose_amd import optim
from litepose_amd.models import pose_resnet as pr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LR = 0.25            # a power of two: lr * g is exact, p - lr * g rounds once however the optimizer evaluates it


@pytest.fixture(scope='module')
def cfg():
    return RC.cfg()


@pytest.fixture(scope='module')
def case():
    return RC.load()


def _module(cfg, backend='native'):
    m = pr.get_train_net(cfg, backend=backend, width_mult=RC.WIDTH)
    m.load_state_dict(RC.state(cfg))
    return m.cuda()


def _forward_backward(case, m, x=None):
    m.train()
    m.zero_grad()
    outs = m(torch.from_numpy(case['x']).cuda() if x is None else x)
    torch.autograd.backward(outs, [torch.from_numpy(case['up%d' % s]).cuda() for s in range(2)])
    return outs


@pytest.fixture(scope='module')
def step(cfg, case):
    m = _module(cfg)
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
        kind = RC.kind_of(k, case['shapes'][k])
        pools[kind] = max(pools.get(kind, 0.0), case['e32'][k])
        mine[k] = (kind, _rel(step['grads'][k], case['grad_64'][k]))
    assert sorted(pools) == sorted(RC.KINDS)
    worst = {}
    for k, (kind, e) in mine.items():
        # conv_bias: the reference's fp32 sums of the grid-valued upstream gradients are exact (pool 0): reported as e / 2^-24
        worst[kind] = max(worst.get(kind, 0.0), e / pools[kind] if pools[kind] else e / RC.GRAD_ROUNDING)
    pool_out = max(_rel(case['out%d_32' % s], case['out%d_64' % s]) for s in range(2))
    worst['output'] = max(_rel(step['outs'][s], case['out%d_64' % s]) for s in range(2)) / pool_out
    for kind in sorted(worst):
        print('%-9s largest e / (largest reference e of the kind) = %.3f' % (kind, worst[kind]))
    for k, (kind, e) in mine.items():
        assert e <= 4 * pools[kind] + RC.GRAD_ROUNDING, (k, kind, e, pools[kind])
    assert worst['output'] <= 4


def test_running_pairs_against_the_reference_step(cfg, case, step):
    m = 0.1
    before = RC.state(cfg)
    pools = {}
    for k in case['buffers']:
        kind = k.rsplit('.', 1)[1]
        pools[kind] = max(pools.get(kind, 0.0), _rel(case['run_32'][k], case['run_64'][k]))
    worst = 0.0
    for k in case['buffers']:
        f = np.asarray(case['run_64'][k], np.float64)
        r0 = (1 - m) * before[k].double().numpy()
        terms = np.abs(r0) + np.abs(f - r0)
        bound = 3 * U * np.linalg.norm(terms) + 4 * pools[k.rsplit('.', 1)[1]] * np.linalg.norm(f)
        err = np.linalg.norm(step['sd'][k].cpu().double().numpy() - f)
        worst = max(worst, err / bound)
        assert err <= bound, (k, err / bound)
        assert not np.array_equal(step['sd'][k].cpu().numpy(), before[k].numpy()), k
    print('running pairs: largest error / bound = %.3f' % worst)
    assert all(int(v) == 1 for k, v in step['sd'].items() if k.endswith('num_batches_tracked'))


def test_no_torch_convolution_runs(cfg, case, step, monkeypatch):
    x = torch.from_numpy(case['x']).cuda()
    with monkeypatch.context() as mp:
        def refuse(*a, **k):
            raise AssertionError('a torch convolution / interpolation ran under backend=native')
        for name in ('conv2d', 'conv_transpose2d', 'interpolate'):
            mp.setattr(torch.nn.functional, name, refuse)
        m = _module(cfg)
        outs = _forward_backward(case, m)
        assert all(po.bitwise_equal(a, b) for a, b in zip(outs, step['outs']))
        xi = x.clone().requires_grad_()
        m2 = _module(cfg)
        outs = _forward_backward(case, m2, xi)
        assert xi.grad is not None and bool(torch.isfinite(xi.grad).all()) and bool(xi.grad.any())
        # asking for the image gradient changes nothing else
        assert all(po.bitwise_equal(a, b) for a, b in zip(outs, step['outs']))
        assert all(po.bitwise_equal(p.grad, step['grads'][k]) for k, p in m2.named_parameters())
    t = _module(cfg, 'torch')
    xt = x.clone().requires_grad_()
    _forward_backward(case, t, xt)
    # the network tolerance of test_an_image_that_requires_a_gradient_takes_torchs_stem
    tol = 2e-5 * max(1.0, float(xt.grad.abs().max()))
    err = float((xi.grad - xt.grad).abs().max())
    print('image gradient: max |native - torch| = %.3e, tolerance %.3e' % (err, tol))
    assert err <= tol


def test_two_steps_give_the_same_bits(cfg, case, step):
    """the outputs and the gradient of EVERY parameter: no layer of this module is torch's"""
    m = _module(cfg)
    outs = _forward_backward(case, m)
    assert all(po.bitwise_equal(a, b) for a, b in zip(outs, step['outs']))
    differ = [k for k, p in m.named_parameters() if not po.bitwise_equal(p.grad, step['grads'][k])]
    assert not differ, differ
    for k, v in m.state_dict().items():
        assert po.bitwise_equal(v, step['sd'][k]), k


def test_one_sgd_step_is_p_minus_lr_g(cfg, case, step):
    m = _module(cfg)
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    _forward_backward(case, m)
    opt.step()
    for k, p in m.named_parameters():
        assert po.bitwise_equal(p.detach(), before[k] - LR * step['grads'][k]), k


def _train_cfg():
    c = RC.cfg()
    if hasattr(c, 'defrost'):
        c.defrost()
    c.DATASET.INPUT_SIZE, c.DATASET.OUTPUT_SIZE, c.DATASET.MAX_NUM_PEOPLE = 64, [16, 32], 6
    return c


def test_do_train_eager_and_captured_end_with_the_same_bits():
    from litepose_amd.core import inference
    from litepose_amd.core.loss import MultiLossFactory
    from litepose_amd.core.trainer import CapturedStep, do_train
    from litepose_amd.dataset import LabelledSet
    cfg = _train_cfg()
    J = cfg.DATASET.NUM_JOINTS
    rng = np.random.RandomState(3)
    sizes = [(40, 56), (33, 47), (64, 64), (48, 36), (50, 50), (37, 61)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    joints = []
    for (h, w), people in zip(sizes, (2, 1, 3, 6, 2, 4)):
        j = np.zeros((people, J, 3))
        j[:, :, 0], j[:, :, 1] = rng.uniform(0, w, (people, J)), rng.uniform(0, h, (people, J))
        j[:, :, 2] = rng.choice([0, 1, 2], (people, J))
        joints.append(j)
    ls = LabelledSet(images, joints, inference.flip_index_for(cfg)[:J], max_num_people=6, sigma=cfg.DATASET.SIGMA)
    batches = list(ls.batches(64, [16, 32], 2, np.random.RandomState(8), random.Random(8)))
    assert [int(b[0].shape[0]) for b in batches] == [2, 2, 2]

    def clone(b):
        return tuple([t.clone() for t in part] if isinstance(part, list) else part.clone() for part in b)

    runs = {}
    for graph in (False, True):
        m = _module(cfg).train()
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        opt = optim.Adam(m.parameters(), lr=1e-3)
        factory = MultiLossFactory(cfg)
        stepper = CapturedStep(cfg, m, factory, opt) if graph else False
        got = do_train(cfg, m, (clone(b) for b in batches), factory, opt, 0, None, None, stepper)
        torch.cuda.synchronize()
        if graph:
            assert (stepper.captures, stepper.replays, stepper.eager_steps) == (1, 2, 1)
        assert m.training
        for k, p in m.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), k
            assert not torch.equal(p.detach(), before[k]), k            # every parameter trained
        for k, v in m.state_dict().items():
            if k.endswith('num_batches_tracked'):
                assert int(v) == 3, k
        runs[graph] = dict(sd={k: v.detach().clone() for k, v in m.state_dict().items()}, got=got)
    for k, v in runs[False]['sd'].items():
        assert po.bitwise_equal(v, runs[True]['sd'][k]), k
    assert runs[False]['got'] == runs[True]['got'], (runs[False]['got'], runs[True]['got'])
    got = runs[True]['got']
    assert got['heatmaps'][0] is not None and got['heatmaps'][1] is not None and got['push'][0] is not None


def test_to_engine_agrees_with_the_eval_mode_forward(cfg, case):
    sd = rr.make_state_dict(cfg, 1234)
    m = pr.get_train_net(cfg, backend='native')
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = torch.from_numpy(case['x']).cuda()
    with torch.no_grad():
        want = m(x)
    eng = m.to_engine()
    assert isinstance(eng, pr.LitePose) and eng.storage == 'f32'
    got = eng(x)
    for s in range(2):
        tol = 2e-5 * max(1.0, float(want[s].abs().max()))               # the network tolerance of tests/test_gpu_train_net.py
        assert got[s].shape == want[s].shape
        assert float((got[s] - want[s]).abs().max()) <= tol, s
    # a state_dict of the engine loads back into the module, strictly
    back = pr.get_train_net(cfg, backend='native')
    back.load_state_dict(eng.state_dict())
    for k, v in m.state_dict().items():
        if not k.endswith('num_batches_tracked'):
            assert torch.equal(back.state_dict()[k], v.cpu()), k
