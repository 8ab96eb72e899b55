"""``get_train_net(..., backend='native')`` runs every layer on the library, the stem convolution and the transposed
convolutions included (tests/_train_net_case.py): a forward and a backward complete while torch's ``conv2d`` and
``conv_transpose2d`` raise, two runs give the same bits for every output and for the gradient of EVERY parameter, and one
SGD step is ``p - lr * g`` bitwise with the first run's gradients.  The one exception stays what it was: an image that
requires a gradient sends the stem through torch's ``conv2d``."""
import pytest
import torch

import _poison as po
import _train_net_case as TC
from test_gpu_train_net import LR, _forward_backward, _module

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def case():
    return TC.load()


@pytest.fixture(scope='module')
def first(case):
    m = _module(case)
    outs = _forward_backward(case, m)
    return dict(outs=[o.detach().clone() for o in outs], grads={k: p.grad.detach().clone() for k, p in m.named_parameters()})


def _refuse(*a, **k):
    raise AssertionError("torch's convolution was called inside backend='native'")


def test_no_torch_convolution_in_a_native_step(case, monkeypatch):
    monkeypatch.setattr(torch.nn.functional, 'conv2d', _refuse)
    monkeypatch.setattr(torch.nn.functional, 'conv_transpose2d', _refuse)
    m = _module(case)
    outs = _forward_backward(case, m)
    assert [tuple(o.shape) for o in outs] == [(TC.N, c, r, r) for c, r in zip(TC.HEADS, TC.OUT_RES)]
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), k


def test_two_runs_give_the_same_bits_for_every_parameter(case, first):
    m = _module(case)
    outs = _forward_backward(case, m)
    assert all(po.bitwise_equal(a, b) for a, b in zip(outs, first['outs']))
    differ = [k for k, p in m.named_parameters() if not po.bitwise_equal(p.grad, first['grads'][k])]
    assert differ == []
    kinds = {TC.kind_of(k, case['shapes'][k]) for k, _ in m.named_parameters()}
    assert {'stem', 'deconv'} <= kinds


def test_one_sgd_step_is_p_minus_lr_g_for_every_parameter(case, first):
    m = _module(case)
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    _forward_backward(case, m)
    opt.step()
    for k, p in m.named_parameters():
        assert po.bitwise_equal(p.detach(), before[k] - LR * first['grads'][k]), k


def test_an_image_that_requires_a_gradient_takes_torchs_stem(case):
    x = torch.from_numpy(case['x']).cuda()
    ups = [torch.from_numpy(case['up%d' % s]).cuda() for s in range(2)]
    got = {}
    for backend in ('native', 'torch'):
        m = _module(case, backend).train()
        xi = x.clone().requires_grad_()
        outs = m(xi)
        torch.autograd.backward(outs, ups)
        assert xi.grad is not None and bool(torch.isfinite(xi.grad).all()) and bool(xi.grad.any())
        got[backend] = (xi.grad, [o.detach() for o in outs], m.first[0][0].weight.grad)
    # the network tolerance of test_to_engine_agrees_with_the_eval_mode_forward
    tol = 2e-5 * max(1.0, float(got['torch'][0].abs().max()))
    err = float((got['native'][0] - got['torch'][0]).abs().max())
    print('image gradient: max |native - torch| = %.3e, tolerance %.3e' % (err, tol))
    assert err <= tol
    assert got['native'][2] is not None and bool(got['native'][2].any())
