"""One training step of a real architecture end to end: search-XS with 17 joints (heads of 34 and 17 channels), N = 4
images of 128 x 128 -- expansions up to 480 channels, 1x1 weight gradients with Cin > 128, odd channel counts in the
heads' data gradients, BatchNorms cut into up to 8 slices per channel, none of which the tiny golden network of
tests/test_gpu_train_net.py has.

No golden file: the truth is the same module with backend='torch' in fp64 on the CPU, the yardstick that module in fp32 on
the CPU (tests/test_train_net_cpu.py holds backend='torch' to the real reference module at 1e-12).  Weights are seeded, and
gamma / beta / the running pairs are moved away from their initial 1 / 0 / 0 / 1, so that no term of a BatchNorm drops out.
The rule is the one of tests/test_gpu_train_net.py, called from there on this case: per parameter tensor
e = |g - g64| / |g64|, pooled by kind, at most 4 x the largest e the fp32 CPU module shows for the kind; the outputs
likewise; the running pairs by its BatchNorm rule.  The factor 4 and its reason are in that module's docstring.

Then: two runs give the same bits for every output and gradient, and the step completes while torch's conv2d and
conv_transpose2d raise.

Measured on MI355X: see DESIGN.md 4f."""
import pytest
import torch

import _poison as po
import _train_forms as FM
import _train_net_case as TC
import test_gpu_train_net as TN
from litepose_amd import arch_zoo, config
from litepose_amd.models import pose_mobilenet as pm

pytestmark = pytest.mark.gpu

ARCH, JOINTS, N, RES = 'search-XS', 17, 4, 128


def _cfg():
    cfg = config.get_cfg()
    cfg.MODEL.NUM_JOINTS = JOINTS
    return cfg


def _module(sd, backend, dtype=torch.float32, device='cpu'):
    m = pm.get_train_net(_cfg(), arch_zoo.get(ARCH), backend=backend)
    m.load_state_dict(sd)
    return m.to(device=device, dtype=dtype).train()


def _step(m, x, ups):
    m.zero_grad()
    outs = m(x)
    torch.autograd.backward(outs, ups)
    return dict(outs=[o.detach().clone() for o in outs], grads={k: p.grad.detach().clone() for k, p in m.named_parameters()},
                sd={k: v.detach().clone() for k, v in m.state_dict().items()})


@pytest.fixture(scope='module')
def case():
    """the dictionary tests/_train_net_case.py's load() gives for the golden network, made here from the two CPU modules"""
    torch.manual_seed(1717)
    sd = pm.get_train_net(_cfg(), arch_zoo.get(ARCH), backend='torch').state_dict()
    g = torch.Generator().manual_seed(17)
    r = lambda t, scale: torch.randn(t.shape, generator=g) * scale       # noqa: E731
    for k, v in sd.items():
        if k.endswith('running_mean'):
            v.copy_(r(v, 0.3))
            gamma, beta = sd[k.replace('running_mean', 'weight')], sd[k.replace('running_mean', 'bias')]
            gamma.copy_(1.0 + r(gamma, 0.25))
            beta.copy_(r(beta, 0.2))
        elif k.endswith('running_var'):
            v.copy_(1.0 + r(v, 0.2).abs())
    x = torch.randn((N, 3, RES, RES), generator=g)
    m64 = _module(sd, 'torch', torch.float64)
    with torch.no_grad():
        shapes = [tuple(o.shape) for o in m64(x.double())]
    assert shapes == [(N, 2 * JOINTS, RES // 4, RES // 4), (N, JOINTS, RES // 2, RES // 2)]
    sd = {k: v.clone() for k, v in sd.items()}                           # the forward above moved m64's own copies only
    ups = [torch.randn(s, generator=g) for s in shapes]
    c = dict(x=x, ups=ups, state=sd, shapes={k: tuple(v.shape) for k, v in sd.items()},
             sd={k: v.numpy().copy() for k, v in sd.items() if not k.endswith('num_batches_tracked')})
    c['params'] = [k for k in c['sd'] if not k.endswith(('running_mean', 'running_var'))]
    c['buffers'] = [k for k in c['sd'] if k.endswith(('running_mean', 'running_var'))]
    for tag, dtype in (('64', torch.float64), ('32', torch.float32)):
        s = _step(_module(sd, 'torch', dtype), x.to(dtype), [u.to(dtype) for u in ups])
        c['grad_' + tag] = {k: s['grads'][k].numpy() for k in c['params']}
        c['run_' + tag] = {k: s['sd'][k].numpy() for k in c['buffers']}
        for i in range(2):
            c['out%d_%s' % (i, tag)] = s['outs'][i].numpy()
    return c


def _native_step(case):
    return _step(_module(case['state'], 'native', device='cuda'), case['x'].cuda(), [u.cuda() for u in case['ups']])


@pytest.fixture(scope='module')
def step(case):
    return _native_step(case)


def test_the_case_runs_the_forms_the_golden_network_does_not():
    """the reason for this file, asked of the library: several BatchNorm slices, Cin > 128, an odd K in a data gradient"""
    shapes = FM.calls(_cfg(), arch_zoo.get(ARCH), RES)
    bn = [FM.bn_slices(N, s[1], s[2] * s[3]) for s in shapes if s[0] == 'bn']
    assert max(bn) >= 8 and sum(v > 1 for v in bn) >= 8
    pw = [s for s in shapes if s[0] == 'pw']
    assert max(s[1] for s in pw) >= 480 and {17, 34} <= {s[2] for s in pw}
    assert any(FM.pw_dw_form(N, s[1], s[2], s[3], s[4])[3] == 'z>0' for s in pw)
    assert any(FM.pw_mm_form(N, s[2], s[1], s[3], s[4], 'dx')[4] == 'Kodd' for s in pw)
    golden = FM.calls(config.get_cfg(), TC.ARCH, TC.RES)
    assert all(FM.bn_slices(TC.N, s[1], s[2] * s[3]) == 1 for s in golden if s[0] == 'bn')


def test_outputs_and_gradients_against_the_fp64_module(case, step):
    TN.test_outputs_and_gradients_against_the_reference_step(case, step)


def test_running_pairs_against_the_fp64_module(case, step):
    TN.test_running_pairs_against_the_reference_step(case, step)


def test_two_steps_give_the_same_bits_for_every_parameter(case, step):
    again = _native_step(case)
    assert all(po.bitwise_equal(a, b) for a, b in zip(again['outs'], step['outs']))
    assert [k for k in step['grads'] if not po.bitwise_equal(again['grads'][k], step['grads'][k])] == []
    assert [k for k in case['buffers'] if not po.bitwise_equal(again['sd'][k], step['sd'][k])] == []


def _refuse(*a, **k):
    raise AssertionError("torch's convolution was called inside backend='native'")


def test_no_torch_convolution_in_the_native_step(case, step, monkeypatch):
    monkeypatch.setattr(torch.nn.functional, 'conv2d', _refuse)
    monkeypatch.setattr(torch.nn.functional, 'conv_transpose2d', _refuse)
    got = _native_step(case)
    for k, g in got['grads'].items():
        assert bool(torch.isfinite(g).all()) and bool(g.any()), k
        assert po.bitwise_equal(g, step['grads'][k]), k
