"""NaN / Inf propagation and containment in the training loss, its gradient and the optimizers, by the method of
tests/_nonfinite.py: one element set to NaN, +inf or -inf, the non-finite outputs are exactly those of the fp64 truth on the
same inputs, with its class and sign (fp64 / plain fp32 arithmetic everywhere here), and whatever the truth leaves as it
was keeps the bits of the clean run.

  lp_pose_loss, lp_pose_loss_grad   against the restatements of tests/_loss_ref.py and tests/_loss_grad_ref.py; the site is in
                                    the middle image of three, so the other two images are held bitwise
  lp_optim_adam, lp_optim_sgd       against torch.optim on the CPU in fp64, one step on given state"""
import numpy as np
import pytest
import torch

import _loss_grad_ref as GR
import _loss_ref as LR
import _nonfinite as NF
import _train_case as tc
from test_gpu_loss_grad import _put, _run as _loss_grad
from test_gpu_optim import E, _adam_call, _layout, _lr, _sgd_call, _views

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ the loss and its gradient
N, J, CC, M, OFF = 3, 3, 6, 3, 4                       # three heatmaps, a plane between the terms, two tag planes
FACTORS = (0.5, 0.25, 2.0)
LT = {'exp': 0, 'max': 1}


def _loss_case(R):
    rng = np.random.RandomState(100 + R)
    c = dict(out=rng.standard_normal((N, CC, R, R)).astype(np.float32),
             heat=rng.uniform(0, 1, (N, J, R, R)).astype(np.float32),
             mask=(rng.uniform(0, 1, (N, R, R)) > 0.3).astype(np.float32))
    cells = rng.choice(2 * R * R, N * M * J, replace=False).reshape(N, M, J)       # every slot its own tag cell
    joints = np.zeros((N, M, J, 2), np.int32)
    joints[..., 0] = cells
    joints[..., 1] = 1
    joints[1, 2, 1, 1] = 0                               # one slot of the middle image's last person is not visible
    c['joints'] = joints
    for k in ('gh', 'gpu', 'gpl'):
        c[k] = rng.uniform(0.5, 2, N).astype(np.float32)
    return c


def _loss_ref(c, lt):
    """-> dict of fp64 tensors: hl, push, pull [N], grad [N,C,R,R]"""
    hl, push, pull = np.zeros(N), np.zeros(N), np.zeros(N)
    grad = np.zeros(c['out'].shape)
    with np.errstate(all='ignore'):
        for n in range(N):
            hl[n] = LR.heat_loss(c['out'][n, :J], c['heat'][n], c['mask'][n], FACTORS[0])
            push[n], pull[n] = LR.tag_loss(c['out'][n, OFF:], c['joints'][n], lt, FACTORS[1], FACTORS[2])
            grad[n, :J] = GR.heat_grad(c['out'][n, :J], c['heat'][n], c['mask'][n], FACTORS[0], c['gh'][n])
            grad[n, OFF:] = GR.tag_grad(c['out'][n, OFF:], c['joints'][n], lt, FACTORS[1], FACTORS[2], c['gpu'][n], c['gpl'][n])
    # one fp32 rounding of a finite fp64 value is finite here: the magnitudes are moderate
    return {k: torch.from_numpy(v) for k, v in dict(hl=hl, push=push, pull=pull, grad=grad).items()}


def _loss_dev(c, lt, shift):
    out, heat, mask = (_put(c[k], shift) for k in ('out', 'heat', 'mask'))
    joints = tc.dev(c['joints'])
    R = c['out'].shape[2]
    hl, push, pull = [torch.empty(N, dtype=torch.float32, device='cuda') for _ in range(3)]
    ws = torch.empty(tc.loss_ws(N, J, R), dtype=torch.uint8, device='cuda')
    tc.call_loss(out, J, OFF, heat, mask, joints, LT[lt], FACTORS, hl, push, pull, ws)
    grad = torch.empty(c['out'].size + shift, dtype=torch.float32, device='cuda')[shift:].view(c['out'].shape)
    grad = _loss_grad(out, J, OFF, heat, mask, joints, LT[lt], tc.dev(c['gh']), tc.dev(c['gpu']), tc.dev(c['gpl']), FACTORS,
                      grad=grad)
    return dict(hl=hl, push=push, pull=pull, grad=grad.contiguous())


def _loss_sites(c):
    """(name, array, index): all in the middle image"""
    R = c['out'].shape[2]
    mask = c['mask'][1]
    open_ = tuple(int(v) for v in np.argwhere(mask == 1)[-1])
    shut = tuple(int(v) for v in np.argwhere(mask == 0)[-1])
    named = int(c['joints'][1, 0, 1, 0])                  # a visible slot
    hidden = int(c['joints'][1, 2, 1, 0])                 # the slot that is not visible: nothing reads its cell
    used = set(int(v) for v in c['joints'][1, :, :, 0].reshape(-1))
    free = next(i for i in range(2 * R * R - 1, -1, -1) if i not in used)
    cell = lambda i: (1, OFF + i // (R * R), (i % (R * R)) // R, i % R)       # noqa: E731
    return [('heat cell, unmasked', 'out', (1, J - 1) + open_), ('heat cell, masked', 'out', (1, 0) + shut),
            ('tag cell a visible joint names', 'out', cell(named)), ('tag cell of a slot that is not visible', 'out', cell(hidden)),
            ('tag cell no joint names', 'out', cell(free)), ('the plane between the terms', 'out', (1, J, R - 1, R - 1)),
            ('target, unmasked', 'heat', (1, 0) + open_), ('target, masked', 'heat', (1, J - 1) + shut),
            ('mask', 'mask', (1,) + open_), ('mask, a zero', 'mask', (1,) + shut),
            ('upstream of the heat term', 'gh', (1,)), ('upstream of push', 'gpu', (1,)), ('upstream of pull', 'gpl', (1,))]


@pytest.mark.parametrize('lt', ['exp', 'max'])
@pytest.mark.parametrize('R, shift', [(66, 0), (65, 0), (66, 1)], ids=['R66', 'R65', 'R66+1float'])
def test_pose_loss_and_its_gradient(R, shift, lt):
    c = _loss_case(R)
    Rf, O = _loss_ref(c, lt), _loss_dev(c, lt, shift)
    hit = 0
    for name, key, idx in _loss_sites(c):
        for vname, value in NF.VALUES.items():
            bad = dict(c)
            bad[key] = c[key].copy()
            bad[key][idx] = value
            Rb, Ob = _loss_ref(bad, lt), _loss_dev(bad, lt, shift)
            sizes = NF.compare_all('loss %s R=%d+%d %s %s:' % (lt, R, shift, name, vname), O, Ob, Rf, Rb, value, True)
            hit += sum(sizes.values())
            for k in O:                                      # the other images of the batch: the clean run's bits
                assert NF.bitwise(Ob[k][0], O[k][0]) and NF.bitwise(Ob[k][2], O[k][2]), (name, vname, k)
            if name in ('tag cell no joint names', 'tag cell of a slot that is not visible', 'the plane between the terms'):
                assert not sum(sizes.values()), name           # nothing reads it
            if name == 'tag cell a visible joint names' and vname == 'nan':
                assert sizes['push'] == 1 and sizes['pull'] == 1 and sizes['grad'] >= J
    assert hit > 0


# ------------------------------------------------------------------ the optimizers
BODY = 27 * 32 + 3                                       # 216 16-byte quads and a tail of three
LENGTHS = [BODY, E + 9, 427 * E, 5 * E - 100]            # 1 + 2 + 427 blocks, then five that cross the chunk of 432 blocks
MIS = {1}
OPT_SITES = [('16-byte body', 0, 16), ('ragged tail', 0, BODY - 1), ('misaligned tensor', 1, E + 8),
             ('before the chunk boundary', 3, 5), ('after the chunk boundary', 3, 3 * E + 5)]


def _opt_state(seed):
    offs, total = _layout(LENGTHS, MIS)
    g = torch.Generator().manual_seed(seed)
    mk = lambda scale: (torch.randn(total, generator=g) * scale).float()      # noqa: E731
    return offs, dict(p=mk(1.0), g=mk(0.1), m=mk(0.05), v=mk(0.01).abs())


def _adam_dev(st, offs, lr, wd):
    d = {k: v.cuda() for k, v in st.items()}
    P, G, Mm, V = (_views(d[k], offs, LENGTHS) for k in ('p', 'g', 'm', 'v'))
    assert P[1].data_ptr() % 16 == 4 and P[0].data_ptr() % 16 == 0
    steps = torch.full((len(LENGTHS),), 3.0, device='cuda')
    _adam_call(P, G, Mm, V, steps, _lr(lr), 0.9, 0.999, 1e-8, wd)
    assert steps.tolist() == [4.0] * len(LENGTHS) and NF.bitwise(d['g'], st['g'].cuda())
    return dict(p=d['p'], m=d['m'], v=d['v'])


def _adam_ref(st, offs, lr, wd):
    d = {k: v.double().clone() for k, v in st.items()}
    P = [torch.nn.Parameter(t) for t in _views(d['p'], offs, LENGTHS)]
    opt = torch.optim.Adam(P, lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    opt.param_groups[0]['lr'] = lr                           # the constructor refuses a NaN; a scheduler can still deliver one
    for i, p in enumerate(P):
        o, n = offs[i], LENGTHS[i]
        p.grad = d['g'][o:o + n]
        opt.state[p] = dict(step=torch.tensor(3.0), exp_avg=d['m'][o:o + n], exp_avg_sq=d['v'][o:o + n])
    opt.step()
    return dict(p=d['p'], m=d['m'], v=d['v'])


def _sgd_dev(st, offs, lr, wd):
    d = {k: v.cuda() for k, v in st.items()}
    P, G, B = (_views(d[k], offs, LENGTHS) for k in ('p', 'g', 'm'))
    _sgd_call(P, G, B, _lr(lr), 0.9, wd, True)
    return dict(p=d['p'], buf=d['m'])


def _sgd_ref(st, offs, lr, wd):
    d = {k: v.double().clone() for k, v in st.items()}
    P = [torch.nn.Parameter(t) for t in _views(d['p'], offs, LENGTHS)]
    opt = torch.optim.SGD(P, lr=1.0, momentum=0.9, weight_decay=wd, nesterov=True)
    opt.param_groups[0]['lr'] = lr
    for i, p in enumerate(P):
        o, n = offs[i], LENGTHS[i]
        p.grad = d['g'][o:o + n].clone()
        opt.state[p] = dict(momentum_buffer=d['m'][o:o + n])
    opt.step()
    return dict(p=d['p'], buf=d['m'])


@pytest.mark.parametrize('which', ['adam', 'sgd'])
def test_optimizer_step(which):
    """one gradient element in turn; then a NaN learning rate.  Only that element of p, m, v (or buf) changes class; every
    other element, the gaps between the tensors included, is bitwise the clean step."""
    dev, ref = (_adam_dev, _adam_ref) if which == 'adam' else (_sgd_dev, _sgd_ref)
    offs, st = _opt_state(7)
    lr, wd = 3e-3, 0.01
    Rf, O = ref(st, offs, lr, wd), dev(st, offs, lr, wd)
    for name, t, i in OPT_SITES:
        for vname, value in NF.VALUES.items():
            bad = dict(st)
            bad['g'] = NF.inject(st['g'], (offs[t] + i,), value)
            sizes = NF.compare_all('%s %s %s:' % (which, name, vname), O, dev(bad, offs, lr, wd), Rf, ref(bad, offs, lr, wd),
                                   value, True)
            assert set(sizes.values()) == {1}, (name, vname, sizes)
    sizes = NF.compare_all('%s lr = NaN:' % which, O, dev(st, offs, NF.NAN, wd), Rf, ref(st, offs, NF.NAN, wd), NF.NAN, True)
    assert sizes['p'] == sum(LENGTHS) and sum(sizes.values()) == sizes['p']


# ------------------------------------------------------------------ the whole module
# backend='native' on the device against backend='torch' on the CPU in fp64 (not torch's device convolutions, whose
# algorithms may spread a NaN wider than the cone): the tiny architecture of tests/_train_net_case.py, one pixel of the batch
# set to NaN.
from _train_run import _loader, _module, setup  # noqa: E402,F401  (setup: the module-scoped fixture)
import _train_net_case as TC  # noqa: E402
from litepose_amd import config, optim  # noqa: E402
from litepose_amd.core.loss import MultiLossFactory  # noqa: E402
from litepose_amd.core.trainer import CapturedStep, do_train  # noqa: E402
from litepose_amd.models import pose_mobilenet as pm  # noqa: E402

PIXELS = [('first', (0, 0, 0, 0)), ('centre', (1, 1, 32, 32)), ('last', (1, 2, 63, 63))]


def _relu6(x):
    """relu6 as two selects.  torch's own hardtanh backward has two answers at a NaN input on the CPU -- its vectorised body
    closes the gate, its scalar tail passes the gradient --, so the mask of a BatchNorm bias gradient would depend on the
    channel's length.  The selects pass a NaN forward and its gradient backward everywhere, as torch.relu does and as the
    scalar tail does; on every other input they are relu6 and its gradient (strict inequalities)."""
    zero, six = torch.zeros((), dtype=x.dtype), torch.full((), 6.0, dtype=x.dtype)
    return torch.where(x <= 0, zero, torch.where(x >= 6, six, x))


class _Reference(object):
    """backend='torch' in fp64 on the CPU, with ``_relu6`` where the module calls torch.nn.functional.relu6"""

    def __init__(self, case):
        m = pm.get_train_net(config.get_cfg(), TC.ARCH, backend='torch')
        m.load_state_dict({k: torch.from_numpy(v) for k, v in case['sd'].items()}, strict=False)
        self.m = m.double()

    def __call__(self, x):
        keep = torch.nn.functional.relu6
        torch.nn.functional.relu6 = _relu6
        try:
            return self.m(x)
        finally:
            torch.nn.functional.relu6 = keep

    def __getattr__(self, name):
        return getattr(self.m, name)

    def train(self):
        self.m.train()
        return self

    def eval(self):
        self.m.eval()
        return self


def _reference(case):
    return _Reference(case)


def _same_masks(what, mine, theirs):
    """the NaN masks agree, tensor by tensor"""
    for (k, a), (k2, b) in zip(mine, theirs):
        assert k == k2
        if a is None or not a.is_floating_point():
            continue
        ma, mb = torch.isnan(a.detach()).cpu(), torch.isnan(b.detach())
        assert torch.equal(ma, mb), '%s %s: %d NaN on the device, %d in the fp64 module' % (what, k, int(ma.sum()), int(mb.sum()))


@pytest.mark.parametrize('name, idx', PIXELS, ids=[p[0] for p in PIXELS])
def test_module_in_train_mode(setup, name, idx):
    """masks of both outputs, every gradient and every BatchNorm buffer"""
    case = setup['case']
    x = NF.inject(torch.from_numpy(case['x']), idx, NF.NAN)
    ups = [torch.from_numpy(case['up%d' % s]) for s in range(2)]
    ref = _reference(case).train()
    outs_r = ref(x.double())
    torch.autograd.backward(outs_r, [u.double() for u in ups])
    m = _module(case)
    outs = m(x.cuda())
    torch.autograd.backward(outs, [u.cuda() for u in ups])
    _same_masks('output', enumerate(outs), enumerate(outs_r))
    _same_masks('gradient', [(k, p.grad) for k, p in m.named_parameters()], [(k, p.grad) for k, p in ref.named_parameters()])
    _same_masks('buffer', m.named_buffers(), ref.named_buffers())
    assert all(bool(torch.isnan(o).any()) for o in outs_r)
    assert any(bool(torch.isnan(b).any()) for k, b in ref.named_buffers() if k.endswith('running_var'))


@pytest.mark.parametrize('name, idx', PIXELS, ids=[p[0] for p in PIXELS])
def test_module_in_eval_mode(setup, name, idx):
    """the cone is the receptive field of the pixel: a layer that scrubs shows as a smaller mask, one that reads a
    neighbour it then multiplies by zero as a larger one"""
    case = setup['case']
    x = NF.inject(torch.from_numpy(case['x']), idx, NF.NAN)
    with torch.no_grad():
        outs_r = _reference(case).eval()(x.double())
        m = _module(case).eval()
        outs, clean = m(x.cuda()), m(torch.from_numpy(case['x']).cuda())
    _same_masks('output', enumerate(outs), enumerate(outs_r))
    for o, c, r in zip(outs, clean, outs_r):
        mask = torch.isnan(r)
        assert bool(mask.any()) and not bool(mask[1 - idx[0]].any())           # the other image is clean ...
        assert NF.bitwise(o[1 - idx[0]], c[1 - idx[0]])                        # ... to the bit
        assert bool(torch.isfinite(c).all())


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'captured'])
@pytest.mark.parametrize('which', ['adam', 'sgd'])
def test_do_train_carries_a_nan_batch(setup, which, graph):
    """Two clean batches, one with a NaN pixel, a clean one (captured: an eager step, the capture, two replays).  The bad
    batch reports NaN loss terms; after its optimizer step the parameters are NaN where the fp64 module's are after a step
    on the same image -- the loss there is the sum of the squared outputs, whose gradient at an output is a multiple of that
    output, as the heatmap term's is --; the clean batch after it still trains a NaN model."""
    cfg, case = setup['cfg'], setup['case']
    m = _module(case)
    mk = (lambda ps: optim.Adam(ps, lr=1e-3)) if which == 'adam' else (lambda ps: optim.SGD(ps, lr=1e-3, momentum=0.9))
    opt = mk(m.parameters())
    factory = MultiLossFactory(cfg)
    stepper = CapturedStep(cfg, m, factory, opt) if graph else False
    batches = [tuple(b) for b in setup['batches'][:4]]
    bad_images = batches[2][0].clone()
    bad_images[0, 0, 0, 0] = NF.NAN
    batches[2] = (bad_images,) + batches[2][1:]
    got = [do_train(cfg, m, _loader([b], False), factory, opt, 0, None, None, stepper) for b in batches]
    torch.cuda.synchronize()
    if graph:
        assert (stepper.captures, stepper.replays, stepper.eager_steps) == (1, 3, 1)

    def terms(g):
        return [v[0] for vals in g.values() for v in vals if v is not None]

    assert terms(got[0]) and all(np.isfinite(terms(got[0]))) and all(np.isfinite(terms(got[1])))
    assert all(np.isnan(terms(got[2]))), got[2]
    assert all(np.isnan(terms(got[3]))), got[3]
    ref = _reference(case).train()
    ropt = (torch.optim.Adam(ref.parameters(), lr=1e-3) if which == 'adam'
            else torch.optim.SGD(ref.parameters(), lr=1e-3, momentum=0.9))
    for b in batches[2:]:
        ropt.zero_grad()
        sum((o * o).sum() for o in ref(b[0].cpu().double())).backward()
        ropt.step()
    _same_masks('parameter', m.named_parameters(), ref.named_parameters())
    _same_masks('buffer', m.named_buffers(), ref.named_buffers())
    assert all(bool(torch.isnan(p).all()) for p in ref.parameters())
