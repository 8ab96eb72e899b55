"""``models.pose_mobilenet.TrainableLitePose`` without a GPU: its names and shapes against ``LitePose.keys()``, and its
``backend='torch'`` form against one training step of the real reference module (tests/golden/golden_train_net.npz,
tests/golden/gen_golden_train_net.py): fp64 against fp64 to 1e-12, fp32 no further from fp64 than the reference's own fp32."""
import numpy as np
import pytest
import torch

import _train_net_case as TC
from litepose_amd import _native as nv, arch_zoo, config
from litepose_amd.models import pose_mobilenet as pm


@pytest.fixture(scope='module')
def case():
    return TC.load()


def _keys(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def _step(case, dtype):
    torch.set_num_threads(1)
    m = pm.get_train_net(config.get_cfg(), TC.ARCH, backend='torch')
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case['sd'].items()}, strict=False)
    m.to(dtype).train()
    outs = m(torch.from_numpy(case['x']).to(dtype))
    sum((o * torch.from_numpy(case['up%d' % s]).to(dtype)).sum() for s, o in enumerate(outs)).backward()
    grads = {k: p.grad.numpy() for k, p in m.named_parameters()}
    return m, [o.detach().numpy() for o in outs], grads, {k: v.numpy() for k, v in m.state_dict().items()}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize('name', ['tiny'] + arch_zoo.names())
def test_names_and_shapes_are_those_of_the_engine(name):
    arch = TC.ARCH if name == 'tiny' else arch_zoo.get(name)
    cfg = config.get_cfg()
    m = pm.get_train_net(cfg, arch, backend='torch')
    assert isinstance(m, torch.nn.Module) and isinstance(m, pm.TrainableLitePose)
    assert _keys(m) == pm.LitePose(cfg, cfg_arch=arch).keys()
    assert [n for n, _ in m.named_buffers()] == [k for k, _ in _keys(m) if not k.endswith(('weight', 'bias'))]


def test_golden_keys_are_the_modules(case):
    m = pm.get_train_net(config.get_cfg(), TC.ARCH, backend='torch')
    assert _keys(m) == [(k, case['shapes'][k]) for k in case['keys']]
    assert [k for k, _ in m.named_parameters()] == case['params']
    assert m.final_channel == list(TC.HEADS)


def test_torch_backend_fp64_reproduces_the_reference_step(case):
    """The same arithmetic as the reference module in fp64; BLAS may reorder sums: 1e-12 relative per tensor."""
    _, outs, grads, sd = _step(case, torch.float64)
    for s in range(2):
        assert _rel(outs[s], case['out%d_64' % s]) <= 1e-12, s
    for k in case['params']:
        assert _rel(grads[k], case['grad_64'][k]) <= 1e-12, k
    for k in case['buffers']:
        assert _rel(sd[k], case['run_64'][k]) <= 1e-12, k
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith('num_batches_tracked'))


def test_torch_backend_fp32_is_as_close_to_fp64_as_the_reference(case):
    """Per tensor, the fp32 step's distance from the fp64 step is no larger than the reference's own, stored beside it
    (the same torch ops in the same order: in practice the same bits)."""
    _, outs, grads, sd = _step(case, torch.float32)
    for s in range(2):
        assert _rel(outs[s], case['out%d_64' % s]) <= _rel(case['out%d_32' % s], case['out%d_64' % s]), s
    for k in case['params']:
        assert _rel(grads[k], case['grad_64'][k]) <= _rel(case['grad_32'][k], case['grad_64'][k]), k
    for k in case['buffers']:
        assert _rel(sd[k], case['run_64'][k]) <= _rel(case['run_32'][k], case['run_64'][k]), k


def test_state_dict_round_trips_with_the_engine(case):
    cfg = config.get_cfg()
    m = pm.get_train_net(cfg, TC.ARCH, backend='torch')
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case['sd'].items()}, strict=False)
    eng = pm.LitePose(cfg, cfg_arch=TC.ARCH)
    try:
        eng.load_state_dict(m.state_dict())
    except nv.LitePoseNativeError as e:         # without a GPU every weight is set and only the upload that follows fails
        assert 'lp_net_finalize' in str(e)
    back = eng.state_dict()
    m2 = pm.get_train_net(cfg, TC.ARCH, backend='torch')
    m2.load_state_dict(back)                                    # strict: every key, no other
    for k, v in m.state_dict().items():
        if not k.endswith('num_batches_tracked'):
            assert torch.equal(m2.state_dict()[k], v), k


def test_backend_is_checked():
    with pytest.raises(ValueError):
        pm.get_train_net(config.get_cfg(), TC.ARCH, backend='eager')
