"""The supernet (litepose_amd.models.pose_supermobilenet) without a GPU: slicing against the reference goldens
(tests/golden/gen_golden_supernet.py), the window transform of 5x5 / 3x3 blocks, the key-scheme refusals, the samplers of
the arch manager, and the refusals of the lp_calib_* entry points that need no device."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import _supernet_ref as sr
from conftest import ROOT
from oracle import spec, synth

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_supernet.npz')
ARCHS = sr.golden_archs()


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _cfg():
    from litepose_amd import config
    return config.get_cfg('crowd_pose')


def _super(seed=sr.SEED):
    from litepose_amd.models import pose_supermobilenet as psm
    m = psm.get_pose_net(_cfg(), is_train=False)
    m.load_state_dict(sr.make_state_dict(seed), strict=True)
    return m


def test_key_scheme_is_the_reference_modules(golden):
    from litepose_amd.models import pose_supermobilenet as psm
    m = psm.SuperLitePose(_cfg())
    assert [k for k, _ in m.keys()] == [str(k) for k in golden['keys']]
    assert dict(m.keys()) == dict(sr.state_dict_shapes())
    assert any('.Linear5x5.' in k for k, _ in m.keys()) and any('.Linear3x3.' in k for k, _ in m.keys())
    # module. prefixes (DataParallel checkpoints) load like the other wrappers'
    m.load_state_dict({'module.' + k: v for k, v in sr.make_state_dict().items()}, strict=True)
    assert torch.equal(m.state_dict()['stage.0.0.Linear3x3.bias'], sr.make_state_dict()['stage.0.0.Linear3x3.bias'])


@pytest.mark.parametrize('ai', range(len(ARCHS)), ids=[n for n, _ in ARCHS])
def test_slices_load_strictly_and_reproduce_the_reference_eval_outputs(golden, ai):
    """sub_state_dict == the restatement's slices bit for bit; it loads strictly into pose_mobilenet (key list and
    shapes of the handle); the oracle network on it gives the reference module's pre-calibration eval outputs of the
    FIRST architecture of the fixture bit for bit at one thread (later ones start from calibrated statistics: those are
    replayed on the device, tests/test_gpu_supernet.py) -- and for every architecture the outputs of a fresh supernet
    equal the restatement's."""
    import litepose_amd.models as models
    torch.set_num_threads(1)
    name, arch = ARCHS[ai]
    m = _super()
    sub = m.sub_state_dict(arch)
    ref = sr.sub_state_dict(sr.make_state_dict(), arch)
    assert list(sub) == list(ref) == list(spec.state_dict_shapes(arch))
    for k in sub:
        assert torch.equal(sub[k], ref[k]), k
    net = models.pose_mobilenet.get_pose_net(_cfg(), cfg_arch=arch)
    assert dict(net.keys()) == {k: tuple(v.shape) for k, v in sub.items()}
    H, W = sr.CASES[0]
    x = synth.make_images(2, H, seed=11, w=W)
    with torch.no_grad():
        out = sr.eval_forward(x, sub, arch)
    if ai == 0:
        for k, t in enumerate(out):
            key = '%dx%d_%s_pre%d' % (H, W, name, k)
            assert tuple(t.shape) == tuple(golden[key + '_shape'])
            assert np.array_equal(t.numpy().reshape(-1)[::13], golden[key + '_sample'])


def test_sequence_of_restatement_calibrations_reproduces_every_golden_eval_output(golden):
    """All three architectures in fixture order on one supernet, calibrated by the CPU restatement (which the generator
    pinned to the reference bit for bit): the oracle network on ``sub_state_dict`` of a SuperLitePose that received the
    moved statistics gives the golden's pre- and post-calibration eval outputs of every architecture, bitwise."""
    torch.set_num_threads(1)
    H, W = sr.CASES[0]
    m = _super()
    sd = sr.make_state_dict()
    xe = synth.make_images(2, H, seed=11, w=W)
    for ai, (name, arch) in enumerate(ARCHS):
        views = sr.sub_state_dict(sd, arch)
        for which in ('pre', 'post'):
            m.load_state_dict(sd, strict=True)                # the supernet as the restatement has moved it so far
            with torch.no_grad():
                out = sr.eval_forward(xe, m.sub_state_dict(arch), arch)
            for k, t in enumerate(out):
                key = '%dx%d_%s_%s%d' % (H, W, name, which, k)
                assert np.array_equal(t.numpy().reshape(-1)[::13], golden[key + '_sample']), key
            if which == 'pre':
                with torch.no_grad():
                    for step in range(sr.STEPS):
                        sr.train_forward(sr.step_images(H, W, ai, step), views, arch)
                got, _ = sr.pack_pairs(sr.pairs_of(views, arch), arch)
                assert np.array_equal(got.astype(np.float32), golden['%dx%d_%s_pairs' % (H, W, name)][-1])


def test_window_transform_differs_from_cropping_and_matches_the_reference(golden):
    H, W = sr.CASES[0]
    m = _super()
    name, arch = ARCHS[2]
    sub = m.sub_state_dict(arch)
    full = m.state_dict()
    for k in (5, 3):
        s, b = [int(v) for v in golden['%dx%d_window_k%d_block' % (H, W, k)]]
        assert arch['backbone_setting'][s]['block_setting'][b][1] == k
        key = 'stage.%d.%d.depth_conv.0.weight' % (s, b)
        w = sub[key]
        assert tuple(w.shape[2:]) == (k, k)
        assert np.array_equal(w.numpy(), golden['%dx%d_window_k%d' % (H, W, k)])
        l, r = 3 - k // 2, 3 + k // 2 + 1
        crop = full[key][:w.shape[0], :, l:r, l:r]
        assert float((w - crop).abs().max()) > 1e-3, 'the Linear%dx%d transform was not applied' % (k, k)


def test_refuses_a_pose_mobilenet_checkpoint_and_archs_beyond_the_supernet():
    from litepose_amd import arch_zoo
    from litepose_amd.models import pose_supermobilenet as psm
    m = psm.SuperLitePose(_cfg())
    with pytest.raises(RuntimeError, match='missing'):
        m.load_state_dict(synth.make_state_dict(arch_zoo.get('search-XS')), strict=True)
    with pytest.raises(RuntimeError, match='missing'):       # Linear* keys are part of the scheme even when not strict
        m.load_state_dict({k: v for k, v in sr.make_state_dict().items() if '.Linear' not in k}, strict=False)
    bad = sr.make_state_dict()
    bad['stage.0.0.inv.0.weight'] = bad['stage.0.0.inv.0.weight'][:64]
    with pytest.raises(RuntimeError, match='size mismatch'):
        m.load_state_dict(bad, strict=True)
    m = _super()
    wide = sr.fixed_sample(ratio=1.0)
    wide['backbone_setting'][1]['channel'] = 72
    with pytest.raises(ValueError, match='wider than the supernet'):
        m.sub_state_dict(wide)
    wide = sr.fixed_sample(ratio=1.0)
    wide['deconv_setting'][0] = 72
    with pytest.raises(ValueError, match='wider than the supernet'):
        m.sub_state_dict(wide)
    deep = sr.fixed_sample(ratio=0.5)
    deep['backbone_setting'][0]['num_blocks'] = 7
    deep['backbone_setting'][0]['block_setting'] = [[6, 7]] * 7
    with pytest.raises(ValueError, match='supernet holds 6'):
        m.sub_state_dict(deep)
    with pytest.raises(Exception, match='load_state_dict'):
        psm.SuperLitePose(_cfg()).sub_state_dict(sr.fixed_sample())


def test_arch_manager_tables_and_samplers():
    from litepose_amd.models import pose_supermobilenet as psm
    am = psm.SuperLitePose(_cfg()).arch_manager
    assert am.fixed_sample(ratio=0.5) == sr.fixed_sample(ratio=0.5)
    assert am.fixed_sample(320, 1.0) == sr.fixed_sample(320, 1.0)
    assert am.width_mult == [1.0, 0.75, 0.5, 0.25] and am.arch_setting == [[32, 4, 2], [64, 6, 2], [96, 8, 2], [160, 8, 1]]
    assert am.is_search is False and am.search_arch is None
    random.seed(5)
    m = _super()
    for _ in range(20):
        a = am.random_sample()
        assert a['img_size'] in (256, 320, 384, 448, 512)
        assert all(st['block_setting'] == [[6, 7]] * st['num_blocks'] for st in a['backbone_setting'])
        m.sub_state_dict(a)                                 # every sample is a sub-network of the supernet
    am.is_search, am.search_arch = True, sr.mixed_arch()
    assert am.random_sample() == sr.mixed_arch()


# ---------------------------------------------------------------- ABI refusals that need no GPU
def _handle_with_weights(arch):
    from litepose_amd import _native as nv
    from litepose_amd.models import pose_mobilenet
    net = pose_mobilenet.get_pose_net(_cfg(), cfg_arch=arch)
    lib = nv.lib()
    for k, v in synth.make_state_dict(arch).items():
        if k.endswith('num_batches_tracked'):
            assert lib.lp_net_set_weight(net._h, k.encode(), None, None, 0) == 0
            continue
        t = v.contiguous()
        shp = (C.c_int64 * max(1, t.dim()))(*t.shape)
        assert lib.lp_net_set_weight(net._h, k.encode(), C.c_void_p(t.data_ptr()), shp, t.dim()) == 0, k
    return net, lib


def test_calib_abi_refusals():
    from litepose_amd import arch_zoo
    import litepose_amd.models as models
    arch = arch_zoo.get('search-XS')
    net, lib = _handle_with_weights(arch)
    fake = C.c_void_p(1 << 20)                              # never dereferenced: every call below is refused first
    steps = C.c_int64(-1)
    # before begin
    assert lib.lp_calib_step(net._h, fake, 4, 64, 64, fake, 1 << 30, None) == -5
    assert b'lp_calib_begin' in lib.lp_last_error()
    assert lib.lp_calib_workspace_bytes(net._h, 4, 64, 64) == 0
    assert lib.lp_calib_end(net._h, C.byref(steps)) == -5
    assert lib.lp_calib_read(net._h, b'first.3', fake, fake, 16, None) == -5
    # null pointers, momentum
    assert lib.lp_calib_begin(None, 0.1) == -1
    assert lib.lp_calib_begin(net._h, 1.5) == -1
    # a handle with a weight missing
    bare = models.pose_mobilenet.get_pose_net(_cfg(), cfg_arch=arch)
    assert lib.lp_calib_begin(bare._h, 0.1) == -4
    # 16-bit storage and the pose_resnet family
    for storage in (1, 2):
        assert lib.lp_net_set_storage(net._h, storage) == 0
        assert lib.lp_calib_begin(net._h, 0.1) == -8
        assert b'fp32 storage only' in lib.lp_last_error()
    assert lib.lp_net_set_storage(net._h, 0) == 0
    import _resnet_ref as rr
    res = models.pose_resnet.get_pose_net(rr.variant_cfg(_cfg(), kernel=3))
    assert res._arch.family == 1
    assert lib.lp_calib_begin(res._h, 0.1) == -8
    # an open calibration: sizes, null pointers, workspace
    assert lib.lp_calib_begin(net._h, 0.1) == 0
    need = lib.lp_calib_workspace_bytes(net._h, 4, 64, 64)
    assert need > 0 and need % 256 == 0
    assert lib.lp_calib_workspace_bytes(net._h, 4, 64, 72) == 0 and b'multiples of 16' in lib.lp_last_error()
    assert lib.lp_calib_workspace_bytes(net._h, 0, 64, 64) == 0 and b'N must be positive' in lib.lp_last_error()
    # the handle's tensors and storage are frozen while the calibration is open
    w = torch.zeros(32, 3, 3, 3)
    shp = (C.c_int64 * 4)(*w.shape)
    assert lib.lp_net_set_weight(net._h, b'first.0.0.weight', C.c_void_p(w.data_ptr()), shp, 4) == -1
    assert b'calibration is open' in lib.lp_last_error()
    assert lib.lp_net_set_storage(net._h, 1) == -1 and lib.lp_net_get_storage(net._h) == 0
    assert lib.lp_calib_step(net._h, None, 4, 64, 64, fake, need, None) == -1
    assert lib.lp_calib_step(net._h, fake, 4, 64, 64, None, need, None) == -1
    assert lib.lp_calib_step(net._h, fake, 0, 64, 64, fake, need, None) == -1
    assert lib.lp_calib_step(net._h, fake, 4, 64, 72, fake, need, None) == -1
    assert lib.lp_calib_step(net._h, fake, 1, 16, 16, fake, 1 << 30, None) == -1        # one value per channel
    assert lib.lp_calib_step(net._h, fake, 4, 64, 64, fake, need - 1, None) == -6
    assert lib.lp_calib_step(net._h, fake, 4, 64, 64, C.c_void_p((1 << 20) + 64), need, None) == -6     # misaligned
    assert lib.lp_calib_read(net._h, None, fake, fake, 16, None) == -1
    assert lib.lp_calib_read(net._h, b'first.3', None, fake, 16, None) == -1
    assert lib.lp_calib_read(net._h, b'first.2', fake, fake, 16, None) == -2
    assert lib.lp_calib_read(net._h, b'first.3', fake, fake, 24, None) == -3
    # closing a calibration in which no step ran changes nothing and needs no device
    assert lib.lp_calib_end(net._h, C.byref(steps)) == 0 and steps.value == 0
    assert lib.lp_calib_step(net._h, fake, 4, 64, 64, fake, need, None) == -5
    assert lib.lp_net_set_weight(net._h, b'first.0.0.weight', C.c_void_p(w.data_ptr()), shp, 4) == 0
