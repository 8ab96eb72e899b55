"""pose_simplenet (reference lib/models/pose_simplenet.py: LitePose without the Fusion Deconv Head) without a GPU: the CPU
restatement against the reference goldens, the library's key scheme of a ``plain_head`` net, strict loading in both
directions, the reference's simplenet.yaml through update_config, and the range check of ``lp_arch.plain_head``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _simplenet_ref as snr
from conftest import ROOT
from oracle import synth

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_simplenet.npz')
YAML = os.path.join(ROOT, 'tests', 'golden', 'simplenet.yaml')
CASES = [('search-XS', (64, 64)), ('search-S', (64, 64)), ('search-M', (96, 160))]


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _cfg():
    from litepose_amd import config
    return config.get_cfg('crowd_pose')


@pytest.mark.parametrize('arch_name,hw', CASES)
def test_restatement_reproduces_the_reference_samples(golden, arch_name, hw):
    from litepose_amd import arch_zoo
    torch.set_num_threads(1)
    arch = arch_zoo.get(arch_name)
    sd = snr.make_state_dict(arch, seed=1234)
    H, W = hw
    x = synth.make_images(1, H, seed=11, w=W)
    with torch.no_grad():
        out = snr.forward(x, sd, arch)
    for k, t in enumerate(out):
        key = '%s_%dx%d_out%d' % (arch_name, H, W, k)
        assert tuple(t.shape) == tuple(golden[key + '_shape'])
        np.testing.assert_allclose(t.numpy().reshape(-1)[::13], golden[key + '_sample'], rtol=0, atol=1e-6)
        a = t.numpy().astype(np.float64)
        np.testing.assert_allclose([a.sum(), np.abs(a).sum(), (a * a).sum(), a.flat[::97].sum()],
                                   golden[key + '_stats'], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('arch_name', ['search-XS', 'search-S', 'search-M'])
def test_plain_head_key_list_equals_the_reference_module(golden, arch_name):
    """lp_net_num_keys / lp_net_key of a plain_head net == the reference pose_simplenet state_dict() keys, in
    registration order; the shapes are the restatement's."""
    from litepose_amd import arch_zoo
    import litepose_amd.models as models
    arch = arch_zoo.get(arch_name)
    m = models.pose_simplenet.get_pose_net(_cfg(), cfg_arch=arch)
    keys = m.keys()
    assert [k for k, _ in keys] == [str(k) for k in golden[arch_name + '_keys']]
    assert dict(keys) == dict(snr.state_dict_shapes(arch))
    assert not any(k.startswith(('deconv_raw.', 'final_raw.')) for k, _ in keys)
    # the pose_mobilenet net of the same arch keeps its raw branches
    mob = [k for k, _ in models.pose_mobilenet.get_pose_net(_cfg(), cfg_arch=arch).keys()]
    assert set(mob) - {k for k, _ in keys} == {k for k in mob if k.startswith(('deconv_raw.', 'final_raw.'))}


def test_strict_load_refuses_the_other_network():
    from litepose_amd import arch_zoo
    import litepose_amd.models as models
    arch = arch_zoo.get('search-XS')
    mob_sd = synth.make_state_dict(arch, seed=1234)
    simple_sd = snr.make_state_dict(arch, seed=1234)
    with pytest.raises(RuntimeError, match='unexpected'):
        models.pose_simplenet.get_pose_net(_cfg(), cfg_arch=arch).load_state_dict(mob_sd, strict=True)
    with pytest.raises(RuntimeError, match='missing'):
        models.pose_mobilenet.get_pose_net(_cfg(), cfg_arch=arch).load_state_dict(simple_sd, strict=True)


def test_update_config_reads_simplenet_yaml():
    """The reference's experiments/crowd_pose/simplenet/simplenet.yaml (a settings-only copy), unchanged."""
    from litepose_amd import config

    class Args(object):
        cfg = YAML
        opts = []
    cfg = config.update_config(config.get_cfg('crowd_pose'), Args())
    assert cfg.MODEL.NAME == 'pose_simplenet'
    assert cfg.DATASET.INPUT_SIZE == 512 and list(cfg.DATASET.OUTPUT_SIZE) == [128, 256]
    assert list(cfg.MODEL.EXTRA.NUM_DECONV_KERNELS) == [4, 4, 4]
    assert cfg.MODEL.NUM_JOINTS == 14 and cfg.LOSS.WITH_AE_LOSS == [True, False]
    # literal strings decode as yacs decodes them: the inference path accepts the stage layout
    assert cfg.TEST.WITH_AE == (True, False) and cfg.TEST.WITH_HEATMAPS == (True, True) and cfg.GPUS == (0,)
    from litepose_amd.core import inference
    inference._check_cfg(cfg)


@pytest.mark.parametrize('value', [-1, 2, 7])
def test_plain_head_out_of_range_is_refused(value):
    from litepose_amd import _native as nv, arch_zoo
    from litepose_amd.models import pose_mobilenet
    a = pose_mobilenet._arch_struct(_cfg(), arch_zoo.get('search-XS'))
    a.plain_head = value
    h = C.c_void_p()
    rc = nv.lib().lp_net_create(C.byref(h), C.byref(a))
    assert rc == -1 and not h.value, rc                    # LP_ERR_INVALID_ARG
    assert b'plain_head' in nv.lib().lp_last_error()
