"""The strip form of mbt_kernel (mbtile_kernels.hip, option "mbt_strip") without a GPU: its LDS layout in the bank model
of tools/lds_model.py, and the option's range on a handle that never touches the device."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lds_model():
    spec = importlib.util.spec_from_file_location('lds_model', os.path.join(ROOT, 'tools', 'lds_model.py'))
    lm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lm)
    return lm


def test_strip_layout_is_conflict_free_in_the_bank_model():
    """[16 pairs][22 rows][42 cells][2 ch], 463 slots per pair: the 96 depthwise row reads of a wave's two passes as
    ds_read_b128, the project's operand reads of all eight waves, the depthwise result and the expand's writes each cost
    exactly the conflict-free cycle count.  One pair per pass -- the lane map that looks natural for a strip -- does not:
    every slot it touches is even."""
    m = _lds_model().mbt_strip()
    assert m['depthwise rows of both passes as 96 ds_read_b128'] == (384, 384)
    assert m['project operands of the 8 waves, 128 ds_read_b64'] == (256, 256)
    assert m['depthwise result, 8 ds_write_b128'] == (64, 64)
    assert m['expand result of three rows, 24 ds_write_b64'] == (96, 96)
    got, free = m['the same with one pair per pass (every slot even: not built)']
    assert free == 384 and got >= 2 * free, (got, free)


def test_strip_lane_map_covers_every_block_once():
    """Per pass the 64 lanes are 2 pairs x 4 row pairs x 8 strips, each once."""
    lm = _lds_model()
    seen = sorted(lm.mbt_strip_lane(lane) for lane in range(64))
    assert seen == sorted((p, r, s) for p in range(2) for r in range(4) for s in range(8))


def test_strip_tile_fits_the_lds_next_to_the_weight_stage():
    """E tile + mbt_kernel's weight stage of the widest variant launch_mbt knows (CK = 3, NMT = 2) under 160 KB."""
    e_bytes = 16 * (22 * 42 * 2 + 4) * 4
    assert (22 * 42 * 2 + 4) % 8 == 4                               # an odd count of 16-byte slots per pair
    assert (42 * 2) % 8 == 4                                        # ... and per row
    ck, nmt = 3, 2
    ntot = ck * 3 * 64 + nmt * 2 * 3 * 64 + 64 + 16 * 28
    assert e_bytes + (ntot + 16 * 28) * 16 <= 160 * 1024


def test_option_mbt_strip_range():
    from litepose_amd import _native as nv
    from litepose_amd import arch_zoo, config
    from litepose_amd.models import pose_mobilenet
    m = pose_mobilenet.get_pose_net(config.get_cfg('crowd_pose'), is_train=False, cfg_arch=arch_zoo.get('search-XS'))
    assert m.get_option('mbt_strip') == 1
    for v in (0, 2, 1):
        m.set_option('mbt_strip', v)
        assert m.get_option('mbt_strip') == v
    for v in (-1, 3):
        with pytest.raises(nv.LitePoseNativeError):
            m.set_option('mbt_strip', v)
        assert m.get_option('mbt_strip') == 1
