"""The strip form of mbt_kernel (round 7; mbtile_kernels.hip, option "mbt_strip"): planes 32 wide as 32-wide x 16-row
strips, one 8-wave workgroup per strip, against the 16x16-tile form -- bit for bit on every stage-1 tap and both outputs
-- and against the oracle; the launch geometry and the default rule.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

from oracle import net_ref, synth
from test_gpu_real_shapes import OUT_ATOL, _model

pytestmark = pytest.mark.gpu

TAPS = ['stage.1.%d' % b for b in range(8)]


def _run(m, x, flip, strip):
    m.set_option('mbt_strip', strip)
    try:
        m.set_profiling(True)
        out = [o.clone() for o in m.forward_native(x, flip)]
        prof = m.profile(launches=True)
        m.set_profiling(False)
        taps = {k: m.tap(k).clone() for k in TAPS}
    finally:
        m.set_option('mbt_strip', 1)
    return out, taps, prof


def _stage1(prof):
    return [(p[0], p[5][0]) for p in prof if p[0].startswith('stage.1.') and p[0].endswith('|mbt_kernel')]


@pytest.fixture(scope='module')
def xs():
    return _model('search-XS')


@pytest.fixture(scope='module')
def oracle_256(xs):
    m, arch, sd = xs
    x = synth.make_images(2, 256, seed=77, w=256)
    with torch.no_grad():
        return [o.numpy() for o in net_ref.forward(x, sd, arch)]


# 16x32 plane: one strip with both image borders; 32x32: a top and a bottom strip; 48x32: a middle strip without a border
# row; 18x32: a ragged second strip of 2 rows
@pytest.mark.parametrize('flip', [0, 2])
@pytest.mark.parametrize('H', [128, 256, 384, 144])
def test_strip_form_is_bitwise_the_tile_form(xs, oracle_256, H, flip):
    m, arch, sd = xs
    N, W = 2, 256
    x = synth.make_images(N, H, seed=77, w=W).cuda()
    out_s, tap_s, prof_s = _run(m, x, flip, 2)
    out_t, tap_t, prof_t = _run(m, x, flip, 0)
    assert [p[0] for p in prof_s] == [p[0] for p in prof_t]
    assert [p[2:5] for p in prof_s] == [p[2:5] for p in prof_t]          # bytes, FLOPs, vector share per launch
    s1, t1 = _stage1(prof_s), _stage1(prof_t)
    assert [n for n, _ in s1] == ['stage.1.%d.inv+depth_conv+point_conv|mbt_kernel' % b for b in range(1, 8)], s1
    nb, ph = N * (2 if flip == 2 else 1), H // 8
    assert [g for _, g in s1] == [nb * ((ph + 15) // 16)] * 7, s1
    assert [g for _, g in t1] == [nb * 2 * ((ph + 15) // 16)] * 7, t1
    diff = [k for k in TAPS if not torch.equal(tap_s[k], tap_t[k])]
    assert not diff, diff
    for a, b in zip(out_s, out_t):
        assert torch.equal(a, b)
    if H == 256 and flip == 0:
        for a, b in zip(out_s, oracle_256):
            np.testing.assert_allclose(a.cpu().numpy(), b, rtol=0, atol=OUT_ATOL)


def test_default_rule_takes_strips_when_they_fill_the_cus(xs):
    """"mbt_strip" = 1: 128 images x 2 strips = 256 launches of stage 1 against the device's CU count; 2 images never."""
    m, arch, sd = xs
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert m.get_option('mbt_strip') == 1
    for n, flip in ((2, 0), (128, 0)):
        x = synth.make_images(n, 256, seed=78, w=256).cuda()
        nb = n * (2 if flip == 2 else 1)
        _, _, prof = _run(m, x, flip, 1)
        grids = [g for _, g in _stage1(prof)]
        want = nb * 2 if nb * 2 >= cus else nb * 4
        assert grids == [want] * 7, (n, flip, cus, grids)
