"""Every fp32 network kernel form, per element, against float64 on the device's own inputs (tests/_fp32_units.py).
Needs a real MI355X.

One row per census row named in ``ROWS`` -- the rows are taken from the census tables BY ID (tests/
test_gpu_kernel_census.py CASES, tests/_custom_space.py, tests/_mbt_space.py, tests/_subnet_space.py), so that no form
is restated here -- at the smallest rows that still select each form.  A row runs the census row's forward (a row that
needs 48 images to pass mb16_kernel's gate runs the 48) and then every unit of the net on at most THREE images: the
first, the first of the mirrored half and the last.  Per unit and image, with e = |device - float64 unit|:
  P   e <= c_max u B at every element (B: the unit's first-order error magnitude);
  R   rms(e / B) <= m rms(|fp32 torch unit - float64 unit| / B).
c_max and m come from tests/test_fp32_units_cpu.py (an emulation on the CPU and mutants of it), never from a device.
test_every_fp32_tag_is_unit_checked: every fp32 tag the sources name was launched by some row here, except the
NOT_REACHED entries that no custom architecture reaches either (tests/_custom_space.py UNREACHABLE).
test_small_magnitudes: search-XS at 64 x 64 with the output heads' weights scaled by 2^-12, and the same net with every
project BatchNorm weight scaled by 2^-8 -- outputs and block updates of about 1e-4, where the absolute criteria of
check_fp32 see nothing; P and R hold at the same constants, and the scaled heads give the unscaled outputs times 2^-12
bit for bit (a power of two commutes with the three-way split).

In the second net the blocks are checked against the class 'block_small' of the CPU test: with B close to |ref| the
rounding of the final add alone is up to 0.5 u B, and the pessimistic emulation of a correct kernel reaches 0.84 there.

Measured on an MI355X, every row passing as the kernels stood -- no form is outside P or R.  "P": the worst element as a
fraction of c_max of its kind, "R": the worst tap as a fraction of m (m = 13: R 0.13 is 1.7 times the error of plain
fp32 torch); in brackets the unit.  All 29 fp32 tags are launched by some row except dw_kernel<7,1>, <5,1>, <3,1>
(NOT_REACHED and UNREACHABLE: only a launch of 131071 images takes them).
  row              input      N f  units   P                   R                   s    forms the row adds
  mb16_nb48_flip   256x256   24 2   40    0.478 (final.1)     0.131 (deconv.0)    0.7  stem4 mbconv2 mbt_s2 mbt mb16 headfuse deconv4 deconv4x3
  xs_native_f32    256x256    3 0   40    0.465 (final.1)     0.129 (deconv.1)    0.4  dw_pair16<7> pw3d
  xs16_f32         16x16      3 2   40    0.453 (stage.3.1)   0.151 (stage.2.0)   0.1  dw_kernel<7,2> dw_pair<5> dw_pair<7> pw2
  s208x336_f32     208x336    3 2   40    0.397 (final.1)     0.121 (deconv.1)    0.7
  opt_mbt0         256x256    2 0   40    0.520 (final.1)     0.128 (deconv.1)    0.4  dwpw
  opt_mbt2         256x256    2 0   40    0.522 (final.1)     0.128 (deconv.1)    0.4
  opt_mbt3         256x256    2 0   40    0.448 (final.1)     0.129 (deconv.1)    0.4
  opt_mbt_s2_0     256x256    2 0   40    0.468 (final.1)     0.128 (deconv.1)    0.4
  opt_mbconv2_0    256x256    2 0   40    0.426 (final.1)     0.128 (deconv.1)    0.4
  opt_pw3d0        256x256    2 0   40    0.492 (final.1)     0.128 (deconv.1)    0.4  pw3
  opt_pw3d2        256x256    2 0   40    0.492 (final.1)     0.140 (deconv.0)    0.5
  opt_stem0_f32    128x192    2 2   40    0.448 (final.1)     0.129 (deconv.1)    0.5  stem_kernel
  mb24_128         128x128    3 2   13    0.326 (final.1)     0.109 (deconv.0)    0.1  mbconv mbconv_s2
  five_128         128x128    3 2   12    0.288 (stem)        0.116 (deconv.1)    0.1  dw_kernel<3,2> dw_kernel<5,2>
  odd_64           64x64      3 2   14    0.282 (stem)        0.116 (stage.3.0)   0.1  deconv_mfma dw_pair16<5>
  pair66_64        64x64      3 2   14    0.284 (stem)        0.130 (deconv.0)    0.1  deconv_pair
  wide72_64        64x64      3 2   14    0.386 (final.1)     0.118 (stage.3.1)   0.1
  d4_256           256x256    3 2   14    0.434 (stem)        0.130 (deconv.0)    0.2
  ksize_256        256x256    3 2   19    0.479 (final.1)     0.133 (deconv.0)    0.2  dw_pair<3> dw_pair16<3>
  plain_mfma_64    64x64      3 2    9    0.282 (stem)        0.116 (stage.3.0)   0.1  (pose_simplenet: stem and blocks only)
  h17_s11F         272x512    3 0   11    0.447 (stage.0.0)   0.085 (deconv.1)    0.1  mbt strip
  h2_s21F          32x512     3 2   11    0.403 (stem)        0.105 (deconv.0)    0.1
  t17_32_64        272x272    2 2   10    0.369 (stage.0.0)   0.084 (deconv.0)    0.1  mbt tile
  t17_48_56        272x272    2 2   10    0.376 (stage.2.0)   0.105 (deconv.0)    0.1
  t00              256x256    3 0   32    0.437 (final.1)     0.128 (deconv.1)    0.3
  t07              512x512    1 2   32    0.366 (final.0)     0.142 (deconv.1)    0.7
  small: heads x 2^-12      |out| <= 3.1e-4   0.324 (final.1)     0.116 (stage.3.2)        outputs == plain x 2^-12, bitwise
  small: + project BN x 2^-8   <= 2.6e-4      0.494 (stage.2.7)   0.115 (deconv.1)   0.5
Over every check_fp32 call of the suite (233 calls): P at most 0.732 (prune_s_native_f32), R at most 0.170 (sub-network
row d10); the mbt_kernel rows 0.439 / 0.106, the dense k x k launches of pose_resnet 0.395 / 0.157 (m = 21)."""
import time

import pytest
import torch

import _custom_space as cs
import _fp32_units as fu
import _mbt_space as ms
import _subnet_space as sp
from oracle import synth

pytestmark = pytest.mark.gpu

# (table, row id): kc = test_gpu_kernel_census.CASES, cs = _custom_space.ROWS, ms = _mbt_space.ROWS, sp = _subnet_space.ROWS
ROWS = [
    ('kc', 'mb16_nb48_flip'),        # the bench forms: stem4, mbconv2, mbt_s2, mbt, mb16 (48 images in the launch), headfuse
    ('kc', 'xs_native_f32'),         # deconv4, deconv4x3
    ('kc', 'xs16_f32'),              # the smallest input: dw_pair<5> + pw2 heads, deconv4 on 1 x 1 planes
    ('kc', 's208x336_f32'),          # ragged planes, 120-channel blocks
    ('kc', 'opt_mbt0'), ('kc', 'opt_mbt2'), ('kc', 'opt_mbt3'), ('kc', 'opt_mbt_s2_0'), ('kc', 'opt_mbconv2_0'),
    ('kc', 'opt_pw3d0'), ('kc', 'opt_pw3d2'), ('kc', 'opt_stem0_f32'),
    ('cs', 'mb24_128'), ('cs', 'five_128'), ('cs', 'odd_64'), ('cs', 'pair66_64'), ('cs', 'wide72_64'), ('cs', 'd4_256'),
    ('cs', 'ksize_256'), ('cs', 'plain_mfma_64'),
    ('ms', 'h17_s11F'), ('ms', 'h2_s21F'), ('ms', 't17_32_64'), ('ms', 't17_48_56'),
    ('sp', 't00'), ('sp', 't07'),
]

COVERED = {}               # tag -> row ids that launched it and passed the unit check
RESULTS = {}               # row id -> (tags, worst P fraction, worst R fraction, seconds)


def _images_of(nb, n, flip):
    return sorted({0, nb - 1} | ({n} if flip == 2 else set()))


def _forward(table, rid):
    """The census row's own forward: (net, arch, sd, head, default forward?, x on the host, flip, outs, launches)."""
    from _net_check import profiled_forward, set_options
    if table == 'kc':
        import test_gpu_kernel_census as kc
        _, an, storage, H, W, N, flip, options, _ = kc._case_by_id()[rid]
        assert storage == 'f32', rid
        m, arch, sd = kc._net(an, 'f32')
        x = synth.make_images(N, H, seed=101 + N, w=W)
        old = set_options(m, options)
        try:
            outs, launches = profiled_forward(m, x.cuda(), flip)
        finally:
            set_options(m, old)
        return m, arch, sd, None, True, x, flip, outs, launches
    if table == 'cs':
        import test_gpu_custom_census as cc
        row = cs.row(rid)
        res = cc._forward(row, 'f32')
        assert not isinstance(res, str), (rid, res)
        m, arch, sd, head, plain, x, outs, launches = res
        return m, arch, sd, head, not plain, x, row[5], outs, launches
    if table == 'ms':
        import test_gpu_mbt_forms as mf
        r = ms.row(rid)
        m, arch, sd = mf._net(r[1])
        x = synth.make_images(r[4], r[2], seed=31, w=r[3])
        old = set_options(m, r[6])
        try:
            outs, launches = profiled_forward(m, x.cuda(), r[5])
        finally:
            set_options(m, old)
        assert (r[7], 'mbt_kernel') in launches, (rid, launches)
        return m, arch, sd, None, True, x, r[5], outs, launches
    import test_gpu_subnet_census as sc
    _, vec, H, W, N, flip = sc._ROW[rid]
    res = sc._forward(vec, 'f32', H, W, N, flip)
    assert not isinstance(res, str), (rid, res)
    m, arch, sd, x, outs, launches = res
    return m, arch, sd, None, True, x, flip, outs, launches


@pytest.mark.parametrize('table,rid', ROWS, ids=['%s-%s' % r for r in ROWS])
def test_row_units(table, rid):
    t0 = time.time()
    m, arch, sd, head, default, x, flip, outs, launches = _forward(table, rid)
    N = x.shape[0]
    xin = x if flip == 0 else (torch.flip(x, [3]) if flip == 1 else torch.cat([x, torch.flip(x, [3])]))
    rows = fu.check_device(m, sd, arch, xin, outs, _images_of(xin.shape[0], N, flip), head, heads=default)
    tags = sorted({t for _, t in launches})
    wp, wr = max(rows.items(), key=lambda kv: kv[1][0]), max(rows.items(), key=lambda kv: kv[1][1])
    RESULTS[rid] = (tags, wp[1][0], wr[1][1], time.time() - t0)
    for t in tags:
        COVERED.setdefault(t, []).append(rid)
    print('%-16s N=%d flip=%d %dx%d  %d units  P %.3f of c_max (%s)  R %.3f of m (%s)  %.1f s  %s'
          % (rid, N, flip, x.shape[2], x.shape[3], len(rows), wp[1][0], wp[0], wr[1][1], wr[0], time.time() - t0,
             ' '.join(tags)))


def fp32_tags():
    """The tags of the sources that an fp32 forward can launch: all of them but the ones only 16-bit rows expect."""
    import test_gpu_kernel_census as kc
    from test_kernel_census_cpu import source_tags
    f32 = set().union(*[set(c[8]) for c in kc.CASES if c[2] == 'f32'], *[set(r[7]) for r in cs.ROWS])
    b16 = set().union(*[set(c[8]) for c in kc.CASES if c[2] != 'f32'], *[set(r[8]) for r in cs.ROWS])
    return source_tags() - (b16 - f32)


def test_every_fp32_tag_is_unit_checked():
    import test_gpu_kernel_census as kc
    if not RESULTS:
        print('no row ran in this process, nothing to cover')
        return
    excused = set(kc.NOT_REACHED) & set(cs.UNREACHABLE)
    missing = sorted(fp32_tags() - set(COVERED) - excused)
    for t in sorted(COVERED):
        print('  %-22s %s' % (t, ' '.join(COVERED[t])))
    if len(RESULTS) == len(ROWS):
        assert not missing, ('fp32 tags no row launched and unit-checked', missing)


def _xs(head_gain, project_scale):
    from _net_check import _cfg
    from litepose_amd import arch_zoo
    from litepose_amd.models import pose_mobilenet
    arch = arch_zoo.get('search-XS')
    sd = synth.make_state_dict(arch, seed=1234, head_gain=head_gain)
    if project_scale != 1.0:
        for k in sd:
            if k.endswith('.point_conv.1.weight'):
                sd[k] = sd[k] * project_scale
    m = pose_mobilenet.get_pose_net(_cfg(), is_train=False, cfg_arch=arch, storage='f32')
    m.load_state_dict(sd, strict=True)
    return m, arch, sd


def test_small_magnitudes():
    t0 = time.time()
    N, flip = 2, 2
    x = synth.make_images(N, 64, seed=103)
    xin = torch.cat([x, torch.flip(x, [3])])
    m1, arch, _ = _xs(1.0, 1.0)
    plain = [o.clone() for o in m1.forward_native(x.cuda(), flip)]
    for gain, scale in ((2.0 ** -12, 1.0), (2.0 ** -12, 2.0 ** -8)):
        m, arch, sd = _xs(gain, scale)
        outs = [o.clone() for o in m.forward_native(x.cuda(), flip)]
        torch.cuda.synchronize()
        rows = fu.check_device(m, sd, arch, xin, outs, _images_of(2 * N, N, flip),
                               kinds={'block': 'block_small'} if scale != 1.0 else None)
        wp, wr = max(rows.items(), key=lambda kv: kv[1][0]), max(rows.items(), key=lambda kv: kv[1][1])
        big = max(float(o.abs().max()) for o in outs)
        print('head gain 2^-12, project BN x %g: |outputs| <= %.3g  P %.3f of c_max (%s)  R %.3f of m (%s)'
              % (scale, big, wp[1][0], wp[0], wr[1][1], wr[0]))
        assert big < 1e-3, big
        if scale == 1.0:
            for a, b in zip(outs, plain):
                assert torch.equal(a, b * gain), 'a power-of-two head gain does not commute with the kernel arithmetic'
    print('small magnitudes: %.1f s' % (time.time() - t0))
