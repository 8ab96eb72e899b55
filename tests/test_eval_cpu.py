"""Batch evaluation of variable-size images, the host half (no GPU): the bucket plan, the fp64 host arithmetic of the
per-image transforms, and argument validation of the per-image entry points before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from oracle import preprocess_ref, transforms_ref

SIZES_256 = {(427, 640): (384, 256), (480, 640): (384, 256), (333, 500): (384, 256), (375, 500): (384, 256),
             (640, 427): (256, 384), (612, 612): (256, 256), (360, 640): (512, 256), (640, 360): (256, 512),
             (200, 600): (768, 256), (600, 200): (256, 768)}


def test_bucket_plan_sizes_padding_and_order():
    from litepose_amd import evaluate as ev
    shapes = [(427, 640), (640, 427), (480, 640), (612, 612), (333, 500), (640, 360), (375, 500), (200, 600),
              (427, 640), (640, 427), (612, 612), (612, 612)]
    for hw, size in SIZES_256.items():
        assert ev.plan([hw], 256, 1.0, 4)[0].size == size, hw
        assert tuple(transforms_ref.get_multi_scale_size(hw, 256, 1.0, 1.0)[0]) == size, hw
    # 448: the 200 x 600 bucket is wider than 1024 (the engine's 'maps' AE path)
    assert ev.plan([(200, 600)], 448, 1.0, 1)[0].size == (1344, 448)
    batches = ev.plan(shapes, 256, 1.0, 2)
    # buckets in order of first appearance, batches in input order inside a bucket, each padded to 2 rows
    assert [(b.size, b.rows, b.real) for b in batches] == [
        ((384, 256), (0, 2), 2), ((384, 256), (4, 6), 2), ((384, 256), (8, 8), 1),
        ((256, 384), (1, 9), 2),
        ((256, 256), (3, 10), 2), ((256, 256), (11, 11), 1),
        ((256, 512), (5, 5), 1),
        ((768, 256), (7, 7), 1)]
    assert all(len(b.rows) == 2 for b in batches)
    assert dict(ev.bucket_histogram(batches)) == {'384x256': 5, '256x384': 2, '256x256': 3, '256x512': 1,
                                                   '768x256': 1}
    # per-row items back in input order; the padding rows carry nothing
    per_batch = [['img%d' % r for r in b.rows[:b.real]] for b in batches]
    assert ev.in_input_order(batches, per_batch) == ['img%d' % i for i in range(len(shapes))]
    with pytest.raises(ValueError):
        ev.in_input_order(batches, [items + ['pad'] for items in per_batch])
    # one batch, min scale 0.5: the buckets are those of get_multi_scale_size(..., 1.0, 0.5)
    b = ev.plan([(427, 640)], 256, 0.5, 8)
    assert b[0].size == tuple(transforms_ref.get_multi_scale_size((427, 640), 256, 1.0, 0.5)[0])
    assert b[0].rows == (0,) * 8 and b[0].real == 1


def _np_final_preds_coef(center, scale, Wp, Hp):
    s = float(scale[0]) * 200.0 / float(Wp)
    return np.array([s, float(center[0]) - s * Wp * 0.5, s, float(center[1]) - s * Hp * 0.5], np.float64)


def test_warp_invert_and_final_preds_coef_exact():
    from litepose_amd.utils import transforms as T
    for hw, size in SIZES_256.items():
        for input_size in (256, 448):
            sz, center, scale = T.get_multi_scale_size(hw, input_size, 1.0, 1.0)
            trans = T.get_affine_transform(center, scale, 0, sz)
            # lp_warp_invert == the NumPy restatement of the same fp64 operations, bit for bit
            assert np.array_equal(T.warp_invert(trans), preprocess_ref.invert_affine(trans).reshape(-1)), hw
            coef = T.final_preds_coef(center, scale, sz)
            assert np.array_equal(coef, _np_final_preds_coef(center, scale, sz[0], sz[1])), hw
            # ... and matches the oracle's get_final_preds on a few points
            rng = np.random.default_rng(hw[0] + input_size)
            pts = np.zeros((1, 5, 14, 5), np.float32)
            pts[..., 0] = rng.uniform(0, sz[0], size=(1, 5, 14))
            pts[..., 1] = rng.uniform(0, sz[1], size=(1, 5, 14))
            pts[..., 2:] = rng.normal(size=(1, 5, 14, 3))
            ref = transforms_ref.get_final_preds([pts[0]], center, scale, list(sz))
            got = pts[0].copy()
            got[..., 0] = (coef[0] * got[..., 0].astype(np.float64) + coef[1]).astype(np.float32)
            got[..., 1] = (coef[2] * got[..., 1].astype(np.float64) + coef[3]).astype(np.float32)
            for p, q in zip(got, ref):
                np.testing.assert_allclose(p, q, rtol=0, atol=1e-4)
    # singular matrix: the zero-determinant form of cv2
    assert np.array_equal(T.warp_invert(np.zeros((2, 3))), preprocess_ref.invert_affine(np.zeros((2, 3))).reshape(-1))


def test_warp_desc_layout():
    from litepose_amd import _native as nv
    from litepose_amd.utils import transforms as T
    assert C.sizeof(nv.LpWarpDesc) == 64 == T.WARP_DESC_DTYPE.itemsize
    for f in ('src_offset', 'H', 'W', 'minv'):
        assert getattr(nv.LpWarpDesc, f).offset == T.WARP_DESC_DTYPE.fields[f][1], f


def test_per_image_entry_points_validate_before_any_device_call():
    from litepose_amd import _native as nv
    lib = nv.lib()
    BAD = -1                                     # LP_ERR_INVALID_ARG
    fake = C.c_void_p(0x1000)                    # never dereferenced: every call below is refused first
    mean = (C.c_float * 3)(0.485, 0.456, 0.406)
    std = (C.c_float * 3)(0.229, 0.224, 0.225)
    zstd = (C.c_float * 3)(0.229, 0.0, 0.225)
    pv = lib.lp_preprocess_batch_v
    assert pv(None, 100, fake, 1, 8, 8, mean, std, None, fake, None) == BAD
    assert pv(fake, 100, None, 1, 8, 8, mean, std, None, fake, None) == BAD
    assert pv(fake, 100, fake, 1, 8, 8, None, std, None, fake, None) == BAD
    assert pv(fake, 100, fake, 1, 8, 8, mean, None, None, fake, None) == BAD
    assert pv(fake, 100, fake, 1, 8, 8, mean, std, None, None, None) == BAD          # no output
    assert pv(fake, 0, fake, 1, 8, 8, mean, std, None, fake, None) == BAD            # empty source buffer
    for n in (0, -1, 65536):
        assert pv(fake, 100, fake, n, 8, 8, mean, std, None, fake, None) == BAD, n
    for hd, wd in ((0, 8), (8, 0), (32768, 8), (8, 32768), (-3, 8)):
        assert pv(fake, 100, fake, 1, hd, wd, mean, std, None, fake, None) == BAD, (hd, wd)
    assert pv(fake, 100, fake, 1, 8, 8, mean, zstd, None, fake, None) == BAD
    fv = lib.lp_final_preds_v
    assert fv(None, fake, 1, 4, 14, 2, fake, None) == BAD
    assert fv(fake, None, 1, 4, 14, 2, fake, None) == BAD
    assert fv(fake, fake, 1, 4, 14, 2, None, None) == BAD
    for n, pcap, J, T in ((0, 4, 14, 2), (65536, 4, 14, 2), (1, 0, 14, 2), (1, 4, 0, 2), (1, 4, 33, 2),
                          (1, 4, 14, 0), (1, 4, 14, 3)):
        assert fv(fake, fake, n, pcap, J, T, fake, None) == BAD, (n, pcap, J, T)
    c2 = (C.c_double * 2)(100.0, 80.0)
    s2 = (C.c_double * 2)(2.0, 1.5)
    out4 = (C.c_double * 4)()
    out6 = (C.c_double * 6)()
    m6 = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    assert lib.lp_final_preds_coef(None, s2, 64, 64, out4) == BAD
    assert lib.lp_final_preds_coef(c2, None, 64, 64, out4) == BAD
    assert lib.lp_final_preds_coef(c2, s2, 64, 64, None) == BAD
    for wp, hp in ((0, 64), (64, 0), (32768, 64)):
        assert lib.lp_final_preds_coef(c2, s2, wp, hp, out4) == BAD
    assert lib.lp_final_preds_coef(c2, s2, 64, 48, out4) == 0
    assert lib.lp_warp_invert(None, out6) == BAD
    assert lib.lp_warp_invert(m6, None) == BAD
    assert lib.lp_warp_invert(m6, out6) == 0 and list(out6) == [1, 0, 0, 0, 1, 0]


def test_evaluate_refuses_multiscale_and_no_projection():
    """The two configurations that stay on the batch-1 shims, refused before anything touches the engine's device."""
    from litepose_amd import config
    from litepose_amd import evaluate as ev

    class _Eng(object):
        pass
    img = [np.zeros((64, 80, 3), np.uint8)]
    eng = _Eng()
    eng.cfg = config.get_cfg()
    eng.cfg.TEST.SCALE_FACTOR = [2, 1]
    with pytest.raises(NotImplementedError, match='batch-1'):
        ev.evaluate(eng, img)
    eng.cfg = config.get_cfg()
    eng.cfg.TEST.PROJECT2IMAGE = False
    with pytest.raises(NotImplementedError, match='batch-1'):
        ev.evaluate(eng, img)
