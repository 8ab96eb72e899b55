"""Multi-scale batch evaluation (TEST.SCALE_FACTOR with several entries, TEST.PROJECT2IMAGE = False), the host half
(no GPU): the bucket plan over all scales, the per-scale warp matrices and valid.py's back-projection row, the scale
lists the reference loop cannot run, and argument validation of lp_tta_merge_scales before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import transforms_ref

SHAPES = [(427, 640), (640, 427), (480, 640), (612, 612), (333, 500), (640, 360), (375, 500), (200, 600),
          (427, 640), (640, 427), (612, 612), (612, 612), (360, 640), (600, 200)]
SCALE_LISTS = ([0.5, 1, 2], [1, 2], [0.75, 1], [2, 0.5, 1])


def _order(sf):
    return sorted([float(s) for s in sf], reverse=True)


@pytest.mark.parametrize('sf', SCALE_LISTS)
def test_multiscale_plan_keys_and_padding(sf):
    from litepose_amd import evaluate as ev
    order = _order(sf)
    mn = min(order)
    batches = ev.plan(SHAPES, 256, mn, 3, order)
    seen = []
    for b in batches:
        assert len(b.rows) == 3 and 1 <= b.real <= 3
        assert b.rows[b.real:] == (b.rows[b.real - 1],) * (3 - b.real)          # padding repeats a real image
        assert len(b.size) == len(order)
        for r in b.rows[:b.real]:
            want = tuple(tuple(int(v) for v in transforms_ref.get_multi_scale_size(SHAPES[r], 256, s, mn)[0])
                         for s in order)
            assert b.size == want, (SHAPES[r], b.size, want)
            seen.append(r)
    assert sorted(seen) == list(range(len(SHAPES)))
    # one bucket per distinct key, in order of first appearance, batches in input order inside it
    keys = [b.size for b in batches]
    firsts = list(dict.fromkeys(keys))
    assert keys == [k for k in firsts for _ in range(keys.count(k))]           # a bucket's batches are contiguous
    starts = []
    for k in firsts:
        rows = [r for b in batches if b.size == k for r in b.rows[:b.real]]
        assert rows == sorted(rows)
        starts.append(rows[0])
    assert starts == sorted(starts)
    hist = ev.bucket_histogram(batches)
    assert sum(hist.values()) == len(SHAPES)
    assert all(name.count('+') == len(order) - 1 for name in hist)
    # the single-scale plan is unchanged by the new argument
    assert ev.plan(SHAPES, 256, mn, 3) == ev.plan(SHAPES, 256, mn, 3, None)


@pytest.mark.parametrize('sf', SCALE_LISTS)
@pytest.mark.parametrize('p2i', [True, False])
def test_scale_transforms_and_back_projection_row(sf, p2i):
    """One warp matrix per scale (get_affine_transform(center, scale_s, 0, size_s)) and the back-projection row of
    valid.py: centre / scale of the LAST scale visited (min(SCALE_FACTOR)), heatmap size of the final maps -- the base
    size with PROJECT2IMAGE, the first scale's stage-1 size without it."""
    from litepose_amd import evaluate as ev
    from litepose_amd.utils import transforms as T
    order = _order(sf)
    mn = min(order)
    tr = ev._ScaleTransforms(256, order, p2i)
    for hw in sorted(set(SHAPES)):
        minvs, coef = tr(hw)
        assert len(minvs) == len(order)
        sizes = []
        for s, minv in zip(order, minvs):                  # valid.py:207-213
            size, center, scale = T.get_multi_scale_size(hw, 256, s, mn)
            assert np.array_equal(minv, T.warp_invert(T.get_affine_transform(center, scale, 0, size))), (hw, s)
            sizes.append(size)
        if p2i:
            heatmap = T.get_multi_scale_size(hw, 256, 1.0, mn)[0]
        else:
            heatmap = (sizes[0][0] // 2, sizes[0][1] // 2)
        assert np.array_equal(coef, T.final_preds_coef(center, scale, heatmap)), hw
        _, c_min, s_min = T.get_multi_scale_size(hw, 256, mn, mn)
        assert np.array_equal(coef, T.final_preds_coef(c_min, s_min, heatmap)), hw
        # against the oracle's get_final_preds on a few points
        rng = np.random.default_rng(hw[0] * 7 + hw[1])
        pts = np.zeros((1, 4, 14, 5), np.float32)
        pts[..., 0] = rng.uniform(0, heatmap[0], size=(1, 4, 14))
        pts[..., 1] = rng.uniform(0, heatmap[1], size=(1, 4, 14))
        ref = transforms_ref.get_final_preds([pts[0]], c_min, s_min, list(heatmap))
        got = pts[0].copy()
        got[..., 0] = (coef[0] * got[..., 0].astype(np.float64) + coef[1]).astype(np.float32)
        got[..., 1] = (coef[2] * got[..., 1].astype(np.float64) + coef[3]).astype(np.float32)
        for p, q in zip(got, ref):
            np.testing.assert_allclose(p[..., :2], q[..., :2], rtol=0, atol=1e-4)


class _Eng(object):
    pass


def _fake_engine(sf, p2i=True):
    from litepose_amd import config
    eng = _Eng()
    eng.cfg = config.get_cfg()
    eng.cfg.TEST.SCALE_FACTOR = list(sf)
    eng.cfg.TEST.PROJECT2IMAGE = p2i
    return eng


def test_scale_lists_the_reference_cannot_run():
    """Refused with a reason before anything touches the engine's device."""
    from litepose_amd import evaluate as ev
    from litepose_amd.core import inference
    img = [np.zeros((64, 80, 3), np.uint8)]
    for sf in ([0.5, 2], [2, 0.75]):
        with pytest.raises(ValueError, match='no entry 1'):
            ev.evaluate(_fake_engine(sf), img)
    for sf in ([1, 1, 2], [2, 1, 2]):
        with pytest.raises(ValueError, match='duplicates'):
            ev.evaluate(_fake_engine(sf, p2i=False), img)
    with pytest.raises(ValueError, match='at most 8'):
        ev.evaluate(_fake_engine([1] + [0.5 + 0.1 * k for k in range(8)]), img)
    # what the reference runs: one scale of any factor, or several distinct ones with a 1
    assert inference.scale_order(_fake_engine([0.5]).cfg) == ([0.5], 0)
    assert inference.scale_order(_fake_engine([0.5, 2, 1]).cfg) == ([2.0, 1.0, 0.5], 1)
    assert inference.scale_order(_fake_engine([1, 2]).cfg) == ([2.0, 1.0], 1)


def test_tuple_input_refuses_offsets_center_scale():
    """A multi-scale input is back-projected by preds_coef only; refused before any device call."""
    from litepose_amd import config, engine
    eng = engine.PoseEngine.__new__(engine.PoseEngine)
    eng.cfg = config.get_cfg()
    eng.cfg.TEST.SCALE_FACTOR = [1, 2]
    x = (torch.zeros(2, 3, 128, 128), torch.zeros(2, 3, 64, 64))
    offs = (torch.zeros(1), torch.zeros(1))
    for call in (eng.submit, eng.infer_batch):
        with pytest.raises(ValueError, match='offsets'):
            call(x, offsets=offs)
        with pytest.raises(ValueError, match='center'):
            call(x, center=(64.0, 64.0), scale=(1.0, 1.0))
        with pytest.raises(ValueError, match='preds_coef'):
            call(x)
        with pytest.raises(ValueError, match='offsets'):
            call(list(x), offsets=offs)


def test_merge_scales_validates_before_any_device_call():
    from litepose_amd import _native as nv
    lib = nv.lib()
    BAD = -1                                     # LP_ERR_INVALID_ARG
    assert C.sizeof(nv.LpScaleMid) == 16
    fake = C.c_void_p(0x1000)                    # never dereferenced: every call below is refused first
    tab = (nv.LpScaleMid * 9)()
    for s in range(9):
        tab[s].mid, tab[s].h1, tab[s].w1 = 0x1000, 64 >> min(s, 3), 48 >> min(s, 3)
    ms = lib.lp_tta_merge_scales

    def call(S=3, first=1, N=2, J=14, T=2, p2i=1, Hf=128, Wf=96, det=fake, tag=fake, t=tab):
        return ms(t, S, first, N, J, T, p2i, Hf, Wf, det, tag, None)

    assert call(t=None) == BAD
    assert call(det=None) == BAD
    assert call(tag=None) == BAD
    for S in (0, -1, 9):
        assert call(S=S, first=0) == BAD, S
    for first in (-1, 3, 8):
        assert call(first=first) == BAD, first
    for N, J, T in ((0, 14, 2), (2, 0, 2), (2, 33, 2), (2, 14, 0), (2, 14, 3)):
        assert call(N=N, J=J, T=T) == BAD, (N, J, T)
    for hf, wf in ((0, 96), (128, 0), (32768, 96), (128, 32768)):
        assert call(Hf=hf, Wf=wf) == BAD, (hf, wf)
    null_mid = (nv.LpScaleMid * 3)()
    for s in range(3):
        null_mid[s].mid, null_mid[s].h1, null_mid[s].w1 = 0x1000, 32, 32
    null_mid[2].mid = None
    assert call(t=null_mid) == BAD
    bad_size = (nv.LpScaleMid * 3)()
    for s in range(3):
        bad_size[s].mid, bad_size[s].h1, bad_size[s].w1 = 0x1000, 32, 32
    bad_size[1].w1 = 0
    assert call(t=bad_size) == BAD
    # without PROJECT2IMAGE the maps are the first scale's stage-1 size (64 x 48 here)
    assert call(p2i=0, Hf=128, Wf=96) == BAD
    assert call(tag=C.c_void_p(0x1004)) == BAD                # a float2 tag store needs 8-byte alignment
