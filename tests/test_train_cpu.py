"""The host side of the training targets and the training loss, without a GPU: ``draw_sample`` against the matrices the
real RandomAffineTransform handed to cv2.warpAffine, the numpy restatements of tests/_loss_ref.py against the real
reference's targets and losses (tests/golden/golden_targets.npz, tests/golden/gen_golden_targets.py), ``gaussian_table``,
``get_joints``, the struct sizes, and every refusal of lp_target_maps / lp_target_masks / lp_pose_loss -- with null or
dummy pointers, since a refusal precedes any dereference and any launch."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import _loss_ref as LR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_targets.npz')
U = 2.0 ** -24               # unit roundoff of fp32


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _aug(gold):
    return {k[4:]: gold[k].item() for k in gold if k.startswith('aug_')}


# ------------------------------------------------------------------ dataset.calibration.draw_sample
def test_draw_sample_replays_the_reference(gold):
    """Seeded like the reference's global generators, draw_sample reproduces what RandomAffineTransform handed to
    cv2.warpAffine -- mat_output per output size, then mat_input -- and the flip.  1e-12 relative as for draw_transform
    (tests/test_search_cpu.py): the 3x3 products go through BLAS, which may contract."""
    from litepose_amd.dataset.calibration import draw_sample, draw_transform
    seed, outs, S = int(gold['seed']), gold['outs'].tolist(), int(gold['input_size'])
    np_rng, py_rng = np.random.RandomState(seed), random.Random(seed)
    np2, py2 = np.random.RandomState(seed), random.Random(seed)
    assert set(gold['flip'].tolist()) == {True, False}
    for n, (h, w) in enumerate(gold['sizes'].tolist()):
        mat, mats, flip = draw_sample(h, w, S, outs, np_rng, py_rng, **_aug(gold))
        assert flip is bool(gold['flip'][n])
        assert len(mats) == len(outs)
        for got, want in [(mat, gold['mat_input'][n])] + [(mats[s], gold['mat_output'][n, s]) for s in range(len(outs))]:
            assert got.shape == (2, 3) and got.dtype == np.float64
            assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (n, got, want)
        assert abs(mat[0, 1]) > 1e-3                            # a real rotation
        # the same draws in the same order as draw_transform: equal generators give the same image transform
        mat_t, flip_t = draw_transform(h, w, S, np2, py2, **_aug(gold))
        assert np.array_equal(mat_t, mat) and flip_t is flip
    assert np_rng.random() == np2.random() and py_rng.random() == py2.random()


# ------------------------------------------------------------------ the restatements against the reference
def _rows(gold):
    first = np.concatenate([[0], np.cumsum(gold['people'])])
    return [(int(first[n]), int(first[n + 1])) for n in range(len(gold['people']))]


@pytest.mark.parametrize('R', [16, 32])
def test_restated_targets_equal_the_reference(gold, R):
    """cells / heatmaps / joints_tensor of _loss_ref from the SOURCE joints and the recorded matrices: the joints tensor
    exactly, the heatmaps exactly with the reference's own table rounded to fp32."""
    s = gold['outs'].tolist().index(R)
    table = gold['gauss_s2'].astype(np.float32)
    M, fi = int(gold['M']), gold['flip_index'].tolist()
    for n, (lo, hi) in enumerate(_rows(gold)):
        cx, cy, ok = LR.cells(gold['joints'][lo:hi], gold['mat_output'][n, s], bool(gold['flip'][n]), fi, R)
        assert np.array_equal(LR.joints_tensor(cx, cy, ok, R, M, True), gold['jt_%d' % R][n]), n
        assert np.array_equal(LR.heatmaps(cx, cy, ok, table, R), gold['heat_%d' % R][n]), n
        if R == 16:
            assert np.array_equal(LR.joints_tensor(cx, cy, ok, R, M, False), gold['jt_16_nt'][n]), n
            assert np.array_equal(LR.heatmaps(cx, cy, ok, gold['gauss_s1'].astype(np.float32), R), gold['heat_16_s1'][n])
    assert gold['jt_%d' % R][:, :, :, 1].sum() > 6                     # the fixture has visible joints
    ident = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    for flip in (0, 1):
        cx, cy, ok = LR.cells(gold['ident_joints_%d' % R], ident, flip, fi, R)
        assert np.array_equal(LR.joints_tensor(cx, cy, ok, R, M, True), gold['ident_jt_%d_f%d' % (R, flip)])
        assert np.array_equal(LR.heatmaps(cx, cy, ok, table, R), gold['ident_heat_%d_f%d' % (R, flip)])
    # the hand-placed rules: (-0.5, -0.9) is cell (0, 0); (-1, 3) and (R, 0) are out; (R - 0.5, 0) is in; v = 0 is skipped
    jt = gold['ident_jt_%d_f0' % R]
    assert jt[0].tolist() == [[0, 1], [2 * R * R + R - 1, 1], [0, 0], [0, 0], [0, 0]]
    assert jt[1, 0].tolist() == [0, 1] and not jt[3].any()


def test_gaussian_table(gold):
    """The library's table against the reference's fp64 table rounded to fp32: one fp32 ulp (exp may differ between two
    machines' libm in the last fp64 bit, which can move the fp32 rounding by one)."""
    from litepose_amd.dataset.targets import gaussian_table
    for sigma, key in ((2, 'gauss_s2'), (1, 'gauss_s1')):
        got, want = gaussian_table(sigma), gold[key].astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (6 * sigma + 3,) * 2 == want.shape
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(want)).all()
        assert got[3 * sigma + 1, 3 * sigma + 1] == 1.0


def _ref_bounds(gold, c, s, R):
    """Bounds on |reference fp32 value - exact value| from the reference's own arithmetic (loss.py), in units of U:
    heat: (pred - gt), the square and the mask product round once each (3 U relative per non-negative term), the three
        nested means add R - 1, R - 1 and J - 1 roundings and three divisions, the factor one more;
    tags: with t = the largest |tag| of the image, J the joints and P <= M persons: a person's mean carries J U t, a
        deviation (J + 1) U t more, so pull (a mean of squares <= (2t)^2) is off by at most (4 J + 12) U (2t)^2 + the
        sums' (J + P + 4) U (2t)^2; push sums P^2 terms <= 1, each off by the exp's 2 U plus 2 |d| exp(-d^2) <= 0.86
        times the difference's error 2 (J + 1) U t (for 'max' the slope is 1), plus P^2 U per term for the fp32 sum,
        then 0.5 / ((P - 1) P)."""
    J, M = int(gold['J']), int(gold['M'])
    heat_rel = (3 + 2 * (R - 1) + (J - 1) + 3 + 1) * U
    out = gold['out_16'] if R == 16 else (gold['out_32'] if c == 0 else gold['out_32_tags'])
    t = np.abs(out).reshape(out.shape[0], -1).max(1).astype(np.float64)
    pull_abs = ((4 * J + 12) + (J + M + 4)) * U * (2 * t) ** 2
    push_abs = M * M * (2 + 2 * (J + 1) * t + M * M) * U * 0.5 / 2
    return heat_rel, push_abs, pull_abs


@pytest.mark.parametrize('loss_type', ['exp', 'max'])
@pytest.mark.parametrize('c', [0, 1])
def test_restated_losses_equal_the_reference(gold, c, loss_type):
    """heat_loss / tag_loss of _loss_ref, recomputed here from the fixture's inputs: equal to the fp64 values stored by the
    generator (1e-15: another machine's exp), and within the reference's own fp32 error of its values."""
    ref, f64 = gold['loss%d_%s_ref' % (c, loss_type)], gold['loss%d_%s_f64' % (c, loss_type)]
    J = int(gold['J'])
    cfg = [dict(heat=(True, True), ae=(True, False)), dict(heat=(False, True), ae=(True, True))][c]
    seen = 0
    for s, R in enumerate((16, 32)):
        out = gold['out_16'] if R == 16 else (gold['out_32'] if c == 0 else gold['out_32_tags'])
        heat_rel, push_abs, pull_abs = _ref_bounds(gold, c, s, R)
        for n in range(out.shape[0]):
            if cfg['heat'][s]:
                f = LR.heat_loss(out[n, :J], gold['heat_%d' % R][n], gold['mask_t_%d' % R][n], 1.0)
                assert abs(f - f64[s, 0, n]) <= 1e-15 * abs(f)
                assert abs(ref[s, 0, n] - f) <= heat_rel * f + U * f, (s, n, ref[s, 0, n], f)
                seen += 1
            else:
                assert np.isnan(ref[s, 0, n]) and np.isnan(f64[s, 0, n])
            if cfg['ae'][s]:
                off = J if cfg['heat'][s] else 0
                push, pull = LR.tag_loss(out[n, off:], gold['jt_%d' % R][n], loss_type, 0.001, 0.001)
                assert abs(push - f64[s, 1, n]) <= 1e-15 * abs(push) and abs(pull - f64[s, 2, n]) <= 1e-15 * abs(pull)
                k = float(np.float32(0.001))
                assert abs(ref[s, 1, n] - push) <= k * push_abs[n] + 2 * U * abs(push), (s, n, ref[s, 1, n], push)
                assert abs(ref[s, 2, n] - pull) <= k * pull_abs[n] + 2 * U * abs(pull), (s, n, ref[s, 2, n], pull)
                people = int((gold['jt_%d' % R][n, :, :, 1].sum(1) > 0).sum())
                if people < 2:
                    assert push == 0 and ref[s, 1, n] == 0          # batchTagLoss: no push below two persons
                elif loss_type == 'exp':
                    assert push > 0
                if people == 0:
                    assert pull == 0 and ref[s, 2, n] == 0
                seen += 1
            else:
                assert np.isnan(ref[s, 1:, n]).all()
    assert seen >= 12
    # the batch values of the reference are the means of its per-image values
    batch = gold['loss%d_%s_batch' % (c, loss_type)]
    for s in range(2):
        if cfg['ae'][s]:
            assert np.allclose(batch[s], ref[s, 1:].astype(np.float64).mean(1), rtol=4 * U, atol=0)


def test_get_joints():
    from litepose_amd.dataset.targets import get_joints
    anno = [dict(keypoints=[1, 2, 2, 3, 4, 0, 5, 6, 1]), dict(keypoints=[0] * 9)]
    j = get_joints(anno, 3)
    assert j.shape == (2, 3, 3) and j.dtype == np.float64 and j[0].tolist() == [[1, 2, 2], [3, 4, 0], [5, 6, 1]]
    c = get_joints(anno, 4, with_center=True)
    assert c[0, 3].tolist() == [(1 + 3 + 5) / 2, (2 + 4 + 6) / 2, 1] and c[1, 3].tolist() == [0, 0, 0]
    assert get_joints([], 3).shape == (0, 3, 3)


def test_loss_epoch_refuses_a_set_without_batches():
    from litepose_amd import config
    from litepose_amd.core.trainer import loss_epoch

    class Nothing(object):
        def batches(self, *a, **k):
            return iter(())
    with pytest.raises(ValueError, match='no batch'):
        loss_epoch(None, Nothing(), config.get_cfg())


# ------------------------------------------------------------------ the C ABI without a device
def test_struct_sizes():
    from litepose_amd import _native as nv
    from litepose_amd.dataset import calibration as cal, targets as tg
    assert C.sizeof(nv.LpTargetDesc) == 56 == tg.TARGET_DESC_DTYPE.itemsize
    assert C.sizeof(nv.LpAugDesc) == 72 == cal.AUG_DESC_DTYPE.itemsize
    assert nv.LpTargetDesc.flip.offset == 48 and nv.LpTargetDesc.reserved.offset == 52
    for name in ('lp_target_maps', 'lp_target_masks', 'lp_pose_loss', 'lp_pose_loss_workspace_bytes'):
        assert name in nv.EXPORTS and hasattr(nv.lib(), name)


OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -6, -8
P = C.c_void_p(0x1000)        # a dummy device pointer: never dereferenced, every case below is refused before any launch


def _maps(**kw):
    from litepose_amd import _native as nv
    a = dict(joints=P, P_tot=4, first=P, desc=P, N=2, J=5, R=16, fi=[1, 0, 2, 4, 3], gauss=P, side=15, sigma3=6.0, M=4,
             tpj=1, heat=P, jout=P)
    a.update(kw)
    fi = None if a['fi'] is None else (C.c_int32 * len(a['fi']))(*a['fi'])
    return nv.lib().lp_target_maps(a['joints'], a['P_tot'], a['first'], a['desc'], a['N'], a['J'], a['R'], fi, a['gauss'],
                                   a['side'], a['sigma3'], a['M'], a['tpj'], a['heat'], a['jout'], None)


@pytest.mark.parametrize('kw, code', [
    (dict(J=0), UNSUPPORTED), (dict(J=33, fi=list(range(33))), UNSUPPORTED), (dict(M=0), UNSUPPORTED),
    (dict(M=65), UNSUPPORTED), (dict(R=0), UNSUPPORTED), (dict(R=1025), UNSUPPORTED), (dict(sigma3=-3.0), UNSUPPORTED),
    (dict(sigma3=4.5), UNSUPPORTED), (dict(sigma3=float('nan')), UNSUPPORTED), (dict(side=16), UNSUPPORTED),
    (dict(side=9), UNSUPPORTED),
    (dict(joints=None), INVALID), (dict(first=None), INVALID), (dict(desc=None), INVALID), (dict(fi=None), INVALID),
    (dict(heat=None, jout=None), INVALID), (dict(gauss=None), INVALID), (dict(N=0), INVALID), (dict(P_tot=-1), INVALID),
    (dict(fi=[1, 0, 2, 5, 3]), INVALID), (dict(fi=[1, 0, -1, 4, 3]), INVALID),
])
def test_target_maps_refusals(kw, code):
    from litepose_amd import _native as nv
    assert _maps(**kw) == code, (kw, nv.lib().lp_last_error())
    assert nv.lib().lp_last_error()


def _masks(**kw):
    from litepose_amd import _native as nv
    a = dict(src=P, src_bytes=64, desc=P, N=2, R=16, out=P)
    a.update(kw)
    return nv.lib().lp_target_masks(a['src'], a['src_bytes'], a['desc'], a['N'], a['R'], a['out'], None)


@pytest.mark.parametrize('kw, code', [
    (dict(desc=None), INVALID), (dict(out=None), INVALID), (dict(src=None), INVALID), (dict(N=0), INVALID),
    (dict(N=65536), INVALID), (dict(R=0), UNSUPPORTED), (dict(R=1025), UNSUPPORTED),
])
def test_target_masks_refusals(kw, code):
    from litepose_amd import _native as nv
    assert _masks(**kw) == code, (kw, nv.lib().lp_last_error())


def _loss(**kw):
    from litepose_amd import _native as nv
    a = dict(out=P, N=2, C=10, R=16, J=5, off=5, heat=P, mask=P, joints=P, M=4, lt=0, hl=P, push=P, pull=P, ws=P,
             ws_bytes=1 << 20)
    a.update(kw)
    return nv.lib().lp_pose_loss(a['out'], a['N'], a['C'], a['R'], a['J'], a['off'], a['heat'], a['mask'], a['joints'],
                                 a['M'], a['lt'], 1.0, 1.0, 1.0, a['hl'], a['push'], a['pull'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('kw, code', [
    (dict(J=0), UNSUPPORTED), (dict(J=33), UNSUPPORTED), (dict(R=0), UNSUPPORTED), (dict(R=1025), UNSUPPORTED),
    (dict(M=0), UNSUPPORTED), (dict(M=65), UNSUPPORTED), (dict(lt=2), UNSUPPORTED), (dict(lt=-1), UNSUPPORTED),
    (dict(out=None), INVALID), (dict(heat=None, off=-1), INVALID), (dict(mask=None), INVALID), (dict(hl=None), INVALID),
    (dict(ws=None), INVALID), (dict(joints=None), INVALID), (dict(push=None), INVALID), (dict(pull=None), INVALID),
    (dict(N=0), INVALID), (dict(C=0), INVALID), (dict(C=4), INVALID), (dict(off=10), INVALID),
    (dict(ws_bytes=2 * 5 * 8 - 1), WORKSPACE), (dict(ws=C.c_void_p(0x1004)), WORKSPACE),
])
def test_pose_loss_refusals(kw, code):
    from litepose_amd import _native as nv
    assert _loss(**kw) == code, (kw, nv.lib().lp_last_error())


def test_pose_loss_workspace_bytes():
    from litepose_amd import _native as nv
    ws = nv.lib().lp_pose_loss_workspace_bytes
    assert ws(2, 5, 16) == 2 * 5 * 8 and ws(2, 5, 64) == 2 * 5 * 8 and ws(2, 5, 65) == 2 * 5 * 2 * 8
    assert ws(64, 14, 128) == 64 * 14 * 4 * 8 and ws(1, 1, 1024) == 256 * 8
    assert ws(0, 5, 16) == 0 and ws(2, 0, 16) == 0 and ws(2, 33, 16) == 0 and ws(2, 5, 0) == 0 and ws(2, 5, 1025) == 0
