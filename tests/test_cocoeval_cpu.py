"""COCO keypoint AP without a GPU: hand-computed cases of the protocol held by BOTH the plain restatement
(tests/_cocoeval_ref.py, the yardstick of the device kernel) and the host half of litepose_amd.coco_eval (accumulate /
summarize fed the restatement's per-detection words); the two bitwise equal on the generated scene; the refusals of
lp_kpt_eval; GroundTruth.from_coco.  Agreement with pycocotools itself is NOT measured here (it is not available): the
expected values below are worked out by hand from the published algorithm."""
import ctypes as C
import math

import numpy as np
import pytest

import _cocoeval_ref as R

SIG = R.COCO_SIGMAS


def _ann(xy, area, v=2, iscrowd=0, bbox=None, num_keypoints=None):
    k = np.zeros((17, 3))
    k[:, :2] = xy
    k[:, 2] = v
    x0, y0 = k[:, 0].min(), k[:, 1].min()
    bb = (x0, y0, k[:, 0].max() - x0, k[:, 1].max() - y0) if bbox is None else bbox
    return {'kpts': k, 'area': float(area), 'bbox': tuple(float(b) for b in bb), 'iscrowd': iscrowd,
            'num_keypoints': int((k[:, 2] > 0).sum()) if num_keypoints is None else num_keypoints}


def _det(xy, score):
    return {'kpts': np.asarray(xy, np.float64).reshape(17, 2), 'score': float(score)}


def _grid(x, y, w, h):
    """17 joints spread over a w x h box at (x, y): keypoint-box area w * h."""
    t = np.arange(17) / 16.0
    return np.stack([x + w * t, y + h * ((np.arange(17) * 5) % 17) / 16.0], axis=1)


def _both(dets, gts, ids=None, area_rng=R.AREA_RNG):
    """The restatement end to end, and coco_eval's host half fed the restatement's words -> (stats_ref, stats_host,
    tables_ref, tables_host, per-image results)."""
    from litepose_amd import coco_eval as ce
    ids = sorted(set(dets) | set(gts)) if ids is None else ids
    per = R.evaluate_set(dets, gts, ids, SIG, R.THR, area_rng)
    tab = R.accumulate(per, R.THR, R.REC, len(area_rng))
    labels = ('all', 'medium', 'large')[:len(area_rng)]
    gt = ce.GroundTruth.from_arrays(*R.ground_truth_arrays(gts, ids))
    rows = [i for i in ids if per[i] is not None and per[i]['src']]
    D = 20
    num = np.zeros(len(rows), np.int64)
    sc = np.zeros((len(rows), D), np.float32)
    mw = np.zeros((len(rows), D), np.uint32)
    iw = np.zeros((len(rows), D), np.uint32)
    for r, i in enumerate(rows):
        e = per[i]
        m, g = R.words(e, len(area_rng), len(R.THR))
        num[r] = len(e['src'])
        sc[r, :num[r]], mw[r, :num[r]], iw[r, :num[r]] = e['scores'], m, g
    slots = [gt.slot[i] for i in rows]
    tab_h = ce.accumulate(np.asarray(slots, np.int64)[::-1], num[::-1], sc[::-1], mw[::-1], iw[::-1], gt,
                          np.ones(len(ids), bool), R.THR, area_rng)       # rows in any order
    return (R.summarize(tab[0], tab[1], R.THR, labels), ce.summarize(tab_h[0], tab_h[1], R.THR, labels), tab, tab_h,
            per)


def _close(stats, name, want):
    assert abs(stats[name] - want) <= 1e-12, (name, stats[name], want)


def test_a_identical_detection_scores_one_everywhere_it_counts():
    xy = _grid(100, 100, 50, 100)
    for stats in _both({1: [_det(xy, .9)]}, {1: [_ann(xy, 5000)]})[:2]:
        assert list(stats) == R.NAMES
        for name in ('AP', 'Ap .5', 'AP .75', 'AP (M)', 'AR', 'AR .5', 'AR .75', 'AR (M)'):
            _close(stats, name, 1.0)                     # pr = 1 / (1 + eps)
        assert stats['AP (L)'] == -1 and stats['AR (L)'] == -1


def test_b_a_false_positive_between_two_hits():
    a, b = _grid(100, 100, 50, 100), _grid(300, 100, 50, 100)
    dets = {1: [_det(a, .9), _det(a + 5000, .8), _det(b, .7)]}
    for stats in _both(dets, {1: [_ann(a, 5000), _ann(b, 5000)]})[:2]:
        # tp 1,1,2 fp 0,1,1: precision 1, 1/2 -> 2/3, 2/3; recall .5, .5, 1: 51 recall points at 1, 50 at 2/3
        _close(stats, 'AP', (51 + 50 * (2.0 / 3)) / 101)
        _close(stats, 'AR', 1.0)


def test_c_oks_value_written_out():
    xy = _grid(100, 100, 50, 100)
    g = _ann(xy, 4000.0)
    g['kpts'][1:, 2] = 0
    g['kpts'][5, 2] = 1                                  # joints 0 (sigma .026) and 5 (sigma .079) are labelled
    d = _det(xy + np.array([3.0, -4.0]), .5)             # every joint off by (3, -4): d^2 = 25
    want = (math.exp(-25.0 / (2 * .026) ** 2 / (4000.0 + 2.0 ** -52) / 2) +
            math.exp(-25.0 / (2 * .079) ** 2 / (4000.0 + 2.0 ** -52) / 2)) / 2
    assert abs(R.oks(d, g, SIG) - want) <= 1e-15
    assert 0.05 < want < 0.95


def test_d_no_labelled_joint_uses_the_doubled_box():
    g = _ann(_grid(100, 100, 50, 100), 5000, v=0, bbox=(100, 100, 50, 100))
    inside = np.stack([np.linspace(51, 199, 17), np.linspace(1, 299, 17)], axis=1)     # x in [50, 200], y in [0, 300]
    assert R.oks(_det(inside, .5), g, SIG) == 1.0
    out = inside.copy()
    out[:, 0] = 230.0                                    # 30 px right of the doubled box, every joint
    want = sum(math.exp(-900.0 / (2 * s) ** 2 / (5000 + 2.0 ** -52) / 2) for s in SIG) / 17
    assert abs(R.oks(_det(out, .5), g, SIG) - want) <= 1e-15 and want < 1.0
    assert R.gt_ignore(g)                                # num_keypoints == 0


def test_e_area_boundaries_are_inclusive():
    xy = _grid(100, 100, 30, 30)
    for area, medium, large in ((1024.0, True, False), (9216.0, True, True), (1023.0, False, False),
                                (9217.0, False, True)):
        per = R.evaluate_image([_det(xy, .9)], [_ann(xy, area)], SIG)
        assert per['gt_ignore'][0] == [False]
        assert per['gt_ignore'][1] == [not medium] and per['gt_ignore'][2] == [not large], area
        # a detection matched to an annotation the range ignores is ignored with it
        assert per['ignore'][1][0] == [not medium] and per['ignore'][2][0] == [not large]
    stats, stats_h = _both({1: [_det(xy, .9)]}, {1: [_ann(xy, 9216.0)]})[:2]
    for s in (stats, stats_h):
        _close(s, 'AP (M)', 1.0)
        _close(s, 'AP (L)', 1.0)


def test_f_a_crowd_takes_two_detections_and_both_are_ignored():
    xy, other = _grid(100, 100, 50, 100), _grid(400, 100, 50, 100)
    gts = [_ann(other, 5000), _ann(xy, 5000, iscrowd=1)]
    per = R.evaluate_image([_det(xy, .9), _det(xy + 1.0, .8), _det(other, .7)], gts, SIG)
    assert per['match'][0][0] == [True, True, True]
    assert per['ignore'][0][0] == [True, True, False]
    # without the crowd flag the second detection finds the annotation taken
    gts[1]['iscrowd'] = 0
    per = R.evaluate_image([_det(xy, .9), _det(xy + 1.0, .8), _det(other, .7)], gts, SIG)
    assert per['match'][0][0] == [True, False, True] and per['ignore'][0][0] == [False, False, False]
    # a detection that could take a counted annotation never takes an ignored one, however good
    gts = [_ann(xy + 2.0, 5000), _ann(xy, 5000, iscrowd=1)]
    per = R.evaluate_image([_det(xy, .9)], gts, SIG)
    assert per['match'][0][0] == [True] and per['ignore'][0][0] == [False]


def test_g_truncation_to_the_best_twenty_keeps_record_order_among_ties():
    xy = _grid(100, 100, 50, 100)
    scores = [.5] * 10 + [.9] * 5 + [.5] * 12             # 27 detections
    per = R.evaluate_image([_det(xy + p, s) for p, s in enumerate(scores)], [_ann(xy, 5000)], SIG)
    assert per['src'] == [10, 11, 12, 13, 14] + list(range(10)) + [15, 16, 17, 18, 19]
    assert len(per['scores']) == 20 and per['scores'][:5] == [.9] * 5


def test_unmatched_detection_outside_the_range_is_ignored_and_empty_images_vanish():
    small = _grid(100, 100, 10, 10)                      # keypoint-box area 100: outside medium and large
    per = R.evaluate_image([_det(small, .9)], [], SIG)
    assert per['match'][1][0] == [False] and per['ignore'][0][0] == [False]
    assert per['ignore'][1][0] == [True] and per['ignore'][2][0] == [True]
    assert R.evaluate_set({}, {}, [3], SIG)[3] is None


@pytest.fixture(scope='module')
def scene():
    return R.scene()


def test_host_accumulate_equals_the_restatement_bitwise(scene):
    from litepose_amd import coco_eval as ce
    stats, stats_h, tab, tab_h, _ = _both(scene['dets'], scene['gts'], scene['all_ids'])
    assert stats == scene['stats']
    for a, b in zip(tab, tab_h):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert list(stats_h) == R.NAMES
    assert [np.float64(v).tobytes() for v in stats_h.values()] == [np.float64(v).tobytes() for v in stats.values()]
    # one area range (a 14-joint set): the six numbers that do not depend on the area
    one = [(0.0, 1e10)]
    s1, s1h = _both(scene['dets'], scene['gts'], scene['all_ids'], one)[:2]
    assert list(s1h) == ['AP', 'Ap .5', 'AP .75', 'AR', 'AR .5', 'AR .75'] and s1h == s1
    assert s1h['AP'] == stats['AP']
    # restricting the evaluated set changes the number (params.imgIds)
    half = scene['all_ids'][::2]
    s2, s2h = _both({i: scene['dets'][i] for i in half if i in scene['dets']}, {i: scene['gts'][i] for i in half},
                    half)[:2]
    assert s2h == s2 and s2['AP'] != stats['AP']
    assert ce.AREA_RANGES == tuple(R.AREA_RNG) and list(ce.COCO_SIGMAS) == R.COCO_SIGMAS


def test_ground_truth_from_coco():
    from litepose_amd import coco_eval as ce
    k = lambda v: [c for j in range(17) for c in (10.0 + j, 20.0 + 2 * j, v)]
    data = {'images': [{'id': 9}, {'id': 4}, {'id': 7}],
            'annotations': [
                {'id': 1, 'image_id': 9, 'category_id': 1, 'keypoints': k(2), 'area': 900.5, 'bbox': [1, 2, 3, 4],
                 'iscrowd': 0, 'num_keypoints': 17},
                {'id': 2, 'image_id': 4, 'category_id': 1, 'keypoints': k(0), 'area': 50.0, 'bbox': [5, 6, 7, 8],
                 'iscrowd': 0, 'num_keypoints': 0},
                {'id': 3, 'image_id': 9, 'category_id': 1, 'keypoints': k(1), 'area': 1e4, 'bbox': [0, 0, 9, 9],
                 'iscrowd': 1, 'num_keypoints': 5},
                {'id': 4, 'image_id': 9, 'category_id': 2, 'keypoints': k(1), 'area': 1.0, 'bbox': [0, 0, 1, 1],
                 'iscrowd': 0, 'num_keypoints': 5},
                {'id': 5, 'image_id': 99, 'category_id': 1, 'keypoints': k(1), 'area': 1.0, 'bbox': [0, 0, 1, 1],
                 'iscrowd': 0, 'num_keypoints': 5}]}
    gt = ce.GroundTruth.from_coco(data)
    assert gt.image_ids.tolist() == [4, 7, 9] and gt.first.tolist() == [0, 1, 1, 3] and gt.num_joints == 17
    assert gt.area.tolist() == [50.0, 900.5, 1e4] and gt.flags.tolist() == [2, 0, 3]
    assert gt.bbox.tolist() == [[5, 6, 7, 8], [1, 2, 3, 4], [0, 0, 9, 9]]
    assert gt.kpts.shape == (3, 17, 3) and gt.kpts[1, 3].tolist() == [13.0, 26.0, 2.0]
    assert gt.kpts.dtype == np.float64 and gt.first.dtype == np.int32 and gt.flags.dtype == np.int32
    crowded = dict(data, annotations=[dict(data['annotations'][0], id=100 + i) for i in range(65)])
    with pytest.raises(ValueError, match='at most 64'):
        ce.GroundTruth.from_coco(crowded)
    ce.GroundTruth.from_coco(dict(data, annotations=crowded['annotations'][:64]))
    import json, tempfile, os
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, 'gt.json')
        with open(p, 'w') as f:
            json.dump(data, f)
        assert ce.GroundTruth.from_coco(p).area.tolist() == gt.area.tolist()


def test_abi_refusals_come_before_any_pointer_is_read():
    from litepose_amd import _native as nv
    lib = nv.lib()
    fake = C.c_void_p(1 << 20)                           # never dereferenced: every call below is refused first
    dbl = C.POINTER(C.c_double)
    sig = (C.c_double * 17)(*R.COCO_SIGMAS)
    thr = (C.c_double * 10)(*R.THR)
    rng = (C.c_double * 6)(*[v for r in R.AREA_RNG for v in r])

    def call(N=4, pcap=30, J=17, T=2, J_eval=17, images=3, n_thr=10, n_area=3, max_dets=20, null=None, h=None):
        dev = [None if null == i else fake for i in range(15)]
        host = [C.cast(None, dbl) if h == i else p for i, p in enumerate((sig, thr, rng))]
        return lib.lp_kpt_eval(dev[0], dev[1], dev[2], N, pcap, J, T, J_eval, dev[3], dev[4], dev[5], dev[6], dev[7],
                               dev[8], images, host[0], host[1], n_thr, host[2], n_area, max_dets, dev[9], dev[10],
                               dev[11], dev[12], dev[13], None, None)

    for i in range(14):
        assert call(null=i) == -1, i
        assert b'null' in lib.lp_last_error()
    for i in range(3):
        assert call(h=i) == -1, i
    assert call(N=0) == -1 and call(images=-1) == -1 and call(n_thr=0) == -1 and call(n_area=0) == -1
    assert call(pcap=0) == -1 and call(J=0) == -1
    for bad in (0, 33, -1):
        assert call(max_dets=bad) == -8
        assert b'max_dets' in lib.lp_last_error()
    assert call(n_thr=11, n_area=3) == -8
    assert b'n_thr * n_area' in lib.lp_last_error()
    assert call(n_thr=1 << 20, n_area=1 << 20) == -8
    for bad in (0, 18, -3):
        assert call(J_eval=bad) == -8
    assert call(J=40, J_eval=33) == -8
    assert b'J_eval' in lib.lp_last_error()
