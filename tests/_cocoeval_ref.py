"""The COCO keypoint evaluation protocol (the published COCOeval algorithm for iouType = 'keypoints') as
plain loops over Python floats -- written to be read against the description, not to be fast -- plus the seeded scene
generator of tests/test_cocoeval_cpu.py and tests/test_gpu_cocoeval.py.  This is the yardstick of lp_kpt_eval and of
litepose_amd.coco_eval; it was written from the protocol's description, NOT checked against pycocotools (not available).

A detection is {'kpts': [J][>=2] (x, y, ...), 'score': float}; an annotation is {'kpts': [J][3] (x, y, v), 'area',
'bbox': (x, y, w, h), 'iscrowd', 'num_keypoints'}.  All arithmetic is float64 (Python floats)."""
import collections
import math

import numpy as np

EPS = float(np.spacing(1))
COCO_SIGMAS = [v / 10.0 for v in (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89)]
CROWDPOSE_SIGMAS = [v / 10.0 for v in (.79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89, .79, .79)]
THR = [float(v) for v in np.linspace(.5, .95, 10)]
REC = [float(v) for v in np.linspace(0, 1, 101)]
AREA_RNG = [(0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]
NAMES = ['AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']


def gt_ignore(g):
    return bool(g['iscrowd']) or g['num_keypoints'] == 0


def det_area(d, J):
    xs = [float(d['kpts'][j][0]) for j in range(J)]
    ys = [float(d['kpts'][j][1]) for j in range(J)]
    return (max(xs) - min(xs)) * (max(ys) - min(ys))


def oks(d, g, sigmas):
    J = len(sigmas)
    k1 = sum(1 for j in range(J) if g['kpts'][j][2] > 0)
    area = float(g['area'])
    total, used = 0.0, 0
    if k1 == 0:
        bx, by, bw, bh = (float(v) for v in g['bbox'])
        x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
    for j in range(J):
        xd, yd = float(d['kpts'][j][0]), float(d['kpts'][j][1])
        if k1 > 0:
            if not g['kpts'][j][2] > 0:
                continue
            dx = xd - float(g['kpts'][j][0])
            dy = yd - float(g['kpts'][j][1])
        else:
            dx = max(0.0, x0 - xd) + max(0.0, xd - x1)
            dy = max(0.0, y0 - yd) + max(0.0, yd - y1)
        var = (sigmas[j] * 2) * (sigmas[j] * 2)
        e = (dx * dx + dy * dy) / var / (area + EPS) / 2
        total = total + math.exp(-e)
        used += 1
    return total / used


def evaluate_image(dets, gts, sigmas, thr=THR, area_rng=AREA_RNG, max_dets=20):
    """-> {'src': record index of each kept detection in score order, 'scores', 'oks': [kept][G],
    'match' / 'ignore': [A][T][kept] bools, 'gt_ignore': [A][G] bools}."""
    J = len(sigmas)
    src = sorted(range(len(dets)), key=lambda i: -dets[i]['score'])[:max_dets]        # sorted() is stable
    table = [[oks(dets[i], g, sigmas) for g in gts] for i in src]
    out = {'src': src, 'scores': [dets[i]['score'] for i in src], 'oks': table, 'match': [], 'ignore': [],
           'gt_ignore': []}
    for lo, hi in area_rng:
        ig = [gt_ignore(g) or g['area'] < lo or g['area'] > hi for g in gts]
        order = [k for k in range(len(gts)) if not ig[k]] + [k for k in range(len(gts)) if ig[k]]
        m_a, i_a = [], []
        for t in thr:
            taken = set()
            m_t, i_t = [], []
            for row, i in enumerate(src):
                best, m = min(t, 1 - 1e-10), None
                for k in order:
                    if k in taken and not gts[k]['iscrowd']:
                        continue
                    if m is not None and not ig[m] and ig[k]:
                        break
                    if table[row][k] < best:
                        continue
                    best, m = table[row][k], k
                if m is not None:
                    taken.add(m)
                    m_t.append(True)
                    i_t.append(ig[m])
                else:
                    a = det_area(dets[i], J)
                    m_t.append(False)
                    i_t.append(a < lo or a > hi)
            m_a.append(m_t)
            i_a.append(i_t)
        out['match'].append(m_a)
        out['ignore'].append(i_a)
        out['gt_ignore'].append(ig)
    return out


def evaluate_set(dets_by_image, gts_by_image, image_ids, sigmas, thr=THR, area_rng=AREA_RNG, max_dets=20):
    """Per image id of the evaluated set (missing keys: nothing) -> {id: evaluate_image result, or None for an image with
    neither detections nor annotations}."""
    out = collections.OrderedDict()
    for i in sorted(image_ids):
        d, g = dets_by_image.get(i, []), gts_by_image.get(i, [])
        out[i] = evaluate_image(d, g, sigmas, thr, area_rng, max_dets) if d or g else None
    return out


def accumulate(per_image, thr=THR, rec=REC, n_area=3):
    T, R = len(thr), len(rec)
    precision = -np.ones((T, R, n_area))
    recall = -np.ones((T, n_area))
    imgs = [per_image[i] for i in sorted(per_image) if per_image[i] is not None]
    for a in range(n_area):
        npig = sum(1 for e in imgs for ig in e['gt_ignore'][a] if not ig)
        if npig == 0:
            continue
        scores = [s for e in imgs for s in e['scores']]
        order = sorted(range(len(scores)), key=lambda i: -scores[i])
        nd = len(order)
        for t in range(T):
            m = [v for e in imgs for v in e['match'][a][t]]
            ig = [v for e in imgs for v in e['ignore'][a][t]]
            tp = fp = 0
            rc, pr = [], []
            for i in order:
                if m[i] and not ig[i]:
                    tp += 1
                if not m[i] and not ig[i]:
                    fp += 1
                rc.append(float(tp) / npig)
                pr.append(float(tp) / (float(fp) + float(tp) + EPS))
            recall[t, a] = rc[-1] if nd else 0
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            for r in range(R):
                pos = 0
                while pos < nd and rc[pos] < rec[r]:         # searchsorted, side = 'left'
                    pos += 1
                precision[t, r, a] = pr[pos] if pos < nd else 0
    return precision, recall


def summarize(precision, recall, thr=THR, labels=('all', 'medium', 'large')):
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    def at(table, a, iou):
        s = table[..., a]
        if iou is not None:
            s = s[[k for k, t in enumerate(thr) if t == iou]]
        return mean(s)

    out = collections.OrderedDict()
    for kind, table in (('AP', precision), ('AR', recall)):
        a = labels.index('all')
        out[kind] = at(table, a, None)
        out['Ap .5' if kind == 'AP' else 'AR .5'] = at(table, a, .5)
        out[kind + ' .75'] = at(table, a, .75)
        if 'medium' in labels:
            out[kind + ' (M)'] = at(table, labels.index('medium'), None)
        if 'large' in labels:
            out[kind + ' (L)'] = at(table, labels.index('large'), None)
    return out


def words(e, a_count, t_count):
    """The per-detection result words of lp_kpt_eval (bit a * n_thr + t) of one evaluate_image result."""
    mw, iw = [], []
    for row in range(len(e['src'])):
        m = i = 0
        for a in range(a_count):
            for t in range(t_count):
                m |= int(e['match'][a][t][row]) << (a * t_count + t)
                i |= int(e['ignore'][a][t][row]) << (a * t_count + t)
        mw.append(m)
        iw.append(i)
    return mw, iw


def results_to_dets(results, J):
    """The evaluator's result dicts (results.records_to_results) -> {image_id: detections} in list order."""
    out = {}
    for r in results:
        k = r['keypoints']
        out.setdefault(r['image_id'], []).append({'kpts': [(k[3 * j], k[3 * j + 1]) for j in range(J)],
                                                  'score': r['score']})
    return out


# ------------------------------------------------------------------ scenes
def person(rng, area, J, cx, cy):
    """An annotation of the given area: joints on a quarter-pixel grid (exact in fp32) inside a box of about 1.5 x area."""
    side = math.sqrt(area * 1.5)
    w, h = side * rng.uniform(0.6, 1.0), side * rng.uniform(0.9, 1.4)
    k = np.zeros((J, 3))
    k[:, 0] = np.round((cx + rng.uniform(-.5, .5, J) * w) * 4) / 4
    k[:, 1] = np.round((cy + rng.uniform(-.5, .5, J) * h) * 4) / 4
    k[:, 2] = rng.choice([0, 1, 2], J, p=[.2, .3, .5])
    k[0, 2] = 2
    return {'kpts': k, 'area': float(area), 'bbox': (float(cx - w / 2), float(cy - h / 2), float(w), float(h)),
            'iscrowd': 0, 'num_keypoints': int((k[:, 2] > 0).sum())}


def scene(seed=7, rows=48, pcap=30, J=17, T=2, J_eval=17, sigmas=COCO_SIGMAS, area_rng=AREA_RNG,
          n_gt=(0, 1, 5, 64, 3, 5, 1, 2, 4, 5, 1, 0, 2, 5, 3, 1, 5, 2, 1, 4, 5, 3, 2), n_det=(0, 1, 20, 27, 6, 3, 27, 9, 1, 20, 4), pad_rows=(13, 47), check=True):
    """-> dict: the fp32 records of ``rows`` rows (``pad_rows`` are padding: id -1, counts and values of a real image),
    ``image_ids`` per row, the annotations ``gts`` {id: [annotation]} of every image of the set (one more than the rows
    show: an image that is never added), and ``dets`` {id: [detection]} as the records hold them.  Image ids are
    scattered, so the ascending-id order differs from the row order.  With ``check`` the conditions the tests need are
    ASSERTED (module docstring of tests/test_gpu_cocoeval.py)."""
    rng = np.random.RandomState(seed)
    D = 3 + T
    kpts = np.zeros((rows, pcap, J, D), np.float32)
    count = np.zeros(rows, np.int32)
    scores = np.zeros((rows, pcap), np.float32)
    live = [r for r in range(rows) if r not in pad_rows]
    ids = rng.permutation(np.arange(100, 100 + 3 * (len(live) + 1), 3))[:len(live) + 1]
    image_ids = [-1] * rows
    gts, dets = {}, {}
    areas = [500.0, 1023.0, 1024.0, 1500.0, 4000.0, 9216.0, 9217.0, 15000.0, 40000.0]
    noise = [0.0, 0.005, 0.01, 0.02, 0.03, 0.05, 0.1]
    for n, r in enumerate(live + [None]):
        iid = int(ids[n])
        G = n_gt[n % len(n_gt)] if r is not None else 2
        gl = []
        for k in range(G):
            g = person(rng, areas[rng.randint(len(areas))], J_eval, rng.uniform(100, 540), rng.uniform(100, 380))
            kind = rng.uniform()
            if kind < .08:                                   # a crowd region with labelled joints
                g['iscrowd'] = 1
            elif kind < .16:                                 # a crowd region as COCO has them: no keypoints
                g['iscrowd'] = 1
                g['kpts'][:, 2] = 0
                g['num_keypoints'] = 0
            elif kind < .24:                                 # a person without labelled keypoints
                g['kpts'][:, 2] = 0
                g['num_keypoints'] = 0
            gl.append(g)
        if G >= 5:                                           # a duplicated annotation: equal OKS by construction
            gl[3] = dict(gl[1], kpts=gl[1]['kpts'].copy())
        gts[iid] = gl
        if r is None:
            break
        image_ids[r] = iid
        nd = n_det[n % len(n_det)]
        count[r] = nd
        for p in range(nd):
            if gl and rng.uniform() < .8:
                g = gl[p % len(gl) if rng.uniform() < .7 else rng.randint(len(gl))]
                level = rng.randint(len(noise))
                s = noise[level] * math.sqrt(g['area'])
                xy = g['kpts'][:, :2] + rng.normal(0, 1, (J_eval, 2)) * s
                if g['num_keypoints'] == 0:                  # aim at the box, inside and outside its doubled form
                    xy = xy + rng.choice([0.0, 1.5]) * g['bbox'][2]
                conf = 0.9 - 0.12 * level
                conf += rng.uniform(-.25, .25)
            else:
                xy = person(rng, areas[rng.randint(len(areas))], J_eval, rng.uniform(100, 540),
                            rng.uniform(100, 380))['kpts'][:, :2]
                conf = rng.uniform(.05, .6)
            kpts[r, p, :J_eval, :2] = xy
            kpts[r, p, J_eval:, :2] = rng.uniform(0, 640, (J - J_eval, 2))       # a centre joint far from the rest
            kpts[r, p, :, 2:] = rng.uniform(0, 1, (J, D - 2))
            scores[r, p] = round(float(np.clip(conf, .01, .99)), 1 if p % 3 == 0 else 3)   # one decimal: ties
        # past count: what a record holds there must not matter
        kpts[r, nd:] = rng.uniform(0, 640, (pcap - nd, J, D))
        scores[r, nd:] = rng.uniform(0, 1, pcap - nd)
        dets[iid] = [{'kpts': kpts[r, p, :, :2].astype(np.float64), 'score': float(scores[r, p])} for p in range(nd)]
    for r in pad_rows:                                       # padding repeats a real row (evaluate()'s plan does)
        kpts[r], count[r], scores[r] = kpts[live[2]], count[live[2]], scores[live[2]]
    sc = {'kpts': kpts, 'count': count, 'scores': scores, 'image_ids': image_ids, 'gts': gts, 'dets': dets,
          'all_ids': sorted(int(v) for v in ids), 'J_eval': J_eval, 'sigmas': list(sigmas), 'area_rng': list(area_rng),
          'pcap': pcap, 'J': J, 'T': T}
    sc['ref'] = evaluate_set(dets, gts, sc['all_ids'], sc['sigmas'], THR, sc['area_rng'])
    labels = ('all', 'medium', 'large')[:len(area_rng)]
    sc['tables'] = accumulate(sc['ref'], THR, REC, len(area_rng))
    sc['stats'] = summarize(sc['tables'][0], sc['tables'][1], THR, labels)
    if check:
        check_scene(sc)
    return sc


def check_scene(sc):
    """The scene decides what it is meant to decide: no OKS on a knife's edge, every range populated, AP mid-range."""
    for e in sc['ref'].values():
        if e is None:
            continue
        for row in e['oks']:
            for v in row:
                assert all(abs(v - t) > 1e-9 for t in THR), ('OKS within 1e-9 of a threshold', v)
            cand = sorted(v for v in row if v > THR[0] - 1e-9)
            for u, v in zip(cand, cand[1:]):
                assert u == v or v - u > 1e-9, ('two OKS values a detection chooses between within 1e-9', u, v)
    for a in range(len(sc['area_rng'])):
        npig = sum(1 for e in sc['ref'].values() if e for ig in e['gt_ignore'][a] if not ig)
        assert npig > 0, ('area range without a countable annotation', a)
    assert 0.2 < sc['stats']['AP'] < 0.9, sc['stats']


def ground_truth_arrays(gts, all_ids):
    """{id: [annotation]} -> the arguments of litepose_amd.coco_eval.GroundTruth.from_arrays."""
    ann, k, area, bbox, crowd, nk = [], [], [], [], [], []
    for i in all_ids:
        for g in gts.get(i, []):
            ann.append(i)
            k.append(np.asarray(g['kpts'], np.float64))
            area.append(g['area'])
            bbox.append(g['bbox'])
            crowd.append(g['iscrowd'])
            nk.append(g['num_keypoints'])
    J = k[0].shape[0] if k else 17
    return (all_ids, ann, np.asarray(k, np.float64).reshape(len(k), J, 3), area,
            np.asarray(bbox, np.float64).reshape(len(k), 4), crowd, nk)
