"""COCO keypoint AP from the engine's device records: the number valid.py prints last and the architecture search ranks
a candidate by (calibrate_test.py returns ``name_values['AP']``).

The protocol is the published ``COCOeval`` algorithm for ``iouType='keypoints'`` (DESIGN.md 4b spells it out).  Its heavy
part -- OKS of every detection against every annotation of its image, and the greedy matching at every threshold and
area range -- is ONE HIP launch per batch (``lp_kpt_eval``, csrc/eval_kernels.hip) on the records as they sit on the
device after ``lp_final_preds_v``; per kept detection it leaves a score, a word of match bits and a word of ignore bits
(12 bytes).  The accumulation into the precision / recall tables and the ten summary numbers is vectorised NumPy here: it
needs a global stable sort, and pycocotools does that part vectorised too.

HONESTY CLAUSE.  pycocotools was not available where this was written and is not part of the reference checkout.  The
protocol is therefore pinned against a plain restatement in tests/_cocoeval_ref.py, written from the description, plus
hand-computed cases -- NOT against pycocotools itself: "parity-unpinned", the status of the cv2 warp.  The JSON route
(``evaluate()`` -> ``results.write_results`` -> ``COCOeval``) stays the way to cross-check where pycocotools exists
(INTEGRATION.md).

crowdposetools' easy / medium / hard split by crowd index is out of scope.  Sigmas, annotation areas and the area
ranges are inputs: a 14-joint set with one area range yields the six numbers that do not depend on the area.
"""
import collections
import ctypes as C
import json

import numpy as np
import torch

from . import _native as nv

# pycocotools cocoeval.py (17 joints) and crowdposetools cocoeval.py (14 joints): the published per-joint sigmas
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
CROWDPOSE_SIGMAS = np.array([.79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89, .79, .79]) / 10.0

AREA_RANGES = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
AREA_LABELS = ('all', 'medium', 'large')
MAX_ANNOTATIONS = 64                     # per image: the kernel's matched set is one 64-bit mask
MAX_DETS = 20


def default_thresholds():
    return np.linspace(.5, .95, 10)


def recall_grid():
    return np.linspace(0, 1, 101)


class GroundTruth(object):
    """The annotation tables of ``lp_kpt_eval`` in ascending image-id order (host arrays; a KeypointEvaluator puts them
    on its device): ``image_ids`` [I], ``first`` [I+1] prefix offsets, ``kpts`` [G,J,3] (x, y, v), ``area`` [G], ``bbox``
    [G,4] (x, y, w, h), ``flags`` [G] (bit 0 iscrowd, bit 1 ignore = iscrowd or num_keypoints == 0)."""

    def __init__(self, image_ids, first, kpts, area, bbox, flags):
        self.image_ids = np.asarray(image_ids, np.int64)
        self.first = np.asarray(first, np.int32)
        self.kpts = np.ascontiguousarray(kpts, np.float64)
        self.area = np.ascontiguousarray(area, np.float64)
        self.bbox = np.ascontiguousarray(bbox, np.float64)
        self.flags = np.ascontiguousarray(flags, np.int32)
        self.num_joints = int(self.kpts.shape[1])
        self.slot = {int(v): i for i, v in enumerate(self.image_ids)}

    @classmethod
    def from_arrays(cls, image_ids, ann_image_ids, kpts, area, bbox, iscrowd=None, num_keypoints=None):
        """``image_ids``: the images of the set (any order, no repeats).  One row per annotation in ``ann_image_ids``
        [G], ``kpts`` [G,J,3], ``area`` [G], ``bbox`` [G,4]; ``iscrowd`` default 0, ``num_keypoints`` default the number
        of joints with v > 0.  An image's annotations keep the order they are given in."""
        ids = np.asarray(list(image_ids), np.int64).reshape(-1)
        if len(set(ids.tolist())) != ids.size:
            raise ValueError('image ids must be unique')
        ids = np.sort(ids)
        ann = np.asarray(ann_image_ids, np.int64).reshape(-1)
        G = ann.size
        kpts = np.asarray(kpts, np.float64)
        if kpts.ndim == 2:
            kpts = kpts.reshape(G, -1, 3)
        if kpts.ndim != 3 or kpts.shape[0] != G or kpts.shape[2] != 3 or kpts.shape[1] < 1:
            raise ValueError('kpts must be [G, J, 3]')
        area = np.asarray(area, np.float64).reshape(-1)
        bbox = np.asarray(bbox, np.float64).reshape(-1, 4)
        crowd = np.zeros(G, np.int64) if iscrowd is None else np.asarray(iscrowd, np.int64).reshape(-1)
        nk = (kpts[:, :, 2] > 0).sum(axis=1) if num_keypoints is None else np.asarray(num_keypoints, np.int64).reshape(-1)
        if not (area.size == bbox.shape[0] == crowd.size == nk.size == G):
            raise ValueError('one area, bbox, iscrowd and num_keypoints per annotation is required')
        slot = {int(v): i for i, v in enumerate(ids)}
        unknown = sorted(set(ann.tolist()) - set(slot))
        if unknown:
            raise ValueError('annotations of images outside the set: %s' % unknown[:5])
        rows = np.array([slot[int(v)] for v in ann], np.int64)
        order = np.argsort(rows, kind='stable')
        per = np.bincount(rows, minlength=ids.size) if G else np.zeros(ids.size, np.int64)
        if per.size and per.max() > MAX_ANNOTATIONS:
            raise ValueError('image %d has %d annotations: at most %d per image are supported'
                             % (ids[int(per.argmax())], per.max(), MAX_ANNOTATIONS))
        first = np.concatenate([[0], np.cumsum(per)])
        flags = (crowd != 0).astype(np.int32) | (((crowd != 0) | (nk == 0)).astype(np.int32) << 1)
        return cls(ids, first, kpts[order], area[order], bbox[order], flags[order])

    @classmethod
    def from_coco(cls, dict_or_path, category_id=1):
        """The ``images`` / ``annotations`` of a COCO keypoint file (a dict, or the path of the JSON): the annotations
        of ``category_id`` whose image is listed, in file order per image.  Needs only json and NumPy."""
        data = dict_or_path
        if not isinstance(data, dict):
            with open(data) as f:
                data = json.load(f)
        ids = [int(im['id']) for im in data['images']]
        known = set(ids)
        anns = [a for a in data.get('annotations', ())
                if int(a.get('category_id', category_id)) == int(category_id) and int(a['image_id']) in known]
        if anns:
            J = len(anns[0]['keypoints']) // 3
        else:
            J = 17
        kpts = np.zeros((len(anns), J, 3))
        for i, a in enumerate(anns):
            k = np.asarray(a['keypoints'], np.float64)
            if k.size != J * 3:
                raise ValueError('annotation %s: %d keypoint values, %d expected' % (a.get('id'), k.size, J * 3))
            kpts[i] = k.reshape(J, 3)
        return cls.from_arrays(ids, [a['image_id'] for a in anns], kpts, [a['area'] for a in anns],
                               np.asarray([a['bbox'] for a in anns], np.float64).reshape(-1, 4),
                               [int(a.get('iscrowd', 0)) for a in anns], [int(a['num_keypoints']) for a in anns])


def accumulate(image_slots, num, scores, match, ignore, gt, evaluated, thresholds, area_ranges):
    """COCOeval.accumulate for one category and one maxDets, vectorised.  Per evaluated row r (any order; one row per
    image at most): ``image_slots`` [R] slot in ``gt``, ``num`` [R] kept detections, ``scores`` [R,D] sorted descending,
    ``match`` / ``ignore`` [R,D] words with bit a * n_thr + t.  ``evaluated``: boolean [I] over the slots of ``gt``
    (npig counts every evaluated image, with detections or not).  -> precision [T,R101,A], recall [T,A], -1 where an
    area range has no countable annotation."""
    thr = np.asarray(thresholds, np.float64)
    rec = recall_grid()
    T, R, A = thr.size, rec.size, len(area_ranges)
    precision = -np.ones((T, R, A))
    rec_out = -np.ones((T, A))
    eps = np.spacing(1)
    image_slots = np.asarray(image_slots, np.int64).reshape(-1)
    num = np.asarray(num, np.int64).reshape(-1)
    order = np.argsort(image_slots, kind='stable')            # ascending image id = ascending slot
    D = scores.shape[1] if scores.ndim == 2 else 0
    keep = (np.arange(D)[None, :] < num[order, None]) if order.size else np.zeros((0, D), bool)
    sc = np.asarray(scores, np.float32)[order][keep].astype(np.float64)
    mw = np.asarray(match).astype(np.uint32)[order][keep]
    iw = np.asarray(ignore).astype(np.uint32)[order][keep]
    inds = np.argsort(-sc, kind='mergesort')
    mw, iw = mw[inds], iw[inds]
    nd = sc.size
    ann_eval = np.repeat(np.asarray(evaluated, bool), np.diff(gt.first))
    for a, (lo, hi) in enumerate(area_ranges):
        gt_ig = ((gt.flags & 2) != 0) | (gt.area < lo) | (gt.area > hi)
        npig = int(np.count_nonzero(~gt_ig & ann_eval))
        if npig == 0:
            continue
        for t in range(T):
            bit = np.uint32(1) << np.uint32(a * T + t)
            m = (mw & bit) != 0
            ig = (iw & bit) != 0
            tp = np.cumsum(m & ~ig).astype(np.float64)
            fp = np.cumsum(~m & ~ig).astype(np.float64)
            rc = tp / npig
            pr = tp / (fp + tp + eps)
            rec_out[t, a] = rc[-1] if nd else 0
            pr = np.maximum.accumulate(pr[::-1])[::-1]      # non-increasing from the right
            pos = np.searchsorted(rc, rec, side='left')
            q = np.zeros(R)
            ok = pos < nd
            q[ok] = pr[pos[ok]]
            precision[:, :, a][t] = q
    return precision, rec_out


def summarize(precision, recall, thresholds, area_labels):
    """COCOeval.summarize for keypoints: the names of COCODataset.py:302 whose area range is present."""
    thr = np.asarray(thresholds, np.float64)

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    def pick(table, a, iou):
        s = table[..., a]
        if iou is not None:
            s = s[np.where(iou == thr)[0]]
        return mean(s)

    out = collections.OrderedDict()
    labels = list(area_labels)
    for kind, table in (('AP', precision), ('AR', recall)):
        if 'all' in labels:
            a = labels.index('all')
            out[kind] = pick(table, a, None)
            out['Ap .5' if kind == 'AP' else 'AR .5'] = pick(table, a, .5)
            out[kind + ' .75'] = pick(table, a, .75)
        if 'medium' in labels:
            out[kind + ' (M)'] = pick(table, labels.index('medium'), None)
        if 'large' in labels:
            out[kind + ' (L)'] = pick(table, labels.index('large'), None)
    return out


class KeypointEvaluator(object):
    """COCO keypoint AP over the images of ``gt``.

        ev = KeypointEvaluator(GroundTruth.from_coco(path))
        engine.evaluate(images, image_ids=ids, evaluator=ev)     # or ev.add(kpts, count, scores, ids) per batch
        ev.summarize()['AP']

    ``sigmas`` default: COCO's 17 or CrowdPose's 14 by the number of evaluated joints.  ``num_joints``: the first
    joints of a record that are evaluated (default: the annotations').  ``evaluated_ids`` restricts the set like
    ``params.imgIds``; an image of the set that was never added counts with zero detections."""

    def __init__(self, gt, sigmas=None, num_joints=None, device=None, evaluated_ids=None, area_ranges=None):
        self.gt = gt
        self.J_eval = int(gt.num_joints if num_joints is None else num_joints)
        if self.J_eval != gt.num_joints:
            raise ValueError('num_joints %d differs from the annotations\' %d' % (self.J_eval, gt.num_joints))
        if sigmas is None:
            if self.J_eval not in (14, 17):
                raise ValueError('sigmas are required for %d joints' % self.J_eval)
            sigmas = COCO_SIGMAS if self.J_eval == 17 else CROWDPOSE_SIGMAS
        self.sigmas = np.ascontiguousarray(sigmas, np.float64).reshape(-1)
        if self.sigmas.size != self.J_eval:
            raise ValueError('one sigma per evaluated joint is required')
        self.thr = default_thresholds()
        self.area_ranges = np.ascontiguousarray(AREA_RANGES if area_ranges is None else area_ranges,
                                                np.float64).reshape(-1, 2)
        if not 1 <= len(self.area_ranges) <= len(AREA_LABELS):
            raise ValueError('one to three area ranges (all, medium, large) are required')
        self.area_labels = AREA_LABELS[:len(self.area_ranges)]
        self.max_dets = MAX_DETS
        if int(np.diff(gt.first).max(initial=0)) > MAX_ANNOTATIONS:
            raise ValueError('an image has more than %d annotations' % MAX_ANNOTATIONS)
        self.device = torch.device('cuda' if device is None else device)
        self.evaluated = np.ones(len(gt.image_ids), bool)
        if evaluated_ids is not None:
            self.evaluated[:] = False
            for v in evaluated_ids:
                if int(v) not in gt.slot:
                    raise ValueError('evaluated id %s is not an image of the ground truth' % v)
                self.evaluated[gt.slot[int(v)]] = True
        self._dev = None
        self._added = set()
        self._queue = []                      # (slots of the rows, device block: num [N], then score / src / match / ignore [N, max_dets])
        self.precision = self.recall = self.stats = None

    def _tables(self):
        if self._dev is None:
            g, dev = self.gt, self.device

            def up(a, shape):                 # never an empty tensor: the C call refuses null pointers
                t = torch.zeros(shape, dtype=torch.from_numpy(a).dtype)
                t[:a.shape[0]] = torch.from_numpy(a)
                return t.to(dev)
            G = max(len(g.area), 1)
            self._dev = (up(g.kpts, (G, self.J_eval, 3)), up(g.area, (G,)), up(g.bbox, (G, 4)), up(g.flags, (G,)),
                         up(g.first, (len(g.first),)))
        return self._dev

    def slots_of(self, image_ids):
        """The ground-truth slot of every id (-1: a padding row, or an image outside ``evaluated_ids``) and the set of
        real ids; raises for an id outside the ground truth and for an id given or added twice.  Changes nothing."""
        slots, seen = [], set()
        for v in image_ids:
            v = int(v)
            if v == -1:
                slots.append(-1)
                continue
            if v not in self.gt.slot:
                raise ValueError('image id %d is not part of the ground truth' % v)
            if v in self._added or v in seen:
                raise ValueError('image id %d was added twice' % v)
            seen.add(v)
            k = self.gt.slot[v]
            slots.append(k if self.evaluated[k] else -1)
        return slots, seen

    def add(self, kpts, count, scores, image_ids):
        """One batch of device records (kpts [N,pcap,J,3+T] fp32, count [N] int32, scores [N,pcap] fp32, as
        ``PoseEngine.submit`` hands them over) with the image id of every row; -1 marks a padding row.  One launch on
        the current stream; the compact outputs stay on the device until ``accumulate``.  An id outside the ground
        truth and an id added twice raise; an image outside ``evaluated_ids`` is skipped."""
        ids = [int(v) for v in image_ids]
        N, pcap, J, D = kpts.shape
        if len(ids) != N or tuple(count.shape) != (N,) or tuple(scores.shape) != (N, pcap):
            raise ValueError('kpts [N,pcap,J,3+T], count [N], scores [N,pcap] and one image id per row are required')
        if kpts.dtype != torch.float32 or scores.dtype != torch.float32 or count.dtype != torch.int32:
            raise ValueError('fp32 records and int32 counts are required')
        if D < 3:
            raise ValueError('kpts rows are (x, y, val, tags...)')
        slots, seen = self.slots_of(ids)
        rows = torch.tensor(slots, dtype=torch.int32).to(kpts.device)
        # num [N], then score / src / match / ignore [N, max_dets]: one block, one D2H
        block = torch.empty(N * (1 + 4 * self.max_dets), dtype=torch.int32, device=kpts.device)
        self._launch(kpts, count, scores, rows, block)
        self._added |= seen
        self._queue.append((np.asarray(slots, np.int64), block))
        self.precision = None

    def _launch(self, kpts, count, scores, rows, block):
        """The one lp_kpt_eval launch of ``add`` on the current stream (``rows``: device int32 slots; ``block``: the
        device int32 output block).  Allocates nothing once the tables are on the device: capturable."""
        N, pcap, J, D = kpts.shape
        M = self.max_dets
        gk, ga, gb, gf, g1 = self._tables()
        reg = [C.c_void_p(block.data_ptr() + 4 * (N + k * N * M)) for k in range(4)]
        dbl = C.POINTER(C.c_double)
        nv.check(nv.lib().lp_kpt_eval(
            nv.dptr(kpts), nv.dptr(count), nv.dptr(scores), N, pcap, J, D - 3, self.J_eval, nv.dptr(rows),
            nv.dptr(gk), nv.dptr(ga), nv.dptr(gb), nv.dptr(gf), nv.dptr(g1), len(self.gt.image_ids),
            self.sigmas.ctypes.data_as(dbl), self.thr.ctypes.data_as(dbl), int(self.thr.size),
            self.area_ranges.ctypes.data_as(dbl), int(len(self.area_ranges)), M,
            reg[0], nv.dptr(block), reg[1], reg[2], reg[3], None, nv.stream_ptr()), 'lp_kpt_eval')

    def _collect(self):
        """ONE D2H of everything queued -> (slots, num, scores, src, match, ignore) of the evaluated rows."""
        M = self.max_dets
        if not self._queue:
            z = np.zeros((0, M))
            return np.zeros(0, np.int64), np.zeros(0, np.int64), z.astype(np.float32), z, z, z
        torch.cuda.synchronize(self.device)
        slots = np.concatenate([s for s, _ in self._queue])
        flat = torch.cat([b for _, b in self._queue]).cpu().numpy()
        out, off = [], 0
        for s, _ in self._queue:
            n = len(s)
            out.append((flat[off:off + n],) + tuple(flat[off + n + k * n * M:off + n + (k + 1) * n * M].reshape(n, M)
                                                    for k in range(4)))
            off += n * (1 + 4 * M)
        num = np.concatenate([o[0] for o in out]).astype(np.int64)
        sc, src, mw, iw = (np.concatenate([o[k] for o in out]) for k in range(1, 5))
        live = slots >= 0
        return (slots[live], num[live], sc[live].view(np.float32), src[live], mw[live].view(np.uint32),
                iw[live].view(np.uint32))

    def accumulate(self):
        slots, num, sc, _, mw, iw = self._collect()
        self.precision, self.recall = accumulate(slots, num, sc, mw, iw, self.gt, self.evaluated, self.thr,
                                                 [tuple(r) for r in self.area_ranges])
        return self.precision, self.recall

    def summarize(self):
        """-> OrderedDict of 'AP', 'Ap .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)'
        (COCODataset.py:302; without a medium / large range those entries are absent)."""
        if self.precision is None:
            self.accumulate()
        out = summarize(self.precision, self.recall, self.thr, self.area_labels)
        self.stats = list(out.values())
        return out
