"""Dataset evaluation on the batched engine: decoded images of any mix of sizes -> the evaluator's result dicts.

The reference evaluates one image at a time (valid.py:195-233): per image ``get_multi_scale_size`` gives the network
input size (``base_size``), centre and scale (lib/utils/transforms.py:155-176), ``resize_align_multi_scale`` warps the
image with that image's own affine (:179-192) and ``get_final_preds`` maps the grouped joints back with the same centre
and scale (:195-202).  Here:

  plan      images are bucketed by their network input size (w_resized, h_resized); inside a bucket batches of
            ``batch_size`` are cut and the last one is padded with repeats of a real image (their records are dropped),
            so every batch of a bucket has ONE shape and the engine's captured graphs are reused.  Buckets run one
            after the other: a buffer set keeps _MAX_SHAPES shapes, interleaving would evict graphs.
  loader    per buffer set: the batch's uint8 sources packed back to back in pinned host memory, a descriptor table
            (lp_warp_desc: offset, size, inverted matrix) and a back-projection table ((sx, tx, sy, ty) per image),
            pinned and on the device, and the bucket's fp32 network input.  One H2D per table and ONE
            ``lp_preprocess_batch_v`` launch per batch, on the caller's stream (StagedLoader's rules: no fifth stream,
            a set is refilled only after its previous batch has been collected).  The next batch is packed in a
            worker thread (host memcpy, the GIL released) while the current one is submitted.
            When a bucket is done its batches are collected and ``PoseEngine.release_shape`` frees its buffers and
            graphs (at batch 64 a shape's network workspace alone is several GB per buffer set).
  records   ``PoseEngine.submit(x, preds_coef=table)``: the back-projection of every image runs on the device with its
            own centre / scale (lp_final_preds_v); records -> pinned host memory (StagedLoader.store / wait) ->
            ``results.records_to_results``, returned in input order.

Multi-scale testing (len(TEST.SCALE_FACTOR) > 1) and TEST.PROJECT2IMAGE = False (any number of scales) take the
multi-scale form of the same loop:

  plan      buckets are keyed by the tuple of network input sizes over all scales (``get_multi_scale_size`` per scale,
            with its int() truncation), not by the scale-1 size alone.
  loader    the sources are packed once; one descriptor table per scale (matrix ``get_affine_transform(center,
            scale_s, 0, size_s)``) and one ``lp_preprocess_batch_v`` launch per scale into that scale's input.
  engine    ``PoseEngine.submit(tuple of inputs, preds_coef=...)``: per scale the network and the stage merge, one
            ``lp_tta_merge_scales``, ``lp_parse`` on the merged maps.  The back-projection row is valid.py's: centre
            and scale of the last scale visited (min(SCALE_FACTOR)), heatmap size (Wf, Hf) of the merged maps -- the
            base size with TEST.PROJECT2IMAGE, else the first scale's stage-1 size.
  memory    every buffer set holds one network workspace per scale: a bucket whose workspaces over all scales and
            sets exceed the free device memory is refused with the largest batch size that fits.
TEST.SCALE_FACTOR lists the reference loop cannot run (several entries without a 1, or duplicates) raise ValueError.
"""
import collections
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import engine as _engine
from . import parallel as _par
from . import results as _results
from .core import inference as _inference
from .utils import transforms as _tf

Batch = collections.namedtuple('Batch', 'size rows real')
Batch.__doc__ = """One engine batch of the plan: ``size`` = (w, h) network input of its bucket, ``rows`` = input indices
(``batch_size`` of them; rows[real:] repeat a real image and are padding), ``real`` = number of real rows."""


def plan(shapes, input_size, min_scale, batch_size, scales=None):
    """Bucket plan (host only).  ``shapes``: (h, w) per image.  Buckets in order of first appearance, batches in input
    order inside a bucket; every batch has ``batch_size`` rows.  ``scales``: None = the single-scale plan (bucket key
    (w, h) at scale 1); a list of scale factors in the order valid.py visits them (sorted, descending) = the
    multi-scale plan, bucket key ((w, h) per scale)."""
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1')
    buckets = collections.OrderedDict()
    for i, hw in enumerate(shapes):
        hw = (int(hw[0]), int(hw[1]))
        if scales is None:
            size, _, _ = _tf.get_multi_scale_size(hw, input_size, 1.0, min_scale)
            key = (int(size[0]), int(size[1]))
        else:
            key = tuple(tuple(int(v) for v in _tf.get_multi_scale_size(hw, input_size, s, min_scale)[0])
                        for s in scales)
        buckets.setdefault(key, []).append(i)
    out = []
    for size, idx in buckets.items():
        for b in range(0, len(idx), batch_size):
            rows = idx[b:b + batch_size]
            out.append(Batch(size, tuple(rows + [rows[-1]] * (batch_size - len(rows))), len(rows)))
    return out


def bucket_histogram(batches):
    """{'WxH': images} of a plan (real rows only)."""
    h = collections.OrderedDict()
    for b in batches:
        k = '+'.join('%dx%d' % sz for sz in _sizes(b.size))
        h[k] = h.get(k, 0) + b.real
    return h


def in_input_order(batches, per_batch):
    """``per_batch[k]``: one item per real row of ``batches[k]`` -> the items indexed by input position."""
    n = sum(b.real for b in batches)
    out = [None] * n
    for b, items in zip(batches, per_batch):
        if len(items) != b.real:
            raise ValueError('one item per real row is required')
        for r in range(b.real):
            if out[b.rows[r]] is not None:
                raise ValueError('input %d planned twice' % b.rows[r])
            out[b.rows[r]] = items[r]
    if any(o is None for o in out):
        raise ValueError('the plan does not cover every input')
    return out


def _sizes(size):
    """A plan's bucket key as a tuple of (w, h), one per scale."""
    return size if isinstance(size[0], tuple) else (size,)


class _Transforms(object):
    """Per source size (h, w): the lp_warp_desc matrix and the lp_final_preds_coef row (both depend on the size only)."""

    def __init__(self, input_size, min_scale):
        self.input_size, self.min_scale = input_size, min_scale
        self._cache = {}

    def __call__(self, hw):
        t = self._cache.get(hw)
        if t is None:
            size, center, scale = _tf.get_multi_scale_size(hw, self.input_size, 1.0, self.min_scale)
            minv = _tf.warp_invert(_tf.get_affine_transform(center, scale, 0, size))
            t = (minv, _tf.final_preds_coef(center, scale, size))
            self._cache[hw] = t
        return t


class _ScaleTransforms(object):
    """Multi-scale form of _Transforms: per source size (h, w) one lp_warp_desc matrix per scale (``scales`` in
    visiting order) and the back-projection row of valid.py: centre / scale of the last scale visited, heatmap size of
    the merged maps (base size with ``project2image``, else the first scale's stage-1 size)."""

    def __init__(self, input_size, scales, project2image):
        self.input_size, self.scales, self.p2i = input_size, list(scales), bool(project2image)
        self.min_scale = min(self.scales)
        self._cache = {}

    def __call__(self, hw):
        t = self._cache.get(hw)
        if t is None:
            minvs, sizes = [], []
            for s in self.scales:
                size, center, scale = _tf.get_multi_scale_size(hw, self.input_size, s, self.min_scale)
                minvs.append(_tf.warp_invert(_tf.get_affine_transform(center, scale, 0, size)))
                sizes.append(size)
            if self.p2i:
                heatmap = _tf.get_multi_scale_size(hw, self.input_size, 1.0, self.min_scale)[0]
            else:
                heatmap = (int(sizes[0][0]) // 2, int(sizes[0][1]) // 2)
            t = (tuple(minvs), _tf.final_preds_coef(center, scale, heatmap))
            self._cache[hw] = t
        return t


class BucketLoader(_engine.StagedLoader):
    """StagedLoader for images of different sizes: one staging set per buffer set of the engine (see the module
    docstring).  The record half (``store`` / ``wait``) is StagedLoader's."""

    def __init__(self, engine, batch_size, src_capacity, transforms, mean=None, std=None, scales=1):
        """``scales``: number of scales (> 1 or a _ScaleTransforms: one descriptor table and network input per scale,
        ``start`` returns their tuple)."""
        dev = engine.device
        self.S = int(scales)
        self.multi = isinstance(transforms, _ScaleTransforms)
        self.nset = engine.buffer_sets()
        self.N = int(batch_size)
        self.mean = tuple(mean) if mean is not None else _tf.IMAGENET_MEAN
        self.std = tuple(std) if std is not None else _tf.IMAGENET_STD
        self.transforms = transforms
        cap = max(int(src_capacity), 1)
        nd = _tf.WARP_DESC_DTYPE.itemsize
        self.host_src = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(self.nset)]
        self.dev_src = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(self.nset)]
        # one table per scale, back to back: [S * N, 64] (one H2D)
        self.host_desc = [torch.zeros((self.S * self.N, nd), dtype=torch.uint8).pin_memory() for _ in range(self.nset)]
        self.dev_desc = [torch.empty((self.S * self.N, nd), dtype=torch.uint8, device=dev) for _ in range(self.nset)]
        self.host_coef = [torch.zeros((self.N, 4), dtype=torch.float64).pin_memory() for _ in range(self.nset)]
        self.dev_coef = [torch.empty((self.N, 4), dtype=torch.float64, device=dev) for _ in range(self.nset)]
        # NumPy views of the pinned buffers: the packing worker touches no torch / HIP call
        self._src_np = [t.numpy() for t in self.host_src]
        self._desc_np = [t.numpy().view(_tf.WARP_DESC_DTYPE).reshape(self.S, self.N) for t in self.host_desc]
        self._coef_np = [t.numpy() for t in self.host_coef]
        self.x = {}                              # (w, h) -> fp32 [N,3,h,w] network input per set, kept for the call
        self.nbytes = [0] * self.nset
        self.h2d_done = [None] * self.nset       # the pinned buffers of a set may be refilled once this has completed
        self.device = dev
        self.stream = None
        self.host_rec = [None] * self.nset
        self.rec_done = [None] * self.nset
        self.ready = [None] * self.nset

    def pack(self, i, batch, images):
        """Host side of set i (no HIP call: runs in the packing worker): sources back to back, descriptors, coefs.
        The caller has made sure the set's previous H2D is complete (``wait_free``)."""
        src, desc, coef = self._src_np[i], self._desc_np[i], self._coef_np[i]
        off = 0
        for r in range(batch.real):
            im = images[batch.rows[r]]
            n = im.size
            if off + n > src.shape[0]:
                raise ValueError('source buffer too small')
            np.copyto(src[off:off + n], im.reshape(-1))
            minv, c = self.transforms((im.shape[0], im.shape[1]))
            for s, m in enumerate(minv if self.multi else (minv,)):
                desc[s, r]['src_offset'], desc[s, r]['H'], desc[s, r]['W'] = off, im.shape[0], im.shape[1]
                desc[s, r]['minv'] = m
            coef[r] = c
            off += n
        for r in range(batch.real, self.N):      # padding: the last real image again (its bytes are already there)
            desc[:, r] = desc[:, batch.real - 1]
            coef[r] = coef[batch.real - 1]
        self.nbytes[i] = off

    def wait_free(self, i):
        if self.h2d_done[i] is not None:
            self.h2d_done[i].synchronize()
            self.h2d_done[i] = None

    def start(self, i, batch=None):
        """H2D of set i's packed sources and tables + the one lp_preprocess_batch_v launch per scale, on the caller's
        stream.  Returns the set's network input for the batch's bucket (multi-scale: the tuple of them)."""
        xs = []
        for w, h in _sizes(batch.size):
            x = self.x.get((w, h))
            if x is None:
                x = [torch.empty((self.N, 3, h, w), dtype=torch.float32, device=self.device) for _ in range(self.nset)]
                self.x[(w, h)] = x
            xs.append(x)
        n = self.nbytes[i]
        src = self.dev_src[i][:n]
        src.copy_(self.host_src[i][:n], non_blocking=True)
        self.dev_desc[i].copy_(self.host_desc[i], non_blocking=True)
        self.dev_coef[i].copy_(self.host_coef[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.h2d_done[i] = ev
        for s, (w, h) in enumerate(_sizes(batch.size)):
            _tf.preprocess_batch_v_device(src, self.dev_desc[i][s * self.N:(s + 1) * self.N], (w, h), out=xs[s][i],
                                          mean=self.mean, std=self.std)
        if self.multi:
            return tuple(x[i] for x in xs)
        return xs[0][i]

    def get(self, i):
        raise NotImplementedError('BucketLoader.start(i, batch) returns the set\'s network input')


def _check_cfg(cfg, engine):
    """-> the scales in visiting order, or None for the single-scale path (one scale, TEST.PROJECT2IMAGE).  The
    multi-scale path needs an engine that has it (PoseEngine: tuple inputs of submit, release_scales,
    ms_workspace_bytes); any other engine object is refused before its device is touched."""
    order, _ = _inference.scale_order(cfg)
    if len(order) == 1 and cfg.TEST.PROJECT2IMAGE:
        return None
    if not all(callable(getattr(engine, m, None)) for m in ('submit', 'release_scales', 'ms_workspace_bytes')):
        raise NotImplementedError('evaluate: multi-scale testing (len(TEST.SCALE_FACTOR) > 1) and TEST.PROJECT2IMAGE '
                                  '= False need an engine with the multi-scale path (PoseEngine.submit with one input '
                                  'per scale, release_scales); this engine has none.  Run the batch-1 drop-in modules '
                                  '(core.inference.get_multi_stage_outputs + aggregate_results, INTEGRATION.md 3)')
    return order


def _check_memory(engine, N, sizes):
    """A multi-scale bucket holds one network workspace per scale in every buffer set: refuse one that cannot fit
    (``sizes``: (w, h) per scale)."""
    hw = [(h, w) for w, h in sizes]
    need = engine.ms_workspace_bytes(N, hw)
    free, _ = torch.cuda.mem_get_info(engine.device)
    avail = free + torch.cuda.memory_reserved(engine.device) - torch.cuda.memory_allocated(engine.device)
    if need <= avail:
        return
    lo, hi = 0, N                              # the workspace grows with the batch: largest n that fits
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if engine.ms_workspace_bytes(mid, hw) <= avail:
            lo = mid
        else:
            hi = mid - 1
    raise ValueError('evaluate: batch_size %d needs %.1f GB of network workspaces for the %d scales %s over %d buffer '
                     'sets, %.1f GB of device memory is free; the largest batch size that fits is %d'
                     % (N, need / 1e9, len(sizes), '+'.join('%dx%d' % s for s in sizes), engine.buffer_sets(),
                        avail / 1e9, lo))


def evaluate(engine, images, image_ids=None, batch_size=64, num_joints=None, stats=None, evaluator=None):
    """valid.py:195-233 over a whole set, batched: ``images`` = HxWx3 uint8 arrays of any mix of sizes ->
    ``results.records_to_results`` dicts in input order, the list ``results.preds_to_results(all_preds, all_scores,
    image_ids)`` of the reference loop.  ``image_ids`` default: the input positions.  ``stats``: optional dict, filled
    with the bucket histogram and the time split (host packing, waiting for the device, records -> dicts).
    ``evaluator``: a ``coco_eval.KeypointEvaluator``; every collected batch's device records go to its ``add`` (one
    launch, padding rows marked -1) before they are copied to the host -- ``evaluator.summarize()`` afterwards is the
    set's AP.  The returned dicts are the same with and without it."""
    cfg = engine.cfg
    scales = _check_cfg(cfg, engine)
    images = [np.ascontiguousarray(im) for im in images]
    for k, im in enumerate(images):
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError('image %d: HxWx3 uint8 expected' % k)
    ids = list(range(len(images))) if image_ids is None else list(image_ids)
    if len(ids) != len(images):
        raise ValueError('one image id per image is required')
    if evaluator is not None:
        evaluator.slots_of(ids)              # an unknown or repeated id raises here, before anything is in flight
    if not images:
        return []
    t_start = time.perf_counter()
    min_scale = min(cfg.TEST.SCALE_FACTOR)
    input_size = int(cfg.DATASET.INPUT_SIZE)
    batches = plan([im.shape[:2] for im in images], input_size, min_scale, int(batch_size), scales)
    cap = max(sum(images[r].size for r in b.rows[:b.real]) for b in batches)
    if scales is None:
        tr = _Transforms(input_size, min_scale)
    else:
        tr = _ScaleTransforms(input_size, scales, cfg.TEST.PROJECT2IMAGE)
    for im in images:                        # filled here: the packing worker only reads the cache
        tr((im.shape[0], im.shape[1]))
    loader = BucketLoader(engine, batch_size, cap, tr, scales=1 if scales is None else len(scales))
    nset = loader.nset
    depth = min(engine.pipeline_depth(), nset - 1)     # a set is refilled only after its last batch was collected
    pcap, J, D = engine.pcap, engine.J, 3 + engine.T
    per_batch = [None] * len(batches)
    stored = [None] * nset                   # batch index whose records sit in set i's pinned host buffer
    t = {'pack_s': 0.0, 'wait_pack_s': 0.0, 'wait_device_s': 0.0, 'format_s': 0.0}

    def pack(i, k):
        t0 = time.perf_counter()
        loader.pack(i, batches[k], images)
        return time.perf_counter() - t0

    def drain(i):
        k = stored[i]
        if k is None:
            return
        t0 = time.perf_counter()
        flat = loader.wait(i)
        t1 = time.perf_counter()
        t['wait_device_s'] += t1 - t0
        kpts, count, scores = _par.unpack_records(flat, pcap, J, D)
        b = batches[k]
        res = _results.records_to_results(kpts[:b.real], count[:b.real], scores[:b.real],
                                          [ids[r] for r in b.rows[:b.real]], num_joints=num_joints)
        cnt = count[:b.real].numpy()
        bounds = np.concatenate([[0], np.cumsum(cnt)])
        per_batch[k] = [res[bounds[r]:bounds[r + 1]] for r in range(b.real)]
        t['format_s'] += time.perf_counter() - t1
        stored[i] = None

    def collect(pend):
        k, i, h = pend.popleft()
        drain(i)
        rec = h.result()
        if evaluator is not None:
            b = batches[k]
            evaluator.add(rec[0], rec[1], rec[2], [ids[r] for r in b.rows[:b.real]] + [-1] * (len(b.rows) - b.real))
        loader.store(i, *rec)
        h.release()
        stored[i] = k

    pend = collections.deque()
    with ThreadPoolExecutor(max_workers=1) as pool:
        fut = pool.submit(pack, 0, 0)
        for k, b in enumerate(batches):
            i = k % nset
            t0 = time.perf_counter()
            t['pack_s'] += fut.result()
            t['wait_pack_s'] += time.perf_counter() - t0
            if k and batches[k - 1].size != b.size:     # a bucket is done: free its buffers and graphs
                while pend:
                    collect(pend)
                if scales is None:
                    pw, ph = batches[k - 1].size
                    engine.release_shape(loader.N, ph, pw)
                else:
                    engine.release_scales(loader.N, [(ph, pw) for pw, ph in batches[k - 1].size])
                for sz in _sizes(batches[k - 1].size):
                    loader.x.pop(sz, None)
            if scales is not None and (k == 0 or batches[k - 1].size != b.size):
                _check_memory(engine, loader.N, b.size)
            x = loader.start(i, b)
            if k + 1 < len(batches):
                nxt = (k + 1) % nset
                loader.wait_free(nxt)            # the H2D of that set's previous batch (long enqueued)
                fut = pool.submit(pack, nxt, k + 1)
            pend.append((k, i, engine.submit(x, preds_coef=loader.dev_coef[i])))
            if len(pend) > depth:
                collect(pend)
        while pend:
            collect(pend)
        for i in range(nset):
            drain(i)
    out = [r for per_image in in_input_order(batches, per_batch) for r in per_image]
    if stats is not None:
        stats.update(t)
        stats['total_s'] = time.perf_counter() - t_start
        stats['batches'] = len(batches)
        stats['buckets'] = bucket_histogram(batches)
        stats['padding_rows'] = sum(len(b.rows) - b.real for b in batches)
        stats['src_bytes'] = int(sum(images[r].size for b in batches for r in b.rows[:b.real]))
    return out
