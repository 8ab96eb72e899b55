"""arch_search/acc_pred.py + calibrate_test.py:44-122: the accuracy of one candidate sub-network."""
import random
import time

import numpy as np
import torch

from .. import config as _config
from ..engine import PoseEngine
from ..models.pose_supermobilenet import SuperLitePose


class AccuracyEvaluator(object):
    """``predict_acc(cfg_arch)`` = ``calibrate_tester.test(copy.deepcopy(model), cfg_arch)``:

      * a copy of the supernet's tensors is calibrated (the reference deep-copies the model: one candidate must not move
        the statistics the next one starts from) on the ``calibration_set``'s augmented batches at ``img_size``;
      * the calibrated sub-network becomes a ``PoseEngine`` and runs the ``search_images`` (``engine.evaluate``: TEST.*
        of ``cfg`` as valid.py reads them);
      * a fresh evaluator from ``evaluator_factory()`` (a ``coco_eval.KeypointEvaluator`` over the search split's
        annotations) is fed the device records; its ``summarize()['AP']`` is returned.

    ``batch_size``: calibration images per step (TRAIN.IMAGES_PER_GPU x GPUs of the reference: 16 in supermobile.yaml).
    ``seed``: every call draws its augmentations from ``numpy.random.RandomState(seed)`` / ``random.Random(seed)``, so a
    candidate's score does not depend on which candidates were scored before it (the reference draws on from its global
    generators).  ``aug``: keyword parameters of ``dataset.calibration.draw_transform``.
    ``last_state_dict`` / ``last_stats`` / ``last_timing`` keep the last candidate's calibrated tensors, ``summarize()``
    dict and time split; its engine's buffers and graphs are released before ``predict_acc`` returns."""

    def __init__(self, cfg, supernet, calibration_set, search_images, search_ids, evaluator_factory, batch_size=16,
                 seed=0, eval_batch_size=64, momentum=0.1, **aug):
        self.cfg = cfg
        self.model = supernet
        self.calibration_set = calibration_set
        self.search_images = list(search_images)
        self.search_ids = list(search_ids)
        if len(self.search_images) != len(self.search_ids):
            raise ValueError('one image id per search image is required')
        self.evaluator_factory = evaluator_factory
        self.batch_size = int(batch_size)
        self.eval_batch_size = int(eval_batch_size)
        self.seed = seed
        self.momentum = momentum
        self.aug = aug
        self.last_state_dict = self.last_stats = self.last_timing = None

    def _calibration_batches(self, reso, timing):
        np_rng, py_rng = np.random.RandomState(self.seed), random.Random(self.seed)
        it = self.calibration_set.batches(reso, self.batch_size, np_rng, py_rng, **self.aug)
        while True:
            t0 = time.perf_counter()
            try:
                x = next(it)
            except StopIteration:
                return
            timing['loader_s'] += time.perf_counter() - t0
            yield x

    def predict_acc(self, cfg_arch):
        timing = {'loader_s': 0.0}
        t0 = time.perf_counter()
        model = SuperLitePose(self.cfg)
        model.load_state_dict(self.model.state_dict())
        reso = int(cfg_arch['img_size'])
        sd = model.calibrate(cfg_arch, self._calibration_batches(reso, timing), momentum=self.momentum)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        cfg = _config.apply_arch(self.cfg.clone(), cfg_arch)
        engine = PoseEngine(cfg, cfg_arch, sd, device=self.calibration_set.device)
        ev = self.evaluator_factory()
        t2 = time.perf_counter()
        stats = {}
        try:
            engine.evaluate(self.search_images, image_ids=self.search_ids, batch_size=self.eval_batch_size,
                            evaluator=ev, stats=stats)
            out = ev.summarize()
            timing['graph_captures'] = engine.graph_stats()['graph_captures']
        finally:
            engine.close()
            model.calibrated_net = None
        t3 = time.perf_counter()
        # calibrate_s includes the loader's share (host draws, descriptor upload and launch: loader_s)
        timing.update(calibrate_s=t1 - t0, engine_s=t2 - t1, evaluate_s=t3 - t2, total_s=t3 - t0)
        self.last_state_dict, self.last_stats, self.last_timing = sd, out, timing
        return out['AP']
