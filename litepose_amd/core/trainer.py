"""lib/core/trainer.py:do_train with the losses and their gradient on the device: ``loss_epoch``, the losses of a model over a
labelled set, and ``do_train``, one epoch of loss, backward and optimizer step for a torch model."""
import random

import torch
import torch.nn.functional as F

from ..nn.functional import train_resize
from .loss import MultiLossFactory


def loss_epoch(model, labelled_set, cfg, batch_size=16, np_rng=None, py_rng=None, loss_factory=None, **aug):
    """``model.forward`` on every batch of ``labelled_set`` (dataset.targets.LabelledSet; DATASET.INPUT_SIZE /
    OUTPUT_SIZE of ``cfg``, the augmentation ``aug`` as ``draw_sample`` takes it) and the ``MultiLossFactory`` of
    ``cfg`` on its outputs -> dict(heatmaps=[...], push=[...], pull=[...]): per stage the average of the per-batch
    means weighted by the batch size, as do_train's AverageMeter accumulates them (trainer.py:83-105); None where the
    term is off.  No backward, no optimizer step; the supernet's random-resolution resize (:49-59) is not applied."""
    factory = MultiLossFactory(cfg) if loss_factory is None else loss_factory
    S = factory.num_stages
    sums = dict(heatmaps=[None] * S, push=[None] * S, pull=[None] * S)
    count = 0
    for images, heatmaps, masks, joints in labelled_set.batches(cfg.DATASET.INPUT_SIZE, list(cfg.DATASET.OUTPUT_SIZE),
                                                                batch_size, np_rng, py_rng, **aug):
        outputs = model.forward(images)
        hl, push, pull = factory(outputs, heatmaps, masks, joints)
        n = int(images.shape[0])
        for key, vals in (('heatmaps', hl), ('push', push), ('pull', pull)):
            for idx, v in enumerate(vals):
                if v is not None:                      # heatmaps: the [N] tensor's mean over the batch (trainer.py:85)
                    w = v.mean().double() * n
                    sums[key][idx] = w if sums[key][idx] is None else sums[key][idx] + w
        count += n
    if count == 0:
        raise ValueError('loss_epoch: the labelled set yielded no batch')
    return {k: [None if v is None else float(v) / count for v in vals] for k, vals in sums.items()}


_KEYS = ('heatmaps', 'push', 'pull')


def _flat(batch):
    for part in batch:
        for t in (part if isinstance(part, (list, tuple)) else [part]):
            yield t


class CapturedStep(object):
    """One training step -- ``zero_grad`` (set to none), forward, loss, backward, ``optimizer.step()`` -- replayed as one
    captured graph.  ``step(images, heatmaps, masks, joints)`` follows the convention of the inference engine's buffer sets
    (DESIGN.md): a batch signature (shapes and dtypes of every tensor) runs eagerly at its first sight; at its second sight
    the batch is copied into static buffers, the step is captured (a capture enqueues nothing) and replayed once -- that
    replay IS the step; every later sight copies and replays.  A run through ``step`` therefore performs exactly the eager
    loop's sequence of updates, and the library's calls give the same bits launched or replayed.

    The loss terms never visit the host inside a step: slot ``k * NUM_STAGES + stage`` (k: heatmaps, push, pull) of a static
    fp32 tensor holds the last batch mean, the same slot of an fp64 tensor the running sum of ``mean.double() * n``;
    ``read()`` fetches both.  ``captures``, ``replays`` and ``eager_steps`` count what happened.

    ``optimizer`` must be a ``litepose_amd.optim`` optimizer: its ``lr`` and step counts live on the device, torch's own
    would be baked into the graph.  ``sync_hyperparameters()`` runs at the top of every step.  The model must be in
    training mode whenever ``step`` is called.  After a step ``p.grad`` holds that step's gradient, as in the eager loop.

    A graph holds raw addresses.  What may happen between two steps, and what ``step`` does about it (DESIGN.md 4f has
    the table with the test that pins each row):

      nothing needed   a changed ``lr`` (a scheduler), ``model.load_state_dict()`` (in place), ``model.eval()`` ... a
                       forward under ``no_grad`` ... ``model.train()``, ``optimizer.state_dict()``, another batch
                       signature, a new epoch (``reset_meters``)
      restores         ``p.grad`` after EVERY replay: ``optimizer.zero_grad()``, ``model.zero_grad()``, an eager step on
                       the same optimizer or another graph's replay in between change nothing about it
      invalidates      ``optimizer.load_state_dict()`` and ``optimizer.add_param_group()``: the optimizer's ``generation``
                       has moved, ``step`` calls ``invalidate()`` itself
      refuses          a changed betas / eps / weight_decay / momentum / nesterov: RuntimeError before anything is copied,
                       run or replayed; call ``invalidate()`` and go on with the new value
      the caller's     ``requires_grad_()`` on a parameter, or any other change of WHICH tensors a step touches: call
                       ``invalidate()``

    ``invalidate()`` drops every graph and forgets every sight (signatures start over: eager, then captured) and calls
    ``optimizer.forget_captures()``; ``invalidations`` counts them, the other counters keep counting.  One ``CapturedStep``
    per optimizer: a second one would see the first one's invalidations as events of its own."""

    def __init__(self, cfg, model, loss_factory, optimizer):
        from .. import optim
        if not isinstance(optimizer, (optim.Adam, optim.SGD)):
            raise TypeError('CapturedStep needs a litepose_amd.optim optimizer (lr and step counts on the device), got %s'
                            % type(optimizer).__name__)
        if not model.training:
            raise ValueError('CapturedStep: the model must be in training mode')
        self.model, self.loss_factory, self.optimizer = model, loss_factory, optimizer
        self.S = int(cfg.LOSS.NUM_STAGES)
        self.captures = self.replays = self.eager_steps = self.invalidations = 0
        self._sights, self._captured = {}, {}
        self._last = self._sums = None
        self._active = [False] * (3 * self.S)
        self._generation = optimizer.generation    # the optimizer's generation the sights and graphs belong to

    def invalidate(self):
        """Drop every graph and forget every sight: each signature runs eagerly at its next sight and is captured at the one
        after, against the optimizer as it then is.  Also ``optimizer.forget_captures()``."""
        if self._captured:
            torch.cuda.synchronize()               # no graph is destroyed while a replay of it may still be running
        self._sights, self._captured = {}, {}
        self.optimizer.forget_captures()
        self._generation = self.optimizer.generation
        self.invalidations += 1

    def reset_meters(self):
        """Zero the running sums (the start of an epoch)."""
        if self._sums is not None:
            self._sums.zero_()

    def read(self):
        """-> (last, sums): per slot the last batch mean and the running sum as Python floats, None where the term is off.
        One host read."""
        if self._last is None:
            return [None] * (3 * self.S), [None] * (3 * self.S)
        both = torch.cat([self._last.double(), self._sums]).tolist()
        n = 3 * self.S
        return ([v if a else None for v, a in zip(both[:n], self._active)],
                [v if a else None for v, a in zip(both[n:], self._active)])

    def _run(self, images, heatmaps, masks, joints):
        n = int(images.shape[0])
        self.optimizer.zero_grad(set_to_none=True)
        outputs = self.model(images)
        terms = self.loss_factory(outputs, heatmaps, masks, joints)
        loss = 0
        for idx in range(self.S):
            for k, vals in enumerate(terms):
                if vals[idx] is None:
                    continue
                v = vals[idx].mean(dim=0)
                slot = k * self.S + idx
                self._active[slot] = True
                d = v.detach()
                self._last[slot].copy_(d)
                self._sums[slot].add_(d.double() * n)
                loss = loss + v
        loss.backward()
        self.optimizer.step()

    def step(self, images, heatmaps, masks, joints):
        if not self.model.training:
            raise ValueError('CapturedStep: the model must be in training mode')
        if self.optimizer.generation != self._generation:    # load_state_dict / add_param_group: the graphs are stale
            self.invalidate()
        self.optimizer.sync_hyperparameters()                # refuses a by-value change here: nothing has been touched yet
        batch = (images, heatmaps, masks, joints)
        if self._last is None:
            self._last = torch.zeros(3 * self.S, dtype=torch.float32, device=images.device)
            self._sums = torch.zeros(3 * self.S, dtype=torch.float64, device=images.device)
        sig = tuple((tuple(t.shape), t.dtype) for t in _flat(batch))
        seen = self._sights.get(sig, 0)
        self._sights[sig] = seen + 1
        if seen == 0:
            self._run(*batch)
            self.eager_steps += 1
            return
        cap = self._captured.get(sig)
        if cap is None:
            static = tuple([torch.empty_like(t) for t in part] if isinstance(part, (list, tuple)) else torch.empty_like(part)
                           for part in batch)
            cap = dict(static=static, graph=torch.cuda.CUDAGraph())
            for dst, src in zip(_flat(static), _flat(batch)):
                dst.copy_(src)
            with torch.cuda.graph(cap['graph']):
                self._run(*static)
            cap['params'] = [p for g in self.optimizer.param_groups for p in g['params']]
            cap['grads'] = [p.grad for p in cap['params']]
            self._captured[sig] = cap
            self.captures += 1
        else:
            for dst, src in zip(_flat(cap['static']), _flat(batch)):
                dst.copy_(src)
        cap['graph'].replay()
        self.replays += 1
        for p, g in zip(cap['params'], cap['grads']):  # whatever the caller, an eager step or another graph left in p.grad
            if p.grad is not g:
                p.grad = g


def _do_train_captured(cfg, model, data_loader, loss_factory, optimizer, epoch, logger, graph):
    S = cfg.LOSS.NUM_STAGES
    freq = getattr(cfg, 'PRINT_FREQ', 1)
    model.train()
    if isinstance(graph, CapturedStep):
        stepper = graph
        if stepper.model is not model or stepper.optimizer is not optimizer or stepper.loss_factory is not loss_factory:
            raise ValueError('do_train: the CapturedStep was built for another model, loss factory or optimizer')
    else:
        stepper = CapturedStep(cfg, model, loss_factory, optimizer)
    stepper.reset_meters()
    count = 0
    for i, (images, heatmaps, masks, joints) in enumerate(data_loader):
        stepper.step(images, heatmaps, masks, joints)
        count += int(images.shape[0])
        if logger is not None and i % freq == 0:
            last, sums = stepper.read()
            logger.info('Epoch: [%d][%d]\t%s' % (epoch, i, '\t'.join(
                'Stage%d-%s: %.3e (%.3e)' % (idx, key, last[k * S + idx], sums[k * S + idx] / count)
                for k, key in enumerate(_KEYS) for idx in range(S) if last[k * S + idx] is not None)))
    if count == 0:
        raise ValueError('do_train: the data loader yielded no batch')
    last, sums = stepper.read()
    return {key: [None if last[k * S + idx] is None else (last[k * S + idx], sums[k * S + idx] / count) for idx in range(S)]
            for k, key in enumerate(_KEYS)}


SUPERNET_NAMES = ('pose_supermobilenet', 'pose_superresnet')


def random_resolution_size(cfg):
    """trainer.py:50: ``256 + 64 * random.randint(0, 4)`` for the reference's input size 512, the same five fractions of
    ``DATASET.INPUT_SIZE`` otherwise.  One draw from Python's ``random``."""
    return (256 + 64 * random.randint(0, 4)) * int(cfg.DATASET.INPUT_SIZE) // 512


def _bucket(model, group):
    """The model's GradBucket for ``group``: built once per (model, group) and kept on the model."""
    from ..parallel import GradBucket
    kept = getattr(model, '_grad_bucket', None)
    if kept is None or kept[0] is not group:
        kept = (group, GradBucket(model.parameters(), group))
        model._grad_bucket = kept
    return kept[1]


def do_train(cfg, model, data_loader, loss_factory, optimizer, epoch=0, teacher=None, logger=None, graph=False,
             random_resolution=None, group=None):
    """One epoch of trainer.py:41-113 for a ``torch.nn.Module`` whose ``model(images)`` gives the list of stage outputs:
    per batch ``(images, heatmaps, masks, joints)`` of ``data_loader`` (device tensors, as ``LabelledSet.batches`` yields
    them) the total loss of :82-105 through ``loss_factory`` (``core.loss.MultiLossFactory``), ``optimizer.zero_grad()``,
    ``loss.backward()`` -- one ``lp_pose_loss_grad`` call per factory call and stage -- and ``optimizer.step()``.

    ``teacher``: a callable on the images resized to 448 x 448 (:61-70); channels ``[0, DATASET.NUM_JOINTS)`` of its stage
    outputs, resized to the stage sizes (a quarter of the input, doubling per stage) and detached, are the targets of a
    second factory call whose heatmap losses join the total (:78-92; its tag terms are computed and dropped, as there).
    Unlike the reference the teacher is applied whatever ``MODEL.NAME`` says.

    -> dict(heatmaps=[...], push=[...], pull=[...]): per stage ``(last, average)`` of the batch means, the average weighted
    by the batch size as do_train's AverageMeter accumulates it; None where the term is off.  ``logger``: an object with
    ``info``; one line per ``cfg.PRINT_FREQ`` batches (every batch where ``cfg`` has no such key).

    ``graph``: True, or a ``CapturedStep`` kept by the caller so that its graphs serve every epoch: each batch goes through
    ``CapturedStep.step`` -- eager at the first sight of a batch signature, captured at the second, replayed from then on --
    with a ``litepose_amd.optim`` optimizer; the same updates and the same returned values as the eager loop, without a
    host read per step (one per logged line and one at the end).  The teacher stays eager-only (ValueError).  A kept
    ``CapturedStep`` survives what a run does between steps and epochs -- a scheduler, validation in ``eval()`` mode,
    ``zero_grad``, eager epochs on the same optimizer, ``model.load_state_dict``; it captures again by itself after
    ``optimizer.load_state_dict`` / ``add_param_group``; it refuses a changed by-value hyperparameter before it touches
    anything, until ``CapturedStep.invalidate()`` (its docstring lists the events).

    ``random_resolution``: the supernet's random-resolution resize (:49-59).  None: as the reference, on iff
    ``cfg.MODEL.NAME`` is ``pose_supermobilenet`` or ``pose_superresnet``.  Per step the size is drawn from Python's
    ``random`` BEFORE the forward (``random_resolution_size``; a sampling supernet draws its architecture after it, the
    reference's order), then ``nn.functional.train_resize`` resizes images, heatmaps, masks and joints in one library call
    (the batch must be DATASET.INPUT_SIZE wide, the joints int32), then the step as otherwise.  With ``graph`` it raises
    ValueError, and so does a model that samples an architecture per step
    (``pose_supermobilenet.TrainableSuperLitePose``): every step has another signature.

    ``group``: a ``torch.distributed`` process group: data-parallel training, the reference's ``DistributedDataParallel``
    (dist_train.py:271, :283).  ``data_loader`` yields THIS rank's part of every batch (``LabelledSet.batches(shard=(rank,
    world))``), and every rank runs the same number of steps.  Per step ``bucket.zero_grad()`` replaces
    ``optimizer.zero_grad()`` and ``bucket.all_reduce_mean()`` sits between ``loss.backward()`` and ``optimizer.step()``: one
    all-reduce of one flat buffer (``parallel.GradBucket``, built once per (model, group) and kept on the model), after
    which every rank steps with the same gradient -- the mean over the ranks of the rank's own batch-mean loss gradient,
    as DDP.  Start the ranks equal (``parallel.broadcast_state``); for BatchNorm statistics over all ranks' images call
    ``models.pose_mobilenet.convert_sync_batchnorm`` first (``MODEL.SYNC_BN``).  The returned meters are the rank's own,
    as in the reference.  Three combinations raise ValueError before anything runs:
      * ``graph`` with a group: the gloo path goes through the host and cannot be captured, and a capture of an RCCL
        collective has never been run here;
      * a ``teacher`` with a group;
      * a model that samples an architecture per step with a group: every rank would have to draw the same architecture.

    Not here: tensorboard scalars, ``fp16_optimizer``, debug image dumps, batch and data timers."""
    if random_resolution is None:
        random_resolution = getattr(cfg.MODEL, 'NAME', None) in SUPERNET_NAMES
    bucket = None
    if group is not None:
        if graph:
            raise ValueError('do_train: graph=True is not supported with a process group: the collectives of a step '
                             'are not captured')
        if teacher is not None:
            raise ValueError('do_train: a teacher is not supported with a process group')
        if hasattr(model, 'arch_manager'):
            raise ValueError('do_train: a model that samples an architecture per step is not supported with a process '
                             'group: every rank would have to draw the same architecture')
        bucket = _bucket(model, group)
    if graph:
        if teacher is not None:
            raise ValueError('do_train: a teacher is not supported with graph=True')
        if random_resolution or hasattr(model, 'arch_manager'):
            raise ValueError('do_train: graph=True does not go with the random-resolution resize or a model that samples '
                             'an architecture per step: every step has another signature')
        return _do_train_captured(cfg, model, data_loader, loss_factory, optimizer, epoch, logger, graph)
    S = cfg.LOSS.NUM_STAGES
    last = dict(heatmaps=[None] * S, push=[None] * S, pull=[None] * S)
    sums = dict(heatmaps=[0.0] * S, push=[0.0] * S, pull=[0.0] * S)
    count = 0
    freq = getattr(cfg, 'PRINT_FREQ', 1)
    model.train()
    for i, (images, heatmaps, masks, joints) in enumerate(data_loader):
        n = int(images.shape[0])
        if random_resolution:
            size = random_resolution_size(cfg)
            if size % 16:
                raise ValueError('do_train: DATASET.INPUT_SIZE %s gives a training size %d that is not a multiple of 16'
                                 % (cfg.DATASET.INPUT_SIZE, size))
            images, heatmaps, masks, joints = train_resize(images, heatmaps, masks, joints, size, cfg.DATASET.INPUT_SIZE)
        t_heatmaps = None
        if teacher is not None:
            size = int(images.shape[-1]) // 4
            with torch.no_grad():
                t_outputs = teacher(F.interpolate(images, size=(448, 448)))
            t_heatmaps = []
            for idx in range(S):
                t_heatmaps.append(F.interpolate(t_outputs[idx][:, :cfg.DATASET.NUM_JOINTS], size=(size, size)).detach())
                size *= 2
        outputs = model(images)
        terms = loss_factory(outputs, heatmaps, masks, joints)
        t_terms = None if teacher is None else loss_factory(outputs, t_heatmaps, masks, joints)
        loss = 0
        for idx in range(S):
            for key, vals in zip(('heatmaps', 'push', 'pull'), terms):
                if vals[idx] is None:
                    continue
                v = vals[idx].mean(dim=0)
                last[key][idx] = v.item()
                sums[key][idx] += last[key][idx] * n
                loss = loss + v
                if key == 'heatmaps' and t_terms is not None:
                    loss = loss + t_terms[0][idx].mean(dim=0)
        if bucket is None:
            optimizer.zero_grad()
            loss.backward()
        else:
            bucket.zero_grad()
            loss.backward()
            bucket.all_reduce_mean()
        optimizer.step()
        count += n
        if logger is not None and i % freq == 0:
            logger.info('Epoch: [%d][%d]\t%s' % (epoch, i, '\t'.join(
                'Stage%d-%s: %.3e (%.3e)' % (idx, key, last[key][idx], sums[key][idx] / count)
                for key in ('heatmaps', 'push', 'pull') for idx in range(S) if last[key][idx] is not None)))
    if count == 0:
        raise ValueError('do_train: the data loader yielded no batch')
    return {k: [None if v is None else (v, sums[k][idx] / count) for idx, v in enumerate(vals)] for k, vals in last.items()}
