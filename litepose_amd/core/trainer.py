"""lib/core/trainer.py:do_train with the losses and their gradient on the device: ``loss_epoch``, the losses of a model over a
labelled set, and ``do_train``, one epoch of loss, backward and optimizer step for a torch model."""
import torch
import torch.nn.functional as F

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


def do_train(cfg, model, data_loader, loss_factory, optimizer, epoch=0, teacher=None, logger=None):
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

    Not here: tensorboard scalars, ``fp16_optimizer``, the supernet's random-resolution resize (:49-59), debug image dumps,
    batch and data timers."""
    S = cfg.LOSS.NUM_STAGES
    last = dict(heatmaps=[None] * S, push=[None] * S, pull=[None] * S)
    sums = dict(heatmaps=[0.0] * S, push=[0.0] * S, pull=[0.0] * S)
    count = 0
    freq = getattr(cfg, 'PRINT_FREQ', 1)
    model.train()
    for i, (images, heatmaps, masks, joints) in enumerate(data_loader):
        n = int(images.shape[0])
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
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        count += n
        if logger is not None and i % freq == 0:
            logger.info('Epoch: [%d][%d]\t%s' % (epoch, i, '\t'.join(
                'Stage%d-%s: %.3e (%.3e)' % (idx, key, last[key][idx], sums[key][idx] / count)
                for key in ('heatmaps', 'push', 'pull') for idx in range(S) if last[key][idx] is not None)))
    if count == 0:
        raise ValueError('do_train: the data loader yielded no batch')
    return {k: [None if v is None else (v, sums[k][idx] / count) for idx, v in enumerate(vals)] for k, vals in last.items()}
