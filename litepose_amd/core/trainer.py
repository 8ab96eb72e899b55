"""The forward half of lib/core/trainer.py:do_train on the device: the losses of a model over a labelled set."""
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
