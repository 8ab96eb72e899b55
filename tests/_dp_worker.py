"""One rank of tests/test_gpu_data_parallel.py: a fresh process per rank, all ranks on GPU 0, gloo between them.

    python tests/_dp_worker.py MODE RANK WORLD PORT OUTDIR

MODE ``step_sync`` / ``step_plain``: the case of tests/_train_net_case.py, rank r takes image r and TWICE its slice of the
golden upstream gradients (times two is exact, and the bucket's mean over two ranks halves it again): one forward, one
backward, ``GradBucket.all_reduce_mean``; with / without ``convert_sync_batchnorm``.
MODE ``train``: rank 1 starts from other weights, ``broadcast_state``, then two ``do_train(group=...)`` steps with the
library's SGD on a four-image LabelledSet sharded two and two -- all of it twice, from the same start.
Everything the parent compares is written to OUTDIR/rank<r>.pt as CPU tensors."""
import datetime
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import _train_net_case as TC  # noqa: E402
from litepose_amd import config, optim, parallel  # noqa: E402
from litepose_amd.models import pose_mobilenet as pm  # noqa: E402

LR = 0.25            # a power of two: lr * g is exact, p - lr * g rounds once however the optimizer evaluates it


def _module(case):
    m = pm.get_train_net(config.get_cfg(), TC.ARCH)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case['sd'].items()}, strict=False)
    return m.cuda()


def _cpu(d):
    return {k: v.detach().cpu().clone() for k, v in d.items()}


def step(case, rank, sync):
    m = _module(case)
    if sync:
        pm.convert_sync_batchnorm(m)
    bucket = parallel.GradBucket(m.parameters())
    m.train()
    bucket.zero_grad()
    outs = m(torch.from_numpy(case['x'][rank:rank + 1]).cuda())
    torch.autograd.backward(outs, [torch.from_numpy(2 * case['up%d' % s][rank:rank + 1]).cuda() for s in range(2)])
    own = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
    bucket.all_reduce_mean()
    names = [k for k, _ in m.named_parameters()]
    assert all(p.grad is v for p, v in zip(bucket.params, bucket.views)) and len(names) == len(bucket.params)
    return dict(outs=[o.detach().cpu() for o in outs], own=own, grads=_cpu(dict(zip(names, bucket.views))),
                sd=_cpu(m.state_dict()))


def _labelled_set(cfg):
    from litepose_amd.core import inference
    from litepose_amd.dataset import LabelledSet
    J = cfg.DATASET.NUM_JOINTS
    rng = np.random.RandomState(3)
    sizes = [(40, 56), (33, 47), (64, 64), (48, 36)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    joints = []
    for (h, w), people in zip(sizes, (2, 1, 3, 6)):
        j = np.zeros((people, J, 3))
        j[:, :, 0], j[:, :, 1] = rng.uniform(0, w, (people, J)), rng.uniform(0, h, (people, J))
        j[:, :, 2] = rng.choice([0, 1, 2], (people, J))
        joints.append(j)
    return LabelledSet(images, joints, inference.flip_index_for(cfg)[:J], max_num_people=6, sigma=cfg.DATASET.SIGMA)


def train(case, rank, world):
    from litepose_amd.core.loss import MultiLossFactory
    from litepose_amd.core.trainer import do_train
    cfg = config.get_cfg()
    cfg.DATASET.INPUT_SIZE, cfg.DATASET.OUTPUT_SIZE, cfg.DATASET.MAX_NUM_PEOPLE = 64, [16, 32], 6
    ls = _labelled_set(cfg)
    factory = MultiLossFactory(cfg)
    runs = []
    for _ in range(2):
        m = _module(case)
        if rank == 1:                                       # other weights, other buffers: broadcast_state must undo it
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.5)
                for b in m.buffers():
                    b.add_(1)
        before_broadcast = _cpu(m.state_dict())
        parallel.broadcast_state(m, 0)
        pm.convert_sync_batchnorm(m)
        opt = optim.SGD(m.parameters(), lr=LR)
        rec = dict(before_broadcast=before_broadcast, start=_cpu(m.state_dict()), steps=[], images=[])
        np_rng, py_rng = np.random.RandomState(8 + rank), random.Random(8 + rank)
        for epoch in range(2):
            p_before = _cpu(dict(m.named_parameters()))
            seen = []

            def loader():
                for batch in ls.batches(64, [16, 32], 4, np_rng, py_rng, shard=(rank, world)):
                    seen.append(int(batch[0].shape[0]))
                    yield batch

            meters = do_train(cfg, m, loader(), factory, opt, epoch=epoch, group=dist.group.WORLD)
            bucket = m._grad_bucket[1]
            assert all(p.grad is v for p, v in zip(bucket.params, bucket.views))
            rec['steps'].append(dict(p_before=p_before, grad=_cpu({k: p.grad for k, p in m.named_parameters()}),
                                     p_after=_cpu(dict(m.named_parameters())), sd=_cpu(m.state_dict()),
                                     heat=meters['heatmaps'][0][0]))
            rec['images'].append(seen)
        rec['bucket_id'] = id(m._grad_bucket[1])
        runs.append(rec)
    return dict(runs=runs)


def main():
    mode, rank, world, port, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    try:
        case = TC.load()
        if mode in ('step_sync', 'step_plain'):
            res = step(case, rank, mode == 'step_sync')
        elif mode == 'train':
            res = train(case, rank, world)
        else:
            raise SystemExit('unknown mode %r' % mode)
        torch.cuda.synchronize()
        torch.save(res, os.path.join(out, 'rank%d.pt' % rank))
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
