#!/usr/bin/env python
"""Wall time of one whole native training step (GPU box): the measurement of DESIGN.md 4f, "the captured step".

    python tools/time_train_step.py [REPS] [ARCH] [BATCHES...] [--optimizer-only] [--sync-bn]

For ARCH (default search-XS at its own resolution) and every batch size (default 16 64), medians of REPS whole steps after
10 warm-ups, each step timed on the host from its first call to a device synchronisation behind it:

    eager, torch.optim.Adam          do_train on one batch, the loop every commit has
    eager, litepose_amd.optim.Adam   the same loop on the library's optimizer
    captured                         CapturedStep.step: copy the batch in, replay the graph

and the optimizer call alone on the module's parameter list with gradients in place (HIP events): torch's Adam / SGD against
the library's, the library's launch count, and the bytes a step must move (4 streams of the parameter set read and 3
written for Adam, 3 and 2 for SGD with momentum) over the time -- the parameter set of search-XS fits the Infinity Cache,
so that figure is not an HBM rate.  Rows the tree cannot run (a commit without litepose_amd.optim) are reported as such,
so the same file runs on an older tree.

--sync-bn (the measurement of DESIGN.md 4h) replaces the step rows by two alternating pairs of the eager loop on the
library's Adam: the plain step, and the data-parallel step forced through a process group of ONE rank (gloo) -- the
synchronised BatchNorm calls and the gradient bucket without any collective: what the extra launches of every BatchNorm
cost, not what a collective costs.

ARCH = pose_resnet (the measurement of DESIGN.md 4f, "pose_resnet"): the network of resnet.yaml at 256 (deconv kernels 3,
filters 16 / 24 / 24), one whole eager step on the library's Adam for ``backend='native'`` against ``backend='torch'``
(torch's convolutions: MIOpen) in the same process, the two rows alternating after warm-up; then ``dense_conv`` forward /
dX / dW alone (HIP events) against ``torch.nn.functional.conv2d`` plus autograd at the layer shapes of that step."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from litepose_amd import _native as nv, arch_zoo, config
from litepose_amd.core import trainer
from litepose_amd.core.loss import MultiLossFactory
from litepose_amd.models import pose_mobilenet as pm

try:
    from litepose_amd import optim as lp_optim
except ImportError:
    lp_optim = None
WARMUP = 10


def batch_of(cfg, res, N):
    J, M = cfg.MODEL.NUM_JOINTS, 30
    rng = np.random.RandomState(1)
    sizes = [res // 4, res // 2]
    heat = [torch.rand(N, J, R, R, device='cuda') for R in sizes]
    mask = [torch.ones(N, R, R, device='cuda') for R in sizes]
    jts = []
    for R in sizes:
        jt = np.zeros((N, M, J, 2), np.int32)
        for n in range(N):
            p = rng.randint(1, 9)
            jt[n, :p, :, 0] = np.arange(J)[None] * R * R + rng.randint(0, R * R, (p, J))
            jt[n, :p, :, 1] = 1
        jts.append(torch.from_numpy(jt).cuda())
    cfg.DATASET.OUTPUT_SIZE = sizes
    return torch.randn(N, 3, res, res, device='cuda'), heat, mask, jts


def wall(fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def events(fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def module(cfg, arch):
    torch.manual_seed(0)
    return pm.get_train_net(cfg, arch, backend='native').cuda().train()


def step_rows(cfg, arch, res, N, reps):
    batch = batch_of(cfg, res, N)
    fac = MultiLossFactory(cfg)
    rows = [('eager, torch.optim.Adam', lambda m: torch.optim.Adam(m.parameters(), lr=1e-4), False)]
    if lp_optim is not None:
        rows += [('eager, litepose_amd.optim.Adam', lambda m: lp_optim.Adam(m.parameters(), lr=1e-4), False),
                 ('captured, litepose_amd.optim.Adam', lambda m: lp_optim.Adam(m.parameters(), lr=1e-4), True)]
    for label, make, captured in rows:
        try:
            m = module(cfg, arch)
            opt = make(m)
            if captured:
                stepper = trainer.CapturedStep(cfg, m, fac, opt)
                med, lo, hi = wall(lambda: stepper.step(*batch), reps)
                assert stepper.captures == 1 and stepper.replays == WARMUP + reps - 1, (stepper.captures, stepper.replays)
            else:
                med, lo, hi = wall(lambda: trainer.do_train(cfg, m, [batch], fac, opt), reps)
            print('batch %3d  %-34s %8.2f ms  (min %.2f, max %.2f)' % (N, label, med, lo, hi), flush=True)
            del m, opt
        except Exception as e:                               # a number that could not be taken is reported as such
            print('batch %3d  %-34s not taken: %s' % (N, label, str(e).splitlines()[0][:160]), flush=True)
    if lp_optim is None:
        print('batch %3d  the library rows: this tree has no litepose_amd.optim' % N, flush=True)


def sync_rows(cfg, arch, res, N, reps):
    import tempfile
    import torch.distributed as dist
    from litepose_amd.nn import functional as F_
    if lp_optim is None or not hasattr(pm, 'convert_sync_batchnorm'):
        print('batch %3d  the synchronised rows: this tree has no data-parallel training' % N, flush=True)
        return
    if not dist.is_initialized():
        rendezvous = tempfile.NamedTemporaryFile(delete=False)
        rendezvous.close()
        dist.init_process_group('gloo', init_method='file://' + rendezvous.name, rank=0, world_size=1)
    batch = batch_of(cfg, res, N)
    fac = MultiLossFactory(cfg)
    for _ in range(2):
        for label, sync in (('eager, plain BatchNorm', False), ('eager, sync path, group of one', True)):
            m = module(cfg, arch)
            opt = lp_optim.Adam(m.parameters(), lr=1e-4)
            F_._force_sync = sync
            try:
                if sync:
                    pm.convert_sync_batchnorm(m)
                    med, lo, hi = wall(lambda: trainer.do_train(cfg, m, [batch], fac, opt, group=dist.group.WORLD), reps)
                else:
                    med, lo, hi = wall(lambda: trainer.do_train(cfg, m, [batch], fac, opt), reps)
            finally:
                F_._force_sync = False
            bns = sum(isinstance(x, torch.nn.BatchNorm2d) for x in m.modules())
            print('batch %3d  %-34s %8.2f ms  (min %.2f, max %.2f)  %d BatchNorms' % (N, label, med, lo, hi, bns), flush=True)
            del m, opt


def optimizer_rows(cfg, arch, reps):
    m = module(cfg, arch)
    params = list(m.parameters())
    g = torch.Generator(device='cuda').manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 1e-3
    numel = [p.numel() for p in params]
    total = sum(numel)
    print('optimizer call alone: %d tensors, %d elements (%.2f MB per stream)' % (len(params), total, total * 4 / 1e6))
    rows = [('torch.optim.Adam', lambda: torch.optim.Adam(params, lr=1e-4), 7, None),
            ('torch.optim.Adam(fused=True)', lambda: torch.optim.Adam(params, lr=1e-4, fused=True), 7, None),
            ('torch.optim.SGD(momentum=0.9)', lambda: torch.optim.SGD(params, lr=1e-4, momentum=0.9), 5, None)]
    if lp_optim is not None:
        import ctypes as C
        n = int(nv.lib().lp_optim_launches(len(numel), (C.c_int64 * len(numel))(*numel)))
        rows += [('litepose_amd.optim.Adam', lambda: lp_optim.Adam(params, lr=1e-4), 7, n + 1),
                 ('litepose_amd.optim.SGD(momentum=0.9)', lambda: lp_optim.SGD(params, lr=1e-4, momentum=0.9), 5, n)]
    for label, make, streams, launches in rows:
        try:
            opt = make()
            ms = events(opt.step, reps)
            note = '%d launches' % launches if launches is not None else 'launches: see a kernel trace'
            print('  %-38s %7.3f ms  %6.2f TB/s over %d streams  %s' % (label, ms, streams * total * 4 / ms / 1e9, streams,
                                                                      note), flush=True)
            if launches is not None:                         # the same call replayed from a graph: its device time alone
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()
                ms = events(graph.replay, reps)
                print('  %-38s %7.3f ms  %6.2f TB/s' % (label + ', replayed', ms, streams * total * 4 / ms / 1e9), flush=True)
        except Exception as e:
            print('  %-38s not taken: %s' % (label, str(e).splitlines()[0][:160]), flush=True)


def resnet_cfg(res=256):
    cfg = config.get_cfg()
    cfg.MODEL.NAME = 'pose_resnet'
    cfg.DATASET.INPUT_SIZE, cfg.DATASET.OUTPUT_SIZE = res, [res // 4, res // 2]
    cfg.MODEL.EXTRA.NUM_DECONV_KERNELS, cfg.MODEL.EXTRA.NUM_DECONV_FILTERS = [3, 3, 3], [16, 24, 24]
    return cfg


# name, Ca, Cb, Cout, plane of the source, K, S, upsample: the layer shapes of a step at 256
RESNET_LAYERS = [('stage entry k7 s2 16->64', 16, 0, 64, 128, 7, 2, False), ('k7 s1 32->128', 32, 0, 128, 32, 7, 1, False),
                 ('k5 48->192', 48, 0, 192, 16, 5, 1, False), ('k3 80->320', 80, 0, 320, 16, 3, 1, False),
                 ('UpConv pair 80+48->16', 80, 48, 16, 16, 3, 1, True), ('head pair 24+32->28', 24, 32, 28, 64, 3, 1, False)]


def resnet_step_rows(cfg, N, reps):
    from litepose_amd.models import pose_resnet as pr
    batch = batch_of(cfg, int(cfg.DATASET.INPUT_SIZE), N)
    fac = MultiLossFactory(cfg)
    runs = {}
    for backend in ('native', 'torch'):
        torch.manual_seed(0)
        m = pr.get_train_net(cfg, backend=backend).cuda().train()
        opt = lp_optim.Adam(m.parameters(), lr=1e-4)
        runs[backend] = (m, opt, [])
        for _ in range(WARMUP):
            trainer.do_train(cfg, m, [batch], fac, opt)
    torch.cuda.synchronize()
    for _ in range(reps):                                    # the two rows alternate: both see the same machine
        for backend in ('native', 'torch'):
            m, opt, t = runs[backend]
            t0 = time.perf_counter()
            trainer.do_train(cfg, m, [batch], fac, opt)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    for backend in ('native', 'torch'):
        t = runs[backend][2]
        print('batch %3d  eager step, backend=%-7s %8.2f ms  (min %.2f, max %.2f)' % (N, backend, np.median(t), min(t), max(t)),
              flush=True)


def resnet_layer_rows(N, reps):
    from litepose_amd.nn import functional as F_
    tf = torch.nn.functional
    g = torch.Generator(device='cuda').manual_seed(5)
    rnd = lambda *shape: torch.randn(shape, device='cuda', generator=g)  # noqa: E731
    print('dense_conv alone at N = %d (HIP events, medians of %d, the two sides alternating): library / torch, ms' % (N, reps))
    for name, ca, cb, cout, hw, k, s, ups in RESNET_LAYERS:
        xa, wa = rnd(N, ca, hw, hw), rnd(cout, ca, k, k) * 0.1
        xb, wb = (rnd(N, cb, hw, hw), rnd(cout, cb, k, k) * 0.1) if cb else (None, None)
        up = (lambda t: tf.interpolate(t, scale_factor=2)) if ups else (lambda t: t)

        def torch_fwd(xa=xa, wa=wa, xb=xb, wb=wb):
            y = tf.conv2d(up(xa), wa, None, s, k // 2)
            return y if xb is None else y + tf.conv2d(up(xb), wb, None, s, k // 2)

        dy = torch.randn_like(torch_fwd())

        def torch_grad(data):
            """autograd's backward alone, towards the sources (data) or towards the weights, through a graph built once"""
            ins = [None if t is None else t.clone().requires_grad_(data == (i % 2 == 0)) for i, t in enumerate((xa, wa, xb, wb))]
            y = torch_fwd(*ins)
            wrt = [t for t in ins if t is not None and t.requires_grad]
            return lambda: torch.autograd.grad(y, wrt, dy, retain_graph=True)

        need_x = (True, False, cb > 0, False, False)
        need_w = (False, True, False, cb > 0, False)
        sides = [('forward', lambda: F_.conv_forward(xa, wa, xb, wb, None, s, ups), lambda: torch_fwd()),
                 ('dX', lambda: F_.conv_backward(dy, xa, wa, xb, wb, s, ups, need_x), torch_grad(True)),
                 ('dW', lambda: F_.conv_backward(dy, xa, wa, xb, wb, s, ups, need_w), torch_grad(False))]
        cells = []
        for what, mine, theirs in sides:
            with torch.no_grad() if what == 'forward' else torch.enable_grad():
                for _ in range(WARMUP):
                    mine(), theirs()
                torch.cuda.synchronize()
                tm, tt = [], []
                for _ in range(reps):
                    for fn, acc in ((mine, tm), (theirs, tt)):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn()
                        b.record()
                        acc.append((a, b))
                torch.cuda.synchronize()
            cells.append('%s %7.3f / %7.3f' % (what, np.median([a.elapsed_time(b) for a, b in tm]),
                                             np.median([a.elapsed_time(b) for a, b in tt])))
        print('  %-26s %s' % (name, '   '.join(cells)), flush=True)


def main(reps, name, batches, optimizer_only, sync_bn=False):
    if name == 'pose_resnet':
        cfg = resnet_cfg()
        print('whole training steps of pose_resnet at %d' % cfg.DATASET.INPUT_SIZE)
        print('command: python tools/time_train_step.py %d pose_resnet %s   (%d warm-ups, medians of %d steps, host clock '
              'with a synchronisation behind every step)' % (reps, ' '.join(str(b) for b in batches), WARMUP, reps), flush=True)
        for N in batches:
            resnet_step_rows(cfg, N, reps)
        resnet_layer_rows(batches[0], reps)
        return
    cfg, arch = config.get_cfg(), arch_zoo.load_arch(name)
    res = int(arch['img_size'])
    print('whole training steps of %s at %d' % (name, res))
    print('command: python tools/time_train_step.py %d %s %s   (%d warm-ups, medians of %d steps, host clock with a '
          'synchronisation behind every step)' % (reps, name, ' '.join(str(b) for b in batches), WARMUP, reps), flush=True)
    if sync_bn:
        for N in batches:
            sync_rows(cfg, arch, res, N, reps)
        return
    if not optimizer_only:
        for N in batches:
            step_rows(cfg, arch, res, N, reps)
    optimizer_rows(cfg, arch, reps)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    main(int(args[0]) if args else 30, args[1] if len(args) > 1 else 'search-XS',
         [int(a) for a in args[2:]] or ([16] if len(args) > 1 and args[1] == 'pose_resnet' else [16, 64]), '--optimizer-only' in sys.argv, '--sync-bn' in sys.argv)
