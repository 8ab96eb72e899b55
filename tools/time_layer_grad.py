#!/usr/bin/env python
"""Device time of the training-mode layers (GPU box): the measurement of DESIGN.md 4f.  Every distinct layer shape of an
architecture (default LitePose-XS at 256) at batch 64 -- 1x1, depthwise, BatchNorm, the stem convolution (forward and
weight gradient: it has no data gradient) and the transposed-convolution pairs: the library's forward and each backward
kernel group (data gradient, weight gradient), and beside them torch's own forward and backward of the same op on the same
tensors (aten's convolution_backward with one output asked for at a time; BatchNorm + activation through autograd).  HIP
events, 10 warm-up calls and REPS repeats, medians, every row from one run.  The bytes are those a call must move
(activations in and out once per pass over them: BatchNorm reads its input twice, its backward reads input and upstream
twice), the FLOPs those of the weight-gradient GEMM (for the transposed-convolution pair, whose three passes are GEMMs of
one size, of each pass).  The repeats re-read the same tensors: where they fit the Infinity Cache this is not an HBM figure.
Last: one full do_train step (loss, backward, SGD) of the native module and of the backend='torch' module.

    python tools/time_layer_grad.py [REPS] [ARCH] [BATCH]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as TF

from litepose_amd import arch_zoo, config
from litepose_amd.models import pose_mobilenet as pm
from litepose_amd.nn import functional as F


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def layer_shapes(cfg, arch, res):
    """One forward of the torch-backend module at batch 1 on the CPU with its layer methods recording: the distinct
    (kind, ...) shapes in network order with how often each occurs."""
    m = pm.get_train_net(cfg, arch, backend='torch').eval()
    seen, conv0, bn0, up0 = {}, m._conv, m._bn, m._up_pair

    def note(key):
        seen[key] = seen.get(key, 0) + 1

    def conv(x, c):
        k, g = c.kernel_size[0], c.groups
        if k == 1 and g == 1:
            note(('pw', c.in_channels, c.out_channels, x.shape[2], x.shape[3]))
        elif g == c.in_channels and g > 1:
            note(('dw', c.in_channels, k, c.stride[0], x.shape[2], x.shape[3]))
        else:
            note(('stem', x.shape[2], x.shape[3]))
        return conv0(x, c)

    def up_pair(refined, w_refined, raw, w_raw):
        note(('deconv', refined.shape[1], raw.shape[1], w_refined.shape[1], refined.shape[2], refined.shape[3]))
        return up0(refined, w_refined, raw, w_raw)

    def bn(x, b, act=None, residual=None):
        note(('bn', x.shape[1], x.shape[2], x.shape[3], act, residual is not None))
        return bn0(x, b, act, residual)

    m._conv, m._bn, m._up_pair = conv, bn, up_pair
    with torch.no_grad():
        m(torch.zeros(1, 3, res, res))
    return list(seen.items())


def rows(shape, N, reps):
    kind = shape[0]
    r = lambda *s: torch.randn(*s, device='cuda')      # noqa: E731
    if kind == 'pw':
        _, ci, co, h, w = shape
        x, wt, dy = r(N, ci, h, w), r(co, ci, 1, 1) * 0.1, r(N, co, h, w)
        nb = (ci + co) * N * h * w * 4
        back = lambda mask: torch.ops.aten.convolution_backward(dy, x, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, mask)  # noqa: E731
        return 'pw %4d -> %4d  %3dx%-3d' % (ci, co, h, w), [
            ('fwd', nb, 0, lambda: F.pw_forward(x, wt), lambda: TF.conv2d(x, wt)),
            ('dX', nb, 0, lambda: F.pw_backward(dy, x, wt, True, False), lambda: back([True, False, False])),
            ('dW', nb, 2 * ci * co * N * h * w, lambda: F.pw_backward(dy, x, wt, False, True), lambda: back([False, True, False]))]
    if kind == 'dw':
        _, c, k, s, h, w = shape
        x, wt = r(N, c, h, w), r(c, 1, k, k) * 0.1
        dy = r(N, c, (h - 1) // s + 1, (w - 1) // s + 1)
        nb = (x.numel() + dy.numel()) * 4
        back = lambda mask: torch.ops.aten.convolution_backward(dy, x, wt, None, [s, s], [k // 2, k // 2], [1, 1], False, [0, 0], c, mask)  # noqa: E731
        return 'dw %4d k%d s%d    %3dx%-3d' % (c, k, s, h, w), [
            ('fwd', nb, 0, lambda: F.dw_forward(x, wt, s), lambda: TF.conv2d(x, wt, None, s, k // 2, 1, c)),
            ('dX', nb, 0, lambda: F.dw_backward(dy, x, wt, s, True, False), lambda: back([True, False, False])),
            ('dW', nb, 2 * k * k * dy.numel(), lambda: F.dw_backward(dy, x, wt, s, False, True), lambda: back([False, True, False]))]
    if kind == 'stem':
        _, h, w = shape
        x, wt, dy = r(N, 3, h, w), r(32, 3, 3, 3) * 0.1, r(N, 32, h // 2, w // 2)
        nb = (x.numel() + dy.numel()) * 4
        back = lambda: torch.ops.aten.convolution_backward(dy, x, wt, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])  # noqa: E731
        return 'stem   3 ->   32  %3dx%-3d' % (h, w), [
            ('fwd', nb, 0, lambda: F.stem_forward(x, wt), lambda: TF.conv2d(x, wt, None, 2, 1)),
            ('dW', nb, 2 * 27 * dy.numel(), lambda: F.stem_backward(dy, x), back)]
    if kind == 'deconv':
        _, ca, cb, co, h, w = shape
        xa, xb, wa, wb, dy = r(N, ca, h, w), r(N, cb, h, w), r(ca, co, 4, 4) * 0.1, r(cb, co, 4, 4) * 0.1, r(N, co, 2 * h, 2 * w)
        nb = (xa.numel() + xb.numel() + dy.numel()) * 4
        fl = 2 * 16 * (ca + cb) * co * N * h * w
        back = lambda x, wt, mask: torch.ops.aten.convolution_backward(dy, x, wt, None, [2, 2], [1, 1], [1, 1], True, [0, 0], 1, mask)  # noqa: E731
        both = lambda mask: (back(xa, wa, mask), back(xb, wb, mask))  # noqa: E731
        return 'dc %3d+%-3d-> %3d  %3dx%-3d' % (ca, cb, co, h, w), [
            ('fwd', nb, fl, lambda: F.deconv_forward(xa, wa, xb, wb),
             lambda: TF.conv_transpose2d(xa, wa, None, 2, 1) + TF.conv_transpose2d(xb, wb, None, 2, 1)),
            ('dX', nb, fl, lambda: F.deconv_backward(dy, xa, wa, xb, wb, True, False), lambda: both([True, False, False])),
            ('dW', nb, fl, lambda: F.deconv_backward(dy, xa, wa, xb, wb, False, True), lambda: both([False, True, False]))]
    _, c, h, w, act, has_res = shape
    x, dy, res = r(N, c, h, w), r(N, c, h, w), r(N, c, h, w) if has_res else None
    ga, be, run = torch.rand(c, device='cuda') + 0.5, r(c), torch.stack([r(c) * 0.1, torch.rand(c, device='cuda') + 0.5])
    _, stat = F.bn_forward(x, ga, be, run, act, res)
    xt, gt, bt = x.clone().requires_grad_(), ga.clone().requires_grad_(), be.clone().requires_grad_()
    tact = {None: lambda z: z, 'relu': torch.relu, 'relu6': TF.relu6}[act]

    def tfwd():
        y = tact(TF.batch_norm(xt, run[0].clone(), run[1].clone(), gt, bt, True, 0.1, 1e-5))
        return y if res is None else y + res
    yt = tfwd()
    size = x.numel() * 4
    return 'bn %4d %-5s%s %3dx%-3d' % (c, act or 'none', '+res' if has_res else '    ', h, w), [
        ('fwd', size * (4 if has_res else 3), 0, lambda: F.bn_forward(x, ga, be, run, act, res), lambda: tfwd()),
        ('bwd', size * 5, 0, lambda: F.bn_backward(dy, x, ga, be, stat, act),
         lambda: torch.autograd.grad(yt, (xt, gt, bt), dy, retain_graph=True))]


def train_step(cfg, arch, res, N, backend, reps):
    from litepose_amd.core.loss import MultiLossFactory
    from litepose_amd.core.trainer import do_train
    torch.manual_seed(0)
    m = pm.get_train_net(cfg, arch, backend=backend).cuda()
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
    batch = (torch.randn(N, 3, res, res, device='cuda'), heat, mask, jts)
    cfg.DATASET.OUTPUT_SIZE = sizes
    fac, opt = MultiLossFactory(cfg), torch.optim.SGD(m.parameters(), lr=1e-4)
    return timed(lambda: do_train(cfg, m, [batch], fac, opt), max(5, reps // 5))


def main(reps, name, N):
    cfg, arch = config.get_cfg(), arch_zoo.load_arch(name)
    res = int(arch['img_size'])
    print('training-mode layers of %s at %d, batch %d' % (name, res, N))
    print('command: python tools/time_layer_grad.py %d %s %d   (HIP events, 10 warm-ups, medians; ms: library | torch)'
          % (reps, name, N), flush=True)
    total = {}
    for shape, count in layer_shapes(cfg, arch, res):
        label, calls = rows(shape, N, reps)
        line = '%s x%-2d' % (label, count)
        for what, nbytes, flops, ours, theirs in calls:
            a, b = timed(ours, reps), timed(theirs, reps)
            total[shape[0], what] = total.get((shape[0], what), 0.0) + a * count
            total['torch ' + shape[0], what] = total.get(('torch ' + shape[0], what), 0.0) + b * count
            line += '  %s %7.3f | %7.3f (%5.2f TB/s%s)' % (what, a, b, nbytes / a / 1e9,
                                                           ', %5.1f TF' % (flops / a / 1e9) if flops else '')
        print(line, flush=True)
    print('sums over the network (ms, every occurrence):')
    for (kind, what), v in sorted(total.items()):
        print('  %-9s %-4s %8.3f' % (kind, what, v))
    for backend in ('native', 'torch'):
        try:
            print('one do_train step, backend=%-6s  %8.2f ms' % (backend, train_step(cfg, arch, res, N, backend, reps)), flush=True)
        except Exception as e:                               # a number that could not be taken is reported as such
            print('one do_train step, backend=%-6s  not taken: %s' % (backend, str(e).splitlines()[0][:160]), flush=True)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50, sys.argv[2] if len(sys.argv) > 2 else 'search-XS',
         int(sys.argv[3]) if len(sys.argv) > 3 else 64)
