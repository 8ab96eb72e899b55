#!/usr/bin/env python
"""Device time of lp_pose_loss_grad (GPU box) beside lp_pose_loss on the same tensors in the same run: the measurement of
DESIGN.md 4e.  Batch 64, J = 14 joints, C = 28 channels (heatmaps, then tag maps from channel 14), M = 30 with 1-8 persons
per image, all-ones masks, R = 128 and R = 64.  HIP events, 10 warm-up calls and REPS repeats, medians.  Each call is timed
twice: through the Python wrapper (one event pair per call: the launch overheads of an idle stream are inside), and as a
captured graph of 20 calls (one event pair per replay, divided by 20).  The bytes are those every call must move:
2 N J R^2 floats in for the heatmap term (the mask's N R^2 on top comes out of cache for J - 1 of its J readers), and for
the gradient N C R^2 floats out.  The repeats re-read the same tensors, which fit the Infinity Cache: not an HBM figure.

    python tools/time_loss_grad.py [REPS]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from litepose_amd.core.loss import loss_buffers, pose_loss, pose_loss_grad

N, J, C, M, CHAIN = 64, 14, 28, 30, 20


def timed(fn, reps, per=1):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) / per


def chain(fn):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(CHAIN):
            fn()
    return g


def main(reps):
    print('lp_pose_loss_grad beside lp_pose_loss: batch %d, J = %d, C = %d, M = %d, 1-8 persons per image' % (N, J, C, M))
    print('command: python tools/time_loss_grad.py %d   (HIP events, 10 warm-ups, medians; graph = %d calls per replay)'
          % (reps, CHAIN), flush=True)
    rng = np.random.RandomState(1)
    for R in (128, 64):
        out = torch.from_numpy(rng.standard_normal((N, C, R, R)).astype(np.float32)).cuda()
        heat = torch.from_numpy(rng.uniform(0, 1, (N, J, R, R)).astype(np.float32)).cuda()
        mask = torch.ones(N, R, R, device='cuda')
        jt = np.zeros((N, M, J, 2), np.int32)
        for n in range(N):
            p = rng.randint(1, 9)
            jt[n, :p, :, 0] = np.arange(J)[None] * R * R + rng.randint(0, R * R, (p, J))
            jt[n, :p, :, 1] = 1
        jt = torch.from_numpy(jt).cuda()
        up = [torch.full((N,), 1.0 / N, device='cuda') for _ in range(3)]
        grad = torch.empty_like(out)
        buf = loss_buffers(N, J, R, out.device)
        read, write = 2 * N * J * R * R * 4, N * C * R * R * 4
        calls = [
            ('lp_pose_loss_grad heat + tags', read + write,
             lambda: pose_loss_grad(out, J, J, heat, mask, jt, 'exp', 1.0, 0.001, 0.001, up[0], up[1], up[2], grad_out=grad)),
            ('lp_pose_loss_grad heat only', read + write,
             lambda: pose_loss_grad(out, J, -1, heat, mask, None, 'exp', 1.0, 0.001, 0.001, up[0], grad_out=grad)),
            ('lp_pose_loss_grad heat only, fresh grad_out', read + write,
             lambda: pose_loss_grad(out, J, -1, heat, mask, None, 'exp', 1.0, 0.001, 0.001, up[0])),
            ('lp_pose_loss heat only', read,
             lambda: pose_loss(out, J, -1, heat, mask, buffers=buf)),
            ('lp_pose_loss heat + tags', read,
             lambda: pose_loss(out, J, J, heat, mask, jt, 'exp', 1.0, 0.001, 0.001, buffers=buf)),
        ]
        for name, nbytes, fn in calls:
            wrapper = timed(fn, reps)
            line = 'R=%-3d %-46s wrapper %7.4f ms (%5.2f TB/s)' % (R, name, wrapper, nbytes / wrapper / 1e9)
            if 'fresh' not in name:                          # an allocation cannot be captured
                g = chain(fn)
                graph = timed(g.replay, reps, CHAIN)
                line += '   in a graph of %d %7.4f ms per call (%5.2f TB/s)' % (CHAIN, graph, nbytes / graph / 1e9)
            print(line + '   %.1f MB' % (nbytes / 1e6), flush=True)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50)
