#!/usr/bin/env python
"""Latency of lp_draw_poses (GPU box) beside the cost of touching every pixel of the same images once.

Two shapes: 64 images of 480x640 with 4 persons each (a batch of validation images with their records), and one image of
448x448 with 2 persons (the demo's frame).  Persons are COCO figures (17 joints, 19 links) of about a third of the image's
height at random places.  Beside each, in the same run, a device copy of the same image buffer (copy_ of a uint8
tensor): the copy reads and writes every pixel once, the drawing only culls primitives per tile and writes the covered
pixels.  Each call is captured into a hipGraph once and replayed, the two alternating, one HIP event pair per replay;
prints the median and the minimum.  Drawing again over drawn images paints the same pixels, so replays do not restore.
Beside the second shape the 2-people N = 1 lp_fast_parse figure of profiles/fast_parse_latency.txt is quoted: the stage
of the demo that runs just before.  profiles/annotate_latency.txt is this program's output.

    python tools/time_annotate.py [REPS] > profiles/annotate_latency.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from litepose_amd.utils import vis

# (x, y) of 17 COCO joints of a standing figure in a 20 x 36 box
FIGURE = np.array([[10, 3], [12, 2], [8, 2], [14, 3], [6, 3], [15, 9], [5, 9], [18, 15], [2, 15], [19, 21], [1, 21],
                   [13, 20], [7, 20], [14, 28], [6, 28], [15, 35], [5, 35]], np.float32)


def captured(fn):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    return g


def records(rng, N, P, H, W):
    k = np.zeros((N, P, 17, 3), np.float32)
    s = H / 3.0 / 36.0
    for n in range(N):
        for p in range(P):
            k[n, p, :, :2] = FIGURE * s + [rng.uniform(0, W - 20 * s), rng.uniform(0, H - 36 * s)]
            k[n, p, :, 2] = 1.0
    return torch.from_numpy(k).cuda(), torch.full((N,), P, dtype=torch.int32, device='cuda')


def fast_parse_line():
    try:
        with open(os.path.join(ROOT, 'profiles', 'fast_parse_latency.txt')) as f:
            for line in f:
                if line.startswith('2 people/image N=1 ') and 'lp_fast_parse' in line:
                    return ' '.join(line.split())
    except OSError:
        pass
    return 'not found'


def main(reps):
    print('lp_draw_poses against a device copy of the same image buffer (COCO figures a third of the image high)')
    print('command: python tools/time_annotate.py %d   (hipGraph replays, one HIP event pair each, the two alternating)'
          % reps, flush=True)
    rng = np.random.default_rng(3)
    for N, H, W, P in ((64, 480, 640, 4), (1, 448, 448, 2)):
        images = torch.from_numpy(rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)).cuda()
        other = images.clone()
        kpts, count = records(rng, N, P, H, W)
        calls = {'lp_draw_poses': lambda: vis.annotate_batch(images, kpts, count, dataset='COCO'),
                 'device copy': lambda: other.copy_(images)}
        graphs = {}
        for k in ('lp_draw_poses', 'device copy'):                   # the drawing first: `other` is compared before the copy
            graphs[k] = captured(calls[k])
            if k == 'lp_draw_poses':
                covered = int((images != other).any(dim=3).sum())
        for g in graphs.values():
            for _ in range(10):
                g.replay()
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
              for k in graphs}
        for r in range(reps):
            for k, g in graphs.items():
                a, b = ev[k][r]
                a.record()
                g.replay()
                b.record()
        torch.cuda.synchronize()
        for k in graphs:
            us = np.array([a.elapsed_time(b) for a, b in ev[k]]) * 1e3
            print('N=%-3d %dx%d %d persons/image  %-14s median %8.1f us  min %8.1f us  (%d replays, %.1f MB of pixels, %d covered)'
                  % (N, H, W, P, k, np.median(us), us.min(), reps, images.numel() / 1e6, covered), flush=True)
    print('for scale, the stage before it in the demo (profiles/fast_parse_latency.txt): ' + fast_parse_line())


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
