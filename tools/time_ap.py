#!/usr/bin/env python
"""What COCO keypoint AP costs after the records exist (GPU box): the lp_kpt_eval launch (OKS + matching at 10 thresholds x
3 area ranges), the one D2H of its compact outputs, and the host accumulate + summarize of litepose_amd.coco_eval --
against the plain-loop restatement of the same protocol in tests/_cocoeval_ref.py on the CPU (per-image evaluation, then
accumulate), which is the shape of the loops pycocotools runs in Python per image x area range x threshold.  pycocotools
itself is not timed: it is not available here, and agreement with it is not measured either (litepose_amd/coco_eval.py).

A synthetic set of 500 images with 8 detections and 4 annotations each (17 joints, record capacity 30, T = 2), jittered
copies of the annotations plus random detections.  The launch is captured into a hipGraph once and replayed, one HIP event
pair per replay; median and minimum.  The host parts are wall-clock medians of 5 runs.  No ratio is fixed in advance:
profiles/ap_eval_latency.txt is this program's output.

    python tools/time_ap.py [REPS] > profiles/ap_eval_latency.txt
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import _cocoeval_ref as R
from litepose_amd import coco_eval as ce

IMAGES, DETS, ANNS, PCAP, J, T = 500, 8, 4, 30, 17, 2


def make_set(seed=3):
    rng = np.random.RandomState(seed)
    kpts = np.zeros((IMAGES, PCAP, J, 3 + T), np.float32)
    scores = np.zeros((IMAGES, PCAP), np.float32)
    count = np.full(IMAGES, DETS, np.int32)
    gts, dets = {}, {}
    for n in range(IMAGES):
        gl = [R.person(rng, [900.0, 4000.0, 20000.0][rng.randint(3)], J, rng.uniform(100, 540), rng.uniform(100, 380))
              for _ in range(ANNS)]
        gts[n] = gl
        for p in range(DETS):
            g = gl[p % ANNS]
            level = rng.uniform(0, .06) if p < 6 else 1.0
            kpts[n, p, :, :2] = g['kpts'][:, :2] + rng.normal(0, 1, (J, 2)) * level * np.sqrt(g['area'])
            scores[n, p] = np.clip(.9 - 8 * level + rng.uniform(-.2, .2), .01, .99)
        dets[n] = [{'kpts': kpts[n, p, :, :2].astype(np.float64), 'score': float(scores[n, p])} for p in range(DETS)]
    return kpts, count, scores, gts, dets


def median_s(fn, runs=5):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main(reps):
    kpts, count, scores, gts, dets = make_set()
    ids = list(range(IMAGES))
    gt = ce.GroundTruth.from_arrays(*R.ground_truth_arrays(gts, ids))
    k, c, s = (torch.from_numpy(a).cuda() for a in (kpts, count, scores))
    print('COCO keypoint AP of %d images x %d detections x %d annotations (17 joints, 10 thresholds x 3 area ranges)'
          % (IMAGES, DETS, ANNS))
    print('command: python tools/time_ap.py %d   (launch: hipGraph replays, one HIP event pair each; host: median of 5)' % reps)

    ev = ce.KeypointEvaluator(gt)
    ev.add(k, c, s, ids)                                         # warm-up: tables uploaded, outputs allocated
    torch.cuda.synchronize()
    block = ev._queue[0][1]

    rows = torch.tensor([gt.slot[i] for i in ids], dtype=torch.int32).cuda()

    def launch():                                                # the call of add() into the same outputs, no allocation
        ev._launch(k, c, s, rows, block)

    launch()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in pairs:
        a.record()
        graph.replay()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) for a, b in pairs]) * 1e3
    print('lp_kpt_eval N=%d            median %10.1f us  min %10.1f us  (%d replays)' % (IMAGES, np.median(us), us.min(), reps))

    t_d2h, _ = median_s(ev._collect)
    t_acc, _ = median_s(lambda: (ev.accumulate(), ev.summarize()))
    stats = ev.summarize()
    print('D2H of the compact outputs    median %10.1f us  (%d bytes)' % (t_d2h * 1e6, block.numel() * 4))
    print('host accumulate + summarize   median %10.1f us  (includes that D2H)' % (t_acc * 1e6))

    def loops():
        per = R.evaluate_set(dets, gts, ids, R.COCO_SIGMAS)
        return R.summarize(*R.accumulate(per))
    t_ref, want = median_s(loops, runs=1)
    print('restatement loops on the CPU  %10.1f us  (tests/_cocoeval_ref.py: evaluate_set + accumulate, one run)' % (t_ref * 1e6))
    print('AP %.6f (device) / %.6f (restatement), the ten stats %s' % (stats['AP'], want['AP'],
                                                                      'equal' if stats == want else 'DIFFER'))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
