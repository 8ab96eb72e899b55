#!/usr/bin/env python
"""Latency of the two parsers on the same merged maps (GPU box): lp_fast_parse (the reference's real-time demo parser,
fast_utils) on the full-resolution det / tag maps of lp_tta_project, and the engine's default lp_parse_mid on the stage merge
they were projected from.  XS@256 (stage-1 merge 128x128, maps 256x256, 14 joints), blob scenes of oracle/synth.py with 8
people (the scenes of tools/time_plateau.py) and, as a second pair of rows, with 2; N = 1 and N = 64.  With 8 people the
reference's Kuhn-Munkres loop needs 5000 - 9600 match / update rounds in one joint, so every such image hits
lp_fast_assign's cap of 4096 rounds and comes back with num = -1 after the full 4096: those rows are the cap's cost, the
2-people rows (3 rounds) the ordinary one.  The number of capped images is printed.

Each call is captured into a hipGraph once and replayed, alternating between the two parsers, one HIP event pair per
replay; prints the median and the minimum.  REPS replays (default 200) -- unless one probe replay of a call takes more than
SLOW_MS: then that call gets as many replays as fit SLOW_BUDGET_S seconds (at least 3), and its row says how many.  That
bounds the run: a batch of 64 capped images is a single wave whose lanes each walk their own 4096 rounds, seconds per
call, and 200 of those would hold a GPU for minutes to measure a failure path.  The whole run stays under five minutes.

The two parsers produce different records by design (first M peaks in raster order and a greedy 1-D tag assignment,
against top-k, munkres, adjust and refine): this compares what a call costs, not what it returns.  profiles/
fast_parse_latency.txt is this program's output.

    python tools/time_fast_parse.py [REPS] > profiles/fast_parse_latency.txt
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from litepose_amd import _native as nv, config
from litepose_amd.core import group
from litepose_amd.fast_utils import group as fast_group
from oracle import synth

J, H1, W1, T, PCAP = 14, 128, 128, 2, 30
SLOW_MS, SLOW_BUDGET_S = 150.0, 15.0


def captured(fn):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    return g


def main(reps):
    lib = nv.lib()
    cfg = config.get_cfg('crowd_pose')
    cfg.DATASET.MAX_NUM_PEOPLE = 10                              # the fast parser's limit; 8 people per scene
    full = group.HeatmapParser(cfg, person_capacity=PCAP)
    fast = fast_group.Params(cfg)
    M = fast.max_num_people
    order = (C.c_int32 * J)(*fast.joint_order[:J])
    print('lp_fast_parse against lp_parse_mid, XS@256 merged maps (stage merge 128x128, maps 256x256, 14 joints), blob scenes')
    print('command: python tools/time_fast_parse.py %d   (hipGraph replays, one HIP event pair each, parsers alternating;' % reps)
    print('a call whose probe replay takes over %.0f ms gets the replays that fit %.0f s)' % (SLOW_MS, SLOW_BUDGET_S), flush=True)
    for people, N in ((8, 1), (8, 64), (2, 1), (2, 64)):
        rng = np.random.default_rng(5)
        mid_np = np.zeros((N, 4, J, H1, W1), np.float32)
        for n in range(N):
            d, t = synth.blob_scene(rng, J, H1, W1, 2, n_people=people, sigma=2.0)
            mid_np[n, 0], mid_np[n, 1], mid_np[n, 2], mid_np[n, 3] = d, d * np.float32(0.97), t[..., 0], t[..., 1]
        mid = torch.from_numpy(mid_np).cuda()
        H, W = 2 * H1, 2 * W1
        det = torch.empty((N, J, H, W), device='cuda')
        tag = torch.empty((N, J, H, W, T), device='cuda')
        nv.check(lib.lp_tta_project(nv.dptr(mid), N, J, H1, W1, H, W, T, nv.dptr(det), nv.dptr(tag), nv.stream_ptr()))
        need = int(lib.lp_parse_workspace_bytes(N, J, M, T, PCAP))
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        ans = torch.zeros((N, PCAP, J, 3 + T), device='cuda')
        cnt = torch.zeros((N,), dtype=torch.int32, device='cuda')
        sc = torch.zeros((N, PCAP), device='cuda')
        fneed = int(lib.lp_fast_parse_workspace_bytes(N, J, M))
        fws = torch.empty(fneed, dtype=torch.uint8, device='cuda')
        fans = torch.zeros((N, M, J, 4), device='cuda')
        fnum = torch.zeros((N,), dtype=torch.int32, device='cuda')
        calls = {
            'lp_parse_mid': lambda: nv.check(lib.lp_parse_mid(
                nv.dptr(mid), N, J, H1, W1, T, C.byref(full._q), PCAP, 1, 1, nv.dptr(ans), nv.dptr(cnt), nv.dptr(sc),
                nv.dptr(ws), need, nv.stream_ptr()), 'lp_parse_mid'),
            'lp_fast_parse': lambda: nv.check(lib.lp_fast_parse(
                nv.dptr(det), nv.dptr(tag), T, N, J, H, W, float(fast.detection_threshold), int(fast.window_size), M, order,
                float(fast.tag_threshold), nv.dptr(fans), nv.dptr(fnum), nv.dptr(fws), fneed, nv.stream_ptr()), 'lp_fast_parse'),
        }
        graphs = {k: captured(f) for k, f in calls.items()}
        n_reps = {}
        for k, g in graphs.items():                              # one probe replay (also the warm-up) sizes the count
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            probe = a.elapsed_time(b)
            n_reps[k] = reps if probe <= SLOW_MS else min(reps, max(3, int(SLOW_BUDGET_S * 1e3 / probe)))
            for _ in range(10 if probe <= SLOW_MS else 0):
                g.replay()
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_reps[k])]
              for k in graphs}
        for r in range(max(n_reps.values())):
            for k, g in graphs.items():
                if r < n_reps[k]:
                    a, b = ev[k][r]
                    a.record()
                    g.replay()
                    b.record()
        torch.cuda.synchronize()
        persons = {'lp_parse_mid': '%d persons' % int(cnt.clamp(max=PCAP).sum()),
                   'lp_fast_parse': '%d persons, %d of %d images at the round cap' % (int(fnum.clamp(min=0).sum()), int((fnum < 0).sum()), N)}
        for k in graphs:
            us = np.array([a.elapsed_time(b) for a, b in ev[k]]) * 1e3
            print('%d people/image N=%-3d %-14s median %10.1f us  min %10.1f us  (%d replays, %s)'
                  % (people, N, k, np.median(us), us.min(), n_reps[k], persons[k]), flush=True)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
