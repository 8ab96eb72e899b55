#!/usr/bin/env python
"""A/B of option "mbt_strip" inside ONE process, on bench.py's serving loop (XS@256, 64 images + 64 mirrored): the option is
flipped between 0 (16x16 tiles) and 1 (32 x 16 strips where they fill the CUs) on one engine, the captured graphs are
dropped and captured again, and the two settings are timed in turn, so clocks and box are the same for both.  Also prints
the single-stream time of the stage-1 mbt_kernel launches of one forward under each setting (event timing of a profiled
forward, one network in flight).
    python tools/mbt_strip_ab.py --rounds 5 --steps 40 --warmup 10"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from litepose_amd import arch_zoo, config, engine  # noqa: E402
from oracle import inference_ref, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--settings', default='0,1', help='values of "mbt_strip" to interleave')
a = ap.parse_args()
settings = [int(v) for v in a.settings.split(',')]
arch = arch_zoo.get('search-XS')
R, B = 256, 64
cfg = config.apply_arch(config.get_cfg(), arch)
sd = synth.make_state_dict(arch, seed=1234, head_gain=0.25)
eng = engine.PoseEngine(cfg, arch, sd, person_capacity=30, options=engine.options_from_env())
x = synth.make_images(B, R, seed=100).cuda()
off0, off1 = synth.lowres_offsets(200, B, 14, R)
f0, f1 = synth.flip_offsets(off0, off1, inference_ref.FLIP_CONFIG['CROWDPOSE'])
offs = (torch.from_numpy(np.concatenate([off0, f0])).cuda(), torch.from_numpy(np.concatenate([off1, f1])).cuda())
depth = eng.pipeline_depth()


def run(k):
    pending = []
    for _ in range(k):
        pending.append(eng.submit(x, offsets=offs))
        if len(pending) > depth:
            h = pending.pop(0)
            h.result()
            h.release()
    for h in pending:
        h.result()
        h.release()


def timed(setting):
    eng.model.set_option('mbt_strip', setting)
    eng.reset_graphs()
    eng.prepare(x, offsets=offs)
    run(a.warmup)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(a.steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


def single_stream(setting, reps=5):
    m = eng.model
    m.set_option('mbt_strip', setting)
    best, net = None, float('inf')
    for _ in range(reps):
        m.set_profiling(True)
        m.forward_native(x, 2)
        torch.cuda.synchronize()
        prof = m.profile(launches=True)
        m.set_profiling(False)
        rows = [p for p in prof if p[0].startswith('stage.1.') and p[0].endswith('|mbt_kernel')]
        t = sorted(p[1] for p in rows)
        cur = (sum(p[1] for p in rows), t[len(t) // 2], len(rows), rows[0][5])
        best = cur if best is None or cur[0] < best[0] else best
        net = min(net, sum(p[1] for p in prof))
    return best + (net,)


res = {s: [] for s in settings}
for r in range(a.rounds):
    for s in settings:
        res[s].append(timed(s))
    print('round %d: %s' % (r, '  '.join('mbt_strip=%d %.4f ms/step' % (s, res[s][-1]) for s in settings)), flush=True)
for s in settings:
    v = np.array(res[s])
    print('mbt_strip=%d: median %.4f  min %.4f  max %.4f ms/step over %d rounds of %d steps'
          % (s, np.median(v), v.min(), v.max(), a.rounds, a.steps))
if len(settings) == 2:
    p, q = (np.array(res[s]) for s in settings)
    print('difference of the medians (first - second): %.4f ms/step; range of the first: %.4f'
          % (np.median(p) - np.median(q), p.max() - p.min()))
for s in settings:
    tot, med, n, geo, net = single_stream(s)
    print('mbt_strip=%d single stream: %d stage-1 mbt_kernel launches, %.1f us in all, median %.1f us each, grid %d x %d threads, '
          'LDS %d B, %d workgroup(s) per CU; network %.3f ms (best of the repetitions)' % (s, n, tot * 1e3, med * 1e3, geo[0], geo[1], geo[2], geo[3], net))
eng.model.set_option('mbt_strip', 1)
