#!/usr/bin/env python
"""One BatchNorm calibration step of an XS-sized supernet sub-network at 256^2 (lp_calib_step) against the PyTorch-ROCm
training-mode forward of tests/_supernet_ref.py on the same box, and the two new kernels against the bytes they must move.

    python tools/calib_time.py [--batches 32 64] [--reps 30]      # interleaved timing, profiler off
    rocprofv3 --kernel-trace -d DIR -o t -- python tools/calib_time.py --trace --batches 32
    python tools/calib_time.py --db DIR/.../t_results.db --batches 32   # per-kernel times of the LAST traced step

Timing: both sides run the same sliced weights and the same device batch; a host clock around work that ends in a device
synchronise, the two alternating, median and min / max of --reps.  Kernel table: the last step's bn_stats_kernel /
bn_apply_kernel dispatches are matched, in launch order, to the BatchNorm layers of the sub-network; bytes = what the
algorithm needs (statistics: one read of the raw tensor; apply: one read + one write, + one read where the block adds a
residual), grouped by plane size, over the kernels' durations."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--batches', type=int, nargs='+', default=[32, 64])
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--arch', default='search-XS')
ap.add_argument('--trace', action='store_true', help='a few steps only: the run rocprofv3 traces')
ap.add_argument('--db', default=None)
args = ap.parse_args()

from litepose_amd import arch_zoo  # noqa: E402
from oracle import spec  # noqa: E402

ARCH = arch_zoo.get(args.arch)


def layer_table(arch, R):
    """(prefix, channels, plane size, residual add in the apply launch) of every BatchNorm in launch order."""
    d = spec.derive(arch)
    r = R // 2
    L = [('first.0.1', 32, r * r, False), ('first.1.1', 32, r * r, False), ('first.3', d['c0'], r * r, False)]
    planes = [r]
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            ro = r // blk['stride']
            L += [(p + '.inv.1', blk['feat'], r * r, False), (p + '.depth_conv.1', blk['feat'], ro * ro, False),
                  (p + '.point_conv.1', blk['oup'], ro * ro, blk['residual'])]
            r = ro
        planes.append(r)
    for i, dc in enumerate(d['deconv']):
        r *= 2
        L.append(('deconv_bnrelu.%d.0' % i, dc['out'], r * r, False))
        if i > 0:
            h = d['heads'][i - 1]
            L += [('final_refined.%d.conv.1' % (i - 1), h['refined_in'], r * r, False),
                  ('final_raw.%d.conv.1' % (i - 1), h['raw_in'], r * r, False)]
    return L


if args.db:
    import sqlite3
    N = args.batches[0]
    L = layer_table(ARCH, args.size)
    rows = sqlite3.connect(args.db).execute('select name, duration from kernels order by start').fetchall()
    st = [d for n, d in rows if 'bn_stats_kernel' in n][-len(L):]
    apl = [d for n, d in rows if 'bn_apply_kernel' in n][-len(L):]
    assert len(st) == len(L) and len(apl) == len(L), (len(st), len(apl), len(L))
    groups = {}
    for (p, c, hw, res), ds, da in zip(L, st, apl):
        g = groups.setdefault(hw, [0, 0, 0.0, 0, 0.0])
        g[0] += 1
        g[1] += 4 * N * c * hw
        g[2] += ds
        g[3] += (12 if res else 8) * N * c * hw
        g[4] += da
    print('%s @ %d^2, batch %d, last traced step: %d BatchNorm layers' % (args.arch, args.size, N, len(L)))
    print('%10s %6s | %10s %9s %8s | %10s %9s %8s' % ('plane', 'layers', 'stats MB', 'us', 'GB/s', 'apply MB', 'us', 'GB/s'))
    tot = [0, 0.0, 0, 0.0]
    for hw in sorted(groups, reverse=True):
        k, bs, ts, ba, ta = groups[hw]
        side = int(round(hw ** 0.5))
        print('%10s %6d | %10.1f %9.1f %8.0f | %10.1f %9.1f %8.0f'
              % ('%dx%d' % (side, side), k, bs / 1e6, ts / 1e3, bs / ts, ba / 1e6, ta / 1e3, ba / ta))
        tot = [tot[0] + bs, tot[1] + ts, tot[2] + ba, tot[3] + ta]
    print('%10s %6d | %10.1f %9.1f %8.0f | %10.1f %9.1f %8.0f'
          % ('all', len(L), tot[0] / 1e6, tot[1] / 1e3, tot[0] / tot[1], tot[2] / 1e6, tot[3] / 1e3, tot[2] / tot[3]))
    agg = {}
    last = len([1 for n, _ in rows if 'bn_stats_kernel' in n]) // len(L)
    for n, d in rows:
        a = agg.setdefault(n.split('(')[0].replace('void ', ''), [0, 0.0])
        a[0] += 1
        a[1] += d
    print('whole trace (%d steps), kernel time by kernel:' % last)
    for n, (k, d) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:12]:
        print('  %-60s %5d launches %10.1f us' % (n[:60], k, d / 1e3))
    sys.exit(0)

import torch  # noqa: E402
import _supernet_ref as sr  # noqa: E402
from litepose_amd import config  # noqa: E402
from litepose_amd.models import pose_mobilenet, pose_supermobilenet  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('calib_time.py times the device: no GPU here')
cfg = config.get_cfg('crowd_pose')
sup = pose_supermobilenet.get_pose_net(cfg)
sup.load_state_dict(sr.make_state_dict(sr.SEED), strict=True)
sub = sup.sub_state_dict(ARCH)
net = pose_mobilenet.LitePose(cfg, cfg_arch=ARCH, storage='f32')
net.load_state_dict(sub, strict=True)
cal = pose_supermobilenet.Calibration(net, 0.1)
tsd = {k: v.cuda() for k, v in sub.items()}
print('%s @ %d^2: %d BatchNorm layers; device %s' % (args.arch, args.size, len(layer_table(ARCH, args.size)),
                                                   torch.cuda.get_device_name(0)))
for N in args.batches:
    x = torch.randn(N, 3, args.size, args.size, generator=torch.Generator().manual_seed(N)).cuda()

    def ours():
        cal.step(x)

    def theirs():
        with torch.no_grad():
            sr.train_forward(x, tsd, ARCH)

    for f in (ours, theirs):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    if args.trace:
        for _ in range(3):
            ours()
        torch.cuda.synchronize()
        print('traced 3 steps at batch', N)
        continue
    t = {'lp_calib_step': [], 'torch train_forward': []}
    for _ in range(args.reps):
        for name, f in (('lp_calib_step', ours), ('torch train_forward', theirs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in t.items():
        v.sort()
        print('batch %3d  %-20s median %8.3f ms  min %8.3f  max %8.3f  (%d reps, interleaved)'
              % (N, name, v[len(v) // 2], v[0], v[-1], len(v)))
cal.end()
