#!/usr/bin/env python
"""Run the bench's engine configuration (XS@256, 64 images + mirrored, pcap 30, synthetic scenes) a few times
on ONE stream, for rocprofv3 traces / PMC passes over every kernel of the path incl. the AE stage:
    LP_STREAMS=1 rocprofv3 --kernel-trace --stats -d out -o t -- python tools/run_engine.py --reps 3
--model simplenet runs the pose_simplenet network (cfg.MODEL.NAME = 'pose_simplenet': no Fusion Deconv Head) instead of
pose_mobilenet, --model resnet the pose_resnet network (dense FusedMBConv blocks; no arch JSON: --arch is ignored and the
input size is --size or 256; with --profile the table also lists every launch with its MACs and its share of the bf16x3
class peak); --profile K prints the kernel-stats table of one forward of the network (lp_net_profile: plain + mirrored
batch, one launch per op; every launch's median over K profiled forwards) and its summed kernel time."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from litepose_amd import arch_zoo, config, engine  # noqa: E402
from oracle import inference_ref, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--arch', default='search-XS')
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--size', type=int, default=0)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--warmup', type=int, default=1)
ap.add_argument('--storage', default='f32', choices=['f32', 'bf16', 'f16'])
ap.add_argument('--model', default='mobilenet', choices=['mobilenet', 'simplenet', 'resnet'])
ap.add_argument('--profile', type=int, default=0, metavar='K',
                help='K profiled forwards of the network; the table holds each launch\'s median over them')
a = ap.parse_args()
arch = arch_zoo.get(a.arch)
R = a.size or arch['img_size']
cfg = config.apply_arch(config.get_cfg(), arch)
cfg.MODEL.NAME = 'pose_' + a.model
if a.model == 'resnet':                           # resnet.yaml's network settings; the restatement's synthetic weights
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import _resnet_ref  # noqa: E402
    R = a.size or 256
    cfg.DATASET.INPUT_SIZE, cfg.DATASET.OUTPUT_SIZE = R, [R // 4, R // 2]
    cfg.MODEL.EXTRA.NUM_DECONV_KERNELS, cfg.MODEL.EXTRA.NUM_DECONV_FILTERS = [3, 3, 3], [16, 24, 24]
    arch, a.arch = None, 'resnet'
    sd = _resnet_ref.make_state_dict(cfg, seed=1234, head_gain=0.25)
else:
    sd = synth.make_state_dict(arch, seed=1234, head_gain=0.25)
if a.model == 'simplenet':                        # pose_simplenet.py registers no raw branches
    sd = {k: v for k, v in sd.items() if not k.startswith(('deconv_raw.', 'final_raw.'))}
eng = engine.PoseEngine(cfg, arch, sd, person_capacity=30, pipeline_halves=False, storage=a.storage, options=engine.options_from_env())
x = synth.make_images(a.batch, R, seed=100).cuda()
off0, off1 = synth.lowres_offsets(200, a.batch, 14, R)
f0, f1 = synth.flip_offsets(off0, off1, inference_ref.FLIP_CONFIG['CROWDPOSE'])
offs = (torch.from_numpy(np.concatenate([off0, f0])).cuda(), torch.from_numpy(np.concatenate([off1, f1])).cuda())
# ONE stream: lp_net_forward without its internal plain/mirrored stream pair, _infer_one directly (infer_batch
# would switch the pair back on), so every kernel's trace duration is an un-shared, back-to-back launch
from litepose_amd import _native as nv  # noqa: E402
nv.check(eng._lib.lp_net_set_streams(eng.model._h, 1))
for _ in range(a.warmup):
    out = eng._infer_one(x, offs, None, None)
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0.record()
for _ in range(a.reps):
    out = eng._infer_one(x, offs, None, None)
t1.record()
torch.cuda.synchronize()
print('persons', int(out[1].sum()), 'path', eng._last[0][0])
# one stream, batch after batch: time per batch of the timed reps (not bench.py's pipelined serving loop)
print('%s %s@%d b%d %s: %.3f ms/step over %d reps' % (cfg.MODEL.NAME, a.arch, R, a.batch, a.storage,
                                                     t0.elapsed_time(t1) / a.reps, a.reps))
if a.profile:
    m = eng.model
    m.set_profiling(True)
    m.forward_native(x, 2)                        # warm
    runs = []
    for _ in range(a.profile):
        m.forward_native(x, 2)
        torch.cuda.synchronize()
        runs.append(m.profile())
    m.set_profiling(False)
    stats = {}
    for i, (name, _, _, _) in enumerate(runs[0]):
        tag = name.rsplit('|', 1)[1]
        c, t = stats.get(tag, (0, 0.0))
        stats[tag] = (c + 1, t + float(np.median([r[i][1] for r in runs])))
    total = sum(t for _, t in stats.values())
    print('kernel stats of one forward (%s, %s@%d, %d images + mirrored, %s; per launch the median of %d profiled '
          'forwards):' % (cfg.MODEL.NAME, a.arch, R, a.batch, a.storage, a.profile))
    print('%-28s %6s %10s %7s' % ('kernel', 'calls', 'ms', '%'))
    for tag, (c, t) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
        print('%-28s %6d %10.4f %6.1f%%' % (tag, c, t, 100.0 * t / total))
    print('%-28s %6d %10.4f' % ('total', sum(c for c, _ in stats.values()), total))
    if a.model == 'resnet':                       # every launch: its MACs from the shapes, priced as bench.py prices bf16x3 work
        print('%-44s %9s %9s %8s' % ('launch|kernel', 'ms', 'GMAC', '%of417TF'))
        for i, (name, _, _, fl) in enumerate(runs[0]):
            ms = float(np.median([r[i][1] for r in runs]))
            print('%-44s %9.4f %9.3f %7.1f%%' % (name, ms, fl / 2e9, 100.0 * fl / (ms * 1e-3) / 417e12))
