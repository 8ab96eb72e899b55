#!/usr/bin/env python
"""Throughput of ``PoseEngine.evaluate`` on a validation-like set: seeded uint8 noise images drawn from a fixed list of
COCO / CrowdPose-like sizes (both orientations), end to end -- host packing, H2D of the uint8 sources, the per-image warp,
the network, the AE stage, per-image back-projection, records -> result dicts.  Prints ONE JSON line:

    img_per_s            over the whole evaluate() call (the first call: graph captures included)
    img_per_s_warm       a second call on the same engine (buckets release their graphs when done: few replays)
    buckets              network input size -> images
    graph_stats          of the engine after both calls
    split                seconds: host packing (worker thread), main thread waiting for the packing, waiting for the
                         device (record read-back), records -> result dicts (Python, per person), total -- which one
                         is the limit
    batch1_img_per_s     the batch-1 drop-in loop (valid.py:195-233 shape) over the first --batch1 images
    speedup_vs_batch1    img_per_s_warm / batch1_img_per_s

--scales 0.5,1,2 sets TEST.SCALE_FACTOR (multi-scale testing), --no-project2image TEST.PROJECT2IMAGE = False; both
legs run the same configuration.

    python tools/eval_mixed.py --images 2048 --batch 64
    python tools/eval_mixed.py --images 512 --batch 16 --scales 0.5,1,2"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from litepose_amd import arch_zoo, config, engine  # noqa: E402
from oracle import synth  # noqa: E402

# H x W: COCO val2017's most frequent sizes and CrowdPose-like ones, landscape and portrait
SIZES = [(427, 640), (480, 640), (640, 427), (640, 480), (612, 612), (640, 360), (360, 640), (375, 500), (500, 375),
         (333, 500), (500, 333), (424, 640), (640, 424), (512, 640), (683, 1024), (200, 600)]


def batch1_loop(cfg, model, images):
    from litepose_amd.core.group import HeatmapParser
    from litepose_amd.core.inference import aggregate_results, get_multi_stage_outputs
    from litepose_amd.utils.transforms import (ToTensorNormalize, get_final_preds, get_multi_scale_size,
                                               resize_align_multi_scale)
    parser = HeatmapParser(cfg)
    tf = ToTensorNormalize()
    sf = cfg.TEST.SCALE_FACTOR
    out = []
    for image in images:
        base_size, center, scale = get_multi_scale_size(image, cfg.DATASET.INPUT_SIZE, 1.0, min(sf))
        fh, tl = None, []
        for s in sorted(sf, reverse=True):
            x, center, scale = resize_align_multi_scale(image, cfg.DATASET.INPUT_SIZE, s, min(sf))
            x = tf(x).unsqueeze(0)
            _, hm, tg = get_multi_stage_outputs(cfg, model, x, cfg.TEST.FLIP_TEST, cfg.TEST.PROJECT2IMAGE, base_size)
            fh, tl = aggregate_results(cfg, s, fh, tl, hm, tg)
        fh = fh / float(len(sf))
        grouped, scores = parser.parse(fh, torch.cat(tl, dim=4), cfg.TEST.ADJUST, cfg.TEST.REFINE)
        out.append((get_final_preds(grouped, center, scale, [fh.size(3), fh.size(2)]), scores))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='search-XS')
    ap.add_argument('--images', type=int, default=2048)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--batch1', type=int, default=64)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--storage', default='f32', choices=['f32', 'bf16', 'f16'])
    # head gain of the synthetic weights: 1.0 gives a few persons per noise image, 6.0 saturates the grouping
    # (hundreds per image: the Python result formatting then dominates the call)
    ap.add_argument('--head-gain', type=float, default=1.0)
    ap.add_argument('--scales', default='1', help='TEST.SCALE_FACTOR, comma separated (e.g. 0.5,1,2)')
    ap.add_argument('--no-project2image', action='store_true', help='TEST.PROJECT2IMAGE = False')
    a = ap.parse_args()
    arch = arch_zoo.get(a.arch)
    cfg = config.apply_arch(config.get_cfg('crowd_pose'), arch)
    cfg.TEST.SCALE_FACTOR = [float(v) for v in a.scales.split(',')]
    cfg.TEST.PROJECT2IMAGE = not a.no_project2image
    sd = synth.make_state_dict(arch, seed=1234, head_gain=a.head_gain)
    rng = np.random.default_rng(a.seed)
    pick = rng.integers(0, len(SIZES), size=a.images)
    images = [rng.integers(0, 256, size=SIZES[k] + (3,), dtype=np.uint8) for k in pick]
    eng = engine.PoseEngine(cfg, arch, sd, storage=a.storage)
    res = {}
    for leg in ('cold', 'warm'):
        torch.cuda.synchronize()
        st = {}
        t0 = time.perf_counter()
        out = eng.evaluate(images, batch_size=a.batch, stats=st)
        torch.cuda.synchronize()
        res[leg] = (time.perf_counter() - t0, st, out)
    assert res['cold'][2] == res['warm'][2]
    # the batch-1 drop-in loop (graph-free, one image at a time) over the first --batch1 images
    import litepose_amd.models as models
    model = models.pose_mobilenet.get_pose_net(cfg, is_train=False, cfg_arch=arch, storage=a.storage)
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    model.eval()
    n1 = min(a.batch1, len(images))
    batch1_loop(cfg, model, images[:2])                     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batch1_loop(cfg, model, images[:n1])
    torch.cuda.synchronize()
    t1 = time.perf_counter() - t0
    st = res['warm'][1]
    line = {
        'metric': 'evaluate_mixed_img_per_s', 'arch': a.arch, 'storage': a.storage, 'images': len(images),
        'batch': a.batch, 'head_gain': a.head_gain, 'img_per_s': round(len(images) / res['cold'][0], 1),
        'img_per_s_warm': round(len(images) / res['warm'][0], 1),
        'persons': len(res['warm'][2]), 'buckets': st['buckets'], 'batches': st['batches'],
        'padding_rows': st['padding_rows'], 'src_mb': round(st['src_bytes'] / 1e6, 1),
        'split_warm_s': {k: round(st[k], 4) for k in ('pack_s', 'wait_pack_s', 'wait_device_s', 'format_s', 'total_s')},
        'split_cold_s': {k: round(res['cold'][1][k], 4) for k in ('pack_s', 'wait_pack_s', 'wait_device_s', 'format_s', 'total_s')},
        'graph_stats': eng.graph_stats(),
        'batch1_images': n1, 'batch1_img_per_s': round(n1 / t1, 1),
        'speedup_vs_batch1': round((len(images) / res['warm'][0]) / (n1 / t1), 2),
        'scales': list(cfg.TEST.SCALE_FACTOR), 'project2image': bool(cfg.TEST.PROJECT2IMAGE),
    }
    print(json.dumps(line))


if __name__ == '__main__':
    main()
