"""search.py's ``main``: score the two fixed sub-networks, run the evolutionary search under an efficiency constraint and
write ``search_result.json``.

    python -m litepose_amd.arch_search --cfg experiments/crowd_pose/mobilenet/supermobile.yaml \\
        --supernet supernet.pth --calib-images calibrate/ --search-images images/ --annotations search.json \\
        --constraint 8 [--out DIR] [KEY VALUE ...]

``--annotations`` is the search split's COCO keypoint file; its ``images`` name the files under ``--search-images``.
``--calib-images`` is a directory whose image files (sorted by name) are the calibrate split.  Images are decoded on the
host with Pillow; everything after that runs on the device.  The constraint is in this library's unit (1e9
multiply-accumulates, ``EfficiencyEvaluator``), not ptflops'."""
import argparse
import json
import os
import time

import numpy as np

_IMAGE_EXT = ('.jpg', '.jpeg', '.png', '.bmp')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='python -m litepose_amd.arch_search',
                                     description='Search the supernet for the best sub-network under a constraint')
    parser.add_argument('--cfg', help='experiment configure file name', required=True, type=str)
    parser.add_argument('--supernet', help='supernet checkpoint (default: TEST.MODEL_FILE of the cfg)', type=str, default='')
    parser.add_argument('--calib-images', help='directory of the calibrate split\'s images', required=True, type=str)
    parser.add_argument('--search-images', help='directory of the search split\'s images', required=True, type=str)
    parser.add_argument('--annotations', help='COCO keypoint JSON of the search split', required=True, type=str)
    parser.add_argument('--constraint', help='efficiency constraint in 1e9 multiply-accumulates', type=float, default=8.0)
    parser.add_argument('--out', help='directory search_result.json is written to', type=str,
                        default=os.path.join('arch_search', 'result'))
    parser.add_argument('--population-size', type=int, default=40)
    parser.add_argument('--max-time-budget', type=int, default=40)
    parser.add_argument('--calib-batch-size', type=int, default=16)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--quiet', action='store_true', help='do not print the progress of the search')
    parser.add_argument('opts', help='Modify config options using the command-line', default=None,
                        nargs=argparse.REMAINDER)
    return parser.parse_args(argv)


def _read_image(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8))


def main(argv=None):
    args = parse_args(argv)
    import torch
    from .. import coco_eval, config
    from ..dataset.calibration import CalibrationSet
    from ..models.pose_supermobilenet import ArchManager, SuperLitePose
    from . import AccuracyEvaluator, EfficiencyEvaluator, EvolutionFinder

    cfg = config.update_config(config.get_cfg(), args)
    ckpt = args.supernet or cfg.TEST.MODEL_FILE
    if not ckpt:
        raise SystemExit('no supernet checkpoint: give --supernet or TEST.MODEL_FILE')
    model = SuperLitePose(cfg)
    model.load_state_dict(torch.load(ckpt, map_location='cpu'), strict=True)

    with open(args.annotations) as f:
        coco = json.load(f)
    gt = coco_eval.GroundTruth.from_coco(coco)
    search_ids = [int(im['id']) for im in coco['images']]
    search_images = [_read_image(os.path.join(args.search_images, im['file_name'])) for im in coco['images']]
    names = sorted(n for n in os.listdir(args.calib_images) if n.lower().endswith(_IMAGE_EXT))
    calib = CalibrationSet([_read_image(os.path.join(args.calib_images, n)) for n in names])

    acc_pred = AccuracyEvaluator(cfg, model, calib, search_images, search_ids,
                                 lambda: coco_eval.KeypointEvaluator(gt), batch_size=args.calib_batch_size,
                                 seed=args.seed)
    eff_pred = EfficiencyEvaluator(cfg)
    arch_manager = ArchManager(cfg)
    for reso, ratio in ((512, 1.0), (256, 0.5)):
        begin = time.time()
        cfg_arch = arch_manager.fixed_sample(reso=reso, ratio=ratio)
        output_acc = acc_pred.predict_acc(cfg_arch)
        output_eff = eff_pred.predict_eff(cfg_arch)
        if not args.quiet:
            print('normal: acc:{}, eff:{}, time:{}'.format(output_acc, output_eff, time.time() - begin))

    arch_selector = EvolutionFinder(cfg, eff_pred, acc_pred, population_size=args.population_size,
                                    max_time_budget=args.max_time_budget)
    arch_selector.set_efficiency_constraint(args.constraint)
    best_valids = arch_selector.run_evolution_search(verbose=not args.quiet)
    if not args.quiet:
        print('Get point: (eff, acc) = ({}, {})'.format(best_valids[2], best_valids[0]))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'search_result.json'), 'w') as f:
        json.dump({0: (arch_selector.efficiency_constraint, best_valids)}, f)


if __name__ == '__main__':
    main()
