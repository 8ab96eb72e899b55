#!/usr/bin/env python
"""Dump the deconv taps (lp_net_tap) and both outputs of the fp32 network on seeded inputs, or compare two dumps byte
for byte.  Used to check a rewritten deconv kernel against the parent commit's on one GPU:
    python tools/dump_deconv_taps.py --out DIR           (in each tree)
    python tools/dump_deconv_taps.py --compare DIR_A DIR_B"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

CASES = [('mobilenet', 'search-XS', 256, 256, 8), ('mobilenet', 'search-XS', 208, 336, 3),
         ('mobilenet', 'search-S', 448, 448, 3), ('mobilenet', 'search-M', 448, 448, 2),
         ('mobilenet', 'search-M', 608, 256, 2), ('simplenet', 'search-XS', 256, 256, 4)]


def dump(out):
    import torch
    from litepose_amd import arch_zoo, config
    import litepose_amd.models as models
    from oracle import spec, synth
    os.makedirs(out, exist_ok=True)
    for model, arch_name, H, W, N in CASES:
        arch = arch_zoo.get(arch_name)
        sd = synth.make_state_dict(arch, seed=1234)
        if model == 'simplenet':
            sd = {k: v for k, v in sd.items() if not k.startswith(('deconv_raw.', 'final_raw.'))}
        net = getattr(models, 'pose_' + model).get_pose_net(config.get_cfg('crowd_pose'), is_train=False, cfg_arch=arch,
                                                            storage='f32')
        net.load_state_dict(sd, strict=True)
        x = synth.make_images(N, H, seed=77, w=W).cuda()
        outs = net.forward_native(x, 2)
        torch.cuda.synchronize()
        key = '%s_%s_%dx%d_b%d' % (model, arch_name, H, W, N)
        for k, o in enumerate(outs):
            np.save(os.path.join(out, '%s_out%d.npy' % (key, k)), o.cpu().numpy())
        for i in range(len(spec.derive(arch)['deconv'])):
            np.save(os.path.join(out, '%s_deconv%d.npy' % (key, i)), net.tap('deconv.%d' % i).cpu().numpy())


def compare(a, b):
    bad = 0
    for f in sorted(os.listdir(a)):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and x.tobytes() == y.tobytes()
        bad += not same
        print('%-48s %-22s %10d bytes  %s' % (f, x.shape, x.nbytes, 'identical' if same else 'DIFFERENT'))
    print('%d of %d files differ' % (bad, len(os.listdir(a))))
    return bad


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(*a.compare) else 0)
    dump(a.out)
