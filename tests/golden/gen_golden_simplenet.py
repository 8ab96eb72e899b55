#!/usr/bin/env python
"""Network outputs of the REAL reference pose_simplenet module (lib/models/pose_simplenet.py: LitePose without the Fusion
Deconv Head) for search-XS and search-S at 64x64 and search-M at 96x160.

Run in the build container only (needs the reference checkout, like gen_golden.py):

    python tests/golden/gen_golden_simplenet.py

Imports the reference module by path (nothing is copied), feeds it the seeded synthetic weights of oracle/synth.py
(randomised BN statistics; the keys of the module only) and images, and stores OUTPUT samples only: every 13th value of
both stage outputs plus four whole-tensor sums per output, and the module's ``state_dict()`` key list per arch (names
only).  While generating, tests/_simplenet_ref.py is asserted bit-identical to the reference module.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402  (puts the repo root on sys.path, loads oracle.*)
import _simplenet_ref as snr  # noqa: E402

CASES = [('search-XS', [(64, 64)]), ('search-S', [(64, 64)]), ('search-M', [(96, 160)])]
STRIDE = 13


def stats(t):
    a = t.numpy().astype(np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), a.flat[::97].sum()])


def main():
    torch.set_num_threads(1)
    gg.load_reference()                                   # the reference's lib/ on sys.path, as gen_golden.py
    ps = gg._load('ref_pose_simplenet', os.path.join(gg.REF, 'lib/models/pose_simplenet.py'))
    from litepose_amd import arch_zoo
    out = {}
    for arch_name, sizes in CASES:
        arch = json.load(open(os.path.join(gg.REF, 'mobile_configs', arch_name + '.json')))
        assert arch_zoo.get(arch_name) == arch, 'arch_zoo table differs from the reference JSON: ' + arch_name
        cfg = gg.make_cfg(input_size=64)
        cfg.MODEL.NAME = 'pose_simplenet'
        model = ps.get_pose_net(cfg, is_train=False, cfg_arch=arch).eval()
        keys = list(model.state_dict().keys())
        assert keys == list(snr.state_dict_shapes(arch).keys()), 'state_dict key scheme/order mismatch'
        assert all(tuple(model.state_dict()[k].shape) == v for k, v in snr.state_dict_shapes(arch).items())
        out[arch_name + '_keys'] = np.array(keys)
        sd = snr.make_state_dict(arch, seed=1234)
        model.load_state_dict(sd, strict=True)
        for H, W in sizes:
            x = gg.synth.make_images(1, H, seed=11, w=W)
            taps = {}
            with torch.no_grad():
                ref_out = model(x)
                ora_out = snr.forward(x, sd, arch, taps=taps)
            assert len(ref_out) == 2
            for k, (a, b) in enumerate(zip(ref_out, ora_out)):
                assert torch.equal(a, b), '_simplenet_ref is not bit-identical to the reference module'
                key = '%s_%dx%d_out%d' % (arch_name, H, W, k)
                out[key + '_sample'] = a.numpy().reshape(-1)[::STRIDE].copy()
                out[key + '_stats'] = stats(a)
                out[key + '_shape'] = np.array(a.shape)
            print(arch_name, (H, W), [tuple(o.shape) for o in ref_out], 'absmax %.4f %.4f'
                  % (float(ref_out[0].abs().max()), float(ref_out[1].abs().max())))
    path = os.path.join(HERE, 'golden_simplenet.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
