#!/usr/bin/env python
"""Network outputs of the REAL reference modules for the custom architectures of tests/_custom_space.py (the rows of the
custom census): lib/models/pose_mobilenet.py, and lib/models/pose_simplenet.py for the plain-head rows.

Run in the build container only (needs the reference checkout, like gen_golden.py):

    python tests/golden/gen_golden_custom.py

Imports the reference modules by path exactly like gen_golden_archs.py / gen_golden_simplenet.py (nothing is copied),
builds every row's architecture with them, asserts the key order of ``state_dict()`` equal to oracle/spec.py's scheme,
loads the seeded synthetic weights of oracle/synth.py and runs ONE image at the row's size.  Stored per row, under the
row id (rows that share a net and a size: under the first one's, ``golden_id``): every 13th value of both stage outputs,
four whole-tensor sums per output and the shapes -- data only.  While generating, oracle/net_ref.py (tests/_simplenet_ref.py for a plain head) is asserted bit-identical to the module.  A row
whose architecture the plan refuses in fp32 (three stages) has no golden: the reference module cannot run it either,
which is asserted here.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402  (puts the repo root on sys.path, loads oracle.*)
import _custom_space as cs  # noqa: E402
import _simplenet_ref as snr  # noqa: E402
from oracle import net_ref, spec, synth  # noqa: E402

STRIDE = 13
SEED_W, SEED_X = 1234, 11


def stats(t):
    a = t.numpy().astype(np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), a.flat[::97].sum()])


def main():
    torch.set_num_threads(1)
    _, _, pm = gg.load_reference()
    ps = gg._load('ref_pose_simplenet', os.path.join(gg.REF, 'lib/models/pose_simplenet.py'))
    out = {}
    for row in cs.ROWS:
        rid, _, H, W = row[:4]
        if cs.golden_id(row) != rid:                    # the same net at the same size as an earlier row
            continue
        arch, head, plain = cs.arch_of(row), cs.head_of(row), bool(row[6].get('_plain'))
        cfg = gg.make_cfg(J=head.num_joints, input_size=64)
        if ('f32', rid) in cs.REFUSED:
            try:
                model = pm.get_pose_net(cfg, is_train=False, cfg_arch=arch).eval()
                with torch.no_grad():
                    model(synth.make_images(1, H, seed=SEED_X, w=W))
            except Exception as e:                      # noqa: BLE001 (whatever the module raises on such a net)
                print(rid, 'the reference module cannot run this net either:', type(e).__name__, e)
                continue
            raise AssertionError('REFUSED lists %s for fp32, the reference module runs it' % rid)
        if plain:
            cfg.MODEL.NAME = 'pose_simplenet'
            model = ps.get_pose_net(cfg, is_train=False, cfg_arch=arch).eval()
            shapes = snr.state_dict_shapes(arch, head)
            sd = snr.make_state_dict(arch, head, seed=SEED_W)
        else:
            model = pm.get_pose_net(cfg, is_train=False, cfg_arch=arch).eval()
            shapes = spec.state_dict_shapes(arch, head)
            sd = synth.make_state_dict(arch, head, seed=SEED_W)
        ref_sd = model.state_dict()
        assert list(ref_sd.keys()) == list(shapes.keys()), 'state_dict key scheme/order mismatch: ' + rid
        assert all(tuple(ref_sd[k].shape) == tuple(v) for k, v in shapes.items()), rid
        model.load_state_dict(sd, strict=True)
        x = synth.make_images(1, H, seed=SEED_X, w=W)
        with torch.no_grad():
            ref_out = model(x)
            ora_out = snr.forward(x, sd, arch, head) if plain else net_ref.forward(x, sd, arch, head)
        assert len(ref_out) == 2
        for k, (a, b) in enumerate(zip(ref_out, ora_out)):
            assert torch.equal(a, b), 'the oracle is not bit-identical to the reference module: ' + rid
            key = '%s_out%d' % (rid, k)
            out[key + '_sample'] = a.numpy().reshape(-1)[::STRIDE].copy()
            out[key + '_stats'] = stats(a)
            out[key + '_shape'] = np.array(a.shape)
        print(rid, (H, W), [tuple(o.shape) for o in ref_out], 'absmax %.4f %.4f'
              % (float(ref_out[0].abs().max()), float(ref_out[1].abs().max())))
    path = os.path.join(HERE, 'golden_custom.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
