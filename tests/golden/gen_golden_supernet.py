#!/usr/bin/env python
"""BatchNorm calibration of supernet sub-networks by the REAL reference module (lib/models/pose_supermobilenet.py).

Run in the build container only (needs the reference checkout, like gen_golden.py):

    python tests/golden/gen_golden_supernet.py

Imports the reference's SuperLitePose by path (nothing is copied), loads the seeded synthetic supernet of
tests/_supernet_ref.py and, for each input size of ``_supernet_ref.CASES`` on a fresh supernet, runs the three
architectures of ``_supernet_ref.golden_archs()`` IN SEQUENCE (the reference's slices are views: one calibration moves
what the next starts from): eval outputs, three training-mode steps on N = 4 images, eval outputs again.  Stored per
size and architecture:
  * ``pairs``   [3 steps][mean, var][sampled channels of every BatchNorm in forward order] -- the reference's running
                pairs after every step (``_supernet_ref.sample_index``: every channel of a layer up to 32, else 32 evenly
                spread ones; a full-width sub-network alone has 32 000 BatchNorm channels, the file stays under 1 MiB)
  * ``sums``    [3][2][layers] float64 sum of each pair over ALL channels of the layer
  * ``dist``    [3][2][layers] max |reference - float64 restatement| over ALL channels: the reference's own distance from
                float64, the yardstick of tests/test_gpu_supernet.py
  * ``pre`` / ``post`` eval-mode outputs before / after calibration: every 13th value and four whole-tensor sums
  * for the mixed architecture, the depthwise filters the reference's own Linear5x5 / Linear3x3 give for one block each
While generating, the restatement is asserted against the reference: slicing and eval outputs bit for bit, the float32
training-mode forward to the last bit of every running pair.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402
import _supernet_ref as sr  # noqa: E402

STRIDE = 13


def stats(t):
    a = t.numpy().astype(np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), a.flat[::97].sum()])


def ref_pairs(model, arch):
    sd = model.state_dict()
    return {p: (sd[p + '.running_mean'][:c].double().numpy().copy(), sd[p + '.running_var'][:c].double().numpy().copy())
            for p, c in sr.bn_layers(arch)}


def main():
    torch.set_num_threads(1)
    gg.load_reference()
    psm = gg._load('ref_pose_supermobilenet', os.path.join(gg.REF, 'lib/models/pose_supermobilenet.py'))
    # the reference calls ConvTranspose2d._output_padding with the argument list of the torch it was written for; newer
    # torch wants the number of spatial dimensions too (a shim on the imported class, generation time only)
    sl = sys.modules['lib.models.layers.super_layers']
    base = torch.nn.ConvTranspose2d._output_padding
    sl.SuperConvTranspose2d._output_padding = \
        lambda self, x, output_size, stride, padding, kernel_size: base(self, x, output_size, stride, padding, kernel_size, 2)
    cfg = gg.make_cfg(input_size=64)
    cfg.MODEL.NAME = 'pose_supermobilenet'
    cfg.MODEL.EXTRA.NUM_DECONV_FILTERS = list(sr.FILTERS)
    out = {}
    for H, W in sr.CASES:
        model = psm.get_pose_net(cfg, is_train=False)
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == list(sr.state_dict_shapes().items()), \
            'supernet key scheme / order / shapes'
        if (H, W) == sr.CASES[0]:
            out['keys'] = np.array(list(model.state_dict().keys()))
        model.load_state_dict(sr.make_state_dict(sr.SEED), strict=True)
        sd32 = sr.make_state_dict(sr.SEED)
        sd64 = sr.to_double(sr.make_state_dict(sr.SEED))
        am = model.arch_manager
        assert am.fixed_sample(ratio=0.5) == sr.fixed_sample(ratio=0.5) and am.fixed_sample(256, 1.0) == sr.fixed_sample(ratio=1.0)
        am.is_search = True
        for ai, (name, arch) in enumerate(sr.golden_archs()):
            tag = '%dx%d_%s' % (H, W, name)
            am.search_arch = copy.deepcopy(arch)
            sub32, sub64 = sr.sub_state_dict(sd32, arch), sr.sub_state_dict(sd64, arch)
            xe = gg.synth.make_images(2, H, seed=11, w=W)

            def eval_outputs(which):
                model.eval()
                with torch.no_grad():
                    ro = model(xe)
                    oo = sr.eval_forward(xe, sub32, arch)
                for k, (a, b) in enumerate(zip(ro, oo)):
                    assert torch.equal(a, b), '%s %s: the oracle network on the slices is not the reference' % (tag, which)
                    out['%s_%s%d_sample' % (tag, which, k)] = a.numpy().reshape(-1)[::STRIDE].copy()
                    out['%s_%s%d_stats' % (tag, which, k)] = stats(a)
                    out['%s_%s%d_shape' % (tag, which, k)] = np.array(a.shape)

            eval_outputs('pre')
            if name == 'mixed':
                for s, st in enumerate(arch['backbone_setting']):
                    for b, (t, k) in enumerate(st['block_setting']):
                        key = '%dx%d_window_k%d' % (H, W, k)
                        if k == 7 or key in out:
                            continue
                        blk = model.stage[s][b]
                        mid = sub32['stage.%d.%d.depth_conv.0.weight' % (s, b)].shape[0]
                        l, r = 3 - k // 2, 3 + k // 2 + 1
                        with torch.no_grad():
                            w = blk.depth_conv[0].weight[:mid, :, l:r, l:r]
                            w = (blk.Linear5x5 if k == 5 else blk.Linear3x3)(w.reshape(mid, 1, -1)).reshape(mid, 1, k, k)
                        assert torch.equal(w, sub32['stage.%d.%d.depth_conv.0.weight' % (s, b)])
                        out[key] = w.numpy().copy()
                        out[key + '_block'] = np.array([s, b])
            model.train()
            P, S, D = [], [], []
            for step in range(sr.STEPS):
                x = sr.step_images(H, W, ai, step)
                with torch.no_grad():
                    model(x)
                    sr.train_forward(x, sub32, arch)
                    sr.train_forward(x.double(), sub64, arch)
                rp, op, hp = ref_pairs(model, arch), sr.pairs_of(sub32, arch), sr.pairs_of(sub64, arch)
                dist = [[], []]
                for p, c in sr.bn_layers(arch):
                    for q in range(2):
                        assert np.array_equal(rp[p][q], op[p][q]), '%s step %d %s: restatement != reference' % (tag, step, p)
                        dist[q].append(np.abs(rp[p][q] - hp[p][q]).max())
                v, s_ = sr.pack_pairs(rp, arch)
                P.append(v.astype(np.float32))
                S.append(s_)
                D.append(np.array(dist))
            out[tag + '_pairs'], out[tag + '_sums'], out[tag + '_dist'] = np.stack(P), np.stack(S), np.stack(D)
            nbt = model.state_dict()
            out[tag + '_nbt'] = np.array([int(nbt[p + '.num_batches_tracked']) for p, _ in sr.bn_layers(arch)])
            eval_outputs('post')
            print(tag, 'layers', len(sr.bn_layers(arch)), 'sampled', out[tag + '_pairs'].shape,
                  'max ref-fp64 dist %.3g' % out[tag + '_dist'].max())
    path = os.path.join(HERE, 'golden_supernet.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
