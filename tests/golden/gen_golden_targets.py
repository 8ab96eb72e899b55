#!/usr/bin/env python
"""Golden fixture of the training targets and the training loss (tests/golden/golden_targets.npz).  Build container only
(needs the reference checkout).  Runs the REAL reference code on the CPU:

  * lib/dataset/transforms/transforms.py (RandomAffineTransform, RandomHorizontalFlip) with a stub ``cv2`` whose
    ``warpAffine`` is oracle.preprocess_ref.warp_affine_u8 and records the matrix it is handed, and a stub ``torchvision``;
  * lib/dataset/target_generators/target_generators.py (HeatmapGenerator, JointsGenerator);
  * lib/core/loss.py (MultiLossFactory, both AE_LOSS_TYPEs), per image and per batch.

Data only: inputs, matrices, transformed joints, heatmaps, joints tensors, masks, the reference's fp64 Gaussian tables,
seeded normal stand-ins for the network outputs, the reference's fp32 losses and the fp64 values of tests/_loss_ref.py.

Shapes: N = 4 images with {0, 1, 2, 4} persons, J = 5, M = 4, output sizes [16, 32], both flip values, rotated matrices;
one extra row per size with the identity matrix and hand-placed joints on the cell boundaries.  Condition on the random
rows, asserted here (the seed moves on until it holds): every transformed coordinate of a v > 0 joint lies at least 1e-9
from an integer -- BLAS may contract the reference's matrix product, and only the identity row tests exact cells."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = '/root/reference'

import _loss_ref as LR  # noqa: E402
from oracle.preprocess_ref import warp_affine_u8  # noqa: E402

J, M, N = 5, 4, 4
FLIP_INDEX = [1, 0, 2, 4, 3]
OUTS = [16, 32]
INPUT_SIZE = 64
SIZES = [(13, 17), (24, 18), (11, 11), (20, 31)]          # h, w: smaller than the larger output, so the border shows
PEOPLE = [0, 1, 2, 4]
AUG = dict(max_rotation=30, min_scale=0.75, max_scale=1.5, scale_type='short', max_translate=40, flip_prob=0.5)
FACTORS = dict(HEATMAPS_LOSS_FACTOR=(1.0, 1.0), PUSH_LOSS_FACTOR=(0.001, 0.001), PULL_LOSS_FACTOR=(0.001, 0.001))
LOSS_CFGS = [dict(WITH_HEATMAPS_LOSS=(True, True), WITH_AE_LOSS=(True, False)),        # every shipped config
             dict(WITH_HEATMAPS_LOSS=(False, True), WITH_AE_LOSS=(True, True))]        # tags from channel 0; tags at R = 32


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(recorded):
    def warp_affine(src, mat, dsize, *a, **k):
        recorded.append((src.ndim, np.array(mat, np.float64).copy(), tuple(dsize)))
        if src.ndim == 2:
            return warp_affine_u8(src[:, :, None], mat, dsize)[:, :, 0]
        return warp_affine_u8(src, mat, dsize)

    cv2 = types.ModuleType('cv2')
    cv2.warpAffine = warp_affine
    tv = types.ModuleType('torchvision')
    tvt = types.ModuleType('torchvision.transforms')
    tvt.functional = types.ModuleType('torchvision.transforms.functional')
    tv.transforms = tvt
    names = ('cv2', 'torchvision', 'torchvision.transforms', 'torchvision.transforms.functional')
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules.update({'cv2': cv2, 'torchvision': tv, 'torchvision.transforms': tvt,
                        'torchvision.transforms.functional': tvt.functional})
    try:
        T = _load('ref_dataset_transforms', os.path.join(REF, 'lib/dataset/transforms/transforms.py'))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    G = _load('ref_target_generators', os.path.join(REF, 'lib/dataset/target_generators/target_generators.py'))
    L = _load('ref_core_loss', os.path.join(REF, 'lib/core/loss.py'))
    return T, G, L


def away_from_integers(joints_t, R):
    v = joints_t[:, :, 2] > 0
    c = joints_t[:, :, :2][v]
    return c.size == 0 or float(np.abs(c - np.rint(c)).min()) >= 1e-9


def random_rows(T, recorded, seed):
    """The N augmented rows under one seed of both global generators -> dict, or None when the condition fails."""
    rng = np.random.RandomState(1000 + seed)
    images, masks, joints = [], [], []
    for (h, w), people in zip(SIZES, PEOPLE):
        images.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        m = np.ones((h, w))
        masks.append(m)
        j = np.zeros((people, J, 3))
        j[:, :, 0] = rng.uniform(-0.15 * w, 1.15 * w, (people, J))
        j[:, :, 1] = rng.uniform(-0.15 * h, 1.15 * h, (people, J))
        j[:, :, 2] = rng.choice([0, 1, 2], (people, J), p=[0.2, 0.4, 0.4])
        joints.append(j)
    masks[1][5:14, 3:11] = 0                                   # a zero block; rows 0, 2, 3 are all-ones masks
    aff = T.RandomAffineTransform(INPUT_SIZE, OUTS, AUG['max_rotation'], AUG['min_scale'], AUG['max_scale'],
                                  AUG['scale_type'], AUG['max_translate'])
    flipper = T.RandomHorizontalFlip(FLIP_INDEX, OUTS, AUG['flip_prob'])
    tf = T.Compose([aff, flipper])
    np.random.seed(seed)
    random.seed(seed)
    rows = dict(mat_input=[], mat_output=[], flip=[], joints_t=[[] for _ in OUTS], mask_t=[[] for _ in OUTS])
    for img, m, j in zip(images, masks, joints):
        del recorded[:]
        marked = img.copy()
        out_img, m_list, j_list = tf(marked, [m.copy() for _ in OUTS], [j.copy() for _ in OUTS])
        assert [r[0] for r in recorded] == [2] * len(OUTS) + [3], recorded
        direct = warp_affine_u8(img, recorded[-1][1], (INPUT_SIZE, INPUT_SIZE))
        flip = not np.array_equal(out_img, direct)
        assert np.array_equal(out_img, direct[:, ::-1] if flip else direct)
        rows['mat_input'].append(recorded[-1][1])
        rows['mat_output'].append([recorded[s][1] for s in range(len(OUTS))])
        rows['flip'].append(flip)
        for s, R in enumerate(OUTS):
            if not away_from_integers(j_list[s], R):
                return None
            rows['joints_t'][s].append(j_list[s])
            rows['mask_t'][s].append(m_list[s].astype(np.float32))
    if set(rows['flip']) != {True, False}:
        return None
    rows.update(images=images, masks=masks, joints=joints)
    return rows


def identity_joints(R):
    """Hand-placed joints of the identity row (4 persons): the exact cell rules and the max merge."""
    j = np.zeros((4, J, 3))
    j[0] = [(-0.5, -0.9, 1), (-1.0, 3, 1), (R - 0.5, 0, 1), (R, 0, 1), (5, 5, 0)]   # in (0,0), out, in, out, skipped
    j[1] = [(0.3, 0.2, 2), (7, 7, 1), (0, 0, 0), (0, 0, 0), (R - 1, R - 1, 1)]      # shares cell (0,0) of joint 0
    j[2] = [(0, 0, 0), (9.5, 8.25, 1), (3, R - 1, 1), (0, 0, 0), (0, 0, 0)]         # window overlaps person 1's joint 1
    j[3] = [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]                  # a person without a visible joint
    return j


def generate(G, joints_t, R, sigma, tag_per_joint):
    hg = G.HeatmapGenerator(R, J, sigma)
    jg = G.JointsGenerator(M, J, R, tag_per_joint)
    heat = np.stack([hg(j).astype(np.float32) for j in joints_t])
    jt = np.stack([jg(j).astype(np.int32) for j in joints_t])
    return heat, jt, hg.g


def losses(L, outs, heats, masks, jts):
    """The real MultiLossFactory per batch and per image (a batch of one: its mean is the image's term), and _loss_ref."""
    NS = types.SimpleNamespace
    res = {}
    for c, lc in enumerate(LOSS_CFGS):
        for lt in ('exp', 'max'):
            cfg = NS(MODEL=NS(NUM_JOINTS=J), DATASET=NS(MAX_NUM_PEOPLE=M, OUTPUT_SIZE=OUTS),
                     LOSS=NS(NUM_STAGES=2, AE_LOSS_TYPE=lt, **dict(FACTORS, **lc)))
            fac = L.MultiLossFactory(cfg)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
            ref = np.full((2, 3, N), np.nan, np.float32)               # stage, (heat, push, pull), image
            f64 = np.full((2, 3, N), np.nan, np.float64)
            batch = np.full((2, 2), np.nan, np.float32)                # stage, (push, pull): the batch means
            o = [outs[c][0], outs[c][1]]
            hl, pu, pl = fac([t(x) for x in o], [t(x) for x in heats], [t(x) for x in masks],
                             [t(x).long() for x in jts])
            for s in range(2):
                if pu[s] is not None:
                    batch[s] = (float(pu[s]), float(pl[s]))
            for n in range(N):
                hl1, pu1, pl1 = fac([t(x[n:n + 1]) for x in o], [t(x[n:n + 1]) for x in heats],
                                    [t(x[n:n + 1]) for x in masks], [t(x[n:n + 1]).long() for x in jts])
                for s in range(2):
                    if hl1[s] is not None:
                        ref[s, 0, n] = hl1[s].numpy()[0]
                        assert hl1[s].numpy()[0] == hl[s].numpy()[n]
                        f64[s, 0, n] = LR.heat_loss(o[s][n, :J], heats[s][n], masks[s][n], FACTORS['HEATMAPS_LOSS_FACTOR'][s])
                    if pu1[s] is not None:
                        ref[s, 1, n], ref[s, 2, n] = float(pu1[s]), float(pl1[s])
                        off = J if lc['WITH_HEATMAPS_LOSS'][s] else 0
                        f64[s, 1, n], f64[s, 2, n] = LR.tag_loss(o[s][n, off:], jts[s][n], lt, FACTORS['PUSH_LOSS_FACTOR'][s],
                                                                 FACTORS['PULL_LOSS_FACTOR'][s])
            res['loss%d_%s_ref' % (c, lt)] = ref
            res['loss%d_%s_f64' % (c, lt)] = f64
            res['loss%d_%s_batch' % (c, lt)] = batch
    return res


def main():
    recorded = []
    T, G, L = load_reference(recorded)
    seed = 0
    rows = random_rows(T, recorded, seed)
    while rows is None:
        seed += 1
        rows = random_rows(T, recorded, seed)
    out = dict(seed=seed, J=J, M=M, flip_index=np.array(FLIP_INDEX), outs=np.array(OUTS), input_size=INPUT_SIZE,
               sizes=np.array(SIZES), people=np.array(PEOPLE), flip=np.array(rows['flip']),
               mat_input=np.stack(rows['mat_input']), mat_output=np.array(rows['mat_output']),     # [N,2,2,3]
               joints=np.concatenate(rows['joints']),
               **{'aug_' + k: np.array(v) for k, v in AUG.items()})
    for n in range(N):
        out['image%d' % n] = rows['images'][n]
        out['mask%d' % n] = rows['masks'][n].astype(np.uint8)
    heats, masks, jts = [], [], []
    for s, R in enumerate(OUTS):
        heat, jt, g = generate(G, rows['joints_t'][s], R, 2, True)
        heats.append(heat)
        jts.append(jt)
        masks.append(np.stack(rows['mask_t'][s]))
        out['joints_t_%d' % R] = np.concatenate(rows['joints_t'][s])
        out['heat_%d' % R], out['jt_%d' % R], out['mask_t_%d' % R] = heat, jt, masks[-1]
    out['gauss_s2'] = g
    heat, jt, g1 = generate(G, rows['joints_t'][0], OUTS[0], 1, False)            # sigma = 1 and tag_per_joint = 0, once
    out['heat_16_s1'], out['jt_16_nt'], out['gauss_s1'] = heat, jt, g1
    # the identity row: the real _affine_joints with the identity matrix, both flip values through the real flip
    aff = T.RandomAffineTransform(INPUT_SIZE, OUTS, 0, 1, 1, 'short', 0)
    for R in OUTS:
        src = identity_joints(R)
        for flip in (0, 1):
            jl = [src.copy()]
            jl[0][:, :, 0:2] = aff._affine_joints(jl[0][:, :, 0:2], np.array([[1.0, 0, 0], [0, 1.0, 0]]))
            assert np.array_equal(jl[0], src)
            if flip:
                fl = T.RandomHorizontalFlip(FLIP_INDEX, [R], 2.0)                  # prob > 1: always
                _, _, jl = fl(np.zeros((2, 2, 3), np.uint8), [np.zeros((R, R))], jl)
            heat, jt, _ = generate(G, [jl[0]], R, 2, True)
            out['ident_joints_%d' % R] = src
            out['ident_heat_%d_f%d' % (R, flip)], out['ident_jt_%d_f%d' % (R, flip)] = heat[0], jt[0]
    assert out['ident_jt_16_f0'][0, 0].tolist() == [0, 1] and out['ident_jt_16_f0'][0, 1].tolist() == [2 * 256 + 15, 1]
    assert out['ident_jt_16_f0'][0, 2].tolist() == [0, 0]
    # network-output stand-ins: seeded normals; cfg 0: [N,2J,16,16] + [N,J,32,32]; cfg 1: [N,2J,...] on both stages
    rng = np.random.RandomState(7)
    outs = [[rng.standard_normal((N, 2 * J, 16, 16)).astype(np.float32), rng.standard_normal((N, J, 32, 32)).astype(np.float32)],
            [None, rng.standard_normal((N, 2 * J, 32, 32)).astype(np.float32)]]
    outs[1][0] = outs[0][0]
    out['out_16'], out['out_32'], out['out_32_tags'] = outs[0][0], outs[0][1], outs[1][1]
    out.update(losses(L, outs, heats, masks, jts))
    path = os.path.join(HERE, 'golden_targets.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes), seed %d, flips %s' % (path, os.path.getsize(path), seed, rows['flip']))


if __name__ == '__main__':
    main()
