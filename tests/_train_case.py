"""Inputs of the training-target and training-loss tests, built from tests/golden/golden_targets.npz: the host tables of
lp_target_maps / lp_target_masks for the fixture's batch, the identity rows, and thin wrappers of the three calls on
torch device tensors.  A plain module (tests/ is on sys.path under pytest)."""
import ctypes as C
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_targets.npz')
IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]])


def load():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    g['N'] = len(g['people'])
    g['first'] = np.concatenate([[0], np.cumsum(g['people'])]).astype(np.int32)
    return g


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(rows):
    """A host descriptor table (structured array) -> uint8 [N, itemsize] device tensor."""
    return dev(np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), -1))


def target_desc(mats, flips, reserved=None):
    from litepose_amd.dataset.targets import TARGET_DESC_DTYPE
    t = np.zeros(len(mats), TARGET_DESC_DTYPE)
    for r, (m, f) in enumerate(zip(mats, flips)):
        t[r]['mat'], t[r]['flip'] = np.asarray(m, np.float64).reshape(-1), int(f)
        if reserved is not None:
            t[r]['reserved'] = reserved[r]
    return t


def batch_desc(g, R, scale=1.0):
    """The fixture's N rows at output size R (``scale``: the recorded matrices times a factor, for a larger plane)."""
    s = g['outs'].tolist().index(R)
    return target_desc([g['mat_output'][n, s] * scale for n in range(g['N'])], g['flip'])


def mask_inputs(g, R):
    """(packed masks uint8, lp_aug_desc rows) of the fixture's batch: row 0 all-ones by src_offset -1, row 1 its mask with
    the zero block, row 2 an explicit all-ones mask, row 3 all-ones by -1.  7 bytes of 1 before each packed mask."""
    from litepose_amd.dataset.calibration import AUG_DESC_DTYPE
    from oracle.preprocess_ref import invert_affine
    s = g['outs'].tolist().index(R)
    buf, offs = np.zeros(0, np.uint8), {}
    for n in (1, 2):
        buf = np.concatenate([buf, np.ones(7, np.uint8)])
        offs[n] = buf.size
        buf = np.concatenate([buf, g['mask%d' % n].reshape(-1)])
    t = np.zeros(g['N'], AUG_DESC_DTYPE)
    for n, (h, w) in enumerate(g['sizes'].tolist()):
        t[n]['src_offset'], t[n]['H'], t[n]['W'] = offs.get(n, -1), h, w
        t[n]['minv'] = invert_affine(g['mat_output'][n, s]).reshape(-1)
        t[n]['flip'] = int(g['flip'][n])
    return buf, t


def call_maps(joints, first, desc, R, g, gauss, sigma, heat, jout, tag_per_joint=1, M=None):
    from litepose_amd import _native as nv
    J = int(g['J'])
    fi = (C.c_int32 * J)(*g['flip_index'].tolist())
    nv.check(nv.lib().lp_target_maps(nv.dptr(joints), joints.shape[0], nv.dptr(first), nv.dptr(desc), first.numel() - 1, J,
                                     R, fi, nv.dptr(gauss), 6 * sigma + 3, float(3 * sigma), int(g['M']) if M is None else M,
                                     tag_per_joint, nv.dptr(heat), nv.dptr(jout), nv.stream_ptr()), 'lp_target_maps')


def call_masks(src, desc, R, out):
    from litepose_amd import _native as nv
    nv.check(nv.lib().lp_target_masks(nv.dptr(src), 0 if src is None else src.numel(), nv.dptr(desc), desc.shape[0], R,
                                      nv.dptr(out), nv.stream_ptr()), 'lp_target_masks')


def call_loss(out, J, off, heat, mask, joints, loss_type, factors, hl, push, pull, ws, ws_bytes=None):
    from litepose_amd import _native as nv
    N, Cc, R = out.shape[0], out.shape[1], out.shape[2]
    M = 1 if joints is None else joints.shape[1]
    nv.check(nv.lib().lp_pose_loss(nv.dptr(out), N, Cc, R, J, off, nv.dptr(heat), nv.dptr(mask), nv.dptr(joints), M,
                                   loss_type, factors[0], factors[1], factors[2], nv.dptr(hl), nv.dptr(push), nv.dptr(pull),
                                   nv.dptr(ws), (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes,
                                   nv.stream_ptr()), 'lp_pose_loss')


def loss_ws(N, J, R):
    from litepose_amd import _native as nv
    return int(nv.lib().lp_pose_loss_workspace_bytes(N, J, R))
