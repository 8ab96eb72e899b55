"""The ``calibrate`` split of the architecture search on the device: the image side of the reference's train loader
(lib/dataset/transforms/transforms.py:54-182, build.py:31-85; make_train_dataloader, lib/dataset/build.py:92-104).

``draw_transform`` restates the random draws of ``RandomAffineTransform.__call__`` and ``RandomHorizontalFlip.__call__``
for one image -- the same numpy / stdlib calls with the same arguments in the same order -- and returns the forward 2x3
``mat_input`` and the flip decision.  ``CalibrationSet`` keeps the decoded images in ONE device buffer and turns a batch
of them into the network input with one descriptor upload and one ``lp_augment_batch_v`` launch: cv2.warpAffine's
fixed-point bilinear warp, the mirror of the warped uint8 image, ToTensor + Normalize.

What the search's calibration does not read -- masks, joints, heatmap targets -- is not produced here: ``draw_sample`` and
``dataset.targets.LabelledSet`` are the labelled loader.  The reference's loader
may run worker processes, each with its own copy of the generators; the draws here follow the single-process order (image
after image: the affine draws from numpy, then the flip draw from ``random``).
"""
import ctypes as C
import random

import numpy as np
import torch

from .. import _native as nv
from ..utils import transforms as _tf

# one row of the descriptor table of lp_augment_batch_v (lp_aug_desc, 72 bytes)
AUG_DESC_DTYPE = np.dtype([('src_offset', '<i8'), ('H', '<i4'), ('W', '<i4'), ('minv', '<f8', (6,)), ('flip', '<i4'),
                           ('reserved', '<i4')])
assert AUG_DESC_DTYPE.itemsize == 72

# DATASET.* of lib/config/default.py:78-85 overlaid with experiments/crowd_pose/mobilenet/supermobile.yaml
AUG_DEFAULTS = dict(max_rotation=30, min_scale=0.75, max_scale=1.5, scale_type='short', max_translate=40, flip_prob=0.5)


def _affine_matrix(center, scale, res, rot=0):
    """RandomAffineTransform._get_affine_matrix (transforms.py:98-122): 3x3, float64."""
    h = 200 * scale
    t = np.zeros((3, 3))
    t[0, 0] = float(res[1]) / h
    t[1, 1] = float(res[0]) / h
    t[0, 2] = res[1] * (-float(center[0]) / h + .5)
    t[1, 2] = res[0] * (-float(center[1]) / h + .5)
    t[2, 2] = 1
    if not rot == 0:
        rot = -rot
        rot_mat = np.zeros((3, 3))
        rot_rad = rot * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
        rot_mat[2, 2] = 1
        t_mat = np.eye(3)
        t_mat[0, 2] = -res[1] / 2
        t_mat[1, 2] = -res[0] / 2
        t_inv = t_mat.copy()
        t_inv[:2, 2] *= -1
        t = np.dot(t_inv, np.dot(rot_mat, np.dot(t_mat, t)))
    return t


def draw_transform(h, w, input_size, np_rng=None, py_rng=None, max_rotation=AUG_DEFAULTS['max_rotation'],
                   min_scale=AUG_DEFAULTS['min_scale'], max_scale=AUG_DEFAULTS['max_scale'],
                   scale_type=AUG_DEFAULTS['scale_type'], max_translate=AUG_DEFAULTS['max_translate'],
                   flip_prob=AUG_DEFAULTS['flip_prob']):
    """The augmentation of one ``h`` x ``w`` image -> (``mat_input`` [2,3] float64 src -> dst, flip).
    ``np_rng``: a ``numpy.random.RandomState`` (default: numpy's global one); ``py_rng``: a ``random.Random`` (default:
    the ``random`` module).  Seeded like the reference's global generators, they replay its draws: scale, rotation, dx
    and dy (only with ``max_translate`` > 0) from numpy, then the flip from ``random``."""
    np_rng = np.random if np_rng is None else np_rng
    py_rng = random if py_rng is None else py_rng
    height, width = h, w
    center = np.array((width / 2, height / 2))
    if scale_type == 'long':
        scale = max(height, width) / 200
    elif scale_type == 'short':
        scale = min(height, width) / 200
    else:
        raise ValueError('Unknown scale type: {}'.format(scale_type))
    aug_scale = np_rng.random() * (max_scale - min_scale) + min_scale
    scale *= aug_scale
    aug_rot = (np_rng.random() * 2 - 1) * max_rotation
    if max_translate > 0:
        dx = np_rng.randint(-max_translate * scale, max_translate * scale)
        dy = np_rng.randint(-max_translate * scale, max_translate * scale)
        center[0] += dx
        center[1] += dy
    mat_input = _affine_matrix(center, scale, (input_size, input_size), aug_rot)[:2]
    flip = bool(py_rng.random() < flip_prob)
    return mat_input, flip


def draw_sample(h, w, input_size, output_sizes, np_rng=None, py_rng=None, max_rotation=AUG_DEFAULTS['max_rotation'],
                min_scale=AUG_DEFAULTS['min_scale'], max_scale=AUG_DEFAULTS['max_scale'],
                scale_type=AUG_DEFAULTS['scale_type'], max_translate=AUG_DEFAULTS['max_translate'],
                flip_prob=AUG_DEFAULTS['flip_prob']):
    """``draw_transform`` for a labelled sample: the same draws in the same order (so the same ``mat_input`` and flip for
    equal generators) -> (``mat_input``, [``mat_output`` per entry of ``output_sizes``], flip): the forward matrices of
    RandomAffineTransform.__call__ for the image and for the masks and joints of every output resolution."""
    np_rng = np.random if np_rng is None else np_rng
    py_rng = random if py_rng is None else py_rng
    height, width = h, w
    center = np.array((width / 2, height / 2))
    if scale_type == 'long':
        scale = max(height, width) / 200
    elif scale_type == 'short':
        scale = min(height, width) / 200
    else:
        raise ValueError('Unknown scale type: {}'.format(scale_type))
    aug_scale = np_rng.random() * (max_scale - min_scale) + min_scale
    scale *= aug_scale
    aug_rot = (np_rng.random() * 2 - 1) * max_rotation
    if max_translate > 0:
        dx = np_rng.randint(-max_translate * scale, max_translate * scale)
        dy = np_rng.randint(-max_translate * scale, max_translate * scale)
        center[0] += dx
        center[1] += dy
    mat_outputs = [_affine_matrix(center, scale, (o, o), aug_rot)[:2] for o in output_sizes]
    mat_input = _affine_matrix(center, scale, (input_size, input_size), aug_rot)[:2]
    flip = bool(py_rng.random() < flip_prob)
    return mat_input, mat_outputs, flip


class CalibrationSet(object):
    """HxWx3 uint8 images of any sizes, packed once into one device buffer.

        cal = CalibrationSet(images)
        for x in cal.batches(256, 16, np.random.RandomState(0), random.Random(0)):
            ...                               # float32 [B,3,256,256] on the device

    Every batch is one descriptor upload and one ``lp_augment_batch_v`` launch on the current stream.  The last batch
    is short when the set is no multiple of ``batch_size``: make_train_dataloader builds its DataLoader without
    ``drop_last``, so the reference drops nothing either."""

    def __init__(self, images, device=None, mean=_tf.IMAGENET_MEAN, std=_tf.IMAGENET_STD):
        images = [np.ascontiguousarray(im) for im in images]
        if not images:
            raise ValueError('CalibrationSet needs at least one image')
        for k, im in enumerate(images):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or not (1 <= im.shape[0] <= 32767) or \
                    not (1 <= im.shape[1] <= 32767):
                raise ValueError('image %d: HxWx3 uint8 expected (sides 1..32767)' % k)
        self.device = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
        self.shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        sizes = [im.size for im in images]
        self.offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        self.src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(self.device)
        self.mean, self.std = tuple(mean), tuple(std)

    def __len__(self):
        return len(self.shapes)

    def describe(self, rows, input_size, np_rng=None, py_rng=None, **aug):
        """The lp_aug_desc table (host, AUG_DESC_DTYPE) of the images ``rows``: one ``draw_transform`` each, in order."""
        desc = np.zeros(len(rows), AUG_DESC_DTYPE)
        for r, k in enumerate(rows):
            h, w = self.shapes[k]
            mat, flip = draw_transform(h, w, input_size, np_rng, py_rng, **aug)
            desc[r]['src_offset'], desc[r]['H'], desc[r]['W'] = self.offsets[k], h, w
            desc[r]['minv'] = _tf.warp_invert(mat)
            desc[r]['flip'] = int(flip)
        return desc

    def augment(self, desc, input_size, out=None, out_u8=None):
        """One upload of the host table ``desc`` and one ``lp_augment_batch_v`` launch -> float32 [B,3,S,S] (and, if
        given, ``out_u8`` uint8 [B,S,S,3])."""
        S, B = int(input_size), len(desc)
        if out is None:
            out = torch.empty((B, 3, S, S), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (B, 3, S, S) or out.dtype != torch.float32:
            raise ValueError('out must be float32 [B,3,S,S]')
        if out_u8 is not None and (tuple(out_u8.shape) != (B, S, S, 3) or out_u8.dtype != torch.uint8):
            raise ValueError('out_u8 must be uint8 [B,S,S,3]')
        d_desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(self.device)
        mean_c, std_c = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        nv.check(nv.lib().lp_augment_batch_v(nv.dptr(self.src), self.src.numel(), nv.dptr(d_desc), B, S, S, mean_c, std_c,
                                             nv.dptr(out_u8), nv.dptr(out), nv.stream_ptr()), 'lp_augment_batch_v')
        return out

    def batches(self, input_size, batch_size, np_rng=None, py_rng=None, **aug):
        """The set in order (the reference's calibration loader does not shuffle), ``batch_size`` images at a time ->
        float32 [B,3,input_size,input_size] device tensors, each its own tensor.  ``aug``: the keyword parameters of
        ``draw_transform``."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError('batch_size must be positive')
        for lo in range(0, len(self), batch_size):
            rows = range(lo, min(lo + batch_size, len(self)))
            yield self.augment(self.describe(rows, input_size, np_rng, py_rng, **aug), input_size)
