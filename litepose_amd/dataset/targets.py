"""The label side of the reference's train loader on the device (lib/dataset/transforms/transforms.py:54-182,
lib/dataset/target_generators/target_generators.py, lib/dataset/COCOKeypoints.py:63-93).

``LabelledSet`` is a ``CalibrationSet`` that keeps the joints (and, where an image has one, its loss mask) of every image
on the device beside the pixels.  A batch is one ``draw_sample`` per image on the host, one descriptor upload per table,
and then ``lp_augment_batch_v`` for the images plus ``lp_target_maps`` and ``lp_target_masks`` once per output
resolution: the tuple the reference's loader yields -- ``(images, [heatmaps], [masks], [joints])`` -- never leaves the
device.  DATASET.SCALE_AWARE_SIGMA and the decoding of COCO segmentations into masks are not covered: the caller hands
over the ``m < 0.5`` mask of COCOKeypoints.get_mask."""
import ctypes as C

import numpy as np
import torch

from .. import _native as nv
from ..utils import transforms as _tf
from .calibration import AUG_DESC_DTYPE, CalibrationSet, draw_sample

# one row of the descriptor table of lp_target_maps (lp_target_desc, 56 bytes)
TARGET_DESC_DTYPE = np.dtype([('mat', '<f8', (6,)), ('flip', '<i4'), ('reserved', '<i4')])
assert TARGET_DESC_DTYPE.itemsize == 56


def gaussian_table(sigma):
    """The table of HeatmapGenerator.__init__ (target_generators.py:22-26) -> float32 [6 sigma + 3, 6 sigma + 3]:
    exp(-(dx^2 + dy^2) / (2 sigma^2)) around the centre entry 3 sigma + 1, evaluated in fp64 with the reference's
    operation order and rounded to fp32 -- what the reference's float32 heatmaps hold of its fp64 table."""
    d = np.arange(6 * sigma + 3, dtype=np.float64) - (3 * sigma + 1)
    return np.exp(-(d[None, :] ** 2 + d[:, None] ** 2) / (2 * sigma ** 2)).astype(np.float32)


def get_joints(anno, num_joints, with_center=False):
    """What COCOKeypoints.get_joints (COCOKeypoints.py:95-122) returns without the sigma column: the annotation dicts of
    one image (those with ``iscrowd == 0 or num_keypoints > 0``, :68-71) -> float64 [people, num_joints, 3] (x, y, v).
    ``with_center``: the last joint is the mean position of the others over the number with v != 0, v = 1 (none: zeros)."""
    labelled = num_joints - 1 if with_center else num_joints
    joints = np.zeros((len(anno), num_joints, 3))
    for person, obj in zip(joints, anno):
        kp = np.asarray(obj['keypoints'], np.float64).reshape(-1, 3)
        person[:labelled] = kp
        seen = np.count_nonzero(kp[:, 2])
        if with_center and seen > 0:
            person[-1, :2] = kp[:, :2].sum(axis=0) / seen
            person[-1, 2] = 1
    return joints


def _upload(table, device):
    return torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).reshape(-1)).to(device)


def target_maps(joints, first, desc, R, flip_index, gauss, sigma, max_num_people, tag_per_joint=True, heat=True,
                joints_out=True):
    """One ``lp_target_maps`` launch.  ``joints`` float64 [P,J,3], ``first`` int32 [N+1], ``desc`` uint8 [N*56] (all on
    the device), ``gauss`` the device copy of ``gaussian_table(sigma)`` -> (heat float32 [N,J,R,R], joints int32
    [N,M,J,2]); ``heat`` / ``joints_out``: True to allocate, a tensor to fill, False to leave out (None is returned)."""
    N, J, M, R = first.numel() - 1, int(joints.shape[1]), int(max_num_people), int(R)
    dev = first.device
    if heat is True:
        heat = torch.empty((N, J, R, R), dtype=torch.float32, device=dev)
    if joints_out is True:
        joints_out = torch.empty((N, M, J, 2), dtype=torch.int32, device=dev)
    heat = None if heat is False else heat
    joints_out = None if joints_out is False else joints_out
    fi = (C.c_int32 * J)(*[int(v) for v in flip_index[:J]])
    nv.check(nv.lib().lp_target_maps(nv.dptr(joints), int(joints.shape[0]), nv.dptr(first), nv.dptr(desc), N, J, R, fi,
                                     nv.dptr(gauss), int(gauss.shape[0]), float(3 * sigma), M, int(bool(tag_per_joint)),
                                     nv.dptr(heat), nv.dptr(joints_out), nv.stream_ptr()), 'lp_target_maps')
    return heat, joints_out


def target_masks(src, desc, N, R, out=None):
    """One ``lp_target_masks`` launch.  ``src``: the packed uint8 masks on the device or None, ``desc``: uint8 [N*72]
    device table of lp_aug_desc rows (``src_offset`` -1: all-ones) -> float32 [N,R,R]."""
    if out is None:
        out = torch.empty((N, int(R), int(R)), dtype=torch.float32, device=desc.device)
    nv.check(nv.lib().lp_target_masks(nv.dptr(src), 0 if src is None else src.numel(), nv.dptr(desc), N, int(R),
                                      nv.dptr(out), nv.stream_ptr()), 'lp_target_masks')
    return out


class LabelledSet(CalibrationSet):
    """Images with their labels, resident on the device.

        ls = LabelledSet(images, joints, flip_index, max_num_people=30, sigma=2)
        for images, heatmaps, masks, joints in ls.batches(256, [64, 128], 16, np.random.RandomState(0), random.Random(0)):
            ...                     # [B,3,256,256] f32; per output size [B,J,R,R] f32, [B,R,R] f32, [B,M,J,2] i32

    ``joints``: per image a float64 [people, J, 3] array in image coordinates (``get_joints``).  ``masks``: None, or per
    image None (nothing to ignore: all ones) or an [H,W] array, non-zero where the loss counts (COCOKeypoints.get_mask).
    An image with more than ``max_num_people`` persons raises, as the reference's JointsGenerator would (IndexError).
    With the same generators the images are bit-identical to ``CalibrationSet.batches``: ``draw_sample`` makes
    ``draw_transform``'s draws."""

    def __init__(self, images, joints, flip_index, max_num_people=30, sigma=2, tag_per_joint=True, masks=None,
                 device=None, mean=_tf.IMAGENET_MEAN, std=_tf.IMAGENET_STD):
        CalibrationSet.__init__(self, images, device, mean, std)
        if len(joints) != len(self):
            raise ValueError('one joints array per image expected')
        joints = [np.asarray(j, np.float64).reshape(-1, np.shape(j)[-2], 3) if np.size(j) else None for j in joints]
        J = len(flip_index)
        for k, j in enumerate(joints):
            if j is not None and j.shape[1] != J:
                raise ValueError('image %d: joints must be [people, %d, 3]' % (k, J))
            if j is not None and j.shape[0] > max_num_people:
                raise IndexError('image %d: %d persons exceed MAX_NUM_PEOPLE = %d' % (k, j.shape[0], max_num_people))
        self.num_joints, self.max_num_people, self.sigma = J, int(max_num_people), sigma
        self.tag_per_joint, self.flip_index = bool(tag_per_joint), [int(v) for v in flip_index]
        self.people = [0 if j is None else int(j.shape[0]) for j in joints]
        self.person_first = [int(v) for v in np.concatenate([[0], np.cumsum(self.people)])]
        # one unused row after the last person: the slice of a batch without persons is never an empty tensor
        host = np.concatenate([j for j in joints if j is not None] + [np.zeros((1, J, 3))])
        self.joints = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)
        self.gauss = torch.from_numpy(gaussian_table(sigma)).to(self.device)
        self.mask_offsets, self.mask_src = [-1] * len(self), None
        if masks is not None:
            if len(masks) != len(self):
                raise ValueError('one mask (or None) per image expected')
            parts, off = [], 0
            for k, m in enumerate(masks):
                if m is None:
                    continue
                m = (np.asarray(m) != 0).astype(np.uint8)
                if m.shape != self.shapes[k]:
                    raise ValueError('image %d: mask must be [H,W] of the image' % k)
                self.mask_offsets[k] = off
                parts.append(m.reshape(-1))
                off += m.size
            if parts:
                self.mask_src = torch.from_numpy(np.concatenate(parts)).to(self.device)

    def describe_labelled(self, rows, input_size, output_sizes, np_rng=None, py_rng=None, **aug):
        """The host tables of the images ``rows``, one ``draw_sample`` each, in order -> (lp_aug_desc table of the images,
        per output size (lp_target_desc table, lp_aug_desc table of the masks), person offsets int32 [B+1])."""
        B = len(rows)
        img = np.zeros(B, AUG_DESC_DTYPE)
        tgt = [np.zeros(B, TARGET_DESC_DTYPE) for _ in output_sizes]
        msk = [np.zeros(B, AUG_DESC_DTYPE) for _ in output_sizes]
        first = np.zeros(B + 1, np.int32)
        for r, k in enumerate(rows):
            h, w = self.shapes[k]
            mat, mats, flip = draw_sample(h, w, input_size, output_sizes, np_rng, py_rng, **aug)
            img[r]['src_offset'], img[r]['H'], img[r]['W'] = self.offsets[k], h, w
            img[r]['minv'] = _tf.warp_invert(mat)
            img[r]['flip'] = int(flip)
            for s, m in enumerate(mats):
                tgt[s][r]['mat'] = np.asarray(m, np.float64).reshape(-1)
                tgt[s][r]['flip'] = int(flip)
                msk[s][r]['src_offset'], msk[s][r]['H'], msk[s][r]['W'] = self.mask_offsets[k], h, w
                msk[s][r]['minv'] = _tf.warp_invert(m)
                msk[s][r]['flip'] = int(flip)
            first[r + 1] = first[r] + self.people[k]
        return img, list(zip(tgt, msk)), first

    def targets(self, rows, tables, first, output_sizes):
        """The label launches of one batch of consecutive images ``rows`` (the set in order, as ``batches`` walks it):
        per output size one upload per table, ``lp_target_maps`` and ``lp_target_masks`` -> ([heatmaps], [masks],
        [joints])."""
        B = len(rows)
        if any(rows[i] + 1 != rows[i + 1] for i in range(B - 1)):
            raise ValueError('rows must be consecutive images of the set: their persons are one slice of the table')
        lo = self.person_first[rows[0]]
        joints = self.joints[lo:lo + max(int(first[-1]), 1)]          # a batch without persons: the next (or the unused) row
        d_first = torch.from_numpy(first).to(self.device)
        heats, masks, jts = [], [], []
        for R, (tgt, msk) in zip(output_sizes, tables):
            h, j = target_maps(joints, d_first, _upload(tgt, self.device), R, self.flip_index, self.gauss, self.sigma,
                               self.max_num_people, self.tag_per_joint)
            heats.append(h)
            jts.append(j)
            masks.append(target_masks(self.mask_src, _upload(msk, self.device), B, R))
        return heats, masks, jts

    def batches(self, input_size, output_sizes, batch_size, np_rng=None, py_rng=None, shard=None, **aug):
        """The set in order, ``batch_size`` images at a time -> ``(images, [heatmaps], [masks], [joints])`` on the device,
        the lists indexed by output size.  ``aug``: the keyword parameters of ``draw_sample``.

        ``shard=(rank, world)``: this rank's contiguous part of every batch (``parallel.shard_range``), for data-parallel
        training: every rank walks the same batches, so the ranks meet in every collective of every step.  A batch with
        fewer images than ranks raises ValueError (a rank without a part would miss the step's collectives).  The random
        streams are drawn for the rank's own images only: give every rank its own ``np_rng`` / ``py_rng``."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError('batch_size must be positive')
        if shard is not None:
            from ..parallel import shard_range
            rank, world = (int(v) for v in shard)
            if not 0 <= rank < world:
                raise ValueError('shard must be (rank, world) with 0 <= rank < world')
        output_sizes = [int(o) for o in output_sizes]
        for lo in range(0, len(self), batch_size):
            rows = list(range(lo, min(lo + batch_size, len(self))))
            if shard is not None:
                if len(rows) < world:
                    raise ValueError('a batch of %d images cannot be sharded over %d ranks' % (len(rows), world))
                a, b = shard_range(len(rows), rank, world)
                rows = rows[a:b]
            img, tables, first = self.describe_labelled(rows, input_size, output_sizes, np_rng, py_rng, **aug)
            images = self.augment(img, input_size)
            heats, masks, jts = self.targets(rows, tables, first, output_sizes)
            yield images, heats, masks, jts
