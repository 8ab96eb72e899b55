"""Drop-in for ``fast_utils.group`` (reference nano_demo/fast_utils/group.py:10-48).

``HeatmapParser(cfg).parse(det, tmap, scale) -> ans[:num]`` with the reference's signature and record layout
(``[num, J, 4]`` = x, y, val, tag with x, y multiplied by ``scale``), for image 0 of the batch, computed by lp_fast_parse
and left on the device.  ``parse_batch`` is the batched generalisation: per image the record equals the reference's
batch-1 result.  The records differ from ``core.group``'s by design (first M peaks in raster order, a one-dimensional
tag, no adjust, no refine).
"""
import ctypes as C

import torch

from .. import _native as nv


class Params(object):
    # fast_utils/group.py:10-31
    def __init__(self, cfg):
        self.num_joints = cfg.DATASET.NUM_JOINTS
        self.max_num_people = cfg.DATASET.MAX_NUM_PEOPLE
        if self.max_num_people > 10:
            raise NotImplementedError('DATASET.MAX_NUM_PEOPLE = %d: the reference\'s assign.cpp keeps its people in [10] '
                                      'arrays (beyond that it is undefined)' % self.max_num_people)
        self.detection_threshold = cfg.TEST.DETECTION_THRESHOLD
        self.tag_threshold = cfg.TEST.TAG_THRESHOLD
        self.use_detection_val = cfg.TEST.USE_DETECTION_VAL
        self.ignore_too_much = cfg.TEST.IGNORE_TOO_MUCH
        self.window_size = cfg.TEST.NMS_KERNEL
        if cfg.DATASET.WITH_CENTER and cfg.TEST.IGNORE_CENTER:
            self.num_joints -= 1
        if cfg.DATASET.WITH_CENTER and not cfg.TEST.IGNORE_CENTER:
            self.joint_order = [i - 1 for i in
                                [18, 1, 2, 3, 4, 5, 6, 7, 12, 13, 8, 9, 10, 11, 14, 15, 16, 17]]
        else:
            self.joint_order = [i - 1 for i in
                                [1, 2, 3, 4, 5, 6, 7, 12, 13, 8, 9, 10, 11, 14, 15, 16, 17]]


class HeatmapParser(object):
    """``parse`` raises when image 0 hit the assignment's round cap (the reference's signature has no way to say so);
    ``parse_batch`` reports it as ``num[n] = -1`` with an all-zero record and leaves the decision to the caller.  The peak
    lists live in a workspace cached per device AND stream: calls of one parser on different streams do not share it."""

    def __init__(self, cfg):
        self.params = Params(cfg)
        self.tag_per_joint = cfg.MODEL.TAG_PER_JOINT
        self._lib = nv.lib()
        self._ws = {}

    def _scratch(self, nbytes, device):
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            self._ws[key] = t
        return t

    def parse_batch(self, det, tmap, scale=1.0):
        """det [N,J,H,W], tmap [N,J,H,W,T] (its first tag map is read in place) or [N,J,H,W], float32 on the device ->
        (ans [N,M,J,4], num [N] int32) on the device; num[n] = -1: image n hit the assignment's round cap (all zero)."""
        p = self.params
        if det.dim() != 4 or tmap.dim() not in (4, 5) or tuple(tmap.shape[:4]) != tuple(det.shape):
            raise ValueError('det [N,J,H,W] and tmap [N,J,H,W,T] expected, got %s and %s' % (tuple(det.shape), tuple(tmap.shape)))
        if det.dtype != torch.float32 or tmap.dtype != torch.float32:
            raise ValueError('float32 maps expected')
        N, J, H, W = det.shape
        if J > len(p.joint_order):
            raise ValueError('%d joints, joint_order names %d' % (J, len(p.joint_order)))
        stride = int(tmap.shape[4]) if tmap.dim() == 5 else 1
        M = int(p.max_num_people)
        order = (C.c_int32 * J)(*[int(v) for v in p.joint_order[:J]])
        ans = torch.empty((N, M, J, 4), dtype=torch.float32, device=det.device)
        num = torch.empty((N,), dtype=torch.int32, device=det.device)
        need = int(self._lib.lp_fast_parse_workspace_bytes(N, J, M))
        ws = self._scratch(need, det.device)
        nv.check(self._lib.lp_fast_parse(nv.dptr(det), nv.dptr(tmap), stride, N, J, H, W, float(p.detection_threshold),
                                         int(p.window_size), M, order, float(p.tag_threshold), nv.dptr(ans), nv.dptr(num),
                                         nv.dptr(ws), need, nv.stream_ptr()), 'lp_fast_parse')
        ans[:, :, :, :2] *= scale
        return ans, num

    def parse(self, det, tmap, scale):
        """fast_utils/group.py:38-48: the persons of image 0, ``ans[:num]`` with x, y scaled, on the device."""
        ans, num = self.parse_batch(det[:1], tmap[:1], scale)
        n = int(num[0])
        if n < 0:
            raise nv.LitePoseNativeError('fast parse: the assignment of image 0 hit its round cap (4096 rounds in one joint)')
        return ans[0, :n]
