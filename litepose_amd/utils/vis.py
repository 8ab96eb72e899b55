"""Drop-in for ``utils.vis`` (reference lib/utils/vis.py:18-118 and nano_demo/utils/vis.py): skeletons drawn on the
device by ``lp_draw_poses`` / ``lp_draw_poses_v``.

The raster rule is this library's own, all-integer and exact; it is PARITY-UNPINNED against cv2:
``cv2.circle(radius 1, thickness 2)`` is stood for by the integer disc of radius 2 (13 pixels) and ``cv2.line(thickness
2)`` by the integer capsule of radius 1, and how far these differ from cv2's pixel sets at boundary pixels is not
measured (cv2 was not available to pin them).  ``save_valid_image`` and the heat-map / tag-map grids are not covered
(they need cv2.imwrite, cv2.resize and the JET colour table).
"""
import ctypes as C

import numpy as np
import torch

from .. import _native as nv

coco_part_labels = [
    'nose', 'eye_l', 'eye_r', 'ear_l', 'ear_r', 'sho_l', 'sho_r', 'elb_l', 'elb_r', 'wri_l', 'wri_r',
    'hip_l', 'hip_r', 'kne_l', 'kne_r', 'ank_l', 'ank_r',
]
coco_part_orders = [
    ('nose', 'eye_l'), ('eye_l', 'eye_r'), ('eye_r', 'nose'), ('eye_l', 'ear_l'), ('eye_r', 'ear_r'),
    ('ear_l', 'sho_l'), ('ear_r', 'sho_r'), ('sho_l', 'sho_r'), ('sho_l', 'hip_l'), ('sho_r', 'hip_r'),
    ('hip_l', 'hip_r'), ('sho_l', 'elb_l'), ('elb_l', 'wri_l'), ('sho_r', 'elb_r'), ('elb_r', 'wri_r'),
    ('hip_l', 'kne_l'), ('kne_l', 'ank_l'), ('hip_r', 'kne_r'), ('kne_r', 'ank_r'),
]
crowd_pose_part_labels = [
    'left_shoulder', 'right_shoulder', 'left_elbow', 'right_elbow', 'left_wrist', 'right_wrist', 'left_hip',
    'right_hip', 'left_knee', 'right_knee', 'left_ankle', 'right_ankle', 'head', 'neck',
]
crowd_pose_part_orders = [
    ('head', 'neck'), ('neck', 'left_shoulder'), ('neck', 'right_shoulder'), ('left_shoulder', 'right_shoulder'),
    ('left_shoulder', 'left_hip'), ('right_shoulder', 'right_hip'), ('left_hip', 'right_hip'),
    ('left_shoulder', 'left_elbow'), ('left_elbow', 'left_wrist'), ('right_shoulder', 'right_elbow'),
    ('right_elbow', 'right_wrist'), ('left_hip', 'left_knee'), ('left_knee', 'left_ankle'),
    ('right_hip', 'right_knee'), ('right_knee', 'right_ankle'),
]


def _config(labels, orders):
    idx = {b: a for a, b in enumerate(labels)}
    return {'part_labels': labels, 'part_idx': idx, 'part_orders': orders,
            'links': [(idx[a], idx[b]) for a, b in orders]}         # the integer table the kernel takes


VIS_CONFIG = {
    'COCO': _config(coco_part_labels, coco_part_orders),
    'CROWDPOSE': _config(crowd_pose_part_labels, crowd_pose_part_orders),
}

DEFAULT_COLOR = (0, 0, 255)                 # vis.py:103,115
IMAGE_DESC_DTYPE = np.dtype([('offset', '<i8'), ('H', '<i4'), ('W', '<i4')])      # lp_image_desc, 16 bytes
assert IMAGE_DESC_DTYPE.itemsize == 16


def image_descriptors(sizes, offsets=None, device='cuda'):
    """The device table of ``annotate_batch(..., sizes=)``: ``sizes`` [(H, W)] of images packed back to back, or at the
    byte ``offsets`` given (as BucketLoader packs them)."""
    d = np.zeros(len(sizes), IMAGE_DESC_DTYPE)
    off = 0
    for i, (h, w) in enumerate(sizes):
        d[i] = (off if offsets is None else int(offsets[i]), int(h), int(w))
        off += int(h) * int(w) * 3
    return torch.from_numpy(d.view(np.uint8).reshape(len(sizes), 16)).to(device)


def annotate_batch(images, kpts, count, dataset='COCO', links=None, palette=None, sizes=None, joint_radius=2,
                   link_radius=1):
    """Draw the persons of device records IN PLACE, one launch, no synchronisation.

    images   uint8 device tensor [N,H,W,3]; or, with ``sizes``, a flat uint8 buffer of N images of different sizes
    kpts     float32 [N,pcap,J,D] rows (x, y, val, ...), D >= 3, and count int32 [N], as PendingBatch.result() /
             PoseEngine.infer_batch (D = 3 + T) or fast_utils.group.HeatmapParser.parse_batch (D = 4, num) hand them over
    links    [(a, b)] joint index pairs (default: VIS_CONFIG[dataset]); palette [(b0, b1, b2)] (default: (0, 0, 255))
    sizes    [(H, W)] of images packed back to back, or a device descriptor table (``image_descriptors``)
    """
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.uint8):
        raise ValueError('images must be a uint8 device tensor')
    if kpts.dim() != 4 or kpts.dtype != torch.float32 or count.dtype != torch.int32:
        raise ValueError('kpts float32 [N,pcap,J,D] and count int32 [N] expected')
    N, pcap, J, D = [int(v) for v in kpts.shape]
    if tuple(count.shape) != (N,):
        raise ValueError('count must be [N]')
    links = VIS_CONFIG[dataset]['links'] if links is None else links
    palette = [DEFAULT_COLOR] if palette is None else palette
    flat = [int(v) for ab in links for v in ab]
    l_c = (C.c_int32 * max(len(flat), 1))(*flat)
    pal = [int(v) for c in palette for v in c]
    p_c = (C.c_uint8 * max(len(pal), 1))(*pal)
    lib = nv.lib()
    if sizes is None:
        if images.dim() != 4 or images.shape[3] != 3 or images.shape[0] != N:
            raise ValueError('images must be [N,H,W,3] with the N of kpts')
        nv.check(lib.lp_draw_poses(nv.dptr(images), N, int(images.shape[1]), int(images.shape[2]), nv.dptr(kpts),
                                   nv.dptr(count), pcap, J, D, l_c, len(links), p_c, len(palette), int(joint_radius),
                                   int(link_radius), nv.stream_ptr()), 'lp_draw_poses')
    else:
        desc = sizes if isinstance(sizes, torch.Tensor) else image_descriptors(sizes, device=images.device)
        if desc.numel() * desc.element_size() != N * IMAGE_DESC_DTYPE.itemsize:
            raise ValueError('sizes must name the N images of kpts')
        nv.check(lib.lp_draw_poses_v(nv.dptr(images), images.numel(), nv.dptr(desc), N, nv.dptr(kpts), nv.dptr(count),
                                     pcap, J, D, l_c, len(links), p_c, len(palette), int(joint_radius),
                                     int(link_radius), nv.stream_ptr()), 'lp_draw_poses_v')
    return images


def _records(joints, device):
    """joints [P,J,>=3] (tensor, array or list of per-person arrays) -> (kpts [1,max(P,1),J,D], count [1]) on the device."""
    if not isinstance(joints, torch.Tensor):
        joints = torch.from_numpy(np.ascontiguousarray(np.asarray(joints, dtype=np.float32)))
    if joints.numel() == 0:
        return torch.zeros((1, 1, 1, 3), device=device), torch.zeros((1,), dtype=torch.int32, device=device)
    if joints.dim() == 2:
        joints = joints[None]
    k = joints.to(device=device, dtype=torch.float32).contiguous()[None]
    return k, torch.full((1,), k.shape[1], dtype=torch.int32, device=device)


def add_joints(image, joints, color, dataset='COCO'):
    """vis.py:68-94: ONE person ``joints`` [J,>=3] drawn into the uint8 [H,W,3] device ``image`` in place."""
    k, c = _records(joints, image.device)
    annotate_batch(image[None], k, c, dataset=dataset, palette=[tuple(int(v) for v in color)])
    return image


def get_annotated_image(image, joints, dataset='COCO', count=None):
    """vis.py:109-118: ``image`` RGB uint8 [H,W,3] -> a BGR copy with every person of ``joints`` [P,J,>=3] drawn in
    (0, 0, 255); the input is not modified.  A device tensor stays on the device; a NumPy image is uploaded and comes
    back as NumPy.  ``count`` (device int32 [1], optional): draw the first ``count`` persons only, without reading it on
    the host (the demo passes the fast parser's ``num``)."""
    host = not isinstance(image, torch.Tensor)
    img = torch.from_numpy(np.ascontiguousarray(image)) if host else image
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('image must be HxWx3 uint8')
    out = img.cuda().flip(2).contiguous()                            # cv2.COLOR_RGB2BGR, a copy
    k, c = _records(joints, out.device)
    annotate_batch(out[None], k, c if count is None else count, dataset=dataset)
    return out.cpu().numpy() if host else out
