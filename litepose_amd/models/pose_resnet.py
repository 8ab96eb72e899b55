"""Drop-in for ``models.pose_resnet`` (reference lib/models/pose_resnet.py; the class is again ``LitePose``).

pose_resnet is LitePose built from dense convolutions: a two-conv 7x7 stem, four stages of ``FusedMBConv`` blocks
(dense k x k expand + 1x1 project, layers.py:67-88), a Fusion Deconv Head whose deconvs are ``UpConv`` (nearest x2 +
dense conv, layers.py:58-65) and 3x3 output convs with bias.  There is no arch JSON: the backbone table is fixed in the
module (pose_resnet.py:24-31) and only the deconv widths / kernels come from ``cfg.MODEL.EXTRA``; ``cfg_arch`` is
accepted and ignored like in the reference (pose_resnet.py:133-134).  The wrapper is ``models.pose_mobilenet.LitePose``
with ``lp_arch.family = 1``; every k x k conv runs in ``convk3_kernel`` (csrc/convk_kernels.hip), fp32 storage only.
"""
from .. import _native as nv
from . import pose_mobilenet as _pm

INPUT_CHANNEL = 16
# r, k, c, n, s (pose_resnet.py:25-31)
BACKBONE_SETTING = [[4, 7, 16, 4, 2], [4, 7, 32, 6, 2], [4, 5, 48, 8, 2], [4, 3, 80, 8, 1]]


def _arch_struct(cfg):
    a = nv.LpArch()
    a.family = 1
    a.plain_head = 0
    a.input_channel = INPUT_CHANNEL
    a.num_stages = len(BACKBONE_SETTING)
    for s, (r, k, c, n, st) in enumerate(BACKBONE_SETTING):
        a.num_blocks[s] = n
        a.stride[s] = st
        a.channel[s] = c
        for b in range(n):
            a.expand[s][b] = r
            a.kernel[s][b] = k
    extra = cfg.MODEL.EXTRA
    a.num_deconv = int(extra.NUM_DECONV_LAYERS)
    ks = [int(k) for k in extra.NUM_DECONV_KERNELS[:a.num_deconv]]
    if len(set(ks)) != 1:
        raise ValueError('NUM_DECONV_KERNELS must hold one size for every layer on this path, got %s' % ks)
    if ks[0] % 2 == 0:
        raise ValueError('pose_resnet needs an odd NUM_DECONV_KERNELS (UpConv: only an odd kernel doubles the plane)')
    a.upconv_kernel = ks[0]
    for i, f in enumerate(list(extra.NUM_DECONV_FILTERS)[:a.num_deconv]):
        a.deconv_filters[i] = int(f)
    dim_tag = cfg.MODEL.NUM_JOINTS if cfg.MODEL.TAG_PER_JOINT else 1
    for i in range(1, a.num_deconv):        # pose_resnet.py:83-89
        oup = (cfg.MODEL.NUM_JOINTS if cfg.LOSS.WITH_HEATMAPS_LOSS[i - 1] else 0) + \
              (dim_tag if cfg.LOSS.WITH_AE_LOSS[i - 1] else 0)
        a.head_channels[i - 1] = int(oup)
    return a


class LitePose(_pm.LitePose):
    def __init__(self, cfg, width_mult=1.0, round_nearest=8, cfg_arch=None, storage=None):
        """``storage``: only 'f32' (or None with ``cfg.FP16.ENABLED`` off): the dense convs have no 16-bit kernels."""
        if storage is None:
            storage = 'bf16' if bool(cfg.FP16.ENABLED) else 'f32'
        if _pm.STORAGE.get(storage, -1) != 0:
            raise NotImplementedError('pose_resnet runs in fp32 storage only (storage=%r / cfg.FP16.ENABLED): the 16-bit '
                                      'dense-convolution path is not built' % (storage,))
        super(LitePose, self).__init__(cfg, width_mult, round_nearest, cfg_arch=None, storage='f32')

    def _make_arch(self, cfg, cfg_arch, plain_head):
        return _arch_struct(cfg)


def get_pose_net(cfg, is_train=False, cfg_arch=None, storage=None):
    """pose_resnet.py:133-151.  ``cfg_arch`` is ignored (the reference's signature takes and drops it); pre-trained
    backbone loading (is_train and INIT_WEIGHTS) is a training feature and out of scope."""
    return LitePose(cfg, storage=storage)
