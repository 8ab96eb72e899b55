"""Drop-in for ``models.pose_resnet`` (reference lib/models/pose_resnet.py; the class is again ``LitePose``).

pose_resnet is LitePose built from dense convolutions: a two-conv 7x7 stem, four stages of ``FusedMBConv`` blocks
(dense k x k expand + 1x1 project, layers.py:67-88), a Fusion Deconv Head whose deconvs are ``UpConv`` (nearest x2 +
dense conv, layers.py:58-65) and 3x3 output convs with bias.  There is no arch JSON: the backbone table is fixed in the
module (pose_resnet.py:24-31) and only the deconv widths / kernels come from ``cfg.MODEL.EXTRA``; ``cfg_arch`` is
accepted and ignored like in the reference (pose_resnet.py:133-134).  The wrapper is ``models.pose_mobilenet.LitePose``
with ``lp_arch.family = 1``; every k x k conv runs in ``convk3_kernel`` (csrc/convk_kernels.hip), fp32 storage only.

``get_train_net(cfg, backend, width_mult, init_from)`` returns ``TrainablePoseResNet``, the same network as a real
``torch.nn.Module`` for training (``core.trainer.do_train``): same ``state_dict``, its layers on
``litepose_amd.nn.functional`` (``dense_conv``, ``pointwise``, ``batch_norm_act``).
"""
from collections import OrderedDict

import torch

from .. import _native as nv
from ..nn import functional as F_
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
    backbone loading (is_train and INIT_WEIGHTS) is ``get_train_net(..., init_from=...)``."""
    return LitePose(cfg, storage=storage)


# ---- the trainable module ----------------------------------------------------------------------------------------
def _dense(cin, cout, k, stride=1, bias=False):
    return torch.nn.Conv2d(cin, cout, k, stride, k // 2, bias=bias)


class TrainablePoseResNet(_pm.LayerWalk, torch.nn.Module):
    """pose_resnet's LitePose as a ``torch.nn.Module`` whose parameters and buffers carry the reference's names, shapes and
    registration order (a reference checkpoint and ``pose_resnet.LitePose.state_dict()`` both load) and whose ``forward``
    returns the list of stage outputs, for ``core.trainer.do_train``.

    ``backend='native'``: every layer runs on ``litepose_amd.nn.functional`` -- forward and backward: every K x K
    convolution on ``dense_conv`` (the 7x7 stem pair, the expand of every ``FusedMBConv``, the ``UpConv`` pairs read through
    the nearest x2 upsample, the biased output convolutions as one two-source call), the 1x1 projections on ``pointwise``,
    every BatchNorm (+ activation, + residual) on ``batch_norm_act``.  No torch convolution runs, also when the image itself
    requires a gradient.  No sum is atomic: one step gives the same bits every time.  float32 on the GPU.
    ``backend='torch'``: every layer on torch's ops: the same module on any device and dtype.

    The modules below only hold parameters under the checkpoint's names; ``forward`` walks them layer by layer."""

    def __init__(self, cfg, backend='native', width_mult=1.0):
        super().__init__()
        if backend not in ('native', 'torch'):
            raise ValueError("backend must be 'native' or 'torch'")
        nn = torch.nn
        self.backend = backend
        self._cfg, self.width_mult = cfg, float(width_mult)
        c_in = _pm._round8(INPUT_CHANNEL * width_mult)
        self.first = nn.Sequential(nn.Sequential(_dense(3, 32, 7, 2), nn.BatchNorm2d(32), nn.ReLU6()),
                                   nn.Sequential(_dense(32, c_in, 7, 1), nn.BatchNorm2d(c_in), nn.ReLU6()))
        channels, stages = [c_in], []
        for r, k, c, n, s in BACKBONE_SETTING:
            c_out = _pm._round8(c * width_mult)
            blocks = []
            for b in range(n):
                stride = s if b == 0 else 1
                mid = _pm._round8(round(c_in * r))
                blk = nn.Module()
                blk.inv = nn.Sequential(_dense(c_in, mid, k, stride), nn.BatchNorm2d(mid), nn.ReLU6())
                blk.point_conv = nn.Sequential(nn.Conv2d(mid, c_out, 1, bias=False), nn.BatchNorm2d(c_out))
                blk.stride, blk.residual = stride, stride == 1 and c_in == c_out
                blocks.append(blk)
                c_in = c_out
            stages.append(nn.Sequential(*blocks))
            channels.append(c_out)
        self.stage = nn.ModuleList(stages)
        extra = cfg.MODEL.EXTRA
        self.num_deconv_layers = int(extra.NUM_DECONV_LAYERS)
        filters = [int(f) for f in extra.NUM_DECONV_FILTERS]
        kernels = [int(k) for k in extra.NUM_DECONV_KERNELS]
        refined, raw, bnrelu = [], [], []
        planes_in = channels[-1]
        for i in range(self.num_deconv_layers):
            if kernels[i] not in (3, 5, 7):
                raise ValueError('pose_resnet needs NUM_DECONV_KERNELS of 3, 5 or 7 (UpConv: only an odd kernel doubles the plane)')
            for lst, c in ((refined, planes_in), (raw, channels[-i - 2])):
                up = nn.Module()
                up.conv = _dense(c, filters[i], kernels[i])
                lst.append(up)
            bnrelu.append(nn.Sequential(nn.BatchNorm2d(filters[i]), nn.ReLU()))
            planes_in = filters[i]
        self.deconv_refined, self.deconv_raw = nn.ModuleList(refined), nn.ModuleList(raw)
        self.deconv_bnrelu = nn.ModuleList(bnrelu)
        J = int(cfg.MODEL.NUM_JOINTS)
        dim_tag = J if cfg.MODEL.TAG_PER_JOINT else 1
        f_refined, f_raw, self.final_channel = [], [], []
        for i in range(1, self.num_deconv_layers):
            out = (J if cfg.LOSS.WITH_HEATMAPS_LOSS[i - 1] else 0) + (dim_tag if cfg.LOSS.WITH_AE_LOSS[i - 1] else 0)
            f_refined.append(_dense(filters[i], out, 3, bias=True))
            f_raw.append(_dense(channels[-i - 3], out, 3, bias=True))
            self.final_channel.append(out)
        self.final_refined, self.final_raw = nn.ModuleList(f_refined), nn.ModuleList(f_raw)
        self.channel = channels

    # ---- layers: LayerWalk's _bn, and the dense convolutions of this family ----
    def _conv(self, x, conv):
        if self.backend == 'native':
            if conv.kernel_size[0] == 1:
                return F_.pointwise(x, conv.weight)
            return F_.dense_conv(x, conv.weight, stride=conv.stride[0])
        return torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding)

    def _pair(self, refined, c_refined, raw, c_raw, upsample):
        """conv(U(refined)) + conv(U(raw)) (+ both biases), U the nearest x2 upsample or the identity"""
        bias = None if c_refined.bias is None else c_refined.bias + c_raw.bias
        if self.backend == 'native':
            return F_.dense_conv(refined, c_refined.weight, raw, c_raw.weight, bias, 1, upsample)
        fn = torch.nn.functional
        up = (lambda t: fn.interpolate(t, scale_factor=2)) if upsample else (lambda t: t)
        return fn.conv2d(up(refined), c_refined.weight, c_refined.bias, 1, c_refined.padding) + \
            fn.conv2d(up(raw), c_raw.weight, c_raw.bias, 1, c_raw.padding)

    def _block(self, x, blk):
        y = self._bn(self._conv(x, blk.inv[0]), blk.inv[1], 'relu6')
        return self._bn(self._conv(y, blk.point_conv[0]), blk.point_conv[1], None, x if blk.residual else None)

    def walk(self, net, x):
        for f in net.first:
            x = self._bn(self._conv(x, f[0]), f[1], 'relu6')
        feats = [x]
        for blocks in net.stage:
            for blk in blocks:
                x = self._block(x, blk)
            feats.append(x)
        outputs = []
        refined, raw = feats[-1], feats[-2]
        for i in range(net.num_deconv_layers):
            y = self._pair(refined, net.deconv_refined[i].conv, raw, net.deconv_raw[i].conv, True)
            refined = self._bn(y, net.deconv_bnrelu[i][0], 'relu')
            raw = feats[-i - 3]
            if i > 0:
                outputs.append(self._pair(refined, net.final_refined[i - 1], raw, net.final_raw[i - 1], False))
        return outputs

    def forward(self, x):
        return self.walk(self, x)

    def to_engine(self, storage=None):
        """A ``pose_resnet.LitePose`` inference handle loaded from this module's ``state_dict`` (``width_mult`` 1.0 only,
        as the inference class)."""
        net = LitePose(self._cfg, width_mult=self.width_mult, storage=storage)
        net.load_state_dict(self.state_dict())
        return net


def get_train_net(cfg, backend='native', width_mult=1.0, init_from=None):
    """The trainable counterpart of ``get_pose_net``: a ``TrainablePoseResNet`` (initialised as torch initialises its
    layers).  ``init_from``: a state dict (the caller loads the file) taken as the reference takes ``MODEL.PRETRAINED``
    when ``is_train and INIT_WEIGHTS`` (pose_resnet.py:135-150): keys that name a ``deconv*`` or ``final*`` tensor are
    dropped, the rest is loaded non-strictly."""
    model = TrainablePoseResNet(cfg, backend, width_mult)
    if init_from is not None:
        model.load_state_dict(OrderedDict((k, v) for k, v in init_from.items() if 'deconv' not in k and 'final' not in k),
                              strict=False)
    return model
