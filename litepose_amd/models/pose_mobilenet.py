"""Drop-in for ``models.pose_mobilenet`` (reference lib/models/pose_mobilenet.py).

``get_pose_net(cfg, is_train, cfg_arch)`` returns a ``LitePose`` object with the
subset of the ``nn.Module`` surface valid.py touches (valid.py:125-165,194):
``__call__/forward``, ``eval()``, ``cuda()``, ``load_state_dict(sd, strict)``,
``state_dict()``.  The network itself is the native engine behind the C ABI
(lp_net_*): Python only moves pointers.

``get_train_net(cfg, cfg_arch, backend)`` returns ``TrainableLitePose``, the same network as a real ``torch.nn.Module``
for training (``core.trainer.do_train``): same ``state_dict``, its blocks on ``litepose_amd.nn.functional``.
"""
import ctypes as C
from collections import OrderedDict

import torch

from .. import _native as nv
from ..nn import functional as F_


def _arch_struct(cfg, cfg_arch, plain_head=False):
    a = nv.LpArch()
    a.plain_head = 1 if plain_head else 0       # 1: pose_simplenet (no deconv_raw / final_raw branches)
    a.input_channel = int(cfg_arch['input_channel'])
    bs = cfg_arch['backbone_setting']
    if len(bs) > nv.LP_MAX_STAGES:
        raise ValueError('too many stages')
    a.num_stages = len(bs)
    for s, st in enumerate(bs):
        a.num_blocks[s] = int(st['num_blocks'])
        a.stride[s] = int(st['stride'])
        a.channel[s] = int(st['channel'])
        for b in range(st['num_blocks']):
            t, k = st['block_setting'][b]
            a.expand[s][b] = int(t)
            a.kernel[s][b] = int(k)
    extra = cfg.MODEL.EXTRA
    a.num_deconv = int(extra.NUM_DECONV_LAYERS)
    if any(int(k) != 4 for k in extra.NUM_DECONV_KERNELS[:a.num_deconv]):
        raise ValueError('only NUM_DECONV_KERNELS == 4 is supported on this path')
    for i, f in enumerate(cfg_arch['deconv_setting'][:a.num_deconv]):
        a.deconv_filters[i] = int(f)
    dim_tag = cfg.MODEL.NUM_JOINTS if cfg.MODEL.TAG_PER_JOINT else 1
    for i in range(1, a.num_deconv):        # pose_mobilenet.py:92-98
        oup = (cfg.MODEL.NUM_JOINTS if cfg.LOSS.WITH_HEATMAPS_LOSS[i - 1] else 0) + \
              (dim_tag if cfg.LOSS.WITH_AE_LOSS[i - 1] else 0)
        a.head_channels[i - 1] = int(oup)
    return a


STORAGE = {'f32': 0, 'fp32': 0, 'float32': 0, 'bf16': 1, 'bfloat16': 1, 'f16': 2, 'fp16': 2, 'float16': 2}
_STORAGE_NAME = {0: 'f32', 1: 'bf16', 2: 'f16'}


class LitePose(object):
    def __init__(self, cfg, width_mult=1.0, round_nearest=8, cfg_arch=None, storage=None, plain_head=False):
        """``storage``: 'f32' (the reference's arithmetic), 'bf16' (activations + folded weights in bf16,
        fp32 accumulation: the counterpart of the reference's reduced-precision switch ``cfg.FP16.ENABLED``,
        valid.py:152-153 -> fp16util.py:87-91 network_to_half, which is also the default when None) or 'f16'
        (the same path in IEEE half, the format network_to_half itself uses; aliases 'fp16', 'float16').
        ``plain_head``: the network of pose_simplenet.py (no raw branches; models.pose_simplenet sets it)."""
        if width_mult != 1.0 or round_nearest != 8:
            raise ValueError('width_mult/round_nearest other than the defaults are not on the path')
        if storage is None:
            storage = 'bf16' if bool(cfg.FP16.ENABLED) else 'f32'
        if storage not in STORAGE:
            raise ValueError('storage must be one of %s' % sorted(STORAGE))
        self.storage = _STORAGE_NAME[STORAGE[storage]]
        self._lib = nv.lib()
        self._arch = self._make_arch(cfg, cfg_arch, plain_head)
        h = C.c_void_p()
        nv.check(self._lib.lp_net_create(C.byref(h), C.byref(self._arch)), 'lp_net_create')
        self._h = h
        self.final_channel = [int(self._arch.head_channels[i]) for i in range(self._arch.num_deconv - 1)]
        self._ws = None
        self._finalized = False
        self.training = False

    def _make_arch(self, cfg, cfg_arch, plain_head):
        """The lp_arch of this network (models.pose_resnet overrides it: its table is fixed in the module)."""
        return _arch_struct(cfg, cfg_arch, plain_head)

    @property
    def size_multiple(self):
        """H and W of a forward are positive multiples of this: max(16, the deepest plane's divisor = 2 for the stem times
        every stage stride).  The library refuses any other size (lp_net_forward, LP_ERR_INVALID_ARG): buffers are sized
        H // div while a stride-2 kernel rounds its output plane up."""
        deep = 2
        for s in range(self._arch.num_stages):
            deep *= int(self._arch.stride[s])
        return max(16, deep)

    def output_divisors(self):
        """Spatial divisors of the two outputs: three x2 deconvs above the deepest plane, heads after the second and the
        third -- (4, 2) for every table whose deepest plane is 1/16 of the input."""
        deep = 2
        for s in range(self._arch.num_stages):
            deep *= int(self._arch.stride[s])
        return max(1, deep // 4), max(1, deep // 8)

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self._lib.lp_net_destroy(h)
            self._h = None

    # ---- nn.Module-shaped surface ------------------------------------------------
    def eval(self):
        return self

    def cuda(self, device=None):
        return self

    def to(self, *a, **k):
        return self

    def keys(self):
        out = []
        shp = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(self._lib.lp_net_num_keys(self._h)):
            k = self._lib.lp_net_key(self._h, i, shp, C.byref(nd))
            out.append((k.decode(), tuple(int(shp[d]) for d in range(nd.value))))
        return out

    def load_state_dict(self, state_dict, strict=True):
        expected = dict(self.keys())
        given = {}
        for k, v in state_dict.items():
            given[k[7:] if k.startswith('module.') else k] = v
        if strict:
            missing = [k for k in expected if k not in given]
            unexpected = [k for k in given if k not in expected]
            if missing or unexpected:
                raise RuntimeError('Error(s) in loading state_dict for LitePose: missing %s unexpected %s'
                                   % (missing[:5], unexpected[:5]))
        for k, v in given.items():
            if k not in expected:
                continue
            if k.endswith('num_batches_tracked'):
                nv.check(self._lib.lp_net_set_weight(self._h, k.encode(), None, None, 0), k)
                continue
            t = torch.as_tensor(v).detach().to('cpu', torch.float32).contiguous()
            if tuple(t.shape) != expected[k]:
                raise RuntimeError('size mismatch for %s: %s vs %s' % (k, tuple(t.shape), expected[k]))
            shp = (C.c_int64 * max(1, t.dim()))(*t.shape)
            nv.check(self._lib.lp_net_set_weight(self._h, k.encode(), C.c_void_p(t.data_ptr()), shp, t.dim()), k)
        nv.check(self._lib.lp_net_set_storage(self._h, STORAGE[self.storage]), 'lp_net_set_storage')
        nv.check(self._lib.lp_net_finalize(self._h, 1 if strict else 0), 'lp_net_finalize')
        self._finalized = True
        return self

    def state_dict(self):
        sd = OrderedDict()
        for k, shp in self.keys():
            if k.endswith('num_batches_tracked'):
                sd[k] = torch.zeros((), dtype=torch.int64)
                continue
            t = torch.empty(shp, dtype=torch.float32)
            nv.check(self._lib.lp_net_get_weight(self._h, k.encode(), C.c_void_p(t.data_ptr()), t.numel()), k)
            sd[k] = t
        return sd

    # ---- forward --------------------------------------------------------------------
    def _workspace(self, n, h, w, device):
        need = int(self._lib.lp_net_workspace_bytes(self._h, n, h, w))
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws, need

    def forward_native(self, x, flip=0):
        """flip: 0 plain, 1 on flip(x,[3]), 2 both (outputs hold 2N images: plain then flipped)."""
        if not self._finalized:
            raise nv.LitePoseNativeError('load_state_dict() has not been called')
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('expected a float32 [N,3,H,W] tensor')
        x = x.contiguous()
        n, _, h, w = x.shape
        nb = 2 * n if flip == 2 else n
        m = self.size_multiple
        if h < m or w < m or h % m or w % m:
            raise ValueError('H and W must be positive multiples of %d for this net, got %dx%d' % (m, h, w))
        d0, d1 = self.output_divisors()
        out0 = torch.empty((nb, self.final_channel[0], h // d0, w // d0), dtype=torch.float32, device=x.device)
        out1 = torch.empty((nb, self.final_channel[1], h // d1, w // d1), dtype=torch.float32, device=x.device)
        ws, need = self._workspace(nb, h, w, x.device)
        nv.check(self._lib.lp_net_forward(self._h, nv.dptr(x), n, h, w, flip, nv.dptr(out0), nv.dptr(out1),
                                          nv.dptr(ws), need, nv.stream_ptr()), 'lp_net_forward')
        return [out0, out1]

    def forward(self, x):
        return self.forward_native(x, 0)

    __call__ = forward

    def tap(self, name):
        cnt = nv.check(self._lib.lp_net_tap(self._h, name.encode(), None, None), 'lp_net_tap')
        t = torch.empty(cnt, dtype=torch.float32, device=self._ws.device)
        nv.check(self._lib.lp_net_tap(self._h, name.encode(), nv.dptr(t), nv.stream_ptr()), 'lp_net_tap')
        return t

    def set_option(self, key, value):
        """Kernel-family switch of this net (include/litepose_amd.h: lp_net_set_option); returns the previous value."""
        prev = nv.check(self._lib.lp_net_get_option(self._h, key.encode()), 'lp_net_get_option')
        nv.check(self._lib.lp_net_set_option(self._h, key.encode(), int(value)), 'lp_net_set_option')
        return prev

    def get_option(self, key):
        return nv.check(self._lib.lp_net_get_option(self._h, key.encode()), 'lp_net_get_option')

    def set_profiling(self, enable):
        nv.check(self._lib.lp_net_set_profiling(self._h, 1 if enable else 0))

    def profile(self, cap=256, split=False, launches=False):
        """Per-launch (name|kernel, ms, algorithmic bytes, algorithmic FLOPs) of the last profiled forward;
        ``split=True`` appends the vector-pipe (depthwise) share of the FLOPs as a fifth field; ``launches=True`` appends
        the launch geometry (grid workgroups, threads per workgroup, LDS bytes, workgroups per CU by the occupancy query)
        as a sixth field (implies ``split``)."""
        names = ((C.c_char * 48) * cap)()
        ms = (C.c_float * cap)()
        by = (C.c_int64 * cap)()
        fl = (C.c_int64 * cap)()
        fv = (C.c_int64 * cap)()
        n = nv.check(self._lib.lp_net_profile2(self._h, names, ms, by, fl, fv, cap), 'lp_net_profile2')
        if launches:
            g, t, l, o = [(C.c_int32 * cap)() for _ in range(4)]
            nv.check(self._lib.lp_net_profile_launches(self._h, g, t, l, o, cap), 'lp_net_profile_launches')
            return [(names[i].value.decode(), float(ms[i]), int(by[i]), int(fl[i]), int(fv[i]),
                     (int(g[i]), int(t[i]), int(l[i]), int(o[i]))) for i in range(n)]
        if split:
            return [(names[i].value.decode(), float(ms[i]), int(by[i]), int(fl[i]), int(fv[i])) for i in range(n)]
        return [(names[i].value.decode(), float(ms[i]), int(by[i]), int(fl[i])) for i in range(n)]


def get_pose_net(cfg, is_train=False, cfg_arch=None, storage=None):
    """pose_mobilenet.py:158-176.  Pre-trained backbone loading (is_train and
    INIT_WEIGHTS) is a training feature and out of scope: weights always arrive through
    ``load_state_dict`` (valid.py:155-157).  ``storage`` (extension): see ``LitePose``."""
    return LitePose(cfg, cfg_arch=cfg_arch, storage=storage)


# ---- the trainable module ----------------------------------------------------------------------------------------
def _round8(v):
    """Channel counts are multiples of 8: the nearest one, but never more than 10 % below ``v``."""
    r = max(8, int(v + 4) // 8 * 8)
    return r + 8 if r < 0.9 * v else r


def _conv(cin, cout, k, stride=1, groups=1):
    return torch.nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False)


class LayerWalk(object):
    """The layer walk of the trainable LitePose modules: ``walk(net, x)`` runs the network whose layers ``net`` holds
    (``first``, ``stage``, ``deconv_refined`` / ``deconv_raw`` / ``deconv_bnrelu``, ``final_refined`` / ``final_raw``,
    ``num_deconv_layers``) on the backend of ``self``.  A layer is anything with the attributes the walk reads: the torch
    modules of ``TrainableLitePose``, or the per-step views of the supernet's tensors that
    ``pose_supermobilenet.TrainableSuperLitePose`` builds."""

    sync_bn_group = None        # convert_sync_batchnorm sets the instance's: the process group of its BatchNorm statistics

    # ---- layers ----
    def _conv(self, x, conv):
        k, groups = conv.kernel_size[0], conv.groups
        if self.backend == 'native' and k == 1 and groups == 1:
            return F_.pointwise(x, conv.weight)
        if self.backend == 'native' and groups == conv.in_channels == conv.out_channels and groups > 1:
            return F_.depthwise(x, conv.weight, conv.stride[0])
        if self.backend == 'native' and conv is self.first[0][0] and not x.requires_grad:
            return F_.stem_conv(x, conv.weight)
        return torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding, 1, groups)

    def _up_pair(self, refined, w_refined, raw, w_raw):
        if self.backend == 'native':
            return F_.deconv_pair(refined, w_refined, raw, w_raw)
        up = torch.nn.functional.conv_transpose2d
        return up(refined, w_refined, None, 2, 1) + up(raw, w_raw, None, 2, 1)

    def _bn(self, x, bn, act=None, residual=None):
        if self.training:
            bn.num_batches_tracked += 1
        if self.backend == 'native':
            return F_.batch_norm_act(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, act, residual, self.training,
                                     bn.momentum, bn.eps, self.sync_bn_group)
        y = torch.nn.functional.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training,
                                           bn.momentum, bn.eps)
        if act == 'relu6':
            y = torch.nn.functional.relu6(y)
        elif act == 'relu':
            y = torch.relu(y)
        return y if residual is None else y + residual

    def _block(self, x, blk):
        y = self._bn(self._conv(x, blk.inv[0]), blk.inv[1], 'relu6')
        y = self._bn(self._conv(y, blk.depth_conv[0]), blk.depth_conv[1], 'relu6')
        return self._bn(self._conv(y, blk.point_conv[0]), blk.point_conv[1], None, x if blk.residual else None)

    def _head(self, x, head):
        c = head.conv
        return self._conv(self._bn(self._conv(x, c[0]), c[1], 'relu'), c[3])

    def walk(self, net, x):
        f = net.first
        x = self._bn(self._conv(x, f[0][0]), f[0][1], 'relu6')
        x = self._bn(self._conv(x, f[1][0]), f[1][1], 'relu6')
        x = self._bn(self._conv(x, f[2]), f[3])
        feats = [x]
        for blocks in net.stage:
            for blk in blocks:
                x = self._block(x, blk)
            feats.append(x)
        outputs = []
        refined, raw = feats[-1], feats[-2]
        for i in range(net.num_deconv_layers):
            y = self._up_pair(refined, net.deconv_refined[i].weight, raw, net.deconv_raw[i].weight)
            refined = self._bn(y, net.deconv_bnrelu[i][0], 'relu')
            raw = feats[-i - 3]
            if i > 0:
                outputs.append(self._head(refined, net.final_refined[i - 1]) + self._head(raw, net.final_raw[i - 1]))
        return outputs


class TrainableLitePose(LayerWalk, torch.nn.Module):
    """LitePose as a ``torch.nn.Module`` whose parameters and buffers carry the names and shapes of ``LitePose.keys()``
    (``load_state_dict`` of a reference checkpoint and of ``LitePose.state_dict()`` both work) and whose ``forward`` returns
    the list of stage outputs, for ``core.trainer.do_train``.

    ``backend='native'``: every layer runs on ``litepose_amd.nn.functional`` -- the library's kernels, forward and
    backward: the 1x1 and depthwise convolutions, every BatchNorm (+ activation, + residual), the dense 3x3 stem
    convolution ``first.0.0`` (``stem_conv``) and the ``ConvTranspose2d`` pairs of the Fusion Deconv Head
    (``deconv_pair``).  No sum in it is atomic: one step gives the same bits every time, for every parameter; with
    ``litepose_amd.optim`` the optimizer is the library's as well.  One exception: the library has no data gradient for the stem, so when the image itself requires
    a gradient ``first.0.0`` runs on torch's ``conv2d``.  float32 on the GPU.
    ``backend='torch'``: every layer on torch's ops: the same module on any device and dtype.

    The modules below only hold parameters under the checkpoint's names; ``forward`` walks them layer by layer."""

    def __init__(self, cfg, cfg_arch, backend='native'):
        super().__init__()
        if backend not in ('native', 'torch'):
            raise ValueError("backend must be 'native' or 'torch'")
        nn = torch.nn
        self.backend = backend
        self._cfg, self._cfg_arch = cfg, cfg_arch
        c_in = _round8(cfg_arch['input_channel'])
        self.first = nn.Sequential(
            nn.Sequential(_conv(3, 32, 3, 2), nn.BatchNorm2d(32), nn.ReLU6()),
            nn.Sequential(_conv(32, 32, 3, 1, 32), nn.BatchNorm2d(32), nn.ReLU6()),
            _conv(32, c_in, 1), nn.BatchNorm2d(c_in))
        channels = [c_in]
        stages = []
        for st in cfg_arch['backbone_setting']:
            c_out = _round8(st['channel'])
            blocks = []
            for b in range(int(st['num_blocks'])):
                t, k = st['block_setting'][b]
                stride = int(st['stride']) if b == 0 else 1
                mid = _round8(round(c_in * t))
                blk = nn.Module()
                blk.inv = nn.Sequential(_conv(c_in, mid, 1), nn.BatchNorm2d(mid), nn.ReLU6())
                blk.depth_conv = nn.Sequential(_conv(mid, mid, int(k), stride, mid), nn.BatchNorm2d(mid), nn.ReLU6())
                blk.point_conv = nn.Sequential(_conv(mid, c_out, 1), nn.BatchNorm2d(c_out))
                blk.stride, blk.residual = stride, stride == 1 and c_in == c_out
                blocks.append(blk)
                c_in = c_out
            stages.append(nn.ModuleList(blocks))
            channels.append(c_out)
        self.stage = nn.ModuleList(stages)
        extra = cfg.MODEL.EXTRA
        self.num_deconv_layers = int(extra.NUM_DECONV_LAYERS)
        if any(int(k) != 4 for k in extra.NUM_DECONV_KERNELS[:self.num_deconv_layers]):
            raise ValueError('only NUM_DECONV_KERNELS == 4 is supported on this path')
        filters = [int(f) for f in cfg_arch['deconv_setting']]
        refined, raw, bnrelu = [], [], []
        planes_in = channels[-1]
        for i in range(self.num_deconv_layers):
            refined.append(nn.ConvTranspose2d(planes_in, filters[i], 4, 2, 1, bias=False))
            raw.append(nn.ConvTranspose2d(channels[-i - 2], filters[i], 4, 2, 1, bias=False))
            bnrelu.append(nn.Sequential(nn.BatchNorm2d(filters[i]), nn.ReLU()))
            planes_in = filters[i]
        self.deconv_refined, self.deconv_raw = nn.ModuleList(refined), nn.ModuleList(raw)
        self.deconv_bnrelu = nn.ModuleList(bnrelu)
        J = int(cfg.MODEL.NUM_JOINTS)
        dim_tag = J if cfg.MODEL.TAG_PER_JOINT else 1
        f_refined, f_raw, self.final_channel = [], [], []
        for i in range(1, self.num_deconv_layers):
            out = (J if cfg.LOSS.WITH_HEATMAPS_LOSS[i - 1] else 0) + (dim_tag if cfg.LOSS.WITH_AE_LOSS[i - 1] else 0)
            for lst, c in ((f_refined, filters[i]), (f_raw, channels[-i - 3])):
                head = nn.Module()
                head.conv = nn.Sequential(_conv(c, c, 5, 1, c), nn.BatchNorm2d(c), nn.ReLU(), _conv(c, out, 1))
                lst.append(head)
            self.final_channel.append(out)
        self.final_refined, self.final_raw = nn.ModuleList(f_refined), nn.ModuleList(f_raw)
        self.channel = channels

    def forward(self, x):
        return self.walk(self, x)

    def to_engine(self, storage=None):
        """A ``LitePose`` inference handle loaded from this module's ``state_dict``: validation on the inference path."""
        net = LitePose(self._cfg, cfg_arch=self._cfg_arch, storage=storage)
        net.load_state_dict(self.state_dict())
        return net


def convert_sync_batchnorm(model, group=None):
    """The counterpart of ``nn.SyncBatchNorm.convert_sync_batchnorm`` (dist_train.py:260, ``MODEL.SYNC_BN``) for a native
    ``TrainableLitePose``: from now on every BatchNorm of a training-mode forward takes its statistics over the batches of
    all ranks of ``group`` (``nn.functional.batch_norm_act(group=...)``; two all-gathers of one fp64 row per layer and
    step).  ``group=None``: the default process group as it is at this call.  Returns ``model``; its modules, parameters
    and ``state_dict`` are unchanged (the group is a plain attribute, ``model.sync_bn_group``), eval mode is unchanged.

    ``backend='torch'`` raises ValueError: those layers are torch's own, use ``torch.nn.SyncBatchNorm.
    convert_sync_batchnorm`` on them."""
    import torch.distributed as dist
    if not isinstance(model, LayerWalk) or not isinstance(model, torch.nn.Module):
        raise TypeError('convert_sync_batchnorm takes a TrainableLitePose, got %s' % type(model).__name__)
    if model.backend != 'native':
        raise ValueError("convert_sync_batchnorm is for backend='native'; a backend='torch' module holds torch's own "
                         'BatchNorm2d layers: use torch.nn.SyncBatchNorm.convert_sync_batchnorm')
    if group is None:
        if not dist.is_initialized():
            raise RuntimeError('convert_sync_batchnorm: group=None needs an initialised default process group')
        group = dist.group.WORLD
    model.sync_bn_group = group
    return model


def get_train_net(cfg, cfg_arch, backend='native'):
    """The trainable counterpart of ``get_pose_net``: a ``TrainableLitePose`` (initialised as torch initialises its
    layers; weights usually arrive through ``load_state_dict``)."""
    return TrainableLitePose(cfg, cfg_arch, backend)
