"""Drop-in for ``models.pose_supermobilenet`` (reference lib/models/pose_supermobilenet.py, layers/super_layers.py,
arch_manager.py): the weight-sharing supernet as the evaluation side of the architecture search uses it
(valid.py:139-145, calibrate_test.py:44-122).

``SuperLitePose`` holds the supernet checkpoint on the host.  ``sub_state_dict(cfg_arch)`` slices it to a sub-network,
which is an ordinary ``pose_mobilenet``; ``calibrate(cfg_arch, batches)`` runs the calibration images through that
sub-network in training mode ON THE DEVICE (lp_calib_*: every BatchNorm normalises with the batch statistics and moves
its running pair), returns the calibrated state dict and writes the moved statistics back into the supernet's own
tensors -- the reference's slices are views, so calibrating one architecture changes what the next one starts from.
The result goes to ``PoseEngine(cfg, cfg_arch, state_dict)`` / ``pose_mobilenet`` like any other checkpoint.
"""
import ctypes as C
import random
import types
from collections import OrderedDict

import torch
import torch.nn.functional as F

from .. import _native as nv
from ..nn import functional as F_
from . import pose_mobilenet

INPUT_CHANNEL = 24
# t, c, n, s (pose_supermobilenet.py:27-33); every block is built for expansion 6 and a 7x7 depthwise
SETTING = [[6, 32, 6, 2], [6, 64, 8, 2], [6, 96, 10, 2], [6, 160, 10, 1]]


def _make_divisible(v, divisor=8, min_value=None):
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


class ArchManager(object):
    """arch_manager.py:18-89: the search space of the supernet and its two samplers."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.expansion = [6]
        self.kernel_size = [7]
        self.input_channel = 24
        self.width_mult = [1.0, 0.75, 0.5, 0.25]
        self.deconv_setting = [int(f) for f in cfg.MODEL.EXTRA.NUM_DECONV_FILTERS]
        self.is_search = False
        self.search_arch = None
        self.arch_setting = [[32, 4, 2], [64, 6, 2], [96, 8, 2], [160, 8, 1]]      # c, n, s

    def rand_channel(self, c):
        return _make_divisible(c * self.width_mult[random.randint(0, len(self.width_mult) - 1)], 8)

    def _sample(self, reso, channel):
        arch = {'img_size': reso, 'input_channel': channel(self.input_channel),
                'deconv_setting': [channel(f) for f in self.deconv_setting], 'backbone_setting': []}
        for c, n, s in self.arch_setting:
            arch['backbone_setting'].append({'num_blocks': n, 'stride': s, 'channel': channel(c),
                                             'block_setting': [[6, 7] for _ in range(n)]})
        return arch

    def random_sample(self):
        if self.is_search:
            return self.search_arch
        # the reference draws img_size, input_channel, the deconv widths and then the stage widths, in this order
        return self._sample(256 + 64 * random.randint(0, 4), self.rand_channel)

    def fixed_sample(self, reso=256, ratio=0.5):
        return self._sample(reso, lambda c: _make_divisible(c * ratio, 8))


def _bn_keys(o, p, c):
    for k in ('weight', 'bias', 'running_mean', 'running_var'):
        o[p + '.' + k] = (c,)
    o[p + '.num_batches_tracked'] = ()


class Calibration(object):
    """One open calibration on a ``pose_mobilenet.LitePose`` handle (lp_calib_begin ... lp_calib_end)."""

    def __init__(self, net, momentum=0.1):
        self.net = net
        self._lib = nv.lib()
        self._ws = None
        nv.check(self._lib.lp_calib_begin(net._h, float(momentum)), 'lp_calib_begin')

    def step(self, x):
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('expected a float32 [N,3,H,W] tensor')
        x = x.contiguous()
        n, _, h, w = x.shape
        need = int(self._lib.lp_calib_workspace_bytes(self.net._h, n, h, w))
        if need == 0:
            raise nv.LitePoseNativeError('lp_calib_workspace_bytes: ' + self._lib.lp_last_error().decode())
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        nv.check(self._lib.lp_calib_step(self.net._h, nv.dptr(x), n, h, w, nv.dptr(self._ws), need, nv.stream_ptr()),
                 'lp_calib_step')

    def read(self, prefix, channels, device):
        """(running_mean, running_var) of the BatchNorm ``prefix`` as they stand on the device."""
        m = torch.empty(channels, dtype=torch.float32, device=device)
        v = torch.empty(channels, dtype=torch.float32, device=device)
        nv.check(self._lib.lp_calib_read(self.net._h, prefix.encode(), nv.dptr(m), nv.dptr(v), channels,
                                         nv.stream_ptr()), 'lp_calib_read')
        return m, v

    def end(self):
        steps = C.c_int64()
        nv.check(self._lib.lp_calib_end(self.net._h, C.byref(steps)), 'lp_calib_end')
        return int(steps.value)


class SuperLitePose(object):
    def __init__(self, cfg, width_mult=1.0, round_nearest=8):
        if width_mult != 1.0 or round_nearest != 8:
            raise ValueError('width_mult/round_nearest other than the defaults are not on the path')
        self.cfg = cfg
        self.arch_manager = ArchManager(cfg)
        extra = cfg.MODEL.EXTRA
        if int(extra.NUM_DECONV_LAYERS) != 3 or any(int(k) != 4 for k in extra.NUM_DECONV_KERNELS[:3]):
            raise ValueError('the path is built for three deconv layers of kernel 4')
        self.filters = [int(f) for f in extra.NUM_DECONV_FILTERS[:3]]
        self.channel = [INPUT_CHANNEL]
        self.stages = []
        inp = INPUT_CHANNEL
        for t, c, n, s in SETTING:
            blocks = []
            for b in range(n):
                blocks.append(dict(inp=inp, feat=round(inp * 6), oup=c, stride=s if b == 0 else 1))
                inp = c
            self.stages.append(blocks)
            self.channel.append(c)
        dim_tag = cfg.MODEL.NUM_JOINTS if cfg.MODEL.TAG_PER_JOINT else 1
        self.final_channel = [(cfg.MODEL.NUM_JOINTS if cfg.LOSS.WITH_HEATMAPS_LOSS[i - 1] else 0) +
                              (dim_tag if cfg.LOSS.WITH_AE_LOSS[i - 1] else 0) for i in range(1, 3)]
        self._shapes = self._key_shapes()
        self._sd = None
        self.training = False
        self.calibrated_net = None          # the pose_mobilenet handle of the last calibrate()

    # ---- key scheme (registration order of the reference module) -------------------
    def _deconv_in(self, i):
        return (self.channel[-1] if i == 0 else self.filters[i - 1]), self.channel[-i - 2]

    def _key_shapes(self):
        o = OrderedDict()
        o['first.0.0.weight'] = (32, 3, 3, 3)
        _bn_keys(o, 'first.0.1', 32)
        o['first.1.0.weight'] = (32, 1, 3, 3)
        _bn_keys(o, 'first.1.1', 32)
        o['first.2.weight'] = (INPUT_CHANNEL, 32, 1, 1)
        _bn_keys(o, 'first.3', INPUT_CHANNEL)
        for s, blocks in enumerate(self.stages):
            for b, blk in enumerate(blocks):
                p = 'stage.%d.%d' % (s, b)
                o[p + '.inv.0.weight'] = (blk['feat'], blk['inp'], 1, 1)
                _bn_keys(o, p + '.inv.1', blk['feat'])
                o[p + '.depth_conv.0.weight'] = (blk['feat'], 1, 7, 7)
                _bn_keys(o, p + '.depth_conv.1', blk['feat'])
                o[p + '.point_conv.0.weight'] = (blk['oup'], blk['feat'], 1, 1)
                _bn_keys(o, p + '.point_conv.1', blk['oup'])
                o[p + '.Linear5x5.weight'] = (25, 25)
                o[p + '.Linear5x5.bias'] = (25,)
                o[p + '.Linear3x3.weight'] = (9, 9)
                o[p + '.Linear3x3.bias'] = (9,)
        for which in (0, 1):
            for i in range(3):
                o['%s.%d.weight' % (('deconv_refined', 'deconv_raw')[which], i)] = \
                    (self._deconv_in(i)[which], self.filters[i], 4, 4)
        for i in range(3):
            _bn_keys(o, 'deconv_bnrelu.%d.0' % i, self.filters[i])
        for which in (0, 1):
            for i in range(1, 3):
                cin = self.filters[i] if which == 0 else self.channel[-i - 3]
                p = '%s.%d.conv' % (('final_refined', 'final_raw')[which], i - 1)
                o[p + '.0.weight'] = (cin, 1, 5, 5)
                _bn_keys(o, p + '.1', cin)
                o[p + '.3.weight'] = (self.final_channel[i - 1], cin, 1, 1)
        return o

    def keys(self):
        return list(self._shapes.items())

    # ---- nn.Module-shaped surface ---------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def cuda(self, device=None):
        return self

    def to(self, *a, **k):
        return self

    def load_state_dict(self, state_dict, strict=True):
        given = OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in state_dict.items())
        missing = [k for k in self._shapes if k not in given]
        unexpected = [k for k in given if k not in self._shapes]
        if strict and (missing or unexpected):
            raise RuntimeError('Error(s) in loading state_dict for SuperLitePose: missing %s unexpected %s'
                               % (missing[:5], unexpected[:5]))
        if missing:
            raise RuntimeError('SuperLitePose needs every tensor of the supernet (weights always arrive through '
                               'load_state_dict): missing %s' % missing[:5])
        sd = OrderedDict()
        for k, shp in self._shapes.items():
            t = torch.as_tensor(given[k]).detach().to('cpu')
            if tuple(t.shape) != shp:
                raise RuntimeError('size mismatch for %s: %s vs %s' % (k, tuple(t.shape), shp))
            sd[k] = t.to(torch.int64).clone() if k.endswith('num_batches_tracked') else t.to(torch.float32).clone()
        self._sd = sd
        return self

    def state_dict(self):
        self._loaded()
        return OrderedDict((k, v.clone()) for k, v in self._sd.items())

    def _loaded(self):
        if self._sd is None:
            raise nv.LitePoseNativeError('load_state_dict() has not been called')

    def forward(self, x):
        raise NotImplementedError('this host-side supernet is not run: slice it (sub_state_dict) or calibrate() a '
                                  'sub-network and run that as pose_mobilenet; the supernet that runs and trains is '
                                  'get_train_net(cfg)')

    __call__ = forward

    # ---- slicing (layers/super_layers.py) -------------------------------------------------
    def _sub_plan(self, cfg_arch):
        """Channel bookkeeping of the sub-network, checked against what the supernet holds."""
        bs = cfg_arch['backbone_setting']
        if len(bs) != len(self.stages):
            raise ValueError('cfg_arch has %d stages, the supernet %d' % (len(bs), len(self.stages)))

        def width(name, c, cap):
            c = int(c)
            if c < 8 or c % 8:
                raise ValueError('%s = %d: widths are positive multiples of 8' % (name, c))
            if c > cap:
                raise ValueError('%s = %d is wider than the supernet (%d)' % (name, c, cap))
            return c

        c0 = width('input_channel', cfg_arch['input_channel'], INPUT_CHANNEL)
        stages, inp = [], c0
        for s, st in enumerate(bs):
            n = int(st['num_blocks'])
            if n < 1 or n > len(self.stages[s]):
                raise ValueError('stage %d: %d blocks, the supernet holds %d' % (s, n, len(self.stages[s])))
            if int(st['stride']) != self.stages[s][0]['stride']:
                raise ValueError('stage %d: stride %s differs from the supernet' % (s, st['stride']))
            c = width('stage %d channel' % s, st['channel'], self.stages[s][0]['oup'])
            blocks = []
            for b in range(n):
                t, k = st['block_setting'][b]
                sup = self.stages[s][b]
                mid = round(inp * t)
                if int(k) not in (3, 5, 7):
                    raise ValueError('stage %d block %d: kernel %s (3, 5 or 7)' % (s, b, k))
                if mid < 8 or mid > sup['feat'] or _make_divisible(mid, 8) != mid:
                    raise ValueError('stage %d block %d: expanded width %d (a multiple of 8, at most %d)'
                                     % (s, b, mid, sup['feat']))
                # the supernet's residual rule looks at ITS widths, pose_mobilenet's at the sub-network's
                if (sup['stride'] == 1 and sup['inp'] == sup['oup']) != (sup['stride'] == 1 and inp == c):
                    raise ValueError('stage %d block %d: the sub-network would add a residual the supernet does not'
                                     % (s, b))
                blocks.append(dict(inp=inp, mid=mid, oup=c, k=int(k)))
                inp = c
            stages.append(blocks)
        ds = list(cfg_arch['deconv_setting'])[:3]
        if len(ds) != 3:
            raise ValueError('deconv_setting needs three widths')
        filters = [width('deconv_setting[%d]' % i, f, self.filters[i]) for i, f in enumerate(ds)]
        channel = [c0] + [blk[-1]['oup'] for blk in stages]
        return dict(c0=c0, stages=stages, filters=filters, channel=channel)

    def _bn_prefixes(self, plan):
        """(prefix, channels) of every BatchNorm of the sub-network."""
        L = [('first.0.1', 32), ('first.1.1', 32), ('first.3', plan['c0'])]
        for s, blocks in enumerate(plan['stages']):
            for b, blk in enumerate(blocks):
                p = 'stage.%d.%d' % (s, b)
                L += [(p + '.inv.1', blk['mid']), (p + '.depth_conv.1', blk['mid']), (p + '.point_conv.1', blk['oup'])]
        for i in range(3):
            L.append(('deconv_bnrelu.%d.0' % i, plan['filters'][i]))
        for i in range(1, 3):
            L.append(('final_refined.%d.conv.1' % (i - 1), plan['filters'][i]))
            L.append(('final_raw.%d.conv.1' % (i - 1), plan['channel'][-i - 3]))
        return L

    def sub_state_dict(self, cfg_arch):
        """The sub-network ``cfg_arch`` as a strict ``pose_mobilenet`` state dict (copies)."""
        self._loaded()
        plan = self._sub_plan(cfg_arch)
        sd, out = self._sd, OrderedDict()

        def bn(p, c):
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                out[p + '.' + k] = sd[p + '.' + k][:c].clone()
            out[p + '.num_batches_tracked'] = sd[p + '.num_batches_tracked'].clone()

        out['first.0.0.weight'] = sd['first.0.0.weight'].clone()
        bn('first.0.1', 32)
        out['first.1.0.weight'] = sd['first.1.0.weight'].clone()
        bn('first.1.1', 32)
        out['first.2.weight'] = sd['first.2.weight'][:plan['c0'], :32].clone()            # SuperConv2d: [:out, :in]
        bn('first.3', plan['c0'])
        for s, blocks in enumerate(plan['stages']):
            for b, blk in enumerate(blocks):
                p = 'stage.%d.%d' % (s, b)
                mid, k = blk['mid'], blk['k']
                out[p + '.inv.0.weight'] = sd[p + '.inv.0.weight'][:mid, :blk['inp']].clone()
                bn(p + '.inv.1', mid)
                l, r = 3 - k // 2, 3 + k // 2 + 1
                w = sd[p + '.depth_conv.0.weight'][:mid, :, l:r, l:r]
                if k in (5, 3):          # the window transform: Linear5x5 / Linear3x3 on the flattened centre crop
                    name = p + ('.Linear5x5' if k == 5 else '.Linear3x3')
                    w = F.linear(w.reshape(mid, 1, -1), sd[name + '.weight'], sd[name + '.bias']).reshape(mid, 1, k, k)
                out[p + '.depth_conv.0.weight'] = w.clone()
                bn(p + '.depth_conv.1', mid)
                out[p + '.point_conv.0.weight'] = sd[p + '.point_conv.0.weight'][:blk['oup'], :mid].clone()
                bn(p + '.point_conv.1', blk['oup'])
        ch, fl = plan['channel'], plan['filters']
        for which in (0, 1):
            for i in range(3):
                cin = (ch[-1] if i == 0 else fl[i - 1]) if which == 0 else ch[-i - 2]
                key = '%s.%d.weight' % (('deconv_refined', 'deconv_raw')[which], i)
                out[key] = sd[key][:cin, :fl[i]].clone()                                  # SuperConvTranspose2d: [:in, :out]
        for i in range(3):
            bn('deconv_bnrelu.%d.0' % i, fl[i])
        for which in (0, 1):
            for i in range(1, 3):
                cin = fl[i] if which == 0 else ch[-i - 3]
                p = '%s.%d.conv' % (('final_refined', 'final_raw')[which], i - 1)
                out[p + '.0.weight'] = sd[p + '.0.weight'][:cin].clone()
                bn(p + '.1', cin)
                out[p + '.3.weight'] = sd[p + '.3.weight'][:self.final_channel[i - 1], :cin].clone()
        return out

    # ---- calibration (calibrate_test.py:57-61) ------------------------------------------------
    def calibrate(self, cfg_arch, batches, momentum=0.1, on_step=None):
        """Run ``batches`` (device float32 [N,3,H,W] tensors) through the sub-network in training mode on the device.
        Returns the calibrated ``pose_mobilenet`` state dict; the moved running statistics are written back into this
        supernet's tensors (prefix ``[:c]``), as the reference's view slices do.  ``on_step(i, calibration)`` is called
        after step ``i`` (``Calibration.read`` gives the running pairs as they stand)."""
        plan = self._sub_plan(cfg_arch)
        net = pose_mobilenet.LitePose(self.cfg, cfg_arch=cfg_arch, storage='f32')
        net.load_state_dict(self.sub_state_dict(cfg_arch), strict=True)
        cal = Calibration(net, momentum)
        try:
            for i, x in enumerate(batches):
                cal.step(x)
                if on_step is not None:
                    on_step(i, cal)
        except BaseException:
            try:                                # close the calibration, but the step's own error is the one to report
                cal.end()
            except nv.LitePoseNativeError:
                pass
            raise
        steps = cal.end()
        out = net.state_dict()
        for p, c in self._bn_prefixes(plan):
            for k in ('running_mean', 'running_var'):
                self._sd[p + '.' + k][:c] = out[p + '.' + k]
            # only the two plain BatchNorm2d of the stem count their batches: SuperBatchNorm2d.forward bypasses the counter
            if p in ('first.0.1', 'first.1.1'):
                self._sd[p + '.num_batches_tracked'] += steps
            out[p + '.num_batches_tracked'] = self._sd[p + '.num_batches_tracked'].clone()
        self.calibrated_net = net
        return out


def get_pose_net(cfg, is_train=False):
    """pose_supermobilenet.py:199-218: the supernet as the evaluation side uses it; weights arrive through
    ``load_state_dict``.  The training side -- the sampled forward, and the pre-trained initialisation with the channel
    re-ordering that follows it (is_train and INIT_WEIGHTS) -- is ``get_train_net``."""
    return SuperLitePose(cfg)


# ---- the trainable supernet -----------------------------------------------------------------------------------------
def _layer(**kw):
    return types.SimpleNamespace(**kw)


class TrainableSuperLitePose(pose_mobilenet.LayerWalk, torch.nn.Module):
    """The weight-sharing supernet as a ``torch.nn.Module`` (reference ``SuperLitePose``): its ``state_dict`` has exactly
    the keys and shapes of ``SuperLitePose.keys()``, so ``SuperLitePose(cfg).load_state_dict(module.state_dict())`` hands a
    trained supernet to calibration and search.

    ``forward(x, cfg_arch=None)`` runs a sub-network whose parameters are slices of the supernet's
    (layers/super_layers.py): ``cfg_arch``, or ``self.arch_manager.random_sample()`` -- which honours ``is_search`` /
    ``search_arch`` -- left in ``last_arch``.  The layers are ``TrainableLitePose``'s walk on the sliced tensors.  BatchNorm
    running statistics are prefix views of the supernet's buffers and move in place; only the two plain BatchNorms of the
    stem advance ``num_batches_tracked`` (``SuperBatchNorm2d.forward`` bypasses the counter).  ``first.0`` and ``first.1``
    are not sliced.  A parameter the sampled sub-network does not touch keeps ``grad is None``.

    ``backend='native'``: the slices of every learnable tensor are gathered into one packed buffer by one library call and
    their gradients come back as full-size tensors, zero outside the slice, from one more
    (``nn.functional.subnet_params``); the descriptor table is built once per architecture, kept on the device, and
    rebuilt when a parameter's ``data_ptr()`` has changed.  float32 on the GPU.
    ``backend='torch'``: the same module on torch slicing, for any device and dtype."""

    def __init__(self, cfg, backend='native'):
        super().__init__()
        if backend not in ('native', 'torch'):
            raise ValueError("backend must be 'native' or 'torch'")
        nn, conv = torch.nn, pose_mobilenet._conv
        self.backend = backend
        self._cfg = cfg
        self._host = [SuperLitePose(cfg)]             # in a list: not a sub-module, never in the state_dict
        host = self._host[0]
        self.arch_manager = ArchManager(cfg)
        self.last_arch = None
        self.first = nn.Sequential(
            nn.Sequential(conv(3, 32, 3, 2), nn.BatchNorm2d(32), nn.ReLU6()),
            nn.Sequential(conv(32, 32, 3, 1, 32), nn.BatchNorm2d(32), nn.ReLU6()),
            conv(32, INPUT_CHANNEL, 1), nn.BatchNorm2d(INPUT_CHANNEL))
        stages = []
        for blocks in host.stages:
            mods = []
            for b in blocks:
                blk = nn.Module()
                feat = b['feat']
                blk.inv = nn.Sequential(conv(b['inp'], feat, 1), nn.BatchNorm2d(feat), nn.ReLU6())
                blk.depth_conv = nn.Sequential(conv(feat, feat, 7, b['stride'], feat), nn.BatchNorm2d(feat), nn.ReLU6())
                blk.point_conv = nn.Sequential(conv(feat, b['oup'], 1), nn.BatchNorm2d(b['oup']))
                blk.Linear5x5, blk.Linear3x3 = nn.Linear(25, 25), nn.Linear(9, 9)
                blk.stride, blk.residual = b['stride'], b['stride'] == 1 and b['inp'] == b['oup']
                mods.append(blk)
            stages.append(nn.Sequential(*mods))
        self.stage = nn.ModuleList(stages)
        up = lambda cin, cout: nn.ConvTranspose2d(cin, cout, 4, 2, 1, bias=False)  # noqa: E731
        self.deconv_refined = nn.ModuleList([up(host._deconv_in(i)[0], host.filters[i]) for i in range(3)])
        self.deconv_raw = nn.ModuleList([up(host._deconv_in(i)[1], host.filters[i]) for i in range(3)])
        self.deconv_bnrelu = nn.ModuleList([nn.Sequential(nn.BatchNorm2d(f), nn.ReLU()) for f in host.filters])
        self.num_deconv_layers = 3
        self.final_channel = list(host.final_channel)
        f_refined, f_raw = [], []
        for i in range(1, 3):
            for lst, c in ((f_refined, host.filters[i]), (f_raw, host.channel[-i - 3])):
                head = nn.Module()
                head.conv = nn.Sequential(conv(c, c, 5, 1, c), nn.BatchNorm2d(c), nn.ReLU(),
                                          conv(c, self.final_channel[i - 1], 1))
                lst.append(head)
        self.final_refined, self.final_raw = nn.ModuleList(f_refined), nn.ModuleList(f_raw)
        self._tables = {}

    # ---- the sub-network: one description for the descriptor table, the torch slices and the per-step layers ----
    def _assemble(self, plan, take):
        """The layers of the sub-network ``plan`` for ``LayerWalk.walk``.  ``take(spec)`` hands out the sliced tensor of one
        learnable tensor (``SubnetTable`` has the fields of ``spec``); the calls come in one fixed order."""
        def pw(m, out, inn):
            w = take(dict(param=m.weight, kind=0, rows=out, cols=inn, shape=(out, inn, 1, 1)))
            return _layer(weight=w, kernel_size=(1, 1), groups=1, in_channels=inn, out_channels=out, stride=(1, 1),
                          padding=(0, 0))

        def dw(w, c, k, stride):
            return _layer(weight=w, kernel_size=(k, k), groups=c, in_channels=c, out_channels=c, stride=(stride, stride),
                          padding=(k // 2, k // 2))

        def bn(m, c):
            return _layer(weight=take(dict(param=m.weight, kind=1, rows=c, shape=(c,))),
                          bias=take(dict(param=m.bias, kind=1, rows=c, shape=(c,))),
                          running_mean=m.running_mean[:c], running_var=m.running_var[:c], momentum=m.momentum, eps=m.eps,
                          num_batches_tracked=0)        # SuperBatchNorm2d does not count its batches

        def up(m, inn, out):
            return _layer(weight=take(dict(param=m.weight, kind=0, rows=inn, cols=out, shape=(inn, out, 4, 4))))

        f = self.first
        net = _layer(first=[f[0], f[1], pw(f[2], plan['c0'], 32), bn(f[3], plan['c0'])], stage=[],
                     num_deconv_layers=3)
        for s, blocks in enumerate(plan['stages']):
            layers = []
            for b, blk in enumerate(blocks):
                m, mid, k = self.stage[s][b], blk['mid'], blk['k']
                inv = [pw(m.inv[0], mid, blk['inp']), bn(m.inv[1], mid)]
                lin = None if k == 7 else (m.Linear5x5 if k == 5 else m.Linear3x3)
                w = take(dict(param=m.depth_conv[0].weight, kind=2, rows=mid, cols=k, shape=(mid, 1, k, k),
                              lin_w=None if lin is None else lin.weight, lin_b=None if lin is None else lin.bias))
                depth = [dw(w, mid, k, m.stride), bn(m.depth_conv[1], mid)]
                point = [pw(m.point_conv[0], blk['oup'], mid), bn(m.point_conv[1], blk['oup'])]
                layers.append(_layer(inv=inv, depth_conv=depth, point_conv=point, stride=m.stride, residual=m.residual))
            net.stage.append(layers)
        ch, fl = plan['channel'], plan['filters']
        net.deconv_refined = [up(self.deconv_refined[i], ch[-1] if i == 0 else fl[i - 1], fl[i]) for i in range(3)]
        net.deconv_raw = [up(self.deconv_raw[i], ch[-i - 2], fl[i]) for i in range(3)]
        net.deconv_bnrelu = [[bn(self.deconv_bnrelu[i][0], fl[i])] for i in range(3)]
        net.final_refined, net.final_raw = [], []
        for i in range(1, 3):
            for lst, mods, c in ((net.final_refined, self.final_refined, fl[i]), (net.final_raw, self.final_raw, ch[-i - 3])):
                m = mods[i - 1].conv
                w = take(dict(param=m[0].weight, kind=1, rows=c * 25, shape=(c, 1, 5, 5)))
                lst.append(_layer(conv=[dw(w, c, 5, 1), bn(m[1], c), None, pw(m[3], self.final_channel[i - 1], c)]))
        return net

    @staticmethod
    def _torch_slice(spec):
        p, shape = spec['param'], spec['shape']
        if spec['kind'] == 0:
            return p[:spec['rows'], :spec['cols']]
        if spec['kind'] == 1:
            return p[:shape[0]]
        k = spec['cols']
        l, r = 3 - k // 2, 3 + k // 2 + 1
        w = p[:spec['rows'], :, l:r, l:r]
        if k != 7:                     # the window transform: Linear5x5 / Linear3x3 on the flattened centre crop
            w = F.linear(w.reshape(shape[0], 1, -1), spec['lin_w'], spec['lin_b']).reshape(shape)
        return w

    def _table(self, cfg_arch, plan):
        key = repr(plan)
        table = self._tables.get(key)
        device = self.first[2].weight.device
        if table is None or table.device != device or table.stale():
            specs = []
            self._assemble(plan, specs.append)
            table = self._tables[key] = F_.SubnetTable(specs, device)
        return table

    def forward(self, x, cfg_arch=None):
        if cfg_arch is None:
            cfg_arch = self.arch_manager.random_sample()
            if cfg_arch is None:
                raise ValueError('arch_manager.is_search is set without a search_arch')
        self.last_arch = cfg_arch
        plan = self._host[0]._sub_plan(cfg_arch)
        if self.backend == 'native':
            table = self._table(cfg_arch, plan)
            views = iter(F_.subnet_params(table, *table.params))
            net = self._assemble(plan, lambda spec: next(views))
        else:
            net = self._assemble(plan, self._torch_slice)
        return self.walk(net, x)

    # ---- initialisation from a pre-trained backbone (pose_supermobilenet.py:167-218) ----
    @torch.no_grad()
    def re_organize_weights(self):
        """Re-order the channels between layers by importance -- the L1 norm of the weights the NEXT layer puts on them,
        descending -- so that a prefix slice keeps the channels that matter most: the output of ``first.2`` / ``first.3``
        by ``stage.0.0.inv``, and the output of every stage but the last by the first expansion of the next (every
        block's ``point_conv`` and, behind the first block, the residual blocks' ``inv`` input follow).  Returns the list of
        permutations, in that order."""
        def reorder(t, dim, idx):
            t.data = torch.index_select(t.data, dim, idx)

        def reorder_bn(bn, idx):
            for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
                reorder(t, 0, idx)

        def importance(w):
            return torch.sort(w.data.abs().sum(dim=(0, 2, 3)), dim=0, descending=True)[1]

        perms = []
        nxt = self.stage[0][0].inv[0].weight
        idx = importance(nxt)
        reorder(self.first[2].weight, 0, idx)
        reorder_bn(self.first[3], idx)
        reorder(nxt, 1, idx)
        perms.append(idx)
        for s in range(len(self.stage) - 1):
            nxt = self.stage[s + 1][0].inv[0].weight
            idx = importance(nxt)
            reorder(nxt, 1, idx)
            for b, blk in enumerate(self.stage[s]):
                reorder_bn(blk.point_conv[1], idx)
                reorder(blk.point_conv[0].weight, 0, idx)
                if b > 0:
                    reorder(blk.inv[0].weight, 1, idx)
            perms.append(idx)
        self._tables = {}
        return perms


def get_train_net(cfg, backend='native', init_from=None):
    """The trainable counterpart of ``get_pose_net``: a ``TrainableSuperLitePose``.  ``init_from``: the state dict of a
    pre-trained backbone (the reference's ``is_train and INIT_WEIGHTS`` path): its ``final*`` and ``deconv*`` tensors are
    dropped, a ``module.`` prefix is stripped, the rest is loaded non-strictly and the channels are re-organised."""
    model = TrainableSuperLitePose(cfg, backend)
    if init_from is not None:
        keep = OrderedDict()
        for k, v in init_from.items():
            if 'final' in k or 'deconv' in k:
                continue
            keep[k[7:] if 'module' in k else k] = v
        model.load_state_dict(keep, strict=False)
        model.re_organize_weights()
    return model
