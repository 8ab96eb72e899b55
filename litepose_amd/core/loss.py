"""Drop-in for lib/core/loss.py on the device: ``HeatmapLoss``, ``AELoss`` and ``MultiLossFactory`` with the reference's
call signatures and return shapes, every term one ``lp_pose_loss`` call (include/litepose_amd.h, "training loss").

The values are what ``do_train`` logs and sums (lib/core/trainer.py:75-105), the loss against teacher heatmaps (the same
call with other targets), and a dense score of a search candidate.  The device arithmetic is fp64 on the fp32 inputs with
one rounding per result, so a value may differ from the reference's fp32 evaluation by that evaluation's own rounding
error.

On a stage output that requires grad (and with grad enabled) the three terms are differentiable with respect to that
output: ``loss.backward()`` reaches it through one ``lp_pose_loss_grad`` call per ``pose_loss`` call (``pose_loss_grad``;
a term that takes no part in the loss arrives as None and goes to the device as NULL).  Targets, masks and joints get no
gradient.  The same fixed-order arithmetic: where several joints share a tag cell, the cell's gradient is their sum in
(person, joint) order, not the unordered atomic sum of the backward of ``torch.gather``.  Without grad the calls are the
forward calls alone and the results carry no ``grad_fn``."""
import torch

from .. import _native as nv

LOSS_TYPES = {'exp': 0, 'max': 1}
# lib/config/default.py:97-104: the LOSS keys litepose_amd.config does not carry
LOSS_DEFAULTS = dict(HEATMAPS_LOSS_FACTOR=(1.0,), AE_LOSS_TYPE='max', PUSH_LOSS_FACTOR=(0.001,), PULL_LOSS_FACTOR=(0.001,))


def pose_loss(out, num_joints, tag_offset=-1, heat=None, mask=None, joints=None, loss_type='exp', heat_factor=1.0,
              push_factor=1.0, pull_factor=1.0, buffers=None):
    """One ``lp_pose_loss`` call on the stage output ``out`` float32 [N,C,R,R] -> (heat_loss [N] or None, push [N] or
    None, pull [N] or None).  ``heat`` [N,J,R,R] with ``mask`` [N,R,R]: the heatmap term; ``tag_offset`` >= 0 with
    ``joints`` int32 [N,M,J,2]: the tag terms on the channels from ``tag_offset``.  ``buffers``: a dict from
    ``loss_buffers`` to write into instead of allocating (the call is then capturable in a graph).  When ``out`` requires
    grad and grad is enabled the results are differentiable with respect to ``out`` (not with ``buffers``: kept buffers
    are overwritten by the next call, an autograd graph would outlive them)."""
    if out.requires_grad and torch.is_grad_enabled():
        if buffers is not None:
            raise ValueError('buffers= cannot be combined with an output that requires grad')
        return _PoseLoss.apply(out, num_joints, tag_offset, heat, mask, joints, loss_type, heat_factor, push_factor,
                               pull_factor)
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[2] != out.shape[3]:
        raise ValueError('expected a float32 [N,C,R,R] output')
    N, Cc, R = int(out.shape[0]), int(out.shape[1]), int(out.shape[2])
    J = int(num_joints)
    out = out.contiguous()
    if buffers is None:
        buffers = loss_buffers(N, J, R, out.device)
    elif buffers['shape'] != (N, J, R):
        raise ValueError('buffers were made for (N, J, R) = %s' % (buffers['shape'],))
    hl = push = pull = ws = None
    M = 1
    if heat is not None:
        if tuple(heat.shape) != (N, J, R, R) or heat.dtype != torch.float32:
            raise ValueError('heat must be float32 [N,J,R,R] of the output size')
        if mask is None or tuple(mask.shape) != (N, R, R) or mask.dtype != torch.float32:
            raise ValueError('mask must be float32 [N,R,R]')
        heat, mask = heat.contiguous(), mask.contiguous()
        hl, ws = buffers['heat'], buffers['workspace']
    else:
        mask = None
    if tag_offset >= 0:
        if joints is None or joints.dim() != 4 or joints.shape[0] != N or joints.shape[3] != 2 or \
                joints.dtype != torch.int32:
            raise ValueError('joints must be int32 [N,M,J,2]')
        joints = joints.contiguous()
        M = int(joints.shape[1])
        if int(joints.shape[2]) != J:
            raise ValueError('joints must hold %d joints per person' % J)
        push, pull = buffers['push'], buffers['pull']
    else:
        joints = None
    nv.check(nv.lib().lp_pose_loss(nv.dptr(out), N, Cc, R, J, int(tag_offset), nv.dptr(heat), nv.dptr(mask),
                                   nv.dptr(joints), M, LOSS_TYPES[loss_type], float(heat_factor), float(push_factor),
                                   float(pull_factor), nv.dptr(hl), nv.dptr(push), nv.dptr(pull), nv.dptr(ws),
                                   0 if ws is None else ws.numel(), nv.stream_ptr()), 'lp_pose_loss')
    return hl, push, pull


def pose_loss_grad(out, num_joints, tag_offset=-1, heat=None, mask=None, joints=None, loss_type='exp', heat_factor=1.0,
                   push_factor=1.0, pull_factor=1.0, g_heat=None, g_push=None, g_pull=None, grad_out=None):
    """One ``lp_pose_loss_grad`` call: the gradient of the terms of ``pose_loss`` (same arguments) with respect to ``out``,
    float32 [N,C,R,R], every element written.  ``g_heat``, ``g_push``, ``g_pull``: float32 [N] upstream gradients of the
    three results, None for a term that adds nothing.  ``grad_out``: a contiguous float32 tensor of ``out``'s shape to
    write into instead of allocating (the call is then capturable in a graph)."""
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[2] != out.shape[3]:
        raise ValueError('expected a float32 [N,C,R,R] output')
    N, Cc, R = int(out.shape[0]), int(out.shape[1]), int(out.shape[2])
    J = int(num_joints)
    out = out.detach().contiguous()
    if grad_out is None:
        grad_out = torch.empty((N, Cc, R, R), dtype=torch.float32, device=out.device)
    elif grad_out.shape != out.shape or grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
        raise ValueError('grad_out must be a contiguous float32 tensor of the shape of out')
    M = 1
    if heat is not None:
        if tuple(heat.shape) != (N, J, R, R) or heat.dtype != torch.float32:
            raise ValueError('heat must be float32 [N,J,R,R] of the output size')
        if mask is None or tuple(mask.shape) != (N, R, R) or mask.dtype != torch.float32:
            raise ValueError('mask must be float32 [N,R,R]')
        heat, mask = heat.contiguous(), mask.contiguous()
    else:
        mask = g_heat = None
    if tag_offset >= 0:
        if joints is None or joints.dim() != 4 or joints.shape[0] != N or joints.shape[3] != 2 or \
                joints.dtype != torch.int32:
            raise ValueError('joints must be int32 [N,M,J,2]')
        joints = joints.contiguous()
        M = int(joints.shape[1])
        if int(joints.shape[2]) != J:
            raise ValueError('joints must hold %d joints per person' % J)
    else:
        joints = g_push = g_pull = None
    ups = []
    for name, g in (('g_heat', g_heat), ('g_push', g_push), ('g_pull', g_pull)):
        if g is not None:
            if tuple(g.shape) != (N,) or g.dtype != torch.float32:
                raise ValueError('%s must be float32 [N]' % name)
            g = g.contiguous()
        ups.append(g)
    nv.check(nv.lib().lp_pose_loss_grad(nv.dptr(out), N, Cc, R, J, int(tag_offset), nv.dptr(heat), nv.dptr(mask),
                                        nv.dptr(joints), M, LOSS_TYPES[loss_type], float(heat_factor), float(push_factor),
                                        float(pull_factor), nv.dptr(ups[0]), nv.dptr(ups[1]), nv.dptr(ups[2]),
                                        nv.dptr(grad_out), nv.stream_ptr()), 'lp_pose_loss_grad')
    return grad_out


class _PoseLoss(torch.autograd.Function):
    """``pose_loss`` with ``pose_loss_grad`` as its backward; differentiable in the stage output only."""

    @staticmethod
    def forward(ctx, out, num_joints, tag_offset, heat, mask, joints, loss_type, heat_factor, push_factor, pull_factor):
        ctx.set_materialize_grads(False)             # a term that is not used arrives as None: NULL for the device
        ctx.save_for_backward(out, heat, mask, joints)
        ctx.args = (num_joints, tag_offset, loss_type, heat_factor, push_factor, pull_factor)
        return pose_loss(out.detach(), num_joints, tag_offset, heat, mask, joints, loss_type, heat_factor, push_factor,
                         pull_factor)

    @staticmethod
    def backward(ctx, g_heat, g_push, g_pull):
        out, heat, mask, joints = ctx.saved_tensors
        num_joints, tag_offset, loss_type, heat_factor, push_factor, pull_factor = ctx.args
        grad = pose_loss_grad(out, num_joints, tag_offset, heat, mask, joints, loss_type, heat_factor, push_factor,
                              pull_factor, g_heat, g_push, g_pull)
        return (grad,) + (None,) * 9


def loss_buffers(N, J, R, device):
    """The outputs and the workspace of one ``pose_loss`` call on an [N,C,R,R] output with J joints, for a caller that
    keeps them across calls: dict(heat, push, pull: float32 [N]; workspace: uint8)."""
    need = int(nv.lib().lp_pose_loss_workspace_bytes(int(N), int(J), int(R)))
    if need == 0:
        raise ValueError('lp_pose_loss does not take N = %d, J = %d, R = %d' % (N, J, R))
    out = {k: torch.empty(int(N), dtype=torch.float32, device=device) for k in ('heat', 'push', 'pull')}
    out.update(workspace=torch.empty(need, dtype=torch.uint8, device=device), shape=(int(N), int(J), int(R)))
    return out


class HeatmapLoss(object):
    """loss.py:30-39: ``forward(pred, gt, mask)`` -> [N], mean((pred - gt)^2 * mask) over the joints and the plane."""

    def forward(self, pred, gt, mask):
        assert pred.size() == gt.size()
        return pose_loss(pred, pred.shape[1], -1, gt, mask)[0]

    __call__ = forward


class AELoss(object):
    """loss.py:42-159: ``forward(tags, joints)`` -> (push, pull) scalars, the batch means of batchTagLoss.  ``tags``:
    [N, K*H*W] or [N, K*H*W, 1] (the reference's flattened tag maps), ``joints`` [N,M,J,2] integer."""

    def __init__(self, loss_type, max_num_people, output_resolution):
        if loss_type not in LOSS_TYPES:
            raise ValueError('Unkown ae loss type')
        self.loss_type, self.max_num_people, self.output_resolution = loss_type, max_num_people, output_resolution

    def per_image(self, tags, joints):
        if tags.dim() == 3:
            tags = tags.squeeze(2)
        R = int(self.output_resolution)
        N = int(tags.shape[0])
        if tags.shape[1] % (R * R):
            raise ValueError('tags must be [N, K * %d * %d]' % (R, R))
        maps = tags.reshape(N, tags.shape[1] // (R * R), R, R)
        _, push, pull = pose_loss(maps, joints.shape[2], 0, joints=joints.to(torch.int32), loss_type=self.loss_type)
        return push, pull

    def forward(self, tags, joints):
        push, pull = self.per_image(tags, joints)
        return push.mean(), pull.mean()

    __call__ = forward


def _loss_key(cfg, key, stages):
    v = cfg.LOSS.get(key, LOSS_DEFAULTS[key])
    if key == 'AE_LOSS_TYPE':
        return v
    v = tuple(v) if isinstance(v, (list, tuple)) else (v,)
    return v * stages if len(v) == 1 and key not in cfg.LOSS else v


class MultiLossFactory(object):
    """loss.py:248-366: ``forward(outputs, heatmaps, masks, joints)``, lists per stage -> (heatmaps_losses,
    push_losses, pull_losses): per stage an [N] tensor, a scalar and a scalar, None where LOSS.WITH_HEATMAPS_LOSS /
    LOSS.WITH_AE_LOSS switch a term off.  One ``lp_pose_loss`` call per stage.  LOSS.HEATMAPS_LOSS_FACTOR,
    AE_LOSS_TYPE, PUSH_LOSS_FACTOR and PULL_LOSS_FACTOR are read from ``cfg.LOSS`` where present, otherwise they take
    the reference's defaults (default.py:97-104; a one-entry default serves every stage)."""

    def __init__(self, cfg):
        self.num_joints = cfg.MODEL.NUM_JOINTS
        self.num_stages = cfg.LOSS.NUM_STAGES
        S = self.num_stages
        self.with_heatmaps = tuple(bool(v) for v in cfg.LOSS.WITH_HEATMAPS_LOSS)
        self.with_ae = tuple(bool(v) for v in cfg.LOSS.WITH_AE_LOSS)
        self.heatmaps_loss_factor = _loss_key(cfg, 'HEATMAPS_LOSS_FACTOR', S)
        self.push_loss_factor = _loss_key(cfg, 'PUSH_LOSS_FACTOR', S)
        self.pull_loss_factor = _loss_key(cfg, 'PULL_LOSS_FACTOR', S)
        self.loss_type = _loss_key(cfg, 'AE_LOSS_TYPE', S)
        if self.loss_type not in LOSS_TYPES:
            raise ValueError('Unkown ae loss type')
        for name, v in (('WITH_HEATMAPS_LOSS', self.with_heatmaps), ('WITH_AE_LOSS', self.with_ae),
                        ('HEATMAPS_LOSS_FACTOR', self.heatmaps_loss_factor), ('PUSH_LOSS_FACTOR', self.push_loss_factor),
                        ('PULL_LOSS_FACTOR', self.pull_loss_factor)):
            assert len(v) == S, 'LOSS.%s and LOSS.NUM_STAGES should have same length, got %d vs %d.' % (name, len(v), S)

    def per_image(self, outputs, heatmaps, masks, joints):
        """The three lists with every term per image ([N] tensors): what ``forward`` averages."""
        for name, v in (('outputs', outputs), ('heatmaps', heatmaps), ('masks', masks), ('joints', joints)):
            assert isinstance(v, list), '%s should be a list, got %s instead.' % (name, type(v))
            assert len(v) == self.num_stages, 'len(%s) and num_stages should been same, got %d vs %d.' \
                % (name, len(v), self.num_stages)
        heatmaps_losses, push_losses, pull_losses = [], [], []
        for idx in range(self.num_stages):
            if not self.with_heatmaps[idx] and not self.with_ae[idx]:      # a stage without a loss: the reference's Nones
                heatmaps_losses.append(None)
                push_losses.append(None)
                pull_losses.append(None)
                continue
            heat = heatmaps[idx] if self.with_heatmaps[idx] else None
            offset = (self.num_joints if self.with_heatmaps[idx] else 0) if self.with_ae[idx] else -1
            hl, push, pull = pose_loss(outputs[idx], self.num_joints, offset, heat, masks[idx], joints[idx],
                                       self.loss_type, self.heatmaps_loss_factor[idx], self.push_loss_factor[idx],
                                       self.pull_loss_factor[idx])
            heatmaps_losses.append(hl)
            push_losses.append(push)
            pull_losses.append(pull)
        return heatmaps_losses, push_losses, pull_losses

    def forward(self, outputs, heatmaps, masks, joints):
        hl, push, pull = self.per_image(outputs, heatmaps, masks, joints)
        mean = lambda t: None if t is None else t.mean()    # noqa: E731
        return hl, [mean(t) for t in push], [mean(t) for t in pull]

    __call__ = forward
