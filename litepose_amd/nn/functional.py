"""The layer kinds of LitePose as differentiable functions on the device (include/litepose_amd.h, "training-mode
layers"): ``pointwise``, ``depthwise`` and ``batch_norm_act``, the three a block is made of, and the two dense layers,
``stem_conv`` (3x3, stride 2, 3 -> 32; weight gradient only) and ``deconv_pair`` (the ConvTranspose2d(k4, s2, p1) pair of
the Fusion Deconv Head, or one of them), each a ``torch.autograd.Function`` over one forward and one backward call of the
C ABI; and ``dense_conv``, the dense K x K convolution of the pose_resnet family (K 3 / 5 / 7, stride 1 / 2, one or two
sources, optionally through a nearest x2 upsample, optionally biased) with every gradient.  float32 CUDA tensors, NCHW; a
tensor of another kind is an error, there is no other path.

What an op keeps between forward and backward is what its backward reads: the raw input (and the weight, which lives on
anyway), and for BatchNorm the fp64 ``(mean, invstd)`` pair of the batch.  The BatchNorm output is not kept: the backward
recomputes ``z`` by the forward's own expression to find the cells the activation passed.  Every sum has one order that
depends on the shapes only: two backward calls give the same bits."""
import torch

from .. import _native as nv

ACTS = {None: 0, 'none': 0, 'relu': 1, 'relu6': 2}


def _f32(t, name, dim=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError('%s must be a float32 CUDA tensor' % name)
    if dim is not None and t.dim() != dim:
        raise ValueError('%s must have %d dimensions' % (name, dim))
    return t.detach().contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------------------------- 1x1
def pw_forward(x, w):
    x, w = _f32(x, 'x', 4), _f32(w.reshape(w.shape[0], -1), 'w', 2)
    N, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(w.shape[0])
    if int(w.shape[1]) != Cin:
        raise ValueError('w must be [Cout, %d(, 1, 1)]' % Cin)
    y = torch.empty((N, Cout, H, W), dtype=torch.float32, device=x.device)
    L = nv.lib()
    ws = _ws(L.lp_pw_forward_workspace_bytes(Cin, Cout), x.device)
    nv.check(L.lp_pw_forward(nv.dptr(x), nv.dptr(w), nv.dptr(y), N, Cin, Cout, H * W, nv.dptr(ws), ws.numel(),
                             nv.stream_ptr()), 'lp_pw_forward')
    return y


def pw_backward(grad_y, x, w, need_x=True, need_w=True):
    """-> (grad_x or None, grad_w [Cout, Cin] or None)"""
    grad_y, x, w = _f32(grad_y, 'grad_y', 4), _f32(x, 'x', 4), _f32(w.reshape(w.shape[0], -1), 'w', 2)
    N, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(w.shape[0])
    if tuple(grad_y.shape) != (N, Cout, H, W) or int(w.shape[1]) != Cin:
        raise ValueError('grad_y, x and w do not belong to one 1x1 convolution')
    gx = torch.empty_like(x) if need_x else None
    gw = torch.empty_like(w) if need_w else None
    if not (need_x or need_w):
        return None, None
    L = nv.lib()
    ws = _ws(L.lp_pw_backward_workspace_bytes(N, Cin, Cout, H * W, int(need_x), int(need_w)), x.device)
    nv.check(L.lp_pw_backward(nv.dptr(grad_y), nv.dptr(x), nv.dptr(w), nv.dptr(gx), nv.dptr(gw), N, Cin, Cout, H * W,
                              nv.dptr(ws), ws.numel(), nv.stream_ptr()), 'lp_pw_backward')
    return gx, gw


class _Pointwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return pw_forward(x, w)

    @staticmethod
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        gx, gw = pw_backward(grad_y, x, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, None if gw is None else gw.reshape(w.shape)


def pointwise(x, w):
    """1x1 convolution without bias: ``x`` [N,Cin,H,W], ``w`` [Cout,Cin] or [Cout,Cin,1,1] -> [N,Cout,H,W]."""
    return _Pointwise.apply(x, w)


# ---------------------------------------------------------------------------------- depthwise
def _dw_dims(x, w, stride):
    N, C, H, W = (int(v) for v in x.shape)
    K = int(w.shape[-1])
    if w.numel() != C * K * K or int(w.shape[0]) != C:
        raise ValueError('w must be [%d(, 1), K, K]' % C)
    return N, C, H, W, K, int(stride)


def dw_forward(x, w, stride=1):
    x, w = _f32(x, 'x', 4), _f32(w, 'w')
    N, C, H, W, K, S = _dw_dims(x, w, stride)
    y = torch.empty((N, C, (H - 1) // S + 1, (W - 1) // S + 1), dtype=torch.float32, device=x.device)
    L = nv.lib()
    ws = _ws(L.lp_dw_forward_workspace_bytes(C, K), x.device)
    nv.check(L.lp_dw_forward(nv.dptr(x), nv.dptr(w), nv.dptr(y), N, C, H, W, K, S, nv.dptr(ws), ws.numel(),
                             nv.stream_ptr()), 'lp_dw_forward')
    return y


def dw_backward(grad_y, x, w, stride=1, need_x=True, need_w=True):
    """-> (grad_x or None, grad_w of w's shape or None)"""
    grad_y, x, w = _f32(grad_y, 'grad_y', 4), _f32(x, 'x', 4), _f32(w, 'w')
    N, C, H, W, K, S = _dw_dims(x, w, stride)
    if tuple(grad_y.shape) != (N, C, (H - 1) // S + 1, (W - 1) // S + 1):
        raise ValueError('grad_y does not have the shape of the output')
    if not (need_x or need_w):
        return None, None
    gx = torch.empty_like(x) if need_x else None
    gw = torch.empty_like(w) if need_w else None
    L = nv.lib()
    ws = _ws(L.lp_dw_backward_workspace_bytes(N, C, H, W, K, S, int(need_w)), x.device)
    nv.check(L.lp_dw_backward(nv.dptr(grad_y), nv.dptr(x), nv.dptr(w), nv.dptr(gx), nv.dptr(gw), N, C, H, W, K, S,
                              nv.dptr(ws), ws.numel(), nv.stream_ptr()), 'lp_dw_backward')
    return gx, gw


class _Depthwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride):
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return dw_forward(x, w, stride)

    @staticmethod
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        gx, gw = dw_backward(grad_y, x, w, ctx.stride, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, None


def depthwise(x, w, stride=1):
    """Depthwise K x K convolution (K 3, 5 or 7), padding K // 2, ``stride`` 1 or 2 (even planes), without bias:
    ``x`` [N,C,H,W], ``w`` [C,K,K] or [C,1,K,K]."""
    return _Depthwise.apply(x, w, stride)


# ---------------------------------------------------------------------------------- stem: dense 3x3, stride 2, 3 -> 32
def _stem_dims(x, w):
    N, C, H, W = (int(v) for v in x.shape)
    if C != 3 or tuple(w.shape) != (32, 3, 3, 3):
        raise ValueError('the stem takes x [N, 3, H, W] and w [32, 3, 3, 3]')
    if H % 2 or W % 2:
        raise ValueError('the stem is defined for even H and W only')
    return N, H, W


def stem_forward(x, w):
    x, w = _f32(x, 'x', 4), _f32(w, 'w', 4)
    N, H, W = _stem_dims(x, w)
    y = torch.empty((N, 32, H // 2, W // 2), dtype=torch.float32, device=x.device)
    nv.check(nv.lib().lp_stem_forward(nv.dptr(x), nv.dptr(w), nv.dptr(y), N, H, W, nv.stream_ptr()), 'lp_stem_forward')
    return y


def stem_backward(grad_y, x):
    """-> grad_w [32, 3, 3, 3]; there is no data gradient."""
    grad_y, x = _f32(grad_y, 'grad_y', 4), _f32(x, 'x', 4)
    N, C, H, W = (int(v) for v in x.shape)
    if C != 3 or H % 2 or W % 2 or tuple(grad_y.shape) != (N, 32, H // 2, W // 2):
        raise ValueError('grad_y and x do not belong to one stem convolution')
    gw = torch.empty((32, 3, 3, 3), dtype=torch.float32, device=x.device)
    L = nv.lib()
    ws = _ws(L.lp_stem_backward_workspace_bytes(N, H, W), x.device)
    nv.check(L.lp_stem_backward(nv.dptr(grad_y), nv.dptr(x), nv.dptr(gw), N, H, W, nv.dptr(ws), ws.numel(),
                                nv.stream_ptr()), 'lp_stem_backward')
    return gw


class _StemConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x)
        return stem_forward(x, w)

    @staticmethod
    def backward(ctx, grad_y):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError('the stem has no data gradient in the library')
        (x,) = ctx.saved_tensors
        return None, stem_backward(grad_y, x) if ctx.needs_input_grad[1] else None


def stem_conv(x, w):
    """The stem: 3x3 convolution, stride 2, padding 1, without bias: ``x`` [N,3,H,W] (even H, W; it must not require a
    gradient: the library has no data gradient for the image), ``w`` [32,3,3,3] -> [N,32,H/2,W/2]."""
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise ValueError('stem_conv has no gradient for x')
    return _StemConv.apply(x, w)


# ---------------------------------------------------------------------------------- ConvTranspose2d(k4, s2, p1) pair
def _deconv_dims(xa, wa, xb, wb):
    N, Ca, h, w = (int(v) for v in xa.shape)
    if wa.dim() != 4 or int(wa.shape[0]) != Ca or tuple(wa.shape[2:]) != (4, 4):
        raise ValueError('wa must be [%d, Cout, 4, 4]' % Ca)
    Cout = int(wa.shape[1])
    if (xb is None) != (wb is None):
        raise ValueError('xb and wb are given together')
    Cb = 0
    if xb is not None:
        Cb = int(xb.shape[1])
        if tuple(xb.shape) != (N, Cb, h, w) or tuple(wb.shape) != (Cb, Cout, 4, 4) or Cb < 1:
            raise ValueError('xb must be [%d, Cb, %d, %d] and wb [Cb, %d, 4, 4]' % (N, h, w, Cout))
    return N, Ca, Cb, Cout, h, w


def deconv_forward(xa, wa, xb=None, wb=None):
    xa, wa = _f32(xa, 'xa', 4), _f32(wa, 'wa')
    if xb is not None or wb is not None:
        xb, wb = _f32(xb, 'xb', 4), _f32(wb, 'wb')
    N, Ca, Cb, Cout, h, w = _deconv_dims(xa, wa, xb, wb)
    y = torch.empty((N, Cout, 2 * h, 2 * w), dtype=torch.float32, device=xa.device)
    L = nv.lib()
    ws = _ws(L.lp_deconv_forward_workspace_bytes(Ca, Cb, Cout), xa.device)
    nv.check(L.lp_deconv_forward(nv.dptr(xa), nv.dptr(wa), nv.dptr(xb), nv.dptr(wb), nv.dptr(y), N, Ca, Cb, Cout, h, w,
                                 nv.dptr(ws), ws.numel(), nv.stream_ptr()), 'lp_deconv_forward')
    return y


def deconv_backward(grad_y, xa, wa, xb=None, wb=None, need_x=True, need_w=True):
    """-> (grad_xa, grad_xb, grad_wa, grad_wb): the data-gradient pair is None without ``need_x``, the weight-gradient
    pair without ``need_w``, and the ``b`` members without a second source."""
    grad_y, xa, wa = _f32(grad_y, 'grad_y', 4), _f32(xa, 'xa', 4), _f32(wa, 'wa')
    if xb is not None or wb is not None:
        xb, wb = _f32(xb, 'xb', 4), _f32(wb, 'wb')
    N, Ca, Cb, Cout, h, w = _deconv_dims(xa, wa, xb, wb)
    if tuple(grad_y.shape) != (N, Cout, 2 * h, 2 * w):
        raise ValueError('grad_y does not have the shape of the output')
    if not (need_x or need_w):
        return None, None, None, None
    gxa = torch.empty_like(xa) if need_x else None
    gxb = torch.empty_like(xb) if need_x and Cb else None
    gwa = torch.empty_like(wa) if need_w else None
    gwb = torch.empty_like(wb) if need_w and Cb else None
    L = nv.lib()
    ws = _ws(L.lp_deconv_backward_workspace_bytes(N, Ca, Cb, Cout, h, w, int(need_x), int(need_w)), xa.device)
    nv.check(L.lp_deconv_backward(nv.dptr(grad_y), nv.dptr(xa), nv.dptr(wa), nv.dptr(xb), nv.dptr(wb), nv.dptr(gxa),
                                  nv.dptr(gxb), nv.dptr(gwa), nv.dptr(gwb), N, Ca, Cb, Cout, h, w, nv.dptr(ws), ws.numel(),
                                  nv.stream_ptr()), 'lp_deconv_backward')
    return gxa, gxb, gwa, gwb


class _DeconvPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xa, wa, xb, wb):
        ctx.save_for_backward(xa, wa, xb, wb)
        return deconv_forward(xa, wa, xb, wb)

    @staticmethod
    def backward(ctx, grad_y):
        xa, wa, xb, wb = ctx.saved_tensors
        nx, nw = ctx.needs_input_grad[0::2], ctx.needs_input_grad[1::2]
        gxa, gxb, gwa, gwb = deconv_backward(grad_y, xa, wa, xb, wb, any(nx), any(nw))
        return (gxa if nx[0] else None, gwa if nw[0] else None, gxb if nx[1] else None, gwb if nw[1] else None)


def deconv_pair(xa, wa, xb=None, wb=None):
    """``conv_transpose2d(xa, wa, stride 2, padding 1) + conv_transpose2d(xb, wb, stride 2, padding 1)``, kernel 4, without
    bias: ``xa`` [N,Ca,h,w], ``wa`` [Ca,Cout,4,4], ``xb`` [N,Cb,h,w], ``wb`` [Cb,Cout,4,4] -> [N,Cout,2h,2w].  Without
    ``xb`` / ``wb`` it is the single transposed convolution."""
    return _DeconvPair.apply(xa, wa, xb, wb)


# ---------------------------------------------------------------------------------- dense K x K convolution
def _conv_dims(xa, wa, xb, wb, bias, stride, upsample):
    N, Ca, H, W = (int(v) for v in xa.shape)
    if wa.dim() != 4 or int(wa.shape[1]) != Ca or wa.shape[2] != wa.shape[3]:
        raise ValueError('wa must be [Cout, %d, K, K]' % Ca)
    Cout, K = int(wa.shape[0]), int(wa.shape[2])
    if (xb is None) != (wb is None):
        raise ValueError('xb and wb are given together')
    Cb = 0
    if xb is not None:
        Cb = int(xb.shape[1])
        if tuple(xb.shape) != (N, Cb, H, W) or tuple(wb.shape) != (Cout, Cb, K, K) or Cb < 1:
            raise ValueError('xb must be [%d, Cb, %d, %d] and wb [%d, Cb, %d, %d]' % (N, H, W, Cout, K, K))
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError('bias must be [%d]' % Cout)
    S, ups = int(stride), int(bool(upsample))
    OH, OW = ((H << ups) - 1) // max(S, 1) + 1, ((W << ups) - 1) // max(S, 1) + 1
    return N, Ca, Cb, Cout, H, W, K, S, ups, OH, OW


def _conv_ws(L, dims, device):
    nbytes = L.lp_conv_workspace_bytes(*dims)
    return _ws(nbytes, device)


def conv_forward(xa, wa, xb=None, wb=None, bias=None, stride=1, upsample=False):
    xa, wa = _f32(xa, 'xa', 4), _f32(wa, 'wa')
    if xb is not None or wb is not None:
        xb, wb = _f32(xb, 'xb', 4), _f32(wb, 'wb')
    if bias is not None:
        bias = _f32(bias, 'bias', 1)
    N, Ca, Cb, Cout, H, W, K, S, ups, OH, OW = _conv_dims(xa, wa, xb, wb, bias, stride, upsample)
    y = torch.empty((N, Cout, OH, OW), dtype=torch.float32, device=xa.device)
    L = nv.lib()
    ws = _conv_ws(L, (N, Ca, Cb, Cout, H, W, K, S, ups), xa.device)
    nv.check(L.lp_conv_forward(nv.dptr(xa), nv.dptr(wa), nv.dptr(xb), nv.dptr(wb), nv.dptr(bias), nv.dptr(y), N, Ca, Cb,
                               Cout, H, W, K, S, ups, nv.dptr(ws), ws.numel(), nv.stream_ptr()), 'lp_conv_forward')
    return y


def conv_backward(grad_y, xa, wa, xb=None, wb=None, stride=1, upsample=False, need=(True, True, True, True, False)):
    """``need`` = which of (grad_xa, grad_wa, grad_xb, grad_wb, grad_bias) to compute -> that 5-tuple, None where not
    asked for (the ``b`` members also without a second source)."""
    grad_y, xa, wa = _f32(grad_y, 'grad_y', 4), _f32(xa, 'xa', 4), _f32(wa, 'wa')
    if xb is not None or wb is not None:
        xb, wb = _f32(xb, 'xb', 4), _f32(wb, 'wb')
    N, Ca, Cb, Cout, H, W, K, S, ups, OH, OW = _conv_dims(xa, wa, xb, wb, None, stride, upsample)
    if tuple(grad_y.shape) != (N, Cout, OH, OW):
        raise ValueError('grad_y does not have the shape of the output')
    nxa, nwa, nxb, nwb, nb = (bool(v) for v in need)
    nxb, nwb = nxb and Cb > 0, nwb and Cb > 0
    if not (nxa or nwa or nxb or nwb or nb):
        return None, None, None, None, None
    gxa = torch.empty_like(xa) if nxa else None
    gwa = torch.empty_like(wa) if nwa else None
    gxb = torch.empty_like(xb) if nxb else None
    gwb = torch.empty_like(wb) if nwb else None
    gb = torch.empty((Cout,), dtype=torch.float32, device=xa.device) if nb else None
    L = nv.lib()
    ws = _conv_ws(L, (N, Ca, Cb, Cout, H, W, K, S, ups), xa.device)
    nv.check(L.lp_conv_backward(nv.dptr(grad_y), nv.dptr(xa), nv.dptr(wa), nv.dptr(xb), nv.dptr(wb), nv.dptr(gxa),
                                nv.dptr(gxb), nv.dptr(gwa), nv.dptr(gwb), nv.dptr(gb), N, Ca, Cb, Cout, H, W, K, S, ups,
                                nv.dptr(ws), ws.numel(), nv.stream_ptr()), 'lp_conv_backward')
    return gxa, gwa, gxb, gwb, gb


class _DenseConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xa, wa, xb, wb, bias, stride, upsample):
        ctx.save_for_backward(xa, wa, xb, wb)
        ctx.stride, ctx.upsample = stride, upsample
        return conv_forward(xa, wa, xb, wb, bias, stride, upsample)

    @staticmethod
    def backward(ctx, grad_y):
        xa, wa, xb, wb = ctx.saved_tensors
        return conv_backward(grad_y, xa, wa, xb, wb, ctx.stride, ctx.upsample, ctx.needs_input_grad[:5]) + (None, None)


def dense_conv(xa, wa, xb=None, wb=None, bias=None, stride=1, upsample=False):
    """Dense K x K convolution (K 3, 5 or 7), padding K // 2, ``stride`` 1 or 2 (even planes), over one source or two
    channel-concatenated ones: ``conv2d(U(xa), wa) + conv2d(U(xb), wb) + bias`` with ``U`` the nearest x2 upsample when
    ``upsample`` (stride 1 only), else the identity.  ``xa`` [N,Ca,H,W], ``wa`` [Cout,Ca,K,K], ``xb`` [N,Cb,H,W], ``wb``
    [Cout,Cb,K,K], ``bias`` [Cout] -> [N,Cout,OH,OW].  Every input that requires a gradient gets one, and only those."""
    return _DenseConv.apply(xa, wa, xb, wb, bias, int(stride), bool(upsample))


# ---------------------------------------------------------------------------------- BatchNorm + act (+ residual)
def bn_forward(x, gamma, beta, running, act=None, residual=None, training=True, momentum=0.1, eps=1e-5):
    """``running``: float32 [2, C] = running_mean | running_var, moved in place when ``training``.
    -> (y, stat): stat float64 [2, C] = mean | invstd of the batch, None in eval mode."""
    x, gamma, beta = _f32(x, 'x', 4), _f32(gamma, 'gamma', 1), _f32(beta, 'beta', 1)
    N, C, H, W = (int(v) for v in x.shape)
    if gamma.numel() != C or beta.numel() != C or tuple(running.shape) != (2, C) or running.dtype != torch.float32:
        raise ValueError('gamma, beta must be [C] and running float32 [2, C]')
    if residual is not None:
        residual = _f32(residual, 'residual', 4)
        if residual.shape != x.shape:
            raise ValueError('residual must have the shape of x')
    y = torch.empty_like(x)
    L = nv.lib()
    stat = ws = None
    if training:
        stat = torch.empty((2, C), dtype=torch.float64, device=x.device)
        ws = _ws(L.lp_bn_workspace_bytes(N, C, H * W), x.device)
    nv.check(L.lp_bn_forward(nv.dptr(x), nv.dptr(gamma), nv.dptr(beta), nv.dptr(running), nv.dptr(residual), nv.dptr(y),
                             nv.dptr(stat), N, C, H * W, ACTS[act], int(bool(training)), float(momentum), float(eps),
                             nv.dptr(ws), 0 if ws is None else ws.numel(), nv.stream_ptr()), 'lp_bn_forward')
    return y, stat


def bn_backward(grad_y, x, gamma, beta, stat, act=None):
    """-> (grad_x, grad_gamma, grad_beta); the residual's gradient is ``grad_y`` itself."""
    grad_y, x, gamma, beta = _f32(grad_y, 'grad_y', 4), _f32(x, 'x', 4), _f32(gamma, 'gamma', 1), _f32(beta, 'beta', 1)
    N, C, H, W = (int(v) for v in x.shape)
    if grad_y.shape != x.shape or tuple(stat.shape) != (2, C) or stat.dtype != torch.float64:
        raise ValueError('grad_y must have the shape of x, stat must be float64 [2, C]')
    gx, gg, gb = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    L = nv.lib()
    ws = _ws(L.lp_bn_workspace_bytes(N, C, H * W), x.device)
    nv.check(L.lp_bn_backward(nv.dptr(grad_y), nv.dptr(x), nv.dptr(gamma), nv.dptr(beta), nv.dptr(stat.contiguous()),
                              nv.dptr(gx), nv.dptr(gg), nv.dptr(gb), N, C, H * W, ACTS[act], nv.dptr(ws), ws.numel(),
                              nv.stream_ptr()), 'lp_bn_backward')
    return gx, gg, gb


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, act, training, momentum, eps):
        running = torch.stack([running_mean.detach(), running_var.detach()]).float().contiguous()
        y, stat = bn_forward(x, gamma, beta, running, act, residual, training, momentum, eps)
        if training:
            running_mean.copy_(running[0])
            running_var.copy_(running[1])
            ctx.save_for_backward(x, gamma, beta, stat)
        ctx.act, ctx.training, ctx.has_res = act, training, residual is not None
        return y

    @staticmethod
    def backward(ctx, grad_y):
        if not ctx.training:
            raise NotImplementedError('backward through an eval-mode batch_norm_act is not part of the library')
        x, gamma, beta, stat = ctx.saved_tensors
        gx, gg, gb = bn_backward(grad_y, x, gamma, beta, stat, ctx.act)
        return gx, gg, gb, (grad_y if ctx.has_res else None), None, None, None, None, None, None


# ---- synchronised over a process group: two calls per pass, one all-gather of a [2C (+ 2)] fp64 row between them
SYNC_MAX_WORLD = 64                  # LP_BN_SYNC_MAX_WORLD
_force_sync = False                  # tools/time_train_step.py: take the synchronised path at world size 1 too


def bn_sync_stats(x):
    """-> this rank's forward row, float64 [2C + 2] = sum | sumsq | count | 0."""
    x = _f32(x, 'x', 4)
    N, C, H, W = (int(v) for v in x.shape)
    row = torch.empty(2 * C + 2, dtype=torch.float64, device=x.device)
    L = nv.lib()
    ws = _ws(L.lp_bn_workspace_bytes(N, C, H * W), x.device)
    nv.check(L.lp_bn_sync_stats(nv.dptr(x), N, C, H * W, nv.dptr(row), nv.dptr(ws), ws.numel(), nv.stream_ptr()),
             'lp_bn_sync_stats')
    return row


def bn_sync_forward(x, gamma, beta, running, rows, act=None, residual=None, momentum=0.1, eps=1e-5):
    """``rows``: float64 [W, 2C + 2], the forward rows of all ranks in rank order.
    -> (y, stat): stat float64 [2C + 2] = mean | invstd | total count | 0; ``running`` [2, C] is moved in place."""
    x, gamma, beta = _f32(x, 'x', 4), _f32(gamma, 'gamma', 1), _f32(beta, 'beta', 1)
    N, C, H, W = (int(v) for v in x.shape)
    if gamma.numel() != C or beta.numel() != C or tuple(running.shape) != (2, C) or running.dtype != torch.float32:
        raise ValueError('gamma, beta must be [C] and running float32 [2, C]')
    if rows.dim() != 2 or rows.shape[1] != 2 * C + 2 or rows.dtype != torch.float64 or not rows.is_contiguous():
        raise ValueError('rows must be contiguous float64 [W, 2C + 2]')
    if residual is not None:
        residual = _f32(residual, 'residual', 4)
        if residual.shape != x.shape:
            raise ValueError('residual must have the shape of x')
    y = torch.empty_like(x)
    stat = torch.empty(2 * C + 2, dtype=torch.float64, device=x.device)
    nv.check(nv.lib().lp_bn_sync_forward(nv.dptr(x), nv.dptr(gamma), nv.dptr(beta), nv.dptr(running), nv.dptr(residual),
                                         nv.dptr(y), nv.dptr(stat), nv.dptr(rows), int(rows.shape[0]), N, C, H * W,
                                         ACTS[act], float(momentum), float(eps), nv.stream_ptr()), 'lp_bn_sync_forward')
    return y, stat


def bn_sync_backward_stats(grad_y, x, gamma, beta, stat, act=None):
    """-> this rank's backward row, float64 [2C] = sum g | sum g * xhat, xhat on the global pair of ``stat``."""
    grad_y, x, gamma, beta = _f32(grad_y, 'grad_y', 4), _f32(x, 'x', 4), _f32(gamma, 'gamma', 1), _f32(beta, 'beta', 1)
    N, C, H, W = (int(v) for v in x.shape)
    if grad_y.shape != x.shape or tuple(stat.shape) != (2 * C + 2,) or stat.dtype != torch.float64:
        raise ValueError('grad_y must have the shape of x, stat must be float64 [2C + 2]')
    row = torch.empty(2 * C, dtype=torch.float64, device=x.device)
    L = nv.lib()
    ws = _ws(L.lp_bn_workspace_bytes(N, C, H * W), x.device)
    nv.check(L.lp_bn_sync_backward_stats(nv.dptr(grad_y), nv.dptr(x), nv.dptr(gamma), nv.dptr(beta), nv.dptr(stat), N, C,
                                         H * W, ACTS[act], nv.dptr(row), nv.dptr(ws), ws.numel(), nv.stream_ptr()),
             'lp_bn_sync_backward_stats')
    return row


def bn_sync_backward(grad_y, x, gamma, beta, stat, rows, rank, act=None):
    """``rows``: float64 [W, 2C], the backward rows of all ranks in rank order -> (grad_x, grad_gamma, grad_beta);
    grad_gamma / grad_beta are rank ``rank``'s own share (average the parameter gradients over the ranks)."""
    grad_y, x, gamma, beta = _f32(grad_y, 'grad_y', 4), _f32(x, 'x', 4), _f32(gamma, 'gamma', 1), _f32(beta, 'beta', 1)
    N, C, H, W = (int(v) for v in x.shape)
    if grad_y.shape != x.shape or tuple(stat.shape) != (2 * C + 2,) or stat.dtype != torch.float64:
        raise ValueError('grad_y must have the shape of x, stat must be float64 [2C + 2]')
    if rows.dim() != 2 or rows.shape[1] != 2 * C or rows.dtype != torch.float64 or not rows.is_contiguous():
        raise ValueError('rows must be contiguous float64 [W, 2C]')
    gx, gg, gb = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    nv.check(nv.lib().lp_bn_sync_backward(nv.dptr(grad_y), nv.dptr(x), nv.dptr(gamma), nv.dptr(beta), nv.dptr(stat),
                                          nv.dptr(rows), int(rows.shape[0]), int(rank), N, C, H * W, ACTS[act],
                                          nv.dptr(gx), nv.dptr(gg), nv.dptr(gb), nv.stream_ptr()), 'lp_bn_sync_backward')
    return gx, gg, gb


class _SyncBatchNormAct(torch.autograd.Function):
    """Training mode over a process group: per pass one row kernel pair, ONE all-gather, one apply kernel."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, act, momentum, eps, group):
        from ..parallel import all_gather_rows, group_rank
        running = torch.stack([running_mean.detach(), running_var.detach()]).float().contiguous()
        rows = all_gather_rows(bn_sync_stats(x), group)
        y, stat = bn_sync_forward(x, gamma, beta, running, rows, act, residual, momentum, eps)
        running_mean.copy_(running[0])
        running_var.copy_(running[1])
        ctx.save_for_backward(x, gamma, beta, stat)
        ctx.act, ctx.has_res, ctx.group, ctx.rank = act, residual is not None, group, group_rank(group)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        from ..parallel import all_gather_rows
        x, gamma, beta, stat = ctx.saved_tensors
        rows = all_gather_rows(bn_sync_backward_stats(grad_y, x, gamma, beta, stat, ctx.act), ctx.group)
        gx, gg, gb = bn_sync_backward(grad_y, x, gamma, beta, stat, rows, ctx.rank, ctx.act)
        return gx, gg, gb, (grad_y if ctx.has_res else None), None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, act=None, residual=None, training=True, momentum=0.1,
                   eps=1e-5, group=None):
    """``act(batch_norm(x)) (+ residual)``, ``act`` None / 'relu' / 'relu6'.  Training mode normalises with the batch's
    statistics and moves ``running_mean`` / ``running_var`` in place (the unbiased variance, as torch); eval mode
    normalises with the running pair, and a backward through it raises ``NotImplementedError``.

    ``group``: a ``torch.distributed`` process group.  In training mode with more than one rank the statistics are those of
    all ranks' batches together (``torch.nn.SyncBatchNorm``): ``lp_bn_sync_stats``, one all-gather of the [2C + 2] fp64 row,
    ``lp_bn_sync_forward``; the backward likewise with one all-gather of the [2C] row.  Every rank ends with the same bits
    in ``running_mean`` / ``running_var``; ``gamma`` / ``beta`` receive this rank's share of their gradient.  ``None``, a
    group of one, or eval mode: the calls above, unchanged."""
    if act not in ACTS:
        raise ValueError('act must be one of %s' % sorted(k for k in ACTS if k))
    if training and group is not None:
        from ..parallel import group_size
        world = group_size(group)
        if world > SYNC_MAX_WORLD:
            raise ValueError('a synchronised batch_norm_act takes at most %d ranks' % SYNC_MAX_WORLD)
        if world > 1 or _force_sync:
            return _SyncBatchNormAct.apply(x, gamma, beta, residual, running_mean, running_var, act, float(momentum),
                                           float(eps), group)
    return _BatchNormAct.apply(x, gamma, beta, residual, running_mean, running_var, act, bool(training), float(momentum),
                               float(eps))


# ---------------------------------------------------------------------------------- supernet: sliced parameters
def _a64(n):
    return (int(n) + 63) // 64 * 64


class SubnetTable(object):
    """The descriptor table of one sampled sub-network (include/litepose_amd.h, lp_subnet_desc), on the device.

    ``specs``: one dict per learnable tensor of the sub-network, in the order ``subnet_params`` returns them:
    ``param`` (the supernet's tensor), ``kind`` 0 / 1 / 2, ``rows``, ``cols``, ``shape`` (of the sliced tensor) and, for a
    window with k < 7, ``lin_w`` / ``lin_b``.  ``params`` is the list of supernet tensors the table reads -- every ``param``
    and, behind its window, the ``lin_w`` / ``lin_b`` pair -- in the order ``subnet_params`` takes them.  The table holds raw
    addresses: ``stale()`` tells whether a parameter's ``data_ptr()`` has changed since it was built."""

    def __init__(self, specs, device):
        rows, self.params, self.views, self.grads = [], [], [], []
        sub = full = 0
        for sp in specs:
            p, kind = sp['param'], int(sp['kind'])
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError('supernet parameters must be contiguous float32 tensors')
            d = nv.LpSubnetDesc(src=p.data_ptr(), sub_offset=sub, full_offset=full, kind=kind, rows=int(sp['rows']),
                                cols=int(sp.get('cols', 0)), t=1)
            shape = tuple(int(v) for v in sp['shape'])
            numel = 1
            for v in shape:
                numel *= v
            self.params.append(p)
            self.grads.append((full, p.numel(), tuple(p.shape)))
            span = p.numel()
            if kind == 0:
                d.R, d.C = int(p.shape[0]), int(p.shape[1])
                d.t = p.numel() // (d.R * d.C)
            elif kind == 1:
                d.R = p.numel()
            else:
                d.R = int(p.shape[0])
                if d.cols != 7:
                    lw, lb = sp['lin_w'], sp['lin_b']
                    kk = d.cols * d.cols
                    if tuple(lw.shape) != (kk, kk) or tuple(lb.shape) != (kk,) or not lw.is_contiguous():
                        raise ValueError('the window transform of a k x k window is [k*k, k*k] with a [k*k] bias')
                    d.lin_w, d.lin_b = lw.data_ptr(), lb.data_ptr()
                    off_l = full + _a64(p.numel())
                    off_b = off_l + _a64(kk * kk)
                    self.params += [lw, lb]
                    self.grads += [(off_l, kk * kk, (kk, kk)), (off_b, kk, (kk,))]
                    span = off_b + kk - full
            self.views.append((sub, numel, shape))
            rows.append(d)
            sub += _a64(numel)
            full += _a64(span)
        self.count, self.sub_elems, self.full_elems = len(rows), sub, full
        table = (nv.LpSubnetDesc * len(rows))(*rows)
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)
        self.device = self.table.device
        self._ptrs = tuple(p.data_ptr() for p in self.params)

    def stale(self):
        return self._ptrs != tuple(p.data_ptr() for p in self.params)


class _SubnetParams(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, *full_params):
        if len(full_params) != len(table.params) or any(a.data_ptr() != b for a, b in zip(full_params, table._ptrs)):
            raise ValueError('subnet_params: the parameters are not the ones the table was built from')
        sub = torch.empty(table.sub_elems, dtype=torch.float32, device=table.device)
        nv.check(nv.lib().lp_subnet_gather(nv.dptr(table.table), table.count, nv.dptr(sub), table.sub_elems,
                                           nv.stream_ptr()), 'lp_subnet_gather')
        ctx.table = table
        return tuple(sub[o:o + n].view(shape) for o, n, shape in table.views)

    @staticmethod
    def backward(ctx, *grads):
        table = ctx.table
        if table.stale():
            raise RuntimeError('subnet_params: a parameter moved between the forward and the backward')
        gsub = torch.empty(table.sub_elems, dtype=torch.float32, device=table.device)
        dst, src = [], []
        for (o, n, shape), g in zip(table.views, grads):
            if g is None:
                gsub[o:o + n].zero_()
            else:
                dst.append(gsub[o:o + n].view(shape))
                src.append(g)
        torch._foreach_copy_(dst, src)
        full = torch.empty(table.full_elems, dtype=torch.float32, device=table.device)
        nv.check(nv.lib().lp_subnet_scatter_grad(nv.dptr(table.table), table.count, nv.dptr(gsub), table.sub_elems,
                                                 nv.dptr(full), table.full_elems, nv.stream_ptr()),
                 'lp_subnet_scatter_grad')
        return (None,) + tuple(full[o:o + n].view(shape) if need else None
                               for (o, n, shape), need in zip(table.grads, ctx.needs_input_grad[1:]))


def subnet_params(descs, *full_params):
    """The learnable tensors of a sampled sub-network as slices of the supernet's ``full_params``: ``descs`` is the
    ``SubnetTable`` built from them (``full_params`` must be ``descs.params``, passed so that autograd sees them).  Forward:
    ONE ``lp_subnet_gather`` into one packed buffer; returns a view of it per tensor, in the table's order.  Backward: the
    upstream gradients are packed (one multi-tensor copy) and ONE ``lp_subnet_scatter_grad`` writes one packed buffer that
    holds the full-size gradient of every parameter -- zero outside its slice -- of which the returned gradients are
    views.  The parameters must not change between forward and backward."""
    return _SubnetParams.apply(descs, *full_params)


def train_resize(images, heatmaps, masks, joints, size, base):
    """The supernet's random-resolution resize of a batch (lib/core/trainer.py:49-59), one ``lp_train_resize`` call:
    ``images`` [N,3,base,base] -> [N,3,size,size]; per stage s ``heatmaps[s]`` [N,J,R,R] and ``masks[s]`` [N,R,R]
    (R = base / 4 * 2^s) -> size / 4 * 2^s, nearest; ``joints[s]`` int32 [N,M,J,2]: the flat cell index is remapped as the
    reference does it (modulus ``base``, multiplier ``size`` for every stage).  -> (images, heatmaps, masks, joints), new
    tensors."""
    images = _f32(images, 'images', 4)
    stages = len(heatmaps)
    if len(masks) != stages or len(joints) != stages:
        raise ValueError('heatmaps, masks and joints are lists of one tensor per stage')
    N, c, I = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    size, base = int(size), int(base)
    if c != 3 or int(images.shape[3]) != I:
        raise ValueError('images must be [N, 3, I, I]')
    heatmaps = [_f32(h, 'heatmaps', 4) for h in heatmaps]
    masks = [_f32(m, 'masks', 3) for m in masks]
    res, J, M = [], None, None
    for h, m, j in zip(heatmaps, masks, joints):
        R = int(h.shape[2])
        if not isinstance(j, torch.Tensor) or j.dtype != torch.int32 or not j.is_cuda or j.dim() != 4 or j.shape[3] != 2:
            raise ValueError('joints must be int32 CUDA tensors [N, M, J, 2]')
        J, M = int(h.shape[1]) if J is None else J, int(j.shape[1]) if M is None else M
        if tuple(h.shape) != (N, J, R, R) or tuple(m.shape) != (N, R, R) or tuple(j.shape) != (N, M, J, 2):
            raise ValueError('heatmaps [N,J,R,R], masks [N,R,R] and joints [N,M,J,2] of a stage do not belong together')
        res.append(R)
    joints = [j.detach().contiguous() for j in joints]
    dev = images.device
    if size < 8 or size % 8:
        raise ValueError('size must be a positive multiple of 8')
    images_o = torch.empty((N, 3, size, size), dtype=torch.float32, device=dev)
    heat_o = [torch.empty((N, J, (size // 4) << s, (size // 4) << s), dtype=torch.float32, device=dev)
              for s in range(stages)]
    mask_o = [torch.empty((N, (size // 4) << s, (size // 4) << s), dtype=torch.float32, device=dev) for s in range(stages)]
    joint_o = [torch.empty_like(j) for j in joints]
    arr = lambda ts: (nv.vp * max(len(ts), 1))(*[t.data_ptr() for t in ts])  # noqa: E731
    nv.check(nv.lib().lp_train_resize(nv.dptr(images), nv.dptr(images_o), N, I, size, base, stages, J or 0, M or 0,
                                      (nv.C.c_int32 * max(stages, 1))(*res), arr(heatmaps), arr(masks), arr(joints),
                                      arr(heat_o), arr(mask_o), arr(joint_o), nv.stream_ptr()), 'lp_train_resize')
    return images_o, heat_o, mask_o, joint_o
