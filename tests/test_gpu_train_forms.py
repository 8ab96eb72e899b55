"""The training-mode layers at the FORMS real training shapes select (tests/_train_forms.py), each at the smallest shape that
has the form: BatchNorm over several slices per channel, the 1x1 at NB = 2 / 3 and PXV = 2, odd channel counts, the 1x1 weight
gradient with Cin > 128, depthwise with C % 4 != 0 and odd planes, the transposed-convolution pair at the widths of the
L architectures.  tests/test_train_forms_cpu.py holds the tables below to the forms every zoo architecture reaches.

Method and bounds are those of tests/test_gpu_layer_grad.py and tests/test_gpu_conv_grad.py, imported from there: fp64
torch on the CPU on the widened fp32 inputs, a sum of n fp32 products held to (n + 1) 2^-24 sum|terms|, the BatchNorm rule
with its constants 5 / 6 and 3, exact zeros where the truth is zero, two calls and a graph replay bitwise.

One bound is derived anew: stat[0], the fp64 mean, against c 2^-53 sum|x| / count.  bn_stats_kernel adds a value into the
channel's sum through at most D fp64 additions: 2 inside its float4 (16-byte form only), ceil(chunk / 256) in its lane's
serial sum over the slice, 8 in the workgroup's tree (6 shuffle levels, 2 over the four waves), and bn_fwd_kernel adds the S
partials in index order: S more.  Each addition rounds its partial sum, which is at most sum|x| of the terms under it, by
2^-53 relative: |sum' - sum| <= D 2^-53 sum|x| to first order (the second order is D^2 2^-106).  The division by the
count rounds once more, and the truth -- torch's own fp64 mean -- is itself a rounded sum: c = D + 2.  (The single-slice
shapes of test_gpu_layer_grad.py have D <= 2 + 2 + 8 + 1 by this count and use c = 3: the bound is far from tight; here it
is kept as derived.)

Sensitivity, on MI355X: scratch builds of layer_kernels.hip with one wrong edit each (not committed).  Against each, this
file and tests/test_gpu_train_net_zoo.py (176 tests) and tests/test_gpu_layer_grad.py, the shapes the suite had before (177
tests).  The figure is the largest |d - f| / bound reported; every bound is 1.

  edit                                              tests/test_gpu_layer_grad.py   the new tests
  bn_bwd_apply_kernel combines only partial 0       177 pass                       39 fail: every test_batch_norm_over_slices*
                                                                                   case ('bn dx' at 3.8e3 .. 6.4e5), the zoo
                                                                                   step's gradients
  bn_fwd_kernel combines only partial 0             177 pass                       40 fail: the same 38 ('bn y' at 8e5 .. 1.7e6),
                                                                                   the zoo step's gradients and running pairs
  bn_fwd_kernel: slice 1, not slice 0, stores       177 pass                       176 pass.  Not an error a value can show: every
    stat and moves the running pair (slice 0                                       workgroup of a channel combines the same partials
    still does when there is one slice)                                            in the same order, so whichever one stores writes
                                                                                   the same bits.  (Two slices storing would race on
                                                                                   the running pair; that is not tested either.)
  bn_walk drops its carry into the next plane       177 pass                       26 fail: every 'rem' case and the 'wide' cases
                                                                                   whose steps cross a plane's end ('bn y' at 2.8e6
                                                                                   and more), the multi-slice buffer contract
                                                                                   (outputs left poisoned); 'even' walks never carry
  pw_pack_kernel drops the odd tail pair when       177 pass                       19 fail: test_pointwise_odd_channels in modes
    transposing                                                                    both and dx ('pw dX' at 3.6e5 .. 5.1e5), the two
                                                                                   PXV = 2 cases of 24 -> 17, the zoo step's gradients
  pw_wgrad_kernel ignores blockIdx.z                177 pass                       17 fail: the 14 test_pointwise_forms cases with
                                                                                   Cin > 128 (two calls differ: columns past 128 are
                                                                                   never written), the zoo step ('pw' at 56 x the
                                                                                   reference's e, two runs differ)
"""
import math

import pytest
import torch
import torch.nn.functional as TF

import _poison as po
import _train_forms as FM
from litepose_amd.nn import functional as F
from test_gpu_conv_grad import _deconv_check, _stem_check
from test_gpu_layer_buffers import test_batch_norm_calls as _bn_buffer_contract
from test_gpu_layer_buffers import test_pointwise_calls as _pw_buffer_contract
from test_gpu_layer_grad import ACT, EDGE, EPS, MOM, U, _bn_inputs, _dw_check, _held, _pw_check, _twice_and_replayed

pytestmark = pytest.mark.gpu

# Every table row: the shape, then the form key (tests/_train_forms.py, without its leading kind) the row is there for;
# tests/test_train_forms_cpu.py asserts the claim with the library's own queries.

# (N, C, H, W): each runs plain and with a residual.  The first two rows run every activation, the others ReLU6.
BN_CASES = [
    ((5, 4, 36, 36), 'vec several two wide ragged'),        # S = 4, chunk = 405 of 324 units, a boundary inside a plane
    ((60, 8, 10, 10), 'vec several two rem ragged'),        # S = 3, chunk = 500 of 25 units: a lane's second step carries
    ((80, 8, 8, 8), 'vec several two even ragged'),         # S = 3, chunk = 427 of 16 units, a boundary inside a plane
    ((40, 5, 5, 7), 'scalar several two rem ragged'),       # S = 3, chunk = 467 of 35 units, a boundary inside a plane
    ((24, 700, 16, 16), 'vec cap two even full'),           # S = 3 = ceil(2048 / 700): the cap a wide layer sets itself
    ((8, 4, 128, 128), 'vec cap two wide full'),            # S = 64, chunk = 512 of 4096 units: 8 slices per plane
    ((16, 8, 16, 16), 'vec several two even full'),         # S = 2, chunk = 512 of 64 units
    ((4, 4, 32, 32), 'vec several two wide full'),          # S = 2, chunk = 512 of 256 units
    ((100, 4, 36, 36), 'vec cap two wide ragged'),          # S = 64, chunk = 507 of 324 units
    ((3600, 4, 6, 6), 'vec cap two rem ragged'),            # S = 64, chunk = 507 of 9 units
    ((2020, 4, 8, 8), 'vec cap two even ragged'),           # S = 64, chunk = 505 of 16 units
    # under the cap a slice grows past 512 units: three steps per lane and more, as every real batch has them
    ((2052, 4, 8, 8), 'vec cap many even ragged'),          # S = 64, chunk = 513 of 16 units
    ((189, 4, 20, 52), 'vec cap many wide full'),           # S = 64, chunk = 768 of 260 units
    ((3641, 4, 6, 6), 'vec cap many rem ragged'),           # S = 64, chunk = 513 of 9 units: two carries per lane
    ((82, 4, 40, 40), 'vec cap many wide ragged'),          # S = 64, chunk = 513 of 400 units
]
BN_ALL_ACTS = 2

# (Cin, Cout, N, H, W): the forward is K = Cin -> M = Cout, the data gradient K = Cout -> M = Cin on the transposed pack
PW_CASES = [
    ((4, 96, 4, 128, 128), ['pw fwd 3 4 Keven Mfull cbfull', 'pw dx 1 4 Keven Mrag cbfull', 'pwdw vec even z0 idle COfull CIrag']),
    ((16, 80, 4, 128, 128), ['pw fwd 2 4 Keven Mrag cbrag', 'pwdw vec even z0 idle COrag CIrag']),
    ((96, 4, 4, 128, 128), ['pw fwd 1 4 Keven Mrag cbfull', 'pw dx 3 4 Keven Mfull cbfull', 'pwdw vec even z0 idle COrag CIfull']),
    ((80, 16, 4, 128, 128), ['pw dx 2 4 Keven Mrag cbrag']),
    ((4, 144, 3, 128, 128), ['pw fwd 3 4 Keven Mrag cbrag']),
    ((144, 4, 3, 128, 128), ['pw dx 3 4 Keven Mrag cbrag', 'pwdw vec even z>0 idle COrag CIrag']),
    ((4, 128, 3, 128, 128), ['pw fwd 2 4 Keven Mfull cbfull']),
    ((128, 4, 3, 128, 128), ['pw dx 2 4 Keven Mfull cbfull', 'pwdw vec even z0 busy COrag CIfull']),
    ((4, 34, 32, 64, 64), ['pw fwd 2 4 Keven Mrag cbfull']),
    ((34, 4, 32, 64, 64), ['pw dx 2 4 Keven Mrag cbfull']),
    ((8, 160, 8, 64, 64), ['pw fwd 2 4 Keven Mfull cbrag']),
    ((160, 8, 8, 64, 64), ['pw dx 2 4 Keven Mfull cbrag', 'pwdw vec even z>0 idle COrag CIfull']),
    ((4, 160, 8, 64, 64), ['pw fwd 3 4 Keven Mfull cbrag']),
    ((160, 4, 8, 64, 64), ['pw dx 3 4 Keven Mfull cbrag']),
    # PXV = 2: HW % 4 == 2
    ((6, 14, 3, 3, 2), ['pw fwd 1 2 Keven Mrag cbfull', 'pw dx 1 2 Keven Mrag cbfull', 'pwdw scalar one z0 idle COrag CIrag']),
    ((24, 17, 3, 3, 2), ['pw dx 1 2 Kodd Mrag cbfull']),
    ((6, 14, 2, 7, 10), ['pw fwd 1 2 Keven Mrag cbfull']),
    ((24, 17, 2, 7, 10), ['pw fwd 1 2 Keven Mrag cbfull']),
    # Cin > 128 in the weight gradient
    ((192, 32, 2, 16, 16), ['pw fwd 1 4 Keven Mfull cbfull', 'pw dx 1 4 Keven Mfull cbfull', 'pwdw vec one z>0 idle COfull CIfull']),
    ((288, 80, 2, 16, 16), ['pwdw vec one z>0 idle COrag CIfull']),
    ((480, 80, 2, 16, 16), ['pw fwd 1 4 Keven Mrag cbfull']),
    ((960, 160, 1, 8, 8), ['pw fwd 1 4 Keven Mfull cbfull']),
    ((144, 32, 2, 32, 32), ['pwdw vec even z>0 idle COfull CIrag']),
    ((32, 32, 2, 32, 32), ['pwdw vec even z0 idle COfull CIfull']),
    ((160, 32, 2, 32, 32), ['pwdw vec even z>0 idle COfull CIfull']),
    ((256, 32, 2, 32, 32), ['pwdw vec even z>0 busy COfull CIfull']),
    ((144, 4, 2, 32, 32), ['pw fwd 1 4 Keven Mrag cbfull']),
    ((160, 4, 2, 32, 32), ['pw fwd 1 4 Keven Mrag cbfull']),
    ((120, 4, 2, 32, 32), ['pwdw vec even z0 busy COrag CIrag']),
    # three slices of the weight gradient, the last one shorter (3 * 784 = 2 * 1024 + 304 pixels), with and without Cin > 128
    ((160, 4, 3, 28, 28), ['pwdw vec ragged z>0 idle COrag CIfull']),
    ((4, 4, 3, 28, 28), ['pwdw vec ragged z0 idle COrag CIrag']),
    ((144, 4, 3, 28, 28), ['pwdw vec ragged z>0 idle COrag CIrag']),
    ((120, 4, 3, 28, 28), ['pwdw vec ragged z0 busy COrag CIrag']),
    ((4, 32, 3, 28, 28), ['pwdw vec ragged z0 idle COfull CIrag']),
]
# odd channel counts (COCO's 17 joints: heads of 34 and 17 channels), on a PXV = 4 and a PXV = 1 plane, in every mode
PW_ODD_CASES = [
    ((24, 17, 2, 8, 8), ['pw dx 1 4 Kodd Mrag cbfull', 'pwdw vec one z0 idle COrag CIrag']),
    ((24, 17, 3, 5, 7), ['pw fwd 1 1 Keven Mrag cbfull', 'pw dx 1 1 Kodd Mrag cbfull']),
    ((16, 17, 2, 8, 8), ['pw fwd 1 4 Keven Mrag cbfull']),
    ((16, 17, 3, 5, 7), ['pw fwd 1 1 Keven Mrag cbfull']),
    ((17, 34, 2, 8, 8), ['pw fwd 1 4 Kodd Mrag cbfull']),
    ((17, 34, 3, 5, 7), ['pw fwd 1 1 Kodd Mrag cbfull', 'pw dx 1 1 Keven Mrag cbfull']),
    ((33, 7, 2, 8, 8), ['pw fwd 1 4 Kodd Mrag cbfull']),
    ((33, 7, 3, 5, 7), ['pw fwd 1 1 Kodd Mrag cbfull']),
    ((32, 17, 2, 8, 8), ['pw dx 1 4 Kodd Mfull cbfull', 'pwdw vec one z0 idle COrag CIfull']),
    ((32, 17, 3, 5, 7), ['pw dx 1 1 Kodd Mfull cbfull', 'pwdw scalar one z0 idle COrag CIfull']),
]

# (K, S, C, N, H, W)
DW_CASES = [
    ((3, 1, 6, 2, 6, 10), '3 1 pairscalar tiles<=4 ragged Crag slice'),
    ((3, 1, 6, 2, 16, 16), '3 1 pair16 tiles<=4 whole Crag slice'),
    ((3, 2, 6, 2, 6, 10), '3 2 dwscalar tiles<=4 ragged Crag slice'),
    ((3, 2, 6, 2, 16, 16), '3 2 dwvec tiles<=4 ragged Crag slice'),
    ((5, 1, 6, 2, 6, 10), '5 1 pairscalar tiles<=4 ragged Crag slice'),
    ((5, 1, 6, 2, 16, 16), '5 1 pair16 tiles<=4 whole Crag slice'),
    ((5, 2, 6, 2, 6, 10), '5 2 dwscalar tiles<=4 ragged Crag slice'),
    ((5, 2, 6, 2, 16, 16), '5 2 dwvec tiles<=4 ragged Crag slice'),
    ((7, 1, 6, 2, 6, 10), '7 1 pairscalar tiles<=4 ragged Crag slice'),
    ((7, 1, 6, 2, 16, 16), '7 1 pair16 tiles<=4 whole Crag slice'),
    ((7, 2, 6, 2, 6, 10), '7 2 dwscalar tiles<=4 ragged Crag slice'),
    ((7, 2, 6, 2, 16, 16), '7 2 dwvec tiles<=4 ragged Crag slice'),
    ((3, 1, 17, 2, 6, 10), '3 1 pairscalar tiles<=4 ragged Crag slice'),
    ((3, 1, 17, 2, 16, 16), '3 1 pair16 tiles<=4 whole Crag slice'),
    ((3, 2, 17, 2, 6, 10), '3 2 dwscalar tiles<=4 ragged Crag slice'),
    ((3, 2, 17, 2, 16, 16), '3 2 dwvec tiles<=4 ragged Crag slice'),
    ((5, 1, 17, 2, 6, 10), '5 1 pairscalar tiles<=4 ragged Crag slice'),
    ((5, 1, 17, 2, 16, 16), '5 1 pair16 tiles<=4 whole Crag slice'),
    ((5, 2, 17, 2, 6, 10), '5 2 dwscalar tiles<=4 ragged Crag slice'),
    ((5, 2, 17, 2, 16, 16), '5 2 dwvec tiles<=4 ragged Crag slice'),
    ((7, 1, 17, 2, 6, 10), '7 1 pairscalar tiles<=4 ragged Crag slice'),
    ((7, 1, 17, 2, 16, 16), '7 1 pair16 tiles<=4 whole Crag slice'),
    ((7, 2, 17, 2, 6, 10), '7 2 dwscalar tiles<=4 ragged Crag slice'),
    ((7, 2, 17, 2, 16, 16), '7 2 dwvec tiles<=4 ragged Crag slice'),
    # odd planes (a 224 input's 7 x 7) at stride 1
    ((3, 1, 6, 2, 7, 7), '3 1 pairscalar tiles<=4 ragged Crag slice'),
    ((3, 1, 6, 2, 17, 33), '3 1 pairscalar tiles>4 ragged Crag slices'),
    ((5, 1, 6, 2, 7, 7), '5 1 pairscalar tiles<=4 ragged Crag slice'),
    ((5, 1, 6, 2, 17, 33), '5 1 pairscalar tiles>4 ragged Crag slices'),
    ((7, 1, 6, 2, 7, 7), '7 1 pairscalar tiles<=4 ragged Crag slice'),
    ((7, 1, 6, 2, 17, 33), '7 1 pairscalar tiles>4 ragged Crag slices'),
    # the 28 x 28 and 56 x 56 planes of a 448 input
    ((3, 1, 8, 2, 28, 28), '3 1 pairvec tiles<=4 ragged Cfull slice'),
    ((3, 1, 8, 2, 56, 56), '3 1 pairvec tiles>4 ragged Cfull slices'),
    ((3, 2, 8, 2, 28, 28), '3 2 dwvec tiles<=4 ragged Cfull slice'),
    ((3, 2, 8, 2, 56, 56), '3 2 dwvec tiles<=4 ragged Cfull slice'),
    ((5, 1, 8, 2, 28, 28), '5 1 pairvec tiles<=4 ragged Cfull slice'),
    ((5, 1, 8, 2, 56, 56), '5 1 pairvec tiles>4 ragged Cfull slices'),
    ((5, 2, 8, 2, 28, 28), '5 2 dwvec tiles<=4 ragged Cfull slice'),
    ((5, 2, 8, 2, 56, 56), '5 2 dwvec tiles<=4 ragged Cfull slice'),
    ((7, 1, 8, 2, 28, 28), '7 1 pairvec tiles<=4 ragged Cfull slice'),
    ((7, 1, 8, 2, 56, 56), '7 1 pairvec tiles>4 ragged Cfull slices'),
    ((7, 2, 8, 2, 28, 28), '7 2 dwvec tiles<=4 ragged Cfull slice'),
    ((7, 2, 8, 2, 56, 56), '7 2 dwvec tiles<=4 ragged Cfull slice'),
    # whole 16 x 16 tiles, more than four of them; more than one weight-gradient slice (N * tiles > LP_DW_WGRAD_SLICE)
    ((3, 1, 4, 2, 16, 80), '3 1 pairvec tiles>4 whole Cfull slices'),
    ((5, 1, 4, 2, 16, 80), '5 1 pairvec tiles>4 whole Cfull slices'),
    ((7, 1, 4, 2, 16, 80), '7 1 pairvec tiles>4 whole Cfull slices'),
    ((7, 2, 4, 9, 32, 32), '7 2 dwvec tiles<=4 whole Cfull slices'),
    ((7, 1, 4, 3, 32, 32), '7 1 pairvec tiles<=4 whole Cfull slices'),
    ((7, 2, 4, 9, 4, 4), '7 2 dwvec tiles<=4 ragged Cfull slices'),
    ((7, 1, 4, 9, 4, 4), '7 1 pairvec tiles<=4 ragged Cfull slices'),
    ((7, 1, 4, 9, 16, 16), '7 1 pair16 tiles<=4 whole Cfull slices'),
    # two tiles per wave in the stride-2 forward: N * C * tiles >= 65536
    ((7, 2, 8, 8192, 4, 4), '7 2 dwvec2 tiles<=4 ragged Cfull slices'),       # few channels: the fp64 truth is quick
]

# (Ca, Cb, Cout, N, h, w)
DECONV_CASES = [
    ((160, 96, 64, 2, 5, 7), 'even Mfull COfull two slice ragged'),
    ((160, 96, 64, 2, 16, 16), 'even Mfull COfull two slice whole'),
    ((64, 64, 48, 2, 5, 7), 'even Mfull COfull two slice ragged'),
    ((64, 64, 48, 2, 16, 16), 'even Mfull COfull two slice whole'),
    ((64, 48, 40, 2, 5, 7), 'even Mrag COfull two slice ragged'),
    ((64, 48, 40, 2, 16, 16), 'even Mrag COfull two slice whole'),
    # more than one weight-gradient slice (17 tiles of 64 cells), an odd and an even count of 32-row blocks
    ((24, 40, 8, 17, 8, 8), 'even Mfull COfull two slices whole'),
    ((48, 32, 8, 17, 8, 8), 'odd Mrag COfull two slices whole'),
    ((48, 48, 8, 17, 8, 8), 'odd Mfull COfull two slices whole'),
    ((24, 16, 8, 17, 8, 8), 'even Mrag COfull two slices whole'),
    ((24, 40, 8, 17, 4, 4), 'even Mfull COfull two slices ragged'),
    ((24, 16, 8, 17, 4, 4), 'even Mrag COfull two slices ragged'),
]

# (N, H, W)
STEM_CASES = [((17, 16, 32), 'slices whole')]                # 17 whole tiles of 8 x 16 output pixels: two slices

_id = lambda c: 'x'.join(str(v) for v in c[0])               # noqa: E731


# ------------------------------------------------------------------ BatchNorm
def _off_the_kinks(x, gamma, beta, rm, rv, act):
    """The precondition of a case (asserted in _bn_check): no generic cell within EDGE of a kink of the activation, where
    fp32 and fp64 may take different sides.  Among 10^5 random cells and more a few always are, whatever the seed: those
    cells of the INPUT are moved by 0.01 (a few cells of thousands per channel: the statistics move z elsewhere by far
    less than EDGE), before the truth and the device see it."""
    if act is None:
        return
    for _ in range(4):
        z = TF.batch_norm(x.double(), rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), True, MOM, EPS)
        near = z.abs() < 2 * EDGE
        if act == 'relu6':
            near |= (z - 6).abs() < 2 * EDGE
        near[:, :3] = False                                  # the three special channels sit on their kinks on purpose
        if not bool(near.any()):
            return
        x[near] += 0.01


def _bn_check(act, with_res, n, c, h, w):
    """test_batch_norm_act of tests/test_gpu_layer_grad.py with the mean's bound derived for the slice count (module
    docstring); the three special channels of _bn_inputs (gamma = 0 on each kink, a constant input) are kept"""
    x, gamma, beta, rm, rv, res, dy = _bn_inputs(c, n, h, w)
    _off_the_kinks(x, gamma, beta, rm, rv, act)
    cnt = n * h * w
    X, G, B = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    R = res.double().requires_grad_() if with_res else None
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    z = TF.batch_norm(X, rm64, rv64, G, B, True, MOM, EPS)
    y = ACT[act](z) + (R if with_res else 0)
    gx, gg, gb = torch.autograd.grad(y, (X, G, B), dy.double())
    z = z.detach()
    generic = torch.ones(c, dtype=torch.bool)
    generic[:2] = False
    if act is not None:                                      # precondition of the case, not of the code under test
        zz = z[:, generic]
        far = zz.abs() if act == 'relu' else torch.minimum(zz.abs(), (zz - 6).abs())
        assert not far.numel() or float(far.min()) >= EDGE, 'the case has a generic cell on a kink: pick another seed'
    xd64 = x.double()
    mean = xd64.mean((0, 2, 3))
    var = xd64.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    bc = lambda t: t.view(1, -1, 1, 1)                       # noqa: E731
    xd, gd, bd, rd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), res.cuda() if with_res else None, dy.cuda()
    running = torch.stack([rm, rv]).cuda()
    yd, stat = F.bn_forward(xd, gd, bd, running, act, rd, True, MOM, EPS)
    ax = (xd64.abs() + bc(mean.abs())) * bc(invstd)          # the terms of xhat
    terms_y = ax * bc(gamma.double().abs()) + bc(beta.double().abs()) + (res.double().abs() if with_res else 0)
    _held(yd, y.detach(), (6 if with_res else 5) * U * terms_y, 'bn y')
    vec, units, S, chunk = FM.bn_geometry(n, c, h * w)
    depth = (2 if vec else 0) + math.ceil(chunk / 256) + 8 + S
    _held(stat[0], mean, (depth + 2) * 2.0 ** -53 * xd64.abs().mean((0, 2, 3)), 'bn mean (fp64, depth %d)' % depth)
    assert torch.allclose(stat[1].cpu(), invstd, rtol=1e-9, atol=0)
    _held(running[0], rm64, 3 * U * ((1 - MOM) * rm.double().abs() + MOM * mean.abs()), 'running_mean')
    unb = var * (cnt / (cnt - 1.0))
    _held(running[1], rv64, 3 * U * ((1 - MOM) * rv.double().abs() + MOM * unb), 'running_var')
    outs = _twice_and_replayed(lambda: F.bn_backward(dyd, xd, gd, bd, stat, act), 'bn backward')
    g = dy.double() * ((z > 0) & ((z < 6) if act == 'relu6' else True) if act else 1.0)
    a1 = g.abs().mean((0, 2, 3))
    a2 = (g.abs() * ax).mean((0, 2, 3))
    k = bc(gamma.double().abs() * invstd)
    _held(outs[0], gx, 3 * U * k * (g.abs() + bc(a1) + ax * bc(a2)), 'bn dx')
    _held(outs[1], gg, 3 * U * a2 * cnt, 'bn dgamma')
    _held(outs[2], gb, 3 * U * a1 * cnt, 'bn dbeta')
    if act is not None:
        assert not bool(outs[0][:, 0].any()), 'gradient through z = 0 must be zero'
    if act == 'relu6':
        assert not bool(outs[0][:, 1].any()), 'gradient through z = 6 must be zero'
    assert float(stat[1][2].cpu()) == pytest.approx(EPS ** -0.5, rel=1e-9)
    # ---- eval mode at the same shape: the running pair is the statistics; nothing but y is written
    before = running.clone()
    ye, none = F.bn_forward(xd, gd, bd, running, act, rd, False, MOM, EPS)
    assert none is None and po.bitwise_equal(before, running)
    rm2, rv2 = before[0].cpu().double(), before[1].cpu().double()
    ze = TF.batch_norm(xd64, rm2, rv2, gamma.double(), beta.double(), False, MOM, EPS)
    inv2 = 1.0 / torch.sqrt(rv2 + EPS)
    terms_e = (xd64.abs() + bc(rm2.abs())) * bc(inv2 * gamma.double().abs()) + bc(beta.double().abs()) + \
        (res.double().abs() if with_res else 0)
    _held(ye, ACT[act](ze) + (res.double() if with_res else 0), (6 if with_res else 5) * U * terms_e, 'bn y (eval)')


@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('act', [None, 'relu'], ids=['none', 'relu'])
@pytest.mark.parametrize('case', BN_CASES[:BN_ALL_ACTS], ids=_id)
def test_batch_norm_over_slices_every_activation(case, act, with_res):
    _bn_check(act, with_res, *case[0])


@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('case', BN_CASES, ids=_id)
def test_batch_norm_over_slices(case, with_res):
    _bn_check('relu6', with_res, *case[0])


# ------------------------------------------------------------------ 1x1
@pytest.mark.parametrize('case', PW_CASES, ids=_id)
def test_pointwise_forms(case):
    _pw_check(*case[0], 'both')


@pytest.mark.parametrize('mode', ['both', 'dx', 'dw'])
@pytest.mark.parametrize('case', PW_ODD_CASES, ids=_id)
def test_pointwise_odd_channels(case, mode):
    _pw_check(*case[0], mode)


# ------------------------------------------------------------------ depthwise
@pytest.mark.parametrize('case', DW_CASES, ids=_id)
def test_depthwise_forms(case):
    k, s, c, n, h, w = case[0]
    _dw_check(k, s, c, n, h, w, modes=('both',))


# ------------------------------------------------------------------ transposed-convolution pair, stem
@pytest.mark.parametrize('case', DECONV_CASES, ids=_id)
def test_deconv_pair_forms(case):
    _deconv_check(*case[0], 'both')


@pytest.mark.parametrize('case', STEM_CASES, ids=_id)
def test_stem_forms(case):
    _stem_check(*case[0])


# ------------------------------------------------------------------ buffers
@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'res'])
def test_multi_slice_batch_norm_buffer_contract(with_res):
    """the Arena contract of tests/test_gpu_layer_buffers.py at four slices per channel: a workspace of exactly
    lp_bn_workspace_bytes, guards intact, one byte less answers LP_ERR_WORKSPACE"""
    n, c, h, w = BN_CASES[0][0]
    assert FM.bn_slices(n, c, h * w) == 4
    _bn_buffer_contract((n, c, h * w), with_res)


@pytest.mark.parametrize('want', ['both', 'x', 'w'])
def test_odd_channel_pointwise_buffer_contract(want):
    """the same contract for a 1x1 of 24 -> 17 channels: the transposed pack's odd tail pair and 17 rows of dW"""
    _pw_buffer_contract((3, 24, 17, 35), want)
    _pw_buffer_contract((2, 24, 17, 64), want)
