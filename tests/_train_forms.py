"""The FORM of a training-layer call: which kernel variant, slice count and edge path its shape selects.

The host code of the training layers picks by size: ``bn_cut`` cuts a channel into slices, ``launch_pw`` picks a tile of
``pw2_kernel<NB, PXV>`` from a cost model, the weight gradients are cut into slices of ``LP_*_WGRAD_SLICE``, the depthwise
forward has four kernel families.  A test at a small shape runs the forms small shapes select, so the tests of the forms a
real training step selects need to know them.  One function per layer kind maps a call's shape to a tuple, its form key.

Every component is either one of the library's host queries -- ``lp_pw_tile_choice``, ``lp_bn_workspace_bytes`` (16 bytes per
channel and slice), the ``*_backward_workspace_bytes`` calls (one partial per slice) -- or a condition that stands as one
comparison in a launcher (``HW % 4``, ``H == 16 && W == 16``, ``units >= 65536``).  No cost model is restated here.

``calls(cfg, arch, res)`` lists the distinct layer calls of a ``TrainableLitePose`` (the walk is ``layer_shapes`` of
tools/time_layer_grad.py, imported from there) and ``call_forms`` the keys each one reaches, forward and backward."""
import importlib.util
import os
import re

from litepose_amd import _native as nv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _macro(name):
    with open(os.path.join(ROOT, 'include', 'litepose_amd.h')) as f:
        return int(re.search(r'#define\s+%s\s+(\d+)' % name, f.read()).group(1))


PW_SLICE, DW_SLICE = _macro('LP_PW_WGRAD_SLICE'), _macro('LP_DW_WGRAD_SLICE')
DECONV_SLICE, STEM_SLICE = _macro('LP_DECONV_WGRAD_SLICE'), _macro('LP_STEM_WGRAD_SLICE')
BN_MAX_SLICES = 64                   # bn_cut: "cut into S <= 64 slices"


def _ceil(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ BatchNorm
def bn_slices(n, c, hw):
    """S of bn_cut: the workspace holds one double2 per channel and slice"""
    b = nv.lib().lp_bn_workspace_bytes(n, c, hw)
    assert b > 0 and b % (16 * c) == 0, (n, c, hw, b)
    return b // (16 * c)


def bn_geometry(n, c, hw):
    """-> vec, units per plane, S, chunk (units per slice: the S slices of ceil(total / S) units cover the total, the last
    one possibly shorter -- what bn_cut's two divisions amount to)"""
    vec = hw % 4 == 0
    units = hw // 4 if vec else hw
    S = bn_slices(n, c, hw)
    chunk = _ceil(n * units, S)
    assert _ceil(n * units, chunk) == S
    return vec, units, S, chunk


def bn_form(n, c, h, w, res):
    """(load form, slices, steps per lane, walk, chunk ragged against 256, residual)
    steps: ceil(chunk / 256) walks of bn_walk per lane -- 'step' 1, 'two' 2 (all an uncapped cut ever gives: it aims at 512
    units per slice), 'many' 3 or more (only under a cap)
    slices: 'one'; 'cap' at the limit -- 64, or the lower one a wide layer sets itself (the largest slice count any batch gives
    this C and plane: asked of the library at a batch 64 times larger); 'several' otherwise
    walk: how bn_walk steps 256 units on -- 'wide' units >= 256 (dn = 0), 'even' units divides 256 (di = 0, never a carry),
    'rem' units < 256 with a remainder (dn > 0 and a carry)"""
    vec, units, S, chunk = bn_geometry(n, c, h * w)
    if S == 1:
        sl = 'one'
    else:
        sl = 'cap' if S == BN_MAX_SLICES or bn_slices(64 * n, c, h * w) == S else 'several'
    walk = 'wide' if units >= 256 else ('even' if 256 % units == 0 else 'rem')
    steps = _ceil(chunk, 256)
    return ('bn', 'vec' if vec else 'scalar', sl, 'step' if steps == 1 else ('two' if steps == 2 else 'many'), walk,
            'ragged' if chunk % 256 else 'full', 'res' if res else 'plain')


def bn_inside_plane(n, c, h, w):
    """a slice boundary falls inside a plane"""
    vec, units, S, chunk = bn_geometry(n, c, h * w)
    return S > 1 and chunk % units != 0


# ------------------------------------------------------------------ 1x1
def pw_tile(n, k, m, hw):
    """(NB, PXV) of the 1x1 over k input channels and m output channels as the training calls run it"""
    v = nv.lib().lp_pw_tile_choice(n, k, 0, m, hw, 0)
    assert v > 0, (n, k, m, hw, v)
    return v // 16, v % 16


def pw_mm_form(n, k, m, h, w, what):
    """what 'fwd' (k = Cin, m = Cout) or 'dx' (k = Cout, m = Cin, weights packed transposed)
    (what, NB, PXV, K odd, M % 32 != 0, cblocks % NB != 0)"""
    nb, pxv = pw_tile(n, k, m, h * w)
    cblocks = _ceil(m, 32)
    return ('pw', what, nb, pxv, 'Kodd' if k % 2 else 'Keven', 'Mrag' if m % 32 else 'Mfull',
            'cbrag' if cblocks % nb else 'cbfull')


def pw_dw_slices(n, cin, cout, hw):
    b = nv.lib().lp_pw_backward_workspace_bytes(n, cin, cout, hw, 0, 1)
    assert b > 0 and b % (4 * cin * cout) == 0
    return b // (4 * cin * cout)


def pw_dw_form(n, cin, cout, h, w):
    """(load form, slices, Cin > 128: blockIdx.z > 0, ceil(Cin / 32) % 4 != 0: idle waves in the last z block, Cout % 32,
    Cin % 32); slices: 'one', 'even' (several, all full), 'ragged' (3 or more, the last one shorter), 'two' (2, ragged)"""
    hw = h * w
    S = pw_dw_slices(n, cin, cout, hw)
    if S == 1:
        sl = 'one'
    elif (n * hw) % PW_SLICE == 0:
        sl = 'even'
    else:
        sl = 'ragged' if S >= 3 else 'two'
    return ('pwdw', 'vec' if hw % 4 == 0 else 'scalar', sl, 'z>0' if cin > 128 else 'z0',
            'idle' if _ceil(cin, 32) % 4 else 'busy', 'COrag' if cout % 32 else 'COfull', 'CIrag' if cin % 32 else 'CIfull')


# ------------------------------------------------------------------ depthwise
def dw_slices(n, c, h, w, k, s):
    b = nv.lib().lp_dw_backward_workspace_bytes(n, c, h, w, k, s, 1)
    assert b > 0 and b % (4 * c * k * k) == 0
    return b // (4 * c * k * k)


def dw_form(n, c, h, w, k, s):
    """(K, S, forward family, tiles > 4: the XCD remap of the paired kernels, plane ragged against 16, C % 4 != 0, more than
    one dW slice).  Families (launch_dw): stride 1 -> 'pair16' (16 x 16), 'pairvec' (W % 4 == 0), 'pairscalar'; stride 2 ->
    'dwvec' / 'dwscalar' by W % 4, with '2' appended when a wave takes two tiles (N C tiles >= 65536).  ragged: of the OUTPUT
    plane, which the forward, and the weight gradient's 16 x 16 units, tile."""
    oh, ow = (h - 1) // s + 1, (w - 1) // s + 1
    tiles = _ceil(oh, 16) * _ceil(ow, 16)
    if s == 1:
        fam = 'pair16' if (h, w) == (16, 16) else ('pairvec' if w % 4 == 0 else 'pairscalar')
        many = tiles > 4 and fam != 'pair16'
    else:
        fam = ('dwvec' if w % 4 == 0 else 'dwscalar') + ('2' if n * c * tiles >= 65536 else '')
        many = False
    return ('dw', k, s, fam, 'tiles>4' if many else 'tiles<=4', 'ragged' if (oh % 16 or ow % 16) else 'whole',
            'Crag' if c % 4 else 'Cfull', 'slices' if dw_slices(n, c, h, w, k, s) > 1 else 'slice')


# ------------------------------------------------------------------ transposed-convolution pair, stem
def deconv_slices(n, ca, cb, cout, h, w):
    b = nv.lib().lp_deconv_backward_workspace_bytes(n, ca, cb, cout, h, w, 0, 1)
    per = 4 * (ca + cb) * cout * 16
    assert b > 0 and b % per == 0
    return b // per


def deconv_form(n, ca, cb, cout, h, w):
    """(row blocks of Ca + Cb: 'one', 'even' or 'odd' -- the data gradient takes two per workgroup --, rows % 32 != 0,
    Cout % 8 != 0, sources, weight-gradient slices 'slice' / 'slices', plane ragged against the 8 x 8 tile)"""
    rbs = _ceil(ca + cb, 32)
    S = deconv_slices(n, ca, cb, cout, h, w)
    return ('deconv', 'one' if rbs == 1 else ('odd' if rbs % 2 else 'even'), 'Mrag' if (ca + cb) % 32 else 'Mfull',
            'COrag' if cout % 8 else 'COfull', 'two' if cb else 'one', 'slices' if S > 1 else 'slice',
            'ragged' if (h % 8 or w % 8) else 'whole')


def stem_form(n, h, w):
    b = nv.lib().lp_stem_backward_workspace_bytes(n, h, w)
    assert b > 0 and b % 3456 == 0
    return ('stem', 'slices' if b // 3456 > 1 else 'slice', 'ragged' if ((h // 2) % 8 or (w // 2) % 16) else 'whole')


# ------------------------------------------------------------------ the calls of a module
def _tool():
    spec = importlib.util.spec_from_file_location('time_layer_grad', os.path.join(ROOT, 'tools', 'time_layer_grad.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_layer_shapes = None


def calls(cfg, arch, res):
    """the distinct (kind, ...) layer shapes of get_train_net(cfg, arch) on a res x res image, in network order"""
    global _layer_shapes
    if _layer_shapes is None:
        _layer_shapes = _tool().layer_shapes
    return [shape for shape, _ in _layer_shapes(cfg, arch, res)]


def call_forms(shape, n):
    """every form key the layer call `shape` (an entry of calls()) reaches at batch n, forward and backward"""
    kind = shape[0]
    if kind == 'pw':
        _, ci, co, h, w = shape
        return [pw_mm_form(n, ci, co, h, w, 'fwd'), pw_mm_form(n, co, ci, h, w, 'dx'), pw_dw_form(n, ci, co, h, w)]
    if kind == 'dw':
        _, c, k, s, h, w = shape
        return [dw_form(n, c, h, w, k, s)]
    if kind == 'stem':
        return [stem_form(n, shape[1], shape[2])]
    if kind == 'deconv':
        _, ca, cb, co, h, w = shape
        return [deconv_form(n, ca, cb, co, h, w)]
    _, c, h, w, act, has_res = shape
    return [bn_form(n, c, h, w, has_res)]
