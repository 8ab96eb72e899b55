"""The range edges of fp16 storage (LP_STORAGE_F16) through every 16-bit kernel form: the table of rows, the state dicts
that push one tensor of one launch into the SUBNORMAL range [2^-24, 2^-14) or past the largest finite half (65504), the
derived bound, and the checks (tests/test_f16_range_cpu.py, tests/test_gpu_f16_range.py).  Importable without a GPU.

A row is ``(id, arch, H, W, N, options, tag, op, position, edge)``.  ``arch`` is a published name or 'custom:NAME' (an
entry of tests/_custom_space.py's ARCHS); ``options`` are the lp_net_set_option switches that select the form (the ones
of tests/test_gpu_kernel_census.py's CASES); ``tag`` is the ``last_kernel_tag`` the launch that STORES ``op`` must carry;
``op`` is that launch's stored tensor (tests/_f16_ref.py names) and the tensor that is compared; ``position`` names which
tensor of the launch is pushed to the edge; ``edge`` is 'sub' or 'top'.

Positions, 'sub' rows.  ``2^U`` below is a magnitude 2^u, u uniform in the row's window (default [-23.5, -14.5]: the
whole subnormal range), random sign, the layer's BatchNorm at (1, 0, 0, 1) so that it adds no bias ("neutral"):
  * one-op forms: 'w' = the op's folded weights are 2^U, its inputs normal, its stored outputs subnormal; 'x' = the
    PRODUCER of the op's input has 2^U weights, so the op reads a subnormal tensor through normal weights (neutral
    BatchNorm on the op: a bias would bury the result).
  * fused blocks (mbtd / mbtb / mbtb_s2; ``op`` = the block's point_conv): 'x' = the block input (and the residual, which
    is the same tensor) subnormal; 'expand' = the expanded tensor E in LDS; 'dw' = the depthwise weights, so the second
    inner tensor; 'project' = the 1x1's weights, so the stored output.  A RESIDUAL block stores pw(D) + x: a subnormal
    inner tensor shows in the output only where x's own spacing is the subnormal one, so the residual rows make x
    subnormal as well ('expand': x subnormal and the expand weights 2^[-3, 1], E higher in the range than x; 'dw' and
    'project': the layers before keep their biases, so their tensors are normal).
  * stem4_kernel: 'conv', 'dw3', 'pw' = the weights of that op are 2^U, the ops after it neutral.
  * headb_kernel (``op`` = final.1.pw, fp32 and unrounded): 'in_refined' / 'in_raw' = that depthwise's input is
    subnormal and the OTHER source's 1x1 weights are zero (its O(1) terms would hide the result in the fp32
    accumulation allowance); 'pw' = both 1x1 weight halves are 2^U.
'top' rows: the BatchNorm gain of ``op`` is multiplied by the row's GAINS entry, so that part of its linear output
passes 65504.

The bound is derived, not measured (``evaluate``): the unit of an element is ``ulp16`` -- one fp16 ulp of the emulated
value, at least the subnormal spacing 2^-24, plus 2^-20 of the magnitude sum of its terms (fp32 accumulation in two
orders).  A launch that stores its own op on the device's own inputs is within 1 unit.  A fused launch is compared with
the emulation chained through the tensors it never stores; each inner element may round the other way (its own unit),
and the next op carries that through |w| (the absolute plan's linear part; ReLU / ReLU6 are 1-Lipschitz), once more for
a second inner tensor; the stored element adds its own unit (the fp32 head: the accumulation term alone).  A flush moves
an inner value by up to 2^10 spacings, far outside."""
import copy

import torch

import _f16_ref
from oracle import synth

F16_ULP_REL = 2.0 ** -10
ACC_REL = 2.0 ** -20          # of an element's term magnitude sum: the fp32 accumulation allowance (see ulp16)
SUB_SPACING = 2.0 ** -24
NORMAL_MIN = 2.0 ** -14
F16_MAX = 65504.0
F16_INF_AT = 65520.0          # the tie between 65504 and 2^16: rounds to even = up, to inf
SUB_BOUND_MAX = 2.0 ** -17    # 2^7 spacings: the flush of one full-size subnormal input is outside every 'sub' bound


def ulp16(exp, mag):
    """The unit of the per-launch bound: one fp16 ulp of the emulated value (2^-10 relative, at least the subnormal
    spacing 2^-24) plus 2^-20 of the sum of the magnitudes of the terms the element adds (tests/_f16_ref.py, absolute
    plan).  The second term is the fp32 accumulation error of two summation orders (the device's MFMA / FMA order, the
    CPU's): invisible at bf16 resolution, at fp16 resolution it shows where the terms cancel -- measured: an output of
    1.3e-3 from terms of magnitude sum 44.8 (2.9e-6 apart, 3 fp16 ulps of the value) in 1-2 of 800 k elements of a 7x7
    depthwise.  Everywhere else it is far below the ulp (an output of 1 from terms of magnitude 10: 1e-5 against 1e-3)."""
    return torch.clamp(exp.abs() * F16_ULP_REL, min=SUB_SPACING) + ACC_REL * mag


XS = 'search-XS'
SUB = (-23.5, -14.5)
_CHAIN = {'mbtb': 0}                       # one launch per block op
_B = 'stage.0.1.point_conv'                # the first residual block of search-XS (16 channels, 32 x 32 at 128 pixels)


def _row(rid, options, tag, op, position, edge='sub', arch=XS, H=128, W=128, N=1):
    return (rid, arch, H, W, N, options, tag, op, position, edge)


# (id, arch, H, W, N, options, tag, op, position, edge).  search-XS at 128 pixels: stem 64 x 64, stage 0 on 32 x 32 (the
# smallest plane launch_dwt admits), stages 2 / 3 on 8 x 8, the heads on 32 x 32 and 64 x 64
ROWS = [
    # ---- one-op forms
    _row('stemb_w', {'stem': 0}, 'stemb_kernel', 'stem.conv3x3s2', 'w'),
    _row('dwb31_w', {'stem': 0}, 'dwb_kernel<3,1>', 'stem.dw3', 'w'),
    _row('dwb31_x', {'stem': 0}, 'dwb_kernel<3,1>', 'stem.dw3', 'x'),
    _row('pwb_stem_w', {'stem': 0}, 'pwb_kernel', 'stem.pw', 'w'),
    _row('pwb_w', _CHAIN, 'pwb_kernel', 'stage.0.1.inv', 'w'),
    _row('pwb_x', _CHAIN, 'pwb_kernel', 'stage.0.0.point_conv', 'x'),
    _row('dwb72_w', _CHAIN, 'dwb_kernel<7,2>', 'stage.0.0.depth_conv', 'w'),
    _row('dwb72_x', _CHAIN, 'dwb_kernel<7,2>', 'stage.0.0.depth_conv', 'x'),
    _row('dwb71_w', {'mbtb': 0, 'dwt': 0}, 'dwb_kernel<7,1>', 'stage.0.1.depth_conv', 'w'),
    _row('dwb71_x', {'mbtb': 0, 'dwt': 0}, 'dwb_kernel<7,1>', 'stage.0.1.depth_conv', 'x'),
    _row('dwt7_w', _CHAIN, 'dwt_kernel<7>', 'stage.0.1.depth_conv', 'w'),
    _row('dwt7_x', _CHAIN, 'dwt_kernel<7>', 'stage.0.1.depth_conv', 'x'),
    _row('dwt5_w', {'headb': 0}, 'dwt_kernel<5>', 'final_refined.0.dw5', 'w'),
    _row('dwt5_x', {'headb': 0}, 'dwt_kernel<5>', 'final_refined.0.dw5', 'x'),
    _row('dwb51_w', {'dwt': 1}, 'dwb_kernel<5,1>', 'final_refined.0.dw5', 'w'),
    _row('dwb51_x', {'dwt': 1}, 'dwb_kernel<5,1>', 'final_refined.0.dw5', 'x'),
    # the stride-2 5x5 / 3x3 depthwise: tests/_custom_space.py's 'five' (row five_128)
    _row('dwb52_w', {}, 'dwb_kernel<5,2>', 'stage.2.0.depth_conv', 'w', arch='custom:five'),
    _row('dwb52_x', {}, 'dwb_kernel<5,2>', 'stage.2.0.depth_conv', 'x', arch='custom:five'),
    _row('dwb32_w', {}, 'dwb_kernel<3,2>', 'stage.3.0.depth_conv', 'w', arch='custom:five'),
    _row('dwb32_x', {}, 'dwb_kernel<3,2>', 'stage.3.0.depth_conv', 'x', arch='custom:five'),
    _row('deconvb_w', {}, 'deconvb_kernel', 'deconv.0', 'w'),
    # both sources of deconv.0 subnormal: 'mb24' has one block in each of its last two stages, so neither source is a
    # residual sum (EXPLICIT below)
    _row('deconvb_x', {}, 'deconvb_kernel', 'deconv.0', 'x', arch='custom:mb24'),
    # ---- fused blocks
    _row('mbtd_x', {}, 'mbtd_kernel', _B, 'x'),
    _row('mbtd_expand', {}, 'mbtd_kernel', _B, 'expand'),
    _row('mbtd_dw', {}, 'mbtd_kernel', _B, 'dw'),
    _row('mbtd_project', {}, 'mbtd_kernel', _B, 'project'),
    _row('mbtb_x', {'mbtd': 0}, 'mbtb_kernel', _B, 'x'),
    _row('mbtb_expand', {'mbtd': 0}, 'mbtb_kernel', _B, 'expand'),
    _row('mbtb_dw', {'mbtd': 0}, 'mbtb_kernel', _B, 'dw'),
    _row('mbtb_project', {'mbtd': 0}, 'mbtb_kernel', _B, 'project'),
    # the widening stride-1 block 48 -> 80 (mbtb_kernel<3, 3, false>): its input is a residual sum, no 'x' row
    _row('mbtb_wide_expand', {}, 'mbtb_kernel', 'stage.3.0.point_conv', 'expand'),
    _row('mbtb_wide_dw', {}, 'mbtb_kernel', 'stage.3.0.point_conv', 'dw'),
    _row('mbtb_wide_project', {}, 'mbtb_kernel', 'stage.3.0.point_conv', 'project'),
    _row('mbtb_s2_x', {}, 'mbtb_s2_kernel', 'stage.0.0.point_conv', 'x'),
    _row('mbtb_s2_expand', {}, 'mbtb_s2_kernel', 'stage.0.0.point_conv', 'expand'),
    _row('mbtb_s2_dw', {}, 'mbtb_s2_kernel', 'stage.0.0.point_conv', 'dw'),
    _row('mbtb_s2_project', {}, 'mbtb_s2_kernel', 'stage.0.0.point_conv', 'project'),
    # ---- the fused stem and head
    _row('stem4_conv', {}, 'stem4_kernel', 'stem.pw', 'conv'),
    _row('stem4_dw3', {}, 'stem4_kernel', 'stem.pw', 'dw3'),
    _row('stem4_pw', {}, 'stem4_kernel', 'stem.pw', 'pw'),
    _row('headb_in_refined', {}, 'headb_kernel', 'final.1.pw', 'in_refined'),
    _row('headb_in_raw', {}, 'headb_kernel', 'final.1.pw', 'in_raw'),
    _row('headb_pw', {}, 'headb_kernel', 'final.1.pw', 'pw'),
    # ---- 'top': every form that stores a linear tensor (deconvb_kernel: ReLU keeps +inf)
    _row('top_pwb', _CHAIN, 'pwb_kernel', 'stage.0.0.point_conv', 'project', 'top'),
    _row('top_pwb_res', _CHAIN, 'pwb_kernel', _B, 'project', 'top'),
    _row('top_mbtd', {}, 'mbtd_kernel', _B, 'project', 'top'),
    _row('top_mbtb', {'mbtd': 0}, 'mbtb_kernel', _B, 'project', 'top'),
    _row('top_mbtb_wide', {}, 'mbtb_kernel', 'stage.3.0.point_conv', 'project', 'top', N=2),
    _row('top_mbtb_s2', {}, 'mbtb_s2_kernel', 'stage.0.0.point_conv', 'project', 'top'),
    _row('top_stem4', {}, 'stem4_kernel', 'stem.pw', 'pw', 'top'),
    _row('top_pwb_stem', {'stem': 0}, 'pwb_kernel', 'stem.pw', 'pw', 'top'),
    _row('top_deconvb', {}, 'deconvb_kernel', 'deconv.0', 'w', 'top', N=2),
]

# 16-bit tags no 'sub' row carries, with the reason (tests/test_f16_range_cpu.py)
UNREACHED = {}

# row id -> {op: (lo, hi)}: windows narrowed (or moved) so that the emulated target tensor stays in the subnormal range
# after the op's summation; tuned on the emulation alone by tests/test_f16_range_cpu.py's preconditions
_LOW = (-23.5, -17.5)
_XE = {'stage.0.0.point_conv': _LOW}      # residual 'expand': x low in the range, E (weights 2^BOOST) above it
WINDOWS = {
    'dwt5_x': {'deconv.1': _LOW}, 'dwb51_x': {'deconv.1': _LOW}, 'deconvb_w': {'deconv.0': (-23.5, -18.5)},
    'headb_in_refined': {'deconv.2': _LOW},
    'mbtd_expand': _XE, 'mbtb_expand': _XE,
    'mbtb_wide_expand': {'stage.3.0.inv': (-23.5, -16.0)},
    'mbtb_wide_project': {'stage.3.0.point_conv': (-23.5, -19.5)},
    'mbtb_s2_project': {'stage.0.0.point_conv': _LOW},
}

# row id -> the factor on the BatchNorm gain of a 'top' row's op, tuned on the emulation alone like WINDOWS
GAINS = {'top_pwb': 32768.0, 'top_pwb_res': 80000.0, 'top_mbtd': 80000.0, 'top_mbtb': 80000.0, 'top_mbtb_wide': 40000.0,
         'top_mbtb_s2': 32768.0, 'top_stem4': 12000.0, 'top_pwb_stem': 12000.0, 'top_deconvb': 16000.0}

# rows whose recipe is written out: {'mags': {op: window}, 'neutral': [ops], 'target': tensor whose shares are measured}
_S3 = ['stage.3.0.inv', 'stage.3.0.depth_conv', 'stage.3.0.point_conv']
EXPLICIT = {
    'deconvb_x': {'mags': {'stage.2.0.point_conv': SUB}, 'neutral': _S3 + ['deconv.0'], 'target': 'stage.2.0.point_conv'},
}

BOOST = (-3.0, 1.0)           # the expand weights of a residual block's 'expand' row
SEED = 5


def row(rid):
    return {r[0]: r for r in ROWS}[rid]


def arch_of(r):
    if r[1].startswith('custom:'):
        import _custom_space
        return copy.deepcopy(_custom_space.ARCHS[r[1][len('custom:'):]])
    from litepose_amd import arch_zoo
    return arch_zoo.get(r[1])


def images(r):
    return synth.make_images(r[4], r[2], seed=41, w=r[3])


def layer_keys(op):
    """(weight keys, BatchNorm prefix or None) of a plan op in the reference's state dict."""
    if op == 'stem.conv3x3s2':
        return ['first.0.0.weight'], 'first.0.1'
    if op == 'stem.dw3':
        return ['first.1.0.weight'], 'first.1.1'
    if op == 'stem.pw':
        return ['first.2.weight'], 'first.3'
    if op.startswith('stage.'):
        return [op + '.0.weight'], op + '.1'
    if op.startswith('deconv.'):
        i = op.split('.')[1]
        return ['deconv_refined.%s.weight' % i, 'deconv_raw.%s.weight' % i], 'deconv_bnrelu.%s.0' % i
    if op.endswith('.dw5'):
        p = op[:-len('.dw5')] + '.conv'
        return [p + '.0.weight'], p + '.1'
    if op.startswith('final.') and op.endswith('.pw'):
        k = op.split('.')[1]
        return ['final_refined.%s.conv.3.weight' % k, 'final_raw.%s.conv.3.weight' % k], None
    raise KeyError(op)


def launch_inner(r):
    """The tensors the row's launch keeps on the CU, in plan order (tests/_net_check.py: fused_inner)."""
    tag, op = r[6], r[7]
    if tag in ('mbtd_kernel', 'mbtb_kernel', 'mbtb_s2_kernel'):
        p = op[:-len('.point_conv')]
        return [p + '.inv', p + '.depth_conv']
    if tag == 'stem4_kernel':
        return ['stem.conv3x3s2', 'stem.dw3']
    if tag == 'headb_kernel':
        k = op.split('.')[1]
        return ['final_refined.%s.dw5' % k, 'final_raw.%s.dw5' % k]
    return []


def recipe(r, ins):
    """{'mags': {op: window}, 'neutral': [ops], 'zero': [weight keys], 'gain': {op: factor}, 'target': tensor} of a row;
    ``ins`` = {op: input names} of the plan."""
    rid, op, pos, edge = r[0], r[7], r[8], r[9]
    out = {'mags': {}, 'neutral': [], 'zero': [], 'gain': {}, 'target': op}
    if edge == 'top':
        out['gain'][op] = GAINS.get(rid, 1.0)
        return out
    if rid in EXPLICIT:
        out.update(copy.deepcopy(EXPLICIT[rid]))
    elif r[6] in ('mbtd_kernel', 'mbtb_kernel', 'mbtb_s2_kernel'):
        p = op[:-len('.point_conv')]
        inv, dw = p + '.inv', p + '.depth_conv'
        src, residual = ins[inv][0], len(ins[op]) == 2
        if pos == 'x' or residual:
            assert len(ins[src]) == 1 and src != 'x', 'the block input must not be a residual sum: %s' % src
            out['mags'][src] = SUB
        if pos == 'x':
            out['neutral'], out['target'] = [inv, dw, op], src
        elif pos == 'expand':
            out['mags'][inv] = BOOST if residual else SUB
            out['neutral'], out['target'] = [dw, op], inv
        elif pos == 'dw':
            out['mags'][dw] = SUB
            out['neutral'], out['target'] = [op], dw
        else:
            assert pos == 'project', pos
            out['mags'][op] = SUB
    elif r[6] == 'stem4_kernel':
        chain = ['stem.conv3x3s2', 'stem.dw3', 'stem.pw']
        k = {'conv': 0, 'dw3': 1, 'pw': 2}[pos]
        out['mags'][chain[k]] = SUB
        out['neutral'], out['target'] = chain[k + 1:], chain[k]
    elif r[6] == 'headb_kernel':
        k = op.split('.')[1]
        if pos == 'pw':
            out['mags'][op] = SUB
        else:
            mine, other = ('refined', 'raw') if pos == 'in_refined' else ('raw', 'refined')
            dw5 = 'final_%s.%s.dw5' % (mine, k)
            src = ins[dw5][0]
            assert len(ins[src]) != 2 or src.startswith('deconv.'), src
            out['mags'][src] = SUB
            out['neutral'], out['target'] = [dw5], src
            out['zero'] = ['final_%s.%s.conv.3.weight' % (other, k)]
    elif pos == 'w':
        out['mags'][op] = SUB
    else:
        assert pos == 'x' and len(ins[op]) == 1, (rid, pos)
        src = ins[op][0]
        assert src.startswith('deconv.') or len(ins[src]) == 1, 'the input must not be a residual sum: %s' % src
        out['mags'][src] = SUB
        out['neutral'], out['target'] = [op], src
    for o, w in WINDOWS.get(rid, {}).items():
        assert o in out['mags'], (rid, o)
        out['mags'][o] = w
    return out


def _neutral(sd, bn):
    for p, v in (('.weight', 1.0), ('.bias', 0.0), ('.running_mean', 0.0), ('.running_var', 1.0)):
        sd[bn + p] = torch.full_like(sd[bn + p], v)


def edge_state_dict(arch, r):
    """The synthetic state dict (seed 1234) with the row's tensor pushed to the edge, see the module docstring; seeded."""
    sd = synth.make_state_dict(arch, seed=1234)
    ins = {n: i for n, i, _ in _f16_ref.plan(sd, arch)}
    rc = recipe(r, ins)
    g = torch.Generator().manual_seed(SEED)
    for op, (lo, hi) in rc['mags'].items():
        keys, bn = layer_keys(op)
        for k in keys:
            w = sd[k]
            mag = 2.0 ** (lo + (hi - lo) * torch.rand(w.shape, generator=g))
            sd[k] = (mag * torch.sign(torch.randn(w.shape, generator=g))).float()
        if bn is not None:
            _neutral(sd, bn)
    for op in rc['neutral']:
        bn = layer_keys(op)[1]
        if bn is not None:
            _neutral(sd, bn)
    for k in rc['zero']:
        sd[k] = torch.zeros_like(sd[k])
    for op, f in rc['gain'].items():
        bn = layer_keys(op)[1]
        sd[bn + '.weight'] = sd[bn + '.weight'] * float(f)
    return sd, rc


class _StoreRounding:
    """``rh`` while the plan folds its weights, then switchable: off, an op returns its value BEFORE the store rounding."""

    def __init__(self):
        self.on = True

    def __call__(self, t):
        return _f16_ref.rh(t) if self.on else t


def _is_head(name):
    return name.startswith('final.') and name.endswith('.pw')


def evaluate(r, sd, arch, x, target, stored=None):
    """Walk the emulation to the row's op.  ``stored(name, shape)`` returns the device's tensor of a stored op (float32 on
    the CPU) or None for a tensor no launch stored; ``stored`` = None: the emulation alone.  The tensors the row's launch
    keeps on the CU are chained through the emulation and carry the bound (module docstring).
    Returns {'exp', 'raw' (the op before its store rounding), 'got' (None without ``stored``), 'bound', 'target' (the
    emulated -- or, for a stored input, the device's -- tensor named by the row's position)}."""
    op = r[7]
    inner = launch_inner(r)
    launch = set(inner) | {op}
    rnd = _StoreRounding()
    plan = _f16_ref.plan(sd, arch)
    mags = {n: fn for n, _, fn in _f16_ref.plan(sd, arch, absolute=True)}
    raw_fn = {n: fn for n, _, fn in _f16_ref.plan(sd, arch, rnd=rnd)}[op]
    vals, err, res, slack = {'x': x}, {}, {}, None
    with torch.no_grad():
        for name, ins, fn in plan:
            args = [vals[k] for k in ins]
            exp = fn(*args)
            if name in launch:
                zeros = [torch.zeros_like(a) for a in args]
                carried = mags[name](*[err.get(k, z) for k, z in zip(ins, zeros)]) - mags[name](*zeros)
                mag = mags[name](*args)
                slack = ACC_REL * mag + carried          # of the value BEFORE the store rounding
                err[name] = (ACC_REL * mag if _is_head(name) else ulp16(exp, mag)) + carried
            got = None
            if stored is not None and name not in inner:
                got = stored(name, exp.shape)
            vals[name] = exp if got is None else got
            if name == op:
                rnd.on = False
                res = {'exp': exp, 'raw': raw_fn(*args), 'got': got, 'bound': err[name], 'slack': slack}
                break
    res['target'] = vals[target]
    return res


def shares(t):
    """(share of nonzero values, share of nonzero values below the smallest normal half) of a tensor."""
    nz = t != 0
    return float(nz.float().mean()), float(((t.abs() < NORMAL_MIN) & nz).float().mean())


def top_shares(exp):
    """(share of finite values at or above 2^14, number of infinite values) of a 'top' row's emulated op."""
    fin = torch.isfinite(exp)
    return float((fin & (exp.abs() >= 2.0 ** 14)).float().mean()), int((~fin).sum())


def check_sub(res):
    """A 'sub' row's assertions on the compared tensor; returns the worst |d| / bound."""
    exp, got, bound = res['exp'], res['got'], res['bound']
    assert bool(torch.isfinite(got).all())
    ratio = (got - exp).abs() / bound
    worst = float(ratio.max())
    assert worst <= 1.0, ('outside the derived bound', worst, int((ratio > 1.0).sum()))
    live = exp.abs() > bound
    assert bool((got[live] != 0).all()), ('zero where the emulation exceeds the bound', int((got[live] == 0).sum()))
    return worst


def check_top(res):
    """A 'top' row's assertions; returns (worst |d| / bound over the finite values, undecided elements).

    The emulation DECIDES an element whose value before the store rounding is further from the tie 65520 than ``slack``
    (evaluate: the fp32 accumulation allowance plus what the launch's inner tensors carry): there the device holds the
    same infinity where the emulation does, and where the emulation is finite a finite value within the bound (1 unit for
    a launch that stores its own op) -- the values in (65504, 65520), which round DOWN, included.  Closer to the tie the
    device's sum may lie on the other side: either 65504 or the infinity, with the emulation's sign."""
    exp, raw, got, bound = res['exp'], res['raw'], res['got'], res['bound']
    fin = torch.isfinite(exp)
    assert not bool(torch.isnan(got).any())
    undecided = (raw.abs() - F16_INF_AT).abs() <= res['slack']
    sure_inf, sure_fin = ~fin & ~undecided, fin & ~undecided
    assert bool((got[sure_inf] == exp[sure_inf]).all()), ('not the emulation\'s infinity', int((got[sure_inf] != exp[sure_inf]).sum()))
    assert bool(torch.isfinite(got[sure_fin]).all()), ('infinite where the emulation is finite', int((~torch.isfinite(got[sure_fin])).sum()))
    both = fin & torch.isfinite(got)
    ratio = (got[both] - exp[both]).abs() / bound[both]
    worst = float(ratio.max())
    assert worst <= 1.0, ('outside the derived bound', worst, int((ratio > 1.0).sum()))
    u = undecided & ~both                        # one side infinite: the emulation's sign, and nothing below 65504
    assert bool((torch.sign(got[u]) == torch.sign(raw[u])).all())
    assert bool((got[u].abs() >= F16_MAX).all())
    return worst, int(undecided.sum())
