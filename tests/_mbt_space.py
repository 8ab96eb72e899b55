"""Every built form of the fp32 mbt_kernel (mbtile_kernels.hip: the 16 x 16 tile body ``mbt_kernel<CK, NMT, RES>`` and the
32-wide x 16-row strip body ``mbt_kernel<CK, NMT, RES, 16>``) as a table of rows the census runs
(tests/test_mbt_forms_cpu.py, tests/test_gpu_mbt_forms.py).  Importable without a GPU.

A row is ``(id, arch, H, W, N, flip, options, launch, key)``: ``arch`` names an entry of ``ARCHS``, ``options`` are
``lp_net_set_option`` switches, ``launch`` the profile name of the block under test and ``key`` the form the library's
host query ``lp_mbt_form`` must report for it: ``(form, CK, NMT, RES)`` with form 'tile' or 'strip', CK = Cin / 16,
NMT = ceil(Cout / 32).

How a net gets a NON-residual stride-1 block on a plane of any height: the last stage has stride 1 (the Fusion Deconv
Head needs it, tests/_custom_space.py) and sits on the 1/16 plane, so its first block maps the channels of stage 2 to its
own at stride 1; the blocks after it are residual at the stage's channels.  Input W = 512 gives 32 columns, input
H = 16 h gives h rows, odd ones included (every plane in front of it has an even height).  ``_last(cin, cout, ts)`` is
that net: cheap 3x3 blocks in front, ``cin`` channels out of stage 2, a last stage of ``cout`` channels whose blocks have
the expand ratios ``ts`` (Cexp = ratio x the block's input channels; a chunk is 32 expanded channels).

What cannot exist, so no row has it: a residual block has Cin == Cout, so the tile variants <2, 2> and <3, 1> and a strip
<2, 1, false> at 32 filters or <1, 1, false> at 16 filters are reachable only as (or never as) non-residual blocks:
  <1, 1, false>  16 -> 8, 24, 32          <1, 1, true>  16 -> 16
  <2, 1, false>  32 -> 8, 16, 24          <2, 1, true>  32 -> 32
  <2, 2, false>  32 -> 40, 48, 56, 64     <3, 2, true>  48 -> 48
  <3, 1, false>  48 -> 8 .. 32            <3, 2, false> 48 -> 40, 56, 64
The 16-channel blocks (CK = 1) are mbt_kernel's only with option "mbt" = 2 (the default leaves them to mbconv2_kernel)."""
import copy

import _custom_space as cs
from oracle import spec

LAUNCH = 'stage.3.%d.inv+depth_conv+point_conv'


def _last(cin, cout, ts):
    return cs.build(16, [(16, 2, [[1, 3]]), (16, 2, [[1, 3]]), (cin, 2, [[3, 3]]), (cout, 1, [[t, 7] for t in ts])],
                    (16, 24, 24))


ARCHS = {
    'a16_32': _last(16, 32, [6, 6]),              # b0 <1,1,F> 3 chunks, b1 <2,1,T> 6 chunks
    'a32_16': _last(32, 16, [6, 6]),              # b0 <2,1,F> 16 filters, 6 chunks, b1 <1,1,T> 3 chunks
    'a32_24': _last(32, 24, [6]),                 # <2,1,F> 24 filters
    'a32_8': _last(32, 8, [6]),                   # <2,1,F> 8 filters
    'a16_24': _last(16, 24, [6]),                 # <1,1,F> 24 filters
    'a16_8': _last(16, 8, [6]),                   # <1,1,F> 8 filters
    'a32_64': _last(32, 64, [6]),                 # <2,2,F> full
    'a32_40': _last(32, 40, [6]),                 # <2,2,F> 40 filters
    'a32_48': _last(32, 48, [6, 6]),              # <2,2,F> 48 filters, b1 <3,2,T>
    'a48_32': _last(48, 32, [6, 6]),              # b0 <3,1,F>, b1 <2,1,T>
    'a48_64': _last(48, 64, [6]),                 # <3,2,F> full
    'a48_56': _last(48, 56, [6]),                 # <3,2,F> 56 filters
    # chunk counts: b0 16 -> 32 with 1 chunk, then 32 -> 32 with 1, 2, 3 and 8 chunks; k16b: 16 -> 32 with 2 chunks
    'k16': _last(16, 32, [2, 1, 2, 3, 8]),
    'k16b': _last(16, 32, [4]),
}

# strip heights: the bottom border inside outer rows 19..21 (1, 2, 3), odd last rows (13, 15), one full strip (16), a second
# strip of one row (17) and one whose own rows end before its halo does (19), 31, a third strip (33, 35)
HEIGHTS = (1, 2, 3, 13, 15, 16, 17, 19, 31, 33, 35)

_T, _F = True, False
_STRIP = {'mbt': 2, 'mbt_strip': 2}
_TILE = {'mbt': 2, 'mbt_strip': 0}

# (id, arch, H, W, N, flip, options, launch, key)
ROWS = []


def _row(rid, arch, h, w, n, flip, options, block, key):
    ROWS.append((rid, arch, 16 * h, 16 * w, n, flip, dict(options), LAUNCH % block, key))


# ---- strip heights, all four strip instantiations per height: 512 x 16 h, N = 3, flip 0 / 2 alternating
#      (grids 3, 6, 9, 18)
for _i, _h in enumerate(HEIGHTS):
    _fl = 2 * (_i & 1)
    _row('h%d_s11F' % _h, 'a16_32', _h, 32, 3, _fl, _STRIP, 0, ('strip', 1, 1, _F))
    _row('h%d_s21T' % _h, 'a16_32', _h, 32, 3, _fl, _STRIP, 1, ('strip', 2, 1, _T))
    _row('h%d_s21F' % _h, 'a32_16', _h, 32, 3, _fl, _STRIP, 0, ('strip', 2, 1, _F))
    _row('h%d_s11T' % _h, 'a32_16', _h, 32, 3, _fl, _STRIP, 1, ('strip', 1, 1, _T))
# ---- one large odd grid: 17 images x 3 strips = 51
_row('g51_s11F', 'a16_32', 33, 32, 17, 0, _STRIP, 0, ('strip', 1, 1, _F))
_row('g51_s21T', 'a16_32', 33, 32, 17, 0, _STRIP, 1, ('strip', 2, 1, _T))
# ---- strip epilogue below a whole M tile: 24 and 8 filters (16: the h*_s21F rows; <1,1,F> at 16 filters cannot exist)
for _a, _ck in (('a32_24', 2), ('a32_8', 2), ('a16_24', 1), ('a16_8', 1)):
    _row('c%s_s' % _a[1:], _a, 2, 32, 2, 2, _STRIP, 0, ('strip', _ck, 1, _F))
# ---- the five non-residual tile instantiations (and 40 / 48 / 56 filters for NMT = 2): a 17 x 17 plane (four tiles,
#      three of them ragged by one) and a 32 x 17 plane with strips off
for _a, _key in (('a16_32', (1, 1)), ('a32_24', (2, 1)), ('a32_64', (2, 2)), ('a32_40', (2, 2)), ('a32_48', (2, 2)),
                 ('a48_32', (3, 1)), ('a48_64', (3, 2)), ('a48_56', (3, 2))):
    _row('t17_%s' % _a[1:], _a, 17, 17, 2, 2, _TILE, 0, ('tile',) + _key + (_F,))
    _row('t32_%s' % _a[1:], _a, 17, 32, 2, 0, _TILE, 0, ('tile',) + _key + (_F,))
# the residual tile forms behind them, on the same planes
_row('t17_32_48_b1', 'a32_48', 17, 17, 2, 2, _TILE, 1, ('tile', 3, 2, _T))
_row('t17_48_32_b1', 'a48_32', 17, 17, 2, 2, _TILE, 1, ('tile', 2, 1, _T))
_row('t17_16_32_b1', 'a16_32', 17, 17, 2, 2, _TILE, 1, ('tile', 2, 1, _T))
_row('t17_32_16_b1', 'a32_16', 17, 17, 2, 2, _TILE, 1, ('tile', 1, 1, _T))
# ---- chunk counts 1, 2, 3 and 8 (Cexp = 32, 64, 96, 256), on strips and on tiles, 32 x 17 plane
for _opt, _f in ((_STRIP, 'strip'), (_TILE, 'tile')):
    _row('k1_%s_ck1' % _f, 'k16', 17, 32, 2, 2, _opt, 0, (_f, 1, 1, _F))
    _row('k2_%s_ck1' % _f, 'k16b', 17, 32, 2, 2, _opt, 0, (_f, 1, 1, _F))
    for _b, _k in ((1, 1), (2, 2), (3, 3), (4, 8)):
        _row('k%d_%s_ck2' % (_k, _f), 'k16', 17, 32, 2, 2, _opt, _b, (_f, 2, 1, _T))

# chunk count the k* rows are there for: id -> Cexp / 32
CHUNKS = {r[0]: int(r[0][1]) for r in ROWS if r[0].startswith('k')}

# (row id) -> text of the LitePoseNativeError, for a row another layer of the net refuses.  Empty: every row runs --
# an 8-filter last stage is accepted by the plan -- and a refusal outside this table fails the row's test
REFUSED = {}

# the two rows of the bitwise batched == per-image / flip-mode test: one <1, 1, false, 16>, one at height 17
INVARIANCE_ROWS = ('h33_s11F', 'h17_s21F')


def row(rid):
    return {r[0]: r for r in ROWS}[rid]


def arch_of(r):
    return copy.deepcopy(ARCHS[r[1]])


def block_of(r):
    """(stage, block) of the row's launch."""
    s, b = r[7].split('.')[1:3]
    return int(s), int(b)


def plane_of(arch, stage, H, W):
    """Plane a block of ``stage`` runs on at stride 1 (its input plane): the stem halves, then every stride up to it."""
    div = 2
    for st in arch['backbone_setting'][:stage + 1]:
        div *= st['stride']
    return H // div, W // div


def shape_of(r):
    """(N', Cin, Cexp, Cout, h, w, K, S, residual) of the row's block: lp_mbt_form's arguments."""
    arch = arch_of(r)
    s, b = block_of(r)
    blk = spec.derive(arch)['stages'][s][b]
    h, w = plane_of(arch, s, r[2], r[3])
    return (r[4] * (2 if r[5] == 2 else 1), blk['inp'], blk['feat'], blk['oup'], h, w, blk['k'], blk['stride'],
            bool(blk['residual']))


def forward_key(r):
    """Rows with the same key share one forward."""
    return (r[1], r[2], r[3], r[4], r[5], tuple(sorted(r[6].items())))


FORMS = {0: 'none', 1: 'tile', 2: 'strip', 3: 's2'}


def decode(v):
    """lp_mbt_form's packed int -> (form, CK, NMT, RES), or None for LP_MBT_NONE (include/litepose_amd.h)."""
    if v == 0:
        return None
    assert v > 0, v
    return (FORMS[v & 15], (v >> 4) & 15, (v >> 8) & 15, bool(v >> 12))
