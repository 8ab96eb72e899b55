"""Census of pose_resnet TABLES: every form of ``convk3_kernel<K,S,NB,PG>`` (csrc/convk_kernels.hip) against float64.

``lp_net_create`` takes any family-1 ``lp_arch`` -- any r/k/c/n/s table, any deconv filters, UpConv kernel 3 / 5 / 7 --
while tests/test_gpu_resnet.py runs the one reference table.  ``CASES`` below are tables chosen so that every branch
the kernel's header promises runs on the device: the six <K,S> forms at both NB, an odd block count and a ragged last
block under NB = 2, a source boundary inside an 8-channel group, the upsampled read with K = 5 and 7, planes smaller
than the halo, waves below the plane, 17..31-wide planes, many tiles per row, expand ratios other than 4.  The
module imports without a GPU: ``launches`` / ``features`` derive, from a row alone, the launch list and what each
launch exercises, and tests/test_resnet_census_cpu.py checks the rows against the literal ``REQUIRED`` list.

Per row, on the device (one profiled forward):
  * both outputs of every image against the FLOAT64 restatement (tests/_resnet_ref.py on float64 tensors) at NET_ATOL,
    the output of EVERY k x k launch (its tap, by launch name) and every block tap at TAP_REL scaled by max(1, the
    tap's magnitude) -- the bounds of tests/_net_check.py; flip = 2: the mirrored half against the restatement on
    ``torch.flip(x, [3])``;
  * the profile's launch names == the derived list, its tags == the derived <K,S> forms;
  * batched == per-image, flip = 2 == an explicit flip, flip = 1 == the flipped input: ``torch.equal``;
  * the worst criterion as a fraction of its bound, per row and per <K,S>/NB form (printed; run with -s);
  * every k x k launch as a single-convolution unit of tests/_fp32_units.py on the DEVICE's own input taps, on the first
    image, the first of the mirrored half and the last: P, every element within c_max u B with B = conv(|x|, |w|) + |b|,
    and R, rms(e / B) within m times that of the reference's fp32 op on the same input (class 'dense': c_max 17, m 21,
    from tests/test_fp32_units_cpu.py).  Measured: P at most 0.395 of c_max (first.0 of A_16x1024), R at most 0.157
    of m (deconv.0 of w1.5_upk7); the worst of each <K,S>/NB form lies between 0.19 and 0.40 / 0.05 and 0.16.

What pins the restatement on these tables: tests/golden/gen_golden_resnet.py asserts it bit-identical to the REAL
module for ``width_mult`` 0.5 / 1.5 and for filters [20, 12, 10] (rows w0.5, w1.5, f20).  The real module cannot build
UpConv kernels 5 / 7 nor another r/k/n/s table: those rows rest on the restatement alone -- the same generic code.

CPU headroom: |float32 restatement - float64 restatement| as a fraction of the bound, measured on the CPU before any
device run (``cpu_headroom``; tests/test_resnet_census_cpu.py keeps every row at or below 0.25, so a device result
has three quarters of the bound to itself):

    row             outputs / NET_ATOL   taps / TAP_REL
    ref_16x16       0.006                0.039
    w0.5            0.022                0.147
    w1.5            0.016                0.103
    f20             0.013                0.080
    A_upk5          0.012                0.052
    B_upk7          0.009                0.052
    A_16x1024       0.007                0.041
    B_1024x16       0.010                0.043
    deep32          0.007                0.065
    A_upk7_16x16    0.008                0.043
    B_upk5_32x48    0.008                0.044
    ref_upk5        0.010                0.070
    w1.5_upk7       0.009                0.045

The divisor hole (bottom of the file): a net whose deepest plane is 1/32 of the input (row deep32) refuses 48x48 and
16x16 with LP_ERR_INVALID_ARG and accepts 64x64, in both families -- before the fix buffers were sized H // div while
a stride-2 launch rounded its output plane up.
"""
import ctypes as C
import os

import pytest
import torch

import _resnet_ref as rr
from _net_check import NET_ATOL, TAP_REL, profiled_forward
from conftest import ROOT
from oracle import synth

YAML = os.path.join(ROOT, 'tests', 'golden', 'resnet.yaml')
LP_ERR_INVALID_ARG = -1

# ------------------------------------------------------------------ tables: (input_channel, [[r, k, c, n, s], ...])
T_REF = rr.width_table(1.0)
T_W05 = rr.width_table(0.5)
T_W15 = rr.width_table(1.5)
# A: small channel counts -- 32-channel expands (NB = 1) at <3,2>, <3,1>, <5,2>, <5,1>; 8 * 5 = 40 (feat % 16 == 8, a
# ragged second block); 16 * 5 = 80 (three blocks, the last ragged)
T_A = (8, [[4, 3, 8, 2, 2], [5, 5, 16, 2, 2], [2, 5, 24, 2, 2], [1, 5, 24, 2, 1]])
# B: ratio 3 -- 16 * 3 = 48 at <3,2> (NB = 2), 24 * 3 = 72 (three blocks, the last ragged) at <3,1> and <7,2>, 96 at
# <7,1>; ratio 1: 32 at <7,2> and <3,1> (NB = 1)
T_B = (16, [[3, 3, 24, 2, 2], [3, 7, 32, 2, 2], [1, 7, 32, 1, 2], [1, 3, 48, 2, 1]])
# C: five stages, strides 2,2,2,2,1: the deepest plane is 1/32 of the input, the outputs sit at 1/8 and 1/4
T_C = (8, [[4, 3, 8, 1, 2], [4, 3, 16, 1, 2], [4, 5, 16, 2, 2], [4, 3, 24, 1, 2], [3, 3, 24, 2, 1]])

F_REF = [16, 24, 24]
F_ODD = [20, 12, 10]

# (id, table, deconv_filters, upconv_kernel, joints [heads: 2 * joints, joints], H, W, N, flip, expect_features)
CASES = [
    ('ref_16x16', T_REF, F_REF, 3, 14, 16, 16, 1, 0,
     ['in16x16', 'plane<K/2:K7', 'dead_wave', 'form<7,1>/NB2', 'form<5,2>/NB2', 'form<3,1>/NB2', 'N1', 'flip0']),
    ('w0.5', T_W05, F_REF, 3, 14, 96, 160, 3, 2,
     ['width0.5', 'form<7,2>/NB1', 'ragged_x', 'ragged_y', 'N3', 'flip2']),
    ('w1.5', T_W15, F_REF, 3, 14, 64, 96, 1, 2,
     ['width1.5', 'NB2:nblk_odd', 'form<7,2>/NB2', 'form<5,1>/NB2']),
    ('f20', T_REF, F_ODD, 3, 14, 64, 48, 5, 0,
     ['filters20_12_10', 'W48', 'two_src:Ca%8!=0', 'TW32:OW17..31', 'N5', 'NB1:Cout%32!=0']),
    ('A_upk5', T_A, F_ODD, 5, 17, 64, 64, 3, 2,
     ['upk5', 'ups:K5', 'expand!=4', 'feat%16==8', 'form<3,2>/NB1', 'form<5,2>/NB1', 'form<5,1>/NB1', 'form<3,1>/NB1',
      'NB2:Cout%32!=0', 'NB2:nblk_odd', 'two_src:Ca%8!=0', 'Ct%16!=0']),
    ('B_upk7', T_B, [24, 12, 20], 7, 14, 64, 80, 1, 0,
     ['upk7', 'ups:K7', 'form<3,2>/NB2', 'form<7,2>/NB2', 'form<7,1>/NB2', 'form<7,2>/NB1', 'NB2:nblk_odd',
      'NB2:Cout%32!=0', 'TW32:OW17..31', 'two_src:Ca%8!=0']),
    ('A_16x1024', T_A, F_REF, 3, 14, 16, 1024, 1, 2, ['in16x1024', 'tilesX>=8', 'dead_wave', 'ragged_y']),
    ('B_1024x16', T_B, F_ODD, 5, 14, 1024, 16, 1, 0, ['in1024x16', 'TW16', 'ups:K5', 'plane<K/2:K7']),
    ('deep32', T_C, F_ODD, 3, 14, 64, 96, 3, 2, ['deep32', 'form<3,2>/NB1', 'form<5,2>/NB2', 'form<3,2>/NB2']),
    ('A_upk7_16x16', T_A, [12, 20, 10], 7, 17, 16, 16, 5, 2,
     ['ups:K7', 'plane<K/2:ups', 'plane<K/2:K5', 'in16x16', 'dead_wave', 'two_src:Ca%8!=0']),
    ('B_upk5_32x48', T_B, F_ODD, 5, 17, 32, 48, 3, 0, ['ups:K5', 'W48', 'NB2:Cout%32!=0', 'form<3,1>/NB2']),
    ('ref_upk5', T_REF, F_REF, 5, 14, 32, 32, 1, 2, ['ups:K5', 'form<5,1>/NB2', 'form<5,1>/NB1']),
    ('w1.5_upk7', T_W15, [40, 20, 12], 7, 14, 32, 32, 1, 0, ['ups:K7', 'form<7,1>/NB2', 'NB2:Cout%32!=0']),
]

# what the rows together must execute (tests/test_resnet_census_cpu.py: the union of the derived features covers it)
REQUIRED = (
    ['form<%d,%d>/NB%d' % (k, s, nb) for k in (3, 5, 7) for s in (1, 2) for nb in (1, 2)] +
    ['NB2:nblk_odd', 'NB2:Cout%32!=0', 'NB1:Cout%32!=0', 'Ct%16!=0', 'two_src:Ca%8!=0',
     'ups:K3', 'ups:K5', 'ups:K7', 'upk5', 'upk7',
     'TW16', 'TW32', 'TW32:OW17..31', 'ragged_x', 'ragged_y', 'tilesX>=8',
     'plane<K/2:K7', 'plane<K/2:K5', 'plane<K/2:ups', 'dead_wave',
     'expand!=4', 'feat%16==8', 'width0.5', 'width1.5', 'filters20_12_10',
     'in16x16', 'in16x1024', 'in1024x16', 'W48', 'deep32',
     'N1', 'N3', 'N5', 'flip0', 'flip2'])


def case(cid):
    for row in CASES:
        if row[0] == cid:
            return row
    raise KeyError(cid)


def base_cfg():
    from litepose_amd import config
    return config.update_config(config.get_cfg('crowd_pose'), YAML)


def row_cfg(row):
    _, table, filters, upk, joints, H, W, N, flip, _ = row
    return rr.variant_cfg(base_cfg(), filters=filters, kernel=upk, joints=joints)


def deepest_divisor(table):
    deep = 2
    for _, _, _, _, s in table[1]:
        deep *= s
    return deep


# ------------------------------------------------------------------ launches and features, from a row alone
def launches(row):
    """The launch list of one forward, in order: (name, K, S, ups, Ca, Cb, Cout, IH, IW); (IH, IW) is the source plane
    handed to the launch (before the nearest x2 of ups = 1); K = 1: the 1x1 project of a block (pw kernels)."""
    _, table, filters, upk, joints, H, W, N, flip, _ = row
    d = rr.derive(row_cfg(row), table)
    out = [('first.0', 7, 2, 0, 3, 0, 32, H, W), ('first.1', 7, 1, 0, 32, 0, d['c0'], H // 2, W // 2)]
    div, xdiv = 2, [2]
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            out.append((p + '.inv', blk['k'], blk['stride'], 0, blk['inp'], 0, blk['feat'], H // div, W // div))
            div *= blk['stride']
            out.append((p + '.point_conv', 1, 1, 0, blk['feat'], 0, blk['oup'], H // div, W // div))
        xdiv.append(div)
    rdiv = xdiv[-1]
    for i, dc in enumerate(d['deconv']):
        assert xdiv[-i - 2] == rdiv, 'raw and refined differ in resolution'
        out.append(('deconv.%d' % i, dc['k'], 1, 1, dc['refined_in'], dc['raw_in'], dc['out'], H // rdiv, W // rdiv))
        rdiv //= 2
        if i > 0:
            h = d['heads'][i - 1]
            assert xdiv[-i - 3] == rdiv
            out.append(('final.%d' % (i - 1), 3, 1, 0, h['refined_in'], h['raw_in'], h['oup'], H // rdiv, W // rdiv))
    return out


def geometry(launch):
    """ck_geo + convk3_go of one k x k launch: NB, nblk, TW, tile rows, tilesX, tilesY, the conv's plane, the output."""
    name, K, S, ups, Ca, Cb, Cout, IH, IW = launch
    CH, CW = IH << ups, IW << ups
    OH, OW = (CH - 1) // S + 1, (CW - 1) // S + 1
    PG = 2 if S == 1 else 1
    twl = 4 if OW <= 16 else 5
    TW, RPG = 1 << twl, 32 >> twl
    tr = 4 * PG * RPG
    return dict(NB=1 if Cout <= 32 else 2, nblk=(Cout + 31) // 32, TW=TW, tr=tr, PG=PG, RPG=RPG,
                tilesX=(OW + TW - 1) // TW, tilesY=(OH + tr - 1) // tr, CH=CH, CW=CW, OH=OH, OW=OW)


def tag_of(launch):
    return 'convk3_kernel<%d,%d>' % (launch[1], launch[2]) if launch[1] > 1 else 'pw'


def launch_features(launch):
    name, K, S, ups, Ca, Cb, Cout, IH, IW = launch
    f = set()
    if K == 1:
        if Ca % 16 == 8:
            f.add('feat%16==8')                               # pack_pw: no bf16x3 split of this 1x1
        return f
    g = geometry(launch)
    f.add('form<%d,%d>/NB%d' % (K, S, g['NB']))
    if g['NB'] == 2 and g['nblk'] % 2:
        f.add('NB2:nblk_odd')                                 # the min(cb0 + i, nblk - 1) re-read and the epilogue's break
    if Cout % 32:
        f.add('NB%d:Cout%%32!=0' % g['NB'])
    if (Ca + Cb) % 16:
        f.add('Ct%16!=0')
    if Cb and Ca % 8:
        f.add('two_src:Ca%8!=0')                              # the source boundary inside an 8-channel group
    if ups:
        f.add('ups:K%d' % K)
    f.add('TW%d' % g['TW'])
    if 17 <= g['OW'] <= 31:
        f.add('TW32:OW17..31')
    if g['OW'] % g['TW']:
        f.add('ragged_x')
    if g['OH'] % g['tr']:
        f.add('ragged_y')
    if g['tilesX'] >= 8:
        f.add('tilesX>=8')
    if min(g['CH'], g['CW']) < K // 2:                        # every halo row / column holds padding on both sides
        f.add('plane<K/2:K%d' % K)
        if ups:
            f.add('plane<K/2:ups')
    if (g['tilesY'] - 1) * g['tr'] + 3 * g['PG'] * g['RPG'] >= g['OH']:
        f.add('dead_wave')                                    # wave 3 of the last tile row starts below the plane
    return f


def features(row):
    cid, table, filters, upk, joints, H, W, N, flip, _ = row
    f = set()
    for l in launches(row):
        f |= launch_features(l)
    if any(r != 4 for r, _, _, _, _ in table[1]):
        f.add('expand!=4')
    if table == T_W05:
        f.add('width0.5')
    if table == T_W15:
        f.add('width1.5')
    if list(filters) == [20, 12, 10]:
        f.add('filters20_12_10')
    if upk != 3:
        f.add('upk%d' % upk)
    f.add('in%dx%d' % (H, W))
    if W == 48:
        f.add('W48')
    if deepest_divisor(table) == 32 and H % 32 == 0 and W % 32 == 0:
        f.add('deep32')
    f.add('N%d' % N)
    f.add('flip%d' % flip)
    return f


# ------------------------------------------------------------------ the net of a row
def arch_struct(row):
    """The lp_arch of a row: what models.pose_resnet._arch_struct builds, from the row's table."""
    from litepose_amd import _native as nv
    from litepose_amd.models import pose_resnet
    _, table, filters, upk, joints, H, W, N, flip, _ = row
    a = pose_resnet._arch_struct(row_cfg(row))                # deconv filters / kernel / heads from the cfg
    a.input_channel = table[0]
    a.num_stages = len(table[1])
    assert a.num_stages <= nv.LP_MAX_STAGES
    for s, (r, k, c, n, st) in enumerate(table[1]):
        a.num_blocks[s], a.stride[s], a.channel[s] = n, st, c
        for b in range(n):
            a.expand[s][b], a.kernel[s][b] = r, k
    return a


def make_model(row):
    """A test-local subclass of the product's LitePose with another ``_make_arch``: the product's own refusals
    (width_mult, 16-bit storage) stay."""
    from litepose_amd.models import pose_resnet

    class TableLitePose(pose_resnet.LitePose):
        def _make_arch(self, cfg, cfg_arch, plain_head):
            return arch_struct(row)

    return TableLitePose(row_cfg(row))


def seed_of(row):
    return 1000 + [r[0] for r in CASES].index(row[0])


def make_weights(row):
    return rr.make_state_dict(row_cfg(row), seed=seed_of(row), table=row[1])


def make_input(row):
    _, _, _, _, _, H, W, N, _, _ = row
    return synth.make_images(N, H, seed=seed_of(row) + 50, w=W)


def conv_launch_names(row):
    return [l[0] for l in launches(row) if l[1] > 1]


def ref64(row, sd, x):
    """The float64 restatement: (outputs, taps incl. 'first.0')."""
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    taps = {}
    with torch.no_grad():
        outs = rr.forward(x.double(), sd64, row_cfg(row), taps=taps, table=row[1])
    return outs, taps


def compared_taps(row):
    """Every tap compared on the device: each k x k launch by name ('first.0', 'first.1' == 'first', 'stage.S.B.inv',
    'deconv.I'; the finals are the outputs) and each block output 'stage.S.B'."""
    cfg = row_cfg(row)
    return ['first.0'] + rr.tap_names(cfg, row[1])


def cpu_headroom(row):
    """(worst |f32 - f64| output / NET_ATOL, worst scaled tap / TAP_REL) of the restatement itself, on the row's input."""
    torch.set_num_threads(max(1, min(8, torch.get_num_threads())))
    sd, x = make_weights(row), make_input(row)
    worst_o, worst_t = 0.0, 0.0
    for xs in ([x] if row[8] == 0 else [x, torch.flip(x, [3])]):
        o64, t64 = ref64(row, sd, xs)
        t32 = {}
        with torch.no_grad():
            o32 = rr.forward(xs, sd, row_cfg(row), taps=t32, table=row[1])
        for a, b in zip(o32, o64):
            worst_o = max(worst_o, float((a.double() - b).abs().max()) / NET_ATOL)
        for nm in compared_taps(row):
            r = t64[nm]
            rel = float((t32[nm].double() - r).abs().max()) / max(1.0, float(r.abs().max()))
            worst_t = max(worst_t, rel / TAP_REL)
    return worst_o, worst_t


# ------------------------------------------------------------------ on the device
_FORM_WORST = {}
_UNIT_WORST = {}              # form -> (worst P as a fraction of c_max, worst R as a fraction of m)


def _launch_of_tap(row):
    by_name = {l[0]: l for l in launches(row)}
    m = {'first': by_name['first.1']}
    for nm, l in by_name.items():
        if l[1] > 1 and not nm.startswith('final.'):
            m.setdefault(nm, l)
    return m


def dense_units(row, sd):
    """Every k x k launch of the row as a single-convolution unit of tests/_fp32_units.py: [(launch, inputs, out, fn)],
    ``inputs`` tap names ('x' = the image), ``out`` a tap name or ('out', I), ``fn(*inputs) -> (ref, B, ref32)`` with
    the weights folded as the device plan folds them (float64, one rounding to fp32; a deconv's BatchNorm scale in both
    weight sets, a head's two biases added in float64) and ref32 the reference's own fp32 ops on the same inputs."""
    import torch.nn.functional as F
    import _fp32_units as fu
    d = rr.derive(row_cfg(row), row[1])
    by_name = {l[0]: l for l in launches(row)}
    out = []

    def unit(name, ins, dst, ws, b, stride, ups, act, f32):
        w = torch.cat(ws, 1)

        def fn(*xs):
            xs = [F.interpolate(t, scale_factor=2) if ups else t for t in xs]
            ref, B = fu.conv_unit(torch.cat(xs, 1), w, b, stride, w.shape[2] // 2)
            ref = ref if act is None else torch.clamp(ref, 0.0, act)
            with torch.no_grad():
                return ref, B, f32(*xs)
        out.append((by_name[name], ins, dst, fn))

    def cbr(name, src, dst, conv, bn, stride):
        w, b = fu.fold(sd, conv + '.weight', bn)
        unit(name, [src], dst, [w], b, stride, 0, 6.0, lambda x: rr._convbnrelu6(x, sd, conv, bn, stride))

    cbr('first.0', 'x', 'first.0', 'first.0.0', 'first.0.1', 2)
    cbr('first.1', 'first.0', 'first', 'first.1.0', 'first.1.1', 1)
    prev, ends = 'first', ['first']
    for s, blocks in enumerate(d['stages']):
        for b, blk in enumerate(blocks):
            p = 'stage.%d.%d' % (s, b)
            cbr(p + '.inv', prev, p + '.inv', p + '.inv.0', p + '.inv.1', blk['stride'])
            prev = p
        ends.append(prev)
    refined, raw = ends[-1], ends[-2]
    for i in range(len(d['deconv'])):
        bn = 'deconv_bnrelu.%d.0' % i
        kr, kw = 'deconv_refined.%d.conv.weight' % i, 'deconv_raw.%d.conv.weight' % i
        wr, sh = fu.fold(sd, kr, bn)
        ww, _ = fu.fold(sd, kw, bn)
        pad = wr.shape[2] // 2
        unit('deconv.%d' % i, [refined, raw], 'deconv.%d' % i, [wr, ww], sh, 1, 1, float('inf'),
             lambda a, c, kr=kr, kw=kw, bn=bn, pad=pad: F.relu(rr._bn(
                 F.conv2d(a, sd[kr], None, 1, pad) + F.conv2d(c, sd[kw], None, 1, pad), sd, bn)))
        refined, raw = 'deconv.%d' % i, ends[-i - 3]
        if i > 0:
            j = i - 1
            wr, _ = fu.fold(sd, 'final_refined.%d.weight' % j, None)
            ww, _ = fu.fold(sd, 'final_raw.%d.weight' % j, None)
            bias = (sd['final_refined.%d.bias' % j].double() + sd['final_raw.%d.bias' % j].double()).float().double()
            unit('final.%d' % j, [refined, raw], ('out', j), [wr, ww], bias, 1, 0, None,
                 lambda a, c, j=j: F.conv2d(a, sd['final_refined.%d.weight' % j], sd['final_refined.%d.bias' % j], 1, 1)
                 + F.conv2d(c, sd['final_raw.%d.weight' % j], sd['final_raw.%d.bias' % j], 1, 1))
    return out


def check_dense_units(row, sd, xin, taps, outs, images):
    """P and R of tests/_fp32_units.py (kind 'dense') for every k x k launch on the device's own input taps
    (``taps``: name -> (N', C, h, w) on the host), for the images ``images`` of the device batch.  Returns
    {launch name: (worst P as a fraction of c_max, worst R as a fraction of m)}; asserts both."""
    import _fp32_units as fu
    rows = {}
    units = dense_units(row, sd)
    for n in images:
        for launch, ins, dst, fn in units:
            ref, B, ref32 = fn(*[xin[n:n + 1] if k == 'x' else taps[k][n:n + 1] for k in ins])
            got = outs[dst[1]][n:n + 1].cpu() if isinstance(dst, tuple) else taps[dst][n:n + 1]
            assert got.shape == ref.shape, (launch[0], got.shape, ref.shape)
            pf, rf = fu.check(got, ref, B, ref32, 'dense', (row[0], launch[0], 'image', n))
            old = rows.get(launch[0], (0.0, 0.0))
            rows[launch[0]] = (max(old[0], pf), max(old[1], rf))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [r[0] for r in CASES])
def test_row_vs_fp64_names_and_bitwise(cid):
    row = case(cid)
    _, table, filters, upk, joints, H, W, N, flip, _ = row
    m = make_model(row)
    sd = make_weights(row)
    m.load_state_dict(sd, strict=True)
    x = make_input(row)
    xd = x.cuda()
    lst = launches(row)
    by_launch = {l[0]: l for l in lst}

    # ---- one profiled forward: names and tags
    outs, prof = profiled_forward(m, xd, flip)
    outs = [o.clone() for o in outs]
    names = compared_taps(row)
    dev_taps = {nm: m.tap(nm).cpu() for nm in names}
    assert [a for a, _ in prof] == [l[0] for l in lst], prof
    for (a, t), l in zip(prof, lst):
        if l[1] > 1:
            assert t == tag_of(l), (a, t, tag_of(l))
        else:
            assert t in ('pw3_kernel', 'pw3d_kernel', 'pw2_kernel', 'pw_kernel') or t.startswith('pw'), (a, t)

    # ---- against float64
    halves = [(0, x)] if flip == 0 else [(0, x), (N, torch.flip(x, [3]))]
    l_of = _launch_of_tap(row)
    finals = {0: [l for l in lst if l[0] == 'final.0'][0], 1: [l for l in lst if l[0] == 'final.1'][0]}
    worst = (0.0, '')
    bad = []

    def note(frac, what, launch):
        nonlocal worst
        worst = max(worst, (frac, what))
        if launch is not None:
            key = 'form<%d,%d>/NB%d' % (launch[1], launch[2], geometry(launch)['NB'])
            if frac > _FORM_WORST.get(key, (0.0, ''))[0]:
                _FORM_WORST[key] = (frac, '%s %s' % (cid, what))

    for base, xs in halves:
        o64, t64 = ref64(row, sd, xs)
        for k in range(2):
            got = outs[k][base:base + N].cpu()
            assert got.shape == o64[k].shape, (got.shape, o64[k].shape)
            err = float((got.double() - o64[k]).abs().max())
            note(err / NET_ATOL, 'out%d' % k, finals[k])
            if not err <= NET_ATOL:
                bad.append(('out%d' % k, base, err))
        for nm in names:
            r = t64[nm]
            got = dev_taps[nm].view((-1,) + tuple(r.shape[1:]))[base:base + N]
            rel = float((got.double() - r).abs().max()) / max(1.0, float(r.abs().max()))
            note(rel / TAP_REL, nm, l_of.get(nm))
            if not rel < TAP_REL:
                bad.append((nm, base, rel))
    print('census %-14s N=%d flip=%d %4dx%-4d worst %.3f of the bound at %s' % (cid, N, flip, H, W, worst[0], worst[1]))
    assert not bad, bad[:8]

    # ---- every k x k launch as a single-convolution unit on the device's own input: P and R (tests/_fp32_units.py), on
    #      the first image, the first of the mirrored half and the last
    xin = x if flip == 0 else torch.cat([x, torch.flip(x, [3])])
    full = {nm: dev_taps[nm].view((-1,) + tuple(t64[nm].shape[1:])) for nm in names}
    images = sorted({0, xin.shape[0] - 1} | ({N} if flip == 2 else set()))
    urows = check_dense_units(row, sd, xin, full, outs, images)
    for nm, (pf, rf) in urows.items():
        key = 'form<%d,%d>/NB%d' % (by_launch[nm][1], by_launch[nm][2], geometry(by_launch[nm])['NB'])
        old = _UNIT_WORST.get(key, (0.0, 0.0))
        _UNIT_WORST[key] = (max(old[0], pf), max(old[1], rf))
    wp, wr = max(urows.items(), key=lambda kv: kv[1][0]), max(urows.items(), key=lambda kv: kv[1][1])
    print('units  %-14s %d launches x %d images: P %.3f of c_max at %s, R %.3f of m at %s'
          % (cid, len(urows), len(images), wp[1][0], wp[0], wr[1][1], wr[0]))

    # ---- bitwise: batched == per-image, flip = 2 == an explicit flip, flip = 1 == the flipped input
    xf = torch.flip(xd, [3]).contiguous()
    plain = [o.clone() for o in m.forward_native(xd, 0)]
    both = [o.clone() for o in m.forward_native(xd, 2)]
    flipped = [o.clone() for o in m.forward_native(xf, 0)]
    only_f = [o.clone() for o in m.forward_native(xd, 1)]
    for k in range(2):
        assert torch.equal(both[k][:N], plain[k]), k
        assert torch.equal(both[k][N:], flipped[k]), k
        assert torch.equal(only_f[k], flipped[k]), k
        assert torch.equal(outs[k], both[k] if flip == 2 else plain[k]), k
        for n in range(N):
            one = m.forward_native(xd[n:n + 1].contiguous(), 0)[k]
            assert torch.equal(one[0], plain[k][n]), (k, n)
            onef = m.forward_native(xd[n:n + 1].contiguous(), 1)[k]
            assert torch.equal(onef[0], flipped[k][n]), (k, n)


@pytest.mark.gpu
def test_worst_fraction_per_form():
    """Printed after the rows (file order): the worst fraction of the bound each <K,S>/NB form reached, and where."""
    if len(_FORM_WORST) == 0:
        print('census: no row ran in this process, nothing to summarise')
        return
    for key in sorted(_FORM_WORST):
        print('census form %-16s worst %.3f of the bound at %s; unit P %.3f of c_max, R %.3f of m'
              % ((key,) + _FORM_WORST[key] + _UNIT_WORST.get(key, (float('nan'), float('nan')))))
    want = {'form<%d,%d>/NB%d' % (k, s, nb) for k in (3, 5, 7) for s in (1, 2) for nb in (1, 2)}
    got = set(_FORM_WORST)
    # the finals are compared as outputs, every other launch through its own tap: all twelve forms are reached
    assert want <= got, sorted(want - got)
    assert max(v[0] for v in _FORM_WORST.values()) < 1.0


# ------------------------------------------------------------------ the divisor hole
def _forward_rc(m, N, H, W):
    """lp_net_forward on real buffers sized for the LARGEST plane a caller could assume (H/2): (status, message)."""
    from litepose_amd import _native as nv
    lib = nv.lib()
    x = torch.zeros((N, 3, H, W), dtype=torch.float32, device='cuda')
    out0 = torch.zeros((N, m.final_channel[0], H // 2, W // 2), dtype=torch.float32, device='cuda')
    out1 = torch.zeros((N, m.final_channel[1], H // 2, W // 2), dtype=torch.float32, device='cuda')
    need = int(lib.lp_net_workspace_bytes(m._h, N, H, W))
    ws = torch.zeros(max(need, 1 << 20), dtype=torch.uint8, device='cuda')
    rc = lib.lp_net_forward(m._h, nv.dptr(x), N, H, W, 0, nv.dptr(out0), nv.dptr(out1), nv.dptr(ws), ws.numel(),
                            nv.stream_ptr())
    msg = lib.lp_last_error()
    torch.cuda.synchronize()
    return rc, msg, need


def _check_refusals(m, tap):
    from litepose_amd import _native as nv
    lib = nv.lib()
    assert m.size_multiple == 32
    for H, W in ((48, 48), (16, 16), (64, 48), (48, 64), (32, 16)):
        rc, msg, need = _forward_rc(m, 1, H, W)
        assert rc == LP_ERR_INVALID_ARG and b'32' in msg, (H, W, rc, msg)
        assert need == 0 and b'32' in lib.lp_last_error()
        cnt = C.c_int64(-7)
        assert lib.lp_net_tap_offset(m._h, tap.encode(), 1, H, W, C.byref(cnt)) == LP_ERR_INVALID_ARG
        assert b'32' in lib.lp_last_error() and cnt.value == -7
        with pytest.raises(ValueError, match='32'):
            m.forward_native(torch.zeros((1, 3, H, W), dtype=torch.float32, device='cuda'), 0)
    rc, msg, need = _forward_rc(m, 1, 64, 64)
    assert rc == 0 and need > 0, (rc, msg)
    cnt = C.c_int64(0)
    assert lib.lp_net_tap_offset(m._h, tap.encode(), 1, 64, 64, C.byref(cnt)) >= 0 and cnt.value > 0
    out = m.forward_native(torch.zeros((2, 3, 64, 96), dtype=torch.float32, device='cuda'), 0)
    assert tuple(out[0].shape[2:]) == (8, 12) and tuple(out[1].shape[2:]) == (16, 24)


@pytest.mark.gpu
def test_divisor_32_table_refuses_sizes_that_are_not_multiples_of_32():
    row = case('deep32')
    m = make_model(row)
    m.load_state_dict(make_weights(row), strict=True)
    _check_refusals(m, 'stage.3.0')


def family0_deep32_arch():
    """A pose_mobilenet arch dict with four stride-2 stages: the same deepest divisor through build_plan."""
    from litepose_amd import arch_zoo
    arch = arch_zoo.get('search-XS')
    for st in arch['backbone_setting']:
        st['num_blocks'] = 2
        st['stride'] = 2
        st['block_setting'] = [[6, 7], [6, 7]]
    return arch


@pytest.mark.gpu
@pytest.mark.parametrize('storage', ['f32', 'bf16'])
def test_family_0_divisor_32_table_refuses_the_same_sizes(storage):
    from litepose_amd import config
    from litepose_amd.models import pose_mobilenet
    arch = family0_deep32_arch()
    m = pose_mobilenet.get_pose_net(config.get_cfg('crowd_pose'), cfg_arch=arch, storage=storage)
    m.load_state_dict(synth.make_state_dict(arch, seed=77), strict=True)
    if storage == 'f32':
        _check_refusals(m, 'stage.3.0')
        return
    assert m.size_multiple == 32                             # the 16-bit path: same rule, before any buffer is laid out
    for H, W in ((48, 48), (16, 16)):
        rc, msg, need = _forward_rc(m, 1, H, W)
        assert rc == LP_ERR_INVALID_ARG and b'32' in msg and need == 0, (H, W, rc, msg)
    rc, msg, need = _forward_rc(m, 1, 64, 64)
    assert rc == 0 and need > 0, (rc, msg)


@pytest.mark.gpu
def test_engine_refuses_a_net_whose_sizes_are_not_multiples_of_16_only():
    """PoseEngine / evaluate bucket images to multiples of 16 (x the scale ratio) and read the maps at H/4 and H/2: a
    net whose deepest plane is 1/32 must not get there."""
    from litepose_amd import config, engine
    arch = family0_deep32_arch()
    with pytest.raises(ValueError, match='32'):
        engine.PoseEngine(config.get_cfg('crowd_pose'), arch, synth.make_state_dict(arch, seed=77))
