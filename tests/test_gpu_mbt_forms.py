"""Every built form of the fp32 mbt_kernel on the device: the rows of tests/_mbt_space.py -- all four strip
instantiations ``mbt_kernel<CK, NMT, RES, 16>`` at strip heights 1 .. 35, the non-residual tile instantiations
``mbt_kernel<CK, NMT, false>`` on ragged planes, filter counts below a whole M tile, 1 / 2 / 3 / 8 chunks, grids that are
no multiple of 8 -- with synthetic weights (oracle.synth.make_state_dict).  Needs a real MI355X.

Per row (rows that share a net, an input and options share the forwards):
  * form: the block under test carries the tag mbt_kernel and its grid is N' x ceil(h / 16) for a strip, N' x ceil(w / 16)
    x ceil(h / 16) for a tile (N' = 2 N under flip = 2; profile(launches=True)): the two forms differ in nothing else, and
    a strip kernel refused for scratch memory would show as the tile grid;
  * oracle: check_fp32 -- every block tap at TAP_REL, both outputs at NET_ATOL, every image and the mirrored half;
  * the block alone in fp64 (tests/_fp32_units.py: BatchNorm folded in fp64 and rounded once to fp32, as the device plan
    does) on the DEVICE's input tap against the device's output tap, bound TAP_REL x max(1, max |ref|): the drift of the
    layers in front is out of the comparison; and per image P (every element within c_max u B) and R (the tap's
    rms(e / B) within m times that of the block in plain fp32 torch), printed as fractions of c_max and m;
  * bitwise: the other form (option "mbt_strip" 2 <-> 0) on the row's images gives the same bits in every tap and both
    outputs.  Order: the other form on the row's images, the other form on FOREIGN images (another seed), then the
    row's form on the row's images -- so the planes hold foreign data when the form under test starts, and a strip, tile
    or row it skipped cannot pass on stale correct bits.  Where the other form is not built (17 x 17 planes, CK = 3,
    NMT = 2) both runs are the tile form and the comparison is one of determinism.
Two rows (INVARIANCE_ROWS): batched == per-image and flip = 2 == an explicit flip, bitwise.  The default rule of option
"mbt_strip" = 1 on the device at its edge: strips at N = the CU count, tiles at N - 1.

Measured on an MI355X (256 CUs), every test passing as the kernels stood -- the census exposed no kernel bug.  "blk": the
fp64 block check as a fraction of its bound; "taps" / "outs": check_fp32's worst tap / output as fractions of TAP_REL /
NET_ATOL; "other form": the grid of the bitwise partner, "same" where the other form is not built.
  id             input    N f  form            channels     plane  grid   blk   taps   outs  other form
  h1_s11F        16x512    3 0  strip<1,1,F>    16-> 96->32   1x32     3  0.005  0.036  0.013  grid 6
  h1_s21T        16x512    3 0  strip<2,1,T>    32->192->32   1x32     3  0.004  0.036  0.013  grid 6
  h1_s21F        16x512    3 0  strip<2,1,F>    32->192->16   1x32     3  0.004  0.051  0.010  grid 6
  h1_s11T        16x512    3 0  strip<1,1,T>    16-> 96->16   1x32     3  0.006  0.051  0.010  grid 6
  h2_s11F        32x512    3 2  strip<1,1,F>    16-> 96->32   2x32     6  0.007  0.050  0.015  grid 12
  h2_s21T        32x512    3 2  strip<2,1,T>    32->192->32   2x32     6  0.014  0.050  0.015  grid 12
  h2_s21F        32x512    3 2  strip<2,1,F>    32->192->16   2x32     6  0.007  0.050  0.012  grid 12
  h2_s11T        32x512    3 2  strip<1,1,T>    16-> 96->16   2x32     6  0.009  0.050  0.012  grid 12
  h3_s11F        48x512    3 0  strip<1,1,F>    16-> 96->32   3x32     3  0.009  0.035  0.015  grid 6
  h3_s21T        48x512    3 0  strip<2,1,T>    32->192->32   3x32     3  0.014  0.035  0.015  grid 6
  h3_s21F        48x512    3 0  strip<2,1,F>    32->192->16   3x32     3  0.009  0.043  0.013  grid 6
  h3_s11T        48x512    3 0  strip<1,1,T>    16-> 96->16   3x32     3  0.007  0.043  0.013  grid 6
  h13_s11F       208x512   3 2  strip<1,1,F>    16-> 96->32  13x32     6  0.018  0.044  0.021  grid 12
  h13_s21T       208x512   3 2  strip<2,1,T>    32->192->32  13x32     6  0.011  0.044  0.021  grid 12
  h13_s21F       208x512   3 2  strip<2,1,F>    32->192->16  13x32     6  0.012  0.053  0.019  grid 12
  h13_s11T       208x512   3 2  strip<1,1,T>    16-> 96->16  13x32     6  0.010  0.053  0.019  grid 12
  h15_s11F       240x512   3 0  strip<1,1,F>    16-> 96->32  15x32     3  0.015  0.052  0.018  grid 6
  h15_s21T       240x512   3 0  strip<2,1,T>    32->192->32  15x32     3  0.011  0.052  0.018  grid 6
  h15_s21F       240x512   3 0  strip<2,1,F>    32->192->16  15x32     3  0.012  0.052  0.014  grid 6
  h15_s11T       240x512   3 0  strip<1,1,T>    16-> 96->16  15x32     3  0.008  0.052  0.014  grid 6
  h16_s11F       256x512   3 2  strip<1,1,F>    16-> 96->32  16x32     6  0.018  0.043  0.024  grid 12
  h16_s21T       256x512   3 2  strip<2,1,T>    32->192->32  16x32     6  0.011  0.043  0.024  grid 12
  h16_s21F       256x512   3 2  strip<2,1,F>    32->192->16  16x32     6  0.014  0.042  0.018  grid 12
  h16_s11T       256x512   3 2  strip<1,1,T>    16-> 96->16  16x32     6  0.007  0.042  0.018  grid 12
  h17_s11F       272x512   3 0  strip<1,1,F>    16-> 96->32  17x32     6  0.019  0.044  0.018  grid 12
  h17_s21T       272x512   3 0  strip<2,1,T>    32->192->32  17x32     6  0.013  0.044  0.018  grid 12
  h17_s21F       272x512   3 0  strip<2,1,F>    32->192->16  17x32     6  0.014  0.044  0.015  grid 12
  h17_s11T       272x512   3 0  strip<1,1,T>    16-> 96->16  17x32     6  0.008  0.044  0.015  grid 12
  h19_s11F       304x512   3 2  strip<1,1,F>    16-> 96->32  19x32    12  0.020  0.040  0.019  grid 24
  h19_s21T       304x512   3 2  strip<2,1,T>    32->192->32  19x32    12  0.010  0.040  0.019  grid 24
  h19_s21F       304x512   3 2  strip<2,1,F>    32->192->16  19x32    12  0.015  0.044  0.016  grid 24
  h19_s11T       304x512   3 2  strip<1,1,T>    16-> 96->16  19x32    12  0.009  0.044  0.016  grid 24
  h31_s11F       496x512   3 0  strip<1,1,F>    16-> 96->32  31x32     6  0.017  0.040  0.018  grid 12
  h31_s21T       496x512   3 0  strip<2,1,T>    32->192->32  31x32     6  0.012  0.040  0.018  grid 12
  h31_s21F       496x512   3 0  strip<2,1,F>    32->192->16  31x32     6  0.013  0.040  0.018  grid 12
  h31_s11T       496x512   3 0  strip<1,1,T>    16-> 96->16  31x32     6  0.009  0.040  0.018  grid 12
  h33_s11F       528x512   3 2  strip<1,1,F>    16-> 96->32  33x32    18  0.023  0.041  0.021  grid 36
  h33_s21T       528x512   3 2  strip<2,1,T>    32->192->32  33x32    18  0.012  0.041  0.021  grid 36
  h33_s21F       528x512   3 2  strip<2,1,F>    32->192->16  33x32    18  0.013  0.048  0.015  grid 36
  h33_s11T       528x512   3 2  strip<1,1,T>    16-> 96->16  33x32    18  0.009  0.048  0.015  grid 36
  h35_s11F       560x512   3 0  strip<1,1,F>    16-> 96->32  35x32     9  0.020  0.039  0.024  grid 18
  h35_s21T       560x512   3 0  strip<2,1,T>    32->192->32  35x32     9  0.013  0.039  0.024  grid 18
  h35_s21F       560x512   3 0  strip<2,1,F>    32->192->16  35x32     9  0.013  0.038  0.018  grid 18
  h35_s11T       560x512   3 0  strip<1,1,T>    16-> 96->16  35x32     9  0.009  0.038  0.018  grid 18
  g51_s11F       528x512  17 0  strip<1,1,F>    16-> 96->32  33x32    51  0.023  0.037  0.021  grid 102
  g51_s21T       528x512  17 0  strip<2,1,T>    32->192->32  33x32    51  0.014  0.037  0.021  grid 102
  c32_24_s       32x512    2 2  strip<2,1,F>    32->192->24   2x32     4  0.007  0.047  0.012  grid 8
  c32_8_s        32x512    2 2  strip<2,1,F>    32->192-> 8   2x32     4  0.006  0.047  0.021  grid 8
  c16_24_s       32x512    2 2  strip<1,1,F>    16-> 96->24   2x32     4  0.007  0.050  0.030  grid 8
  c16_8_s        32x512    2 2  strip<1,1,F>    16-> 96-> 8   2x32     4  0.006  0.050  0.018  grid 8
  t17_16_32      272x272   2 2  tile <1,1,F>    16-> 96->32  17x17    16  0.015  0.036  0.018  same
  t32_16_32      272x512   2 0  tile <1,1,F>    16-> 96->32  17x32     8  0.019  0.044  0.018  grid 4
  t17_32_24      272x272   2 2  tile <2,1,F>    32->192->24  17x17    16  0.012  0.046  0.018  same
  t32_32_24      272x512   2 0  tile <2,1,F>    32->192->24  17x32     8  0.015  0.044  0.015  grid 4
  t17_32_64      272x272   2 2  tile <2,2,F>    32->192->64  17x17    16  0.019  0.046  0.016  same
  t32_32_64      272x512   2 0  tile <2,2,F>    32->192->64  17x32     8  0.020  0.044  0.018  same
  t17_32_40      272x272   2 2  tile <2,2,F>    32->192->40  17x17    16  0.011  0.046  0.018  same
  t32_32_40      272x512   2 0  tile <2,2,F>    32->192->40  17x32     8  0.013  0.044  0.017  same
  t17_32_48      272x272   2 2  tile <2,2,F>    32->192->48  17x17    16  0.021  0.060  0.036  same
  t32_32_48      272x512   2 0  tile <2,2,F>    32->192->48  17x32     8  0.021  0.051  0.036  same
  t17_48_32      272x272   2 2  tile <3,1,F>    48->288->32  17x17    16  0.025  0.049  0.027  same
  t32_48_32      272x512   2 0  tile <3,1,F>    48->288->32  17x32     8  0.023  0.050  0.027  same
  t17_48_64      272x272   2 2  tile <3,2,F>    48->288->64  17x17    16  0.023  0.043  0.033  same
  t32_48_64      272x512   2 0  tile <3,2,F>    48->288->64  17x32     8  0.024  0.044  0.027  same
  t17_48_56      272x272   2 2  tile <3,2,F>    48->288->56  17x17    16  0.027  0.052  0.021  same
  t32_48_56      272x512   2 0  tile <3,2,F>    48->288->56  17x32     8  0.022  0.060  0.018  same
  t17_32_48_b1   272x272   2 2  tile <3,2,T>    48->288->48  17x17    16  0.024  0.060  0.036  same
  t17_48_32_b1   272x272   2 2  tile <2,1,T>    32->192->32  17x17    16  0.015  0.049  0.027  same
  t17_16_32_b1   272x272   2 2  tile <2,1,T>    32->192->32  17x17    16  0.010  0.036  0.018  same
  t17_32_16_b1   272x272   2 2  tile <1,1,T>    16-> 96->16  17x17    16  0.009  0.046  0.018  same
  k1_strip_ck1   272x512   2 2  strip<1,1,F>    16-> 32->32  17x32     8  0.014  0.045  0.022  grid 16
  k2_strip_ck1   272x512   2 2  strip<1,1,F>    16-> 64->32  17x32     8  0.017  0.045  0.016  grid 16
  k1_strip_ck2   272x512   2 2  strip<2,1,T>    32-> 32->32  17x32     8  0.016  0.045  0.022  grid 16
  k2_strip_ck2   272x512   2 2  strip<2,1,T>    32-> 64->32  17x32     8  0.016  0.045  0.022  grid 16
  k3_strip_ck2   272x512   2 2  strip<2,1,T>    32-> 96->32  17x32     8  0.011  0.045  0.022  grid 16
  k8_strip_ck2   272x512   2 2  strip<2,1,T>    32->256->32  17x32     8  0.014  0.045  0.022  grid 16
  k1_tile_ck1    272x512   2 2  tile <1,1,F>    16-> 32->32  17x32    16  0.014  0.045  0.022  grid 8
  k2_tile_ck1    272x512   2 2  tile <1,1,F>    16-> 64->32  17x32    16  0.017  0.045  0.016  grid 8
  k1_tile_ck2    272x512   2 2  tile <2,1,T>    32-> 32->32  17x32    16  0.016  0.045  0.022  grid 8
  k2_tile_ck2    272x512   2 2  tile <2,1,T>    32-> 64->32  17x32    16  0.016  0.045  0.022  grid 8
  k3_tile_ck2    272x512   2 2  tile <2,1,T>    32-> 96->32  17x32    16  0.011  0.045  0.022  grid 8
  k8_tile_ck2    272x512   2 2  tile <2,1,T>    32->256->32  17x32    16  0.014  0.045  0.022  grid 8
Worst of all rows: blk 0.027 (t17_48_56), taps 0.060, outputs 0.036 of their bounds: a block error of 1e-6 of the tap's
magnitude would show.  The per-element columns added since (not in the table above): P at most 0.439 of c_max, R at most
0.106 of m over the 85 rows (tests/_fp32_units.py: c_max 0.75, m 13), and check_fp32's unit check of the whole net on
three images of every group.  No row is refused (REFUSED is empty: an 8-filter last stage, one-row planes and odd plane heights
all run).  Wall time: this file 6.7 s (85 tests in one process; the slowest 1.1 s, g51 with 17 images; the default rule
with 256 + 255 images 0.5 s).

Sensitivity, ARGUED from the code: none of the seven wrong edits was run on a device (three of them read or write out
of bounds; runs of the others were not possible in this work).  What each does and which rows see it:
  (a) ``gok`` without ``yy < H``: halo rows below the image are expanded from memory behind the plane (a read out of
      bounds for the last image) instead of staying zero; the depthwise of every last strip reads them.  Every strip
      row fails (bitwise, block, oracle); so does tests/test_gpu_mbt_strip.py, whose planes all have a bottom border.
  (b) ``oy + 1 < H`` -> ``oy < H`` in the depthwise select: with an odd H the depthwise result of row H (outside the
      image) stays in the E tile, no later expand overwrites it, and the next chunk's depthwise reads it as padding.  Rows
      with an odd height and two or more chunks fail: h3, h13, h15, h17, h19, h31, h33, h35, g51, k2 / k3 / k8_strip.  The
      existing strip test has even heights only (``oy`` is even): it passes.
  (c) the strip epilogue without its ``break``: with 8, 16 or 24 filters a workgroup stores up to 32 channels: the first
      channels of the NEXT image, and past the tensor for the last image (a write out of bounds).  The overwritten image
      is restored when its own workgroup stores later, so only the rows with one strip per image and several images
      (c*_s, h1 - h16 at 16 filters) can see it, and not reliably: this edit is what the bound in the code is read for,
      not what a test proves.  One octet too FEW is deterministic: the octet keeps the foreign images' values, and every
      row fails, as does the existing test at 32 filters.
  (d) ``dpar`` as ``c & 1``: every depthwise reads the filter rows of another chunk (chunk 0 a buffer nothing wrote).
      Every strip row fails at every chunk count, as does the existing test (6 chunks).
  (e) waves 4 / 5 expanding rows 21 / 19 instead of 20 / 21: tile row 20 (image row y0 + 17) stays zero.  Every strip with
      18 rows or more below its top fails: h19 - h35, g51; so does the existing test at heights 32 and 48.  h17 and below
      pass: they have no such row.
  (f) ``xcd_contiguous_id`` without ``min(xcd, r)``: with a grid of 8 q + r, r != 0, several workgroups take one unit
      and the last units are taken by none (grid 3: units 1 and 2).  The function serves both forms, so the bitwise
      partner is wrong too; the skipped units keep the FOREIGN images' results, which the block check and the oracle
      see: every row whose grid is no multiple of 8 fails (3, 4, 6, 9, 12, 18, 51).  The existing strip test runs both
      forms on the same images in a row and compares them with each other: it can pass on stale bits.
  (g) the tile form adding x with RES = false: an error of the size of x itself (a read behind the image's channels where
      Cout > Cin).  Every non-residual tile row fails (t17_*, t32_*, k1 / k2_tile_ck1), bitwise too where the strip form
      exists.  Of the existing tests only the sub-network census rows with the 48 -> 40 block above 256 x 256 run such a
      form."""
import time

import pytest
import torch

import _fp32_units as fu
import _mbt_space as ms
from oracle import spec, synth

pytestmark = pytest.mark.gpu

_NETS = {}
_RUNS = {}


def _net(arch_name):
    from _net_check import _model_for
    if arch_name not in _NETS:
        arch = ms.ARCHS[arch_name]
        m, sd = _model_for(arch, 'f32', seed=1234)
        _NETS[arch_name] = (m, arch, sd)
    return _NETS[arch_name]


def _tap_names(arch):
    from _net_check import fp32_tap_names
    return fp32_tap_names(spec.derive(arch))


def _run(m, arch, x, flip, options):
    """One profiled forward under ``options``: (outputs, {tap: tensor}, profile with launch geometry), all cloned."""
    from _net_check import set_options
    old = set_options(m, options)
    try:
        m.set_profiling(True)
        try:
            outs = [o.clone() for o in m.forward_native(x, flip)]
            torch.cuda.synchronize()
            prof = m.profile(launches=True)
        finally:
            m.set_profiling(False)
        taps = {k: m.tap(k).clone() for k in _tap_names(arch)}
    finally:
        set_options(m, old)
    return outs, taps, prof


def _other(options):
    o = dict(options)
    o['mbt_strip'] = 0 if options.get('mbt_strip', 1) == 2 else 2
    return o


def _group(r):
    """The forwards and the oracle check of the row's group, once: a dict, or the refusal's text."""
    from _net_check import check_fp32
    from litepose_amd import _native as nv
    key = ms.forward_key(r)
    if key in _RUNS:
        return _RUNS[key]
    t0 = time.time()
    _, an, H, W, N, flip, options = r[:7]
    try:
        m, arch, sd = _net(an)
        x = synth.make_images(N, H, seed=31, w=W).cuda()
        xf = synth.make_images(N, H, seed=32, w=W).cuda()
        other = _run(m, arch, x, flip, _other(options))
        _run(m, arch, xf, flip, _other(options))                    # foreign data in every plane
        outs, taps, prof = _run(m, arch, x, flip, options)
    except nv.LitePoseNativeError as e:
        _RUNS[key] = str(e)
        return _RUNS[key]
    g = dict(m=m, arch=arch, sd=sd, x=x, outs=outs, taps=taps, prof=prof, other=other, oracle=None, err=None)
    try:
        # the net's taps are the last forward's: the row's form
        g['oracle'] = check_fp32(m, arch, sd, x.cpu(), flip, outs, chunk=8, tap_images=8 if N > 8 else None)
    except AssertionError as e:
        g['err'] = e
    g['wall'] = time.time() - t0
    _RUNS[key] = g
    return g


@pytest.mark.parametrize('rid', [r[0] for r in ms.ROWS])
def test_row(rid):
    from _net_check import NET_ATOL, TAP_REL
    t0 = time.time()
    r = ms.row(rid)
    _, an, H, W, N, flip, options, launch, key = r
    g = _group(r)
    if isinstance(g, str):
        print('%s: REFUSED: %s' % (rid, g))
        assert rid in ms.REFUSED and ms.REFUSED[rid] in g, ('a refusal outside REFUSED', rid, g)
        return
    assert rid not in ms.REFUSED, ('REFUSED lists this row, the forward ran', rid)
    nb, cin, cexp, cout, h, w, _, _, res = ms.shape_of(r)
    # ---- form: the tag and the grid
    hit = [p for p in g['prof'] if p[0].split('|')[0] == launch]
    assert len(hit) == 1 and hit[0][0] == launch + '|mbt_kernel', (rid, [p[0] for p in g['prof'] if p[0].startswith('stage.3')])
    strips, tiles = nb * ((h + 15) // 16), nb * ((w + 15) // 16) * ((h + 15) // 16)
    want = strips if key[0] == 'strip' else tiles
    assert hit[0][5][0] == want and hit[0][5][1] == 512, (rid, key, hit[0][5], strips, tiles)
    # ---- the block alone in fp64 on the device's own input
    s, b = ms.block_of(r)
    d = spec.derive(g['arch'])
    blk = d['stages'][s][b]
    src = 'stage.%d.%d' % ((s, b - 1) if b else (s - 1, len(d['stages'][s - 1]) - 1))
    xin = g['taps'][src].view(nb, cin, h, w).cpu()
    got = g['taps']['stage.%d.%d' % (s, b)].view(nb, cout, h, w).cpu()
    ref, B, ref32 = fu.block_fn(g['sd'], 'stage.%d.%d' % (s, b), blk)(xin)
    bound = TAP_REL * max(1.0, float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    frac = err / bound
    pr = [fu.measure(got[n:n + 1], ref[n:n + 1], B[n:n + 1], ref32[n:n + 1]) for n in range(nb)]
    unit_p, unit_r = max(v[0] for v in pr) / fu.C_MAX['block'], max(v[1] for v in pr) / fu.M
    # ---- bitwise against the other form
    o_outs, o_taps, o_prof = g['other']
    diff = [k for k in g['taps'] if not torch.equal(g['taps'][k], o_taps[k])]
    same = [torch.equal(a, c) for a, c in zip(g['outs'], o_outs)]
    ohit = [p for p in o_prof if p[0].split('|')[0] == launch]
    distinct = ohit[0][5][0] != hit[0][5][0]
    ora = g['oracle']
    print('%-14s %dx%d N=%d f=%d %-5s<%d,%d,%s> %2d->%3d->%2d plane %2dx%2d grid %3d  blk %.3f  P %.3f R %.3f  taps %s outs %s  other form %s  %.2f s (group %.2f s)'
          % (rid, H, W, N, flip, key[0], key[1], key[2], 'FT'[key[3]], cin, cexp, cout, h, w, hit[0][5][0], frac, unit_p, unit_r,
             '%.3f' % (ora[0] / TAP_REL) if ora else 'FAIL', '%.3f' % (ora[2] / NET_ATOL) if ora else 'FAIL',
             'grid %d' % ohit[0][5][0] if distinct else 'same', time.time() - t0, g['wall']))
    assert err <= bound, ('the block alone against fp64', rid, err, bound, frac)
    assert unit_p <= 1.0, ('P: an element of the block beyond c_max u B', rid, unit_p)
    assert unit_r <= 1.0, ('R: the block beyond m times the fp32 reference', rid, unit_r)
    if g['err'] is not None:
        raise g['err']
    assert not diff and all(same), ('not bit-identical to the other form', rid, diff, same)
    if key[0] == 'strip':
        assert distinct and ohit[0][5][0] == tiles, (rid, ohit[0][5])
    elif w == 32 and key[1] <= 2 and key[2] == 1:
        assert distinct and ohit[0][5][0] == strips, (rid, ohit[0][5])
    else:
        assert not distinct, (rid, ohit[0][5])


@pytest.mark.parametrize('rid', ms.INVARIANCE_ROWS)
def test_batched_equals_per_image_and_flip_modes_bitwise(rid):
    """test_batched_forward_is_bitwise_per_image (tests/test_gpu_parity.py) on two strip rows."""
    from _net_check import set_options
    t0 = time.time()
    r = ms.row(rid)
    m = _net(r[1])[0]
    N = r[4]
    x = synth.make_images(N, r[2], seed=31, w=r[3]).cuda()
    old = set_options(m, r[6])
    try:
        both = [o.clone() for o in m.forward_native(x, 2)]
        plain = [o.clone() for o in m.forward_native(x, 0)]
        mirr = [o.clone() for o in m.forward_native(x, 1)]
        for k in range(2):
            assert torch.equal(both[k][:N], plain[k])
            assert torch.equal(both[k][N:], mirr[k])
        for n in range(N):
            one = m.forward_native(x[n:n + 1], 0)
            for k in range(2):
                assert torch.equal(one[k][0], plain[k][n])
        fl = m.forward_native(torch.flip(x, [3]).contiguous(), 0)
        for k in range(2):
            assert torch.equal(fl[k], mirr[k])
    finally:
        set_options(m, old)
    print('%s: batched == per image, flip modes agree; %.2f s' % (rid, time.time() - t0))


def test_default_rule_at_the_cu_count():
    """"mbt_strip" = 1 on a 32 x 16 plane, one strip per image: strips at N = the CU count, tiles (two per image) at
    N - 1 -- ``>=`` against ``>`` -- for <1,1,false,16> (block 0) and <2,1,true,16> (block 1), shown by the grids; the host
    query given the same CU count says the same."""
    from _net_check import set_options
    from litepose_amd import _native as nv
    t0 = time.time()
    m, arch, sd = _net('a16_32')
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    one = synth.make_images(1, 256, seed=33, w=512).cuda()
    assert m.get_option('mbt_strip') == 1
    old = set_options(m, {'mbt': 2})
    try:
        for n in (cus, cus - 1):
            x = one.expand(n, -1, -1, -1).contiguous()
            m.set_profiling(True)
            try:
                m.forward_native(x, 0)
                torch.cuda.synchronize()
                prof = m.profile(launches=True)
            finally:
                m.set_profiling(False)
            grids = [p[5][0] for p in prof if p[0] in (ms.LAUNCH % 0 + '|mbt_kernel', ms.LAUNCH % 1 + '|mbt_kernel')]
            want = n if n >= cus else 2 * n
            assert grids == [want, want], (n, cus, grids)
            for shape in ((n, 16, 96, 32, 16, 32, 7, 1, 0), (n, 32, 192, 32, 16, 32, 7, 1, 1)):
                f = ms.decode(nv.lib().lp_mbt_form(*shape, 2, 1, 1, cus))
                assert f[0] == ('strip' if n >= cus else 'tile'), (n, cus, f)
                assert ms.decode(nv.lib().lp_mbt_form(*shape, 2, 1, 1, 0)) == f      # cus <= 0 asks the device
    finally:
        set_options(m, old)
    print('default rule: %d CUs, strips at %d images, tiles at %d; %.2f s' % (cus, cus, cus - 1, time.time() - t0))
