"""Where the constants of tests/_fp32_units.py come from, and that its two criteria have teeth.  No device.

The pessimistic model of a CORRECT kernel (``pw_emul``): every 1x1 as the truncating three-way bf16 split of both
operands and the six products of ``mma6`` in its order, each product added to an fp32 accumulator one at a time; the
depthwise as k*k fp32 multiply-adds.  The true MFMA accumulation is not modelled and nothing here asserts it.  Mutants
of that model: (a) ``mid*mid`` never issued, (b) ``hi*lo`` and ``lo*hi`` never issued, (c) the activation split into
two pieces -- each applied to the expand and to the project of a block and to the 1x1 of a head, a stem and a single
convolution; (d) one column of the depthwise input read as zero; (e) one output pixel taken from its neighbour.

Units: every distinct (Cin, Cexp, Cout, k, stride, residual) of the architectures the fp32 device rows run (published,
tests/_custom_space.py, tests/_mbt_space.py, the sub-network rows: 110 blocks, 16 -> 96 -> 16, 24 -> 144 -> 32 and
120 -> 720 -> 120 among them) on 8 x 8 planes with oracle.synth weights, three of them also on 32 x 32; the blocks of
the small-magnitude device row ('block_small'); the stems and heads of search-XS and search-L on 64 x 64 / 128 x 128
planes; single convolutions of 16, 720 and 1024 products (the longest transposed convolution) and, for the dense k x k
launches of pose_resnet, 72 and 9408.  P is a maximum over the tap, so the cheap kinds are emulated at the plane sizes
of the device rows: plain fp32 torch itself reaches e / (u B) = 1.08 on a 128 x 128 head output, 0.6 on 8 x 8.

Measured (``python tests/test_fp32_units_cpu.py`` prints every unit).  P = max e / (u B), R = rms(e / B) over that of
the fp32 torch unit; per mutant the SMALLEST R of the kind; "old": mutants (a)-(c) that 2e-5 * max(1, max |ref|) accepts.
  kind         units  emulation P   R      (a) exp / proj   (b) exp / proj   (c) exp / proj   (d) P >=  (e) P >=   old
  block          114     0.368    3.14      30.4 / 31.3      46.5 / 49.3      27.5 / 26.3     1.7e4     2.8e4   644 / 684
  block_small     10     0.843    1.06       1.4 / 1.3        1.7 / 1.8        1.3 / 1.3      2.4e4     7.5e4    60 / 60
  stem             2     0.450    1.12          61.7            102.5             54.7        4.5e5     4.7e5     6 / 6
  head             4     1.006    1.31          83.1            134.6             75.0        1.3e6     1.6e6    12 / 12
  conv             3    10.75     5.90          73.9            117.2             65.0          -         -       8 / 9
  dense            2     8.32    11.29          49.2             73.8             42.9          -         -       6 / 6
  unit                      emulation P  R     (a) exp / proj   (b) exp / proj   (c) exp / proj   R / old criterion of (c) proj
  16 -> 96 -> 16 k7 res        0.16   1.66      53.1 / 51.8      76.6 / 79.8      49.0 / 43.2      43.2 / 0.39
  24 -> 144 -> 32 k7 s2        0.16   1.85      55.0 / 51.7      78.2 / 84.6      46.2 / 44.3      44.3 / 0.47
  120 -> 720 -> 120 k7 res     0.08   2.73      34.6 / 34.9      53.4 / 54.9      31.3 / 30.0      30.0 / 0.28
  64 -> 384 -> 24 k7 s2        0.08   1.88      30.4 / 31.3      46.5 / 49.3      27.5 / 26.3      26.3 / 0.39   (the weakest)
Hence M = 13 (half of 26.3; the emulation is at most 5.9 <= M / 2) and C_MAX = twice the emulation's P per kind: block
0.75, block_small 1.7, stem 0.95, head 2.1, conv 22, dense 17.  Every mutant (a)-(c) is rejected by R, every (d) and (e)
by P (by four orders of magnitude), and the old criterion accepts 736 of the 777 mutants (a)-(c).
Two classes stand apart, and the tests say so:
  * dense: over 9408 products the fully sequential model drifts to R = 11.3 while the weakest mutant has 42.9.  The class
    has its own m = 21 (half of 42.9); the emulation passes it but is not a factor 2 below it.  (On the device these
    launches measure R <= 3.3: the MFMA's own sum of 16 products is better than one at a time.)
  * block_small: project BatchNorm weights x 2^-8.  The project's products are 2^-8 of the output, below the rounding
    of the final add, so no criterion on the output can reject (a)-(c) there (R 1.3 to 13); the class exists for its
    c_max -- B is close to |ref|, the final add alone costs up to 0.5 -- and (d), (e) fail P as everywhere."""
import numpy as np
import pytest
import torch

import _fp32_units as fu
from oracle import spec, synth

ORDER = (('l', 'h'), ('h', 'l'), ('m', 'm'), ('m', 'h'), ('h', 'm'), ('h', 'h'))    # mma6, smallest first
MUTANTS = {'a': dict(drop={('m', 'm')}), 'b': dict(drop={('l', 'h'), ('h', 'l')}), 'c': dict(pieces=2)}
TAP_REL = 2e-5


def _trunc(x):
    return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def split3(x, pieces=3):
    """The truncating 8 + 8 + 8 split of split3_pair; ``pieces`` = 2: the last piece never made."""
    h = _trunc(x)
    r = x - h
    m = _trunc(r)
    l = _trunc(r - m) if pieces == 3 else np.zeros_like(x)
    return {'h': h, 'm': m, 'l': l}


def pw_emul(x, w, b, drop=(), pieces=3):
    """A 1x1 convolution the way a split-MFMA kernel computes it, pessimistically: per 16-wide k step the six product
    classes of mma6 in its order, every bf16 x bf16 product (exact in fp32) added to the fp32 accumulator one at a
    time; the bias added last.  x (N, C, H, W) fp32 tensor, w (O, C, 1, 1) and b fp32 values."""
    n, c, hh, ww = x.shape
    X = x.permute(1, 0, 2, 3).reshape(c, -1).numpy().astype(np.float32)
    W = w.reshape(w.shape[0], c).numpy().astype(np.float32)
    xs, ws = split3(X, pieces), split3(W)
    acc = np.zeros((W.shape[0], X.shape[1]), np.float32)
    for k0 in range(0, c, 16):
        for pa, pb in ORDER:
            if (pa, pb) in drop:
                continue
            A, Bm = ws[pa], xs[pb]
            for k in range(k0, min(c, k0 + 16)):
                acc += A[:, k:k + 1] * Bm[k:k + 1, :]
    if b is not None:
        acc += b.numpy().astype(np.float32)[:, None]
    return torch.from_numpy(acc).view(-1, n, hh, ww).permute(1, 0, 2, 3).contiguous()


def _f32(wb):
    return tuple(None if t is None else t.float() for t in wb)


def block_emul(x, sd, p, blk, expand=None, project=None, halo=False, pixel=False):
    """The block in fp32 with both 1x1 emulated; ``expand`` / ``project``: a MUTANTS entry for that 1x1; ``halo``: one
    column of the depthwise input read as zero; ``pixel``: one output pixel taken from its neighbour."""
    w1, b1 = _f32(fu.fold(sd, p + '.inv.0.weight', p + '.inv.1'))
    wd, bd = _f32(fu.fold(sd, p + '.depth_conv.0.weight', p + '.depth_conv.1'))
    w3, b3 = _f32(fu.fold(sd, p + '.point_conv.0.weight', p + '.point_conv.1'))
    y = torch.clamp(pw_emul(x, w1, b1, **(expand or {})), 0.0, 6.0)
    if halo:
        y = y.clone()
        y[:, :, :, 5] = 0.0
    y = torch.clamp(fu.dw(y, wd, bd, blk['stride'], blk['k'] // 2), 0.0, 6.0)
    y = pw_emul(y, w3, b3, **(project or {}))
    if blk['residual']:
        y = y + x
    if pixel:
        y = y.clone()
        y[:, :, 1, 1] = y[:, :, 1, 2]
    return y


def head_emul(a, b, sd, i, mut=None, halo=False, pixel=False):
    out = 0.0
    for x, p in ((a, 'final_refined.%d.conv' % i), (b, 'final_raw.%d.conv' % i)):
        wdw, bdw = _f32(fu.fold(sd, p + '.0.weight', p + '.1'))
        w3, _ = _f32(fu.fold(sd, p + '.3.weight', None))
        if halo:
            x = x.clone()
            x[:, :, :, 5] = 0.0
        y = torch.relu(fu.dw(x, wdw, bdw, 1, 2))
        out = out + pw_emul(y, w3, None, **(mut or {}))
    if pixel:
        out = out.clone()
        out[:, :, 1, 1] = out[:, :, 1, 2]
    return out


def stem_emul(x, sd, mut=None, halo=False, pixel=False):
    import torch.nn.functional as F
    w0, b0 = _f32(fu.fold(sd, 'first.0.0.weight', 'first.0.1'))
    w1, b1 = _f32(fu.fold(sd, 'first.1.0.weight', 'first.1.1'))
    w2, b2 = _f32(fu.fold(sd, 'first.2.weight', 'first.3'))
    y = torch.clamp(F.conv2d(x, w0, b0, 2, 1), 0.0, 6.0)
    if halo:
        y = y.clone()
        y[:, :, :, 5] = 0.0
    y = torch.clamp(fu.dw(y, w1, b1, 1, 1), 0.0, 6.0)
    y = pw_emul(y, w2, b2, **(mut or {}))
    if pixel:
        y = y.clone()
        y[:, :, 1, 1] = y[:, :, 1, 2]
    return y


def old_criterion(got, ref32):
    """The criterion every fp32 comparison had: the fraction of 2e-5 * max(1, max |ref|); <= 1 passes."""
    return float((got - ref32).abs().max()) / (TAP_REL * max(1.0, float(ref32.abs().max())))


# ------------------------------------------------------------------ the units the device rows have
def block_shapes():
    """{(Cin, Cexp, Cout, k, stride, residual): (arch, 'stage.S.B')} over every architecture an fp32 census row runs:
    the published ones, tests/_custom_space.py, tests/_mbt_space.py and the sub-network rows."""
    out = {}
    for arch in _all_archs():
        for s, blocks in enumerate(spec.derive(arch)['stages']):
            for b, blk in enumerate(blocks):
                key = (blk['inp'], blk['feat'], blk['oup'], blk['k'], blk['stride'], bool(blk['residual']))
                out.setdefault(key, (arch, 'stage.%d.%d' % (s, b), blk))
    return out


def _all_archs():
    import _custom_space as cs
    import _mbt_space as ms
    import _subnet_space as sp
    from litepose_amd import arch_zoo
    return [arch_zoo.get(n) for n in arch_zoo.names()] + [a for n, a in sorted(cs.ARCHS.items()) if n != 'three'] \
        + [a for _, a in sorted(ms.ARCHS.items())] + [sp.arch_of(r[1]) for r in sp.ROWS]


def conv_lengths():
    """{'deconv': the longest sum of a transposed convolution any fp32 row runs (4 live taps x both sources),
    'dense': (shortest, longest) sum of a k x k launch of tests/test_gpu_resnet_census.py}."""
    import test_gpu_resnet_census as rc
    dec = max(4 * (c['refined_in'] + c['raw_in']) for a in _all_archs() for c in spec.derive(a)['deconv'])
    ks = [(l[4] + l[5]) * l[1] * l[1] for row in rc.CASES for l in rc.launches(row) if l[1] > 1]
    return {'deconv': dec, 'dense': (min(ks), max(ks))}


_SD = {}


def _sd(arch):
    k = id(arch)
    if k not in _SD:
        _SD[k] = (arch, synth.make_state_dict(arch, seed=1234))
    return _SD[k][1]


def _tap(c, seed, h=8, w=8, positive=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, c, h, w, generator=g)
    return torch.relu(x) if positive else x


_CACHE = {}


def _block_row(sd, p, blk, key, seed, plane, label=''):
    x = _tap(key[0], seed, plane, plane)
    ref, B, ref32 = fu.block_fn(sd, p, blk)(x)
    row = {'kind': 'block_small' if 'small' in label else 'block',
           'name': '%d->%d->%d k%d s%d %s' % (key[:5] + ('res' if key[5] else 'non',)) + label}
    row['emul'] = fu.measure(block_emul(x, sd, p, blk), ref, B, ref32)
    for mid, mut in sorted(MUTANTS.items()):
        for where in ('expand', 'project'):
            got = block_emul(x, sd, p, blk, **{where: mut})
            row[mid + '.' + where] = fu.measure(got, ref, B, ref32) + (old_criterion(got, ref32),)
    for mid, kw in (('d', dict(halo=True)), ('e', dict(pixel=True))):
        got = block_emul(x, sd, p, blk, **kw)
        row[mid] = fu.measure(got, ref, B, ref32) + (old_criterion(got, ref32),)
    return row


BIG = ((16, 96, 16), (24, 144, 32), (120, 720, 120))          # these also on a 32 x 32 plane


def small_sd(arch):
    """The weights of the small-magnitude device row (tests/test_gpu_fp32_units.py): the heads' 1x1 scaled by 2^-12 and
    every project BatchNorm weight by 2^-8 -- a residual block's update is then far below its input, and the rounding
    of the final add, half an ulp of |ref| with B close to |ref|, is most of e / (u B)."""
    sd = synth.make_state_dict(arch, seed=1234, head_gain=2.0 ** -12)
    return {k: (v * 2.0 ** -8 if k.endswith('.point_conv.1.weight') else v) for k, v in sd.items()}


def measured():
    """Every unit: {'kind', 'name', 'emul': (P, R), mutant id: (P, R, old criterion)}.  Blocks on 8 x 8 planes (the
    statistics follow the channel counts), three of them also on 32 x 32; heads on 128 x 128 and stems on 64 x 64 planes,
    single convolutions on 32 x 32 (16 x 16 for the longest): P is a maximum, and a maximum over the 10^5 to 10^6
    elements of a device tap is larger than one over the 10^3 of an 8 x 8 plane (plain fp32 torch itself reaches
    e / (u B) = 1.08 on a 128 x 128 head output and 0.6 on an 8 x 8 one)."""
    if 'rows' in _CACHE:
        return _CACHE['rows']
    from litepose_amd import arch_zoo
    rows = []
    shapes = block_shapes()
    for n, key in enumerate(sorted(shapes)):
        arch, p, blk = shapes[key]
        rows.append(_block_row(_sd(arch), p, blk, key, 1000 + n, 8))
        if key[:3] in BIG and key[3] == 7:
            rows.append(_block_row(_sd(arch), p, blk, key, 3000 + n, 32, ' 32x32'))
    xs = arch_zoo.get('search-XS')
    ssd = small_sd(xs)
    seen = set()
    for s, blocks in enumerate(spec.derive(xs)['stages']):
        for b, blk in enumerate(blocks):
            key = (blk['inp'], blk['feat'], blk['oup'], blk['k'], blk['stride'], bool(blk['residual']))
            if key not in seen:
                seen.add(key)
                rows.append(_block_row(ssd, 'stage.%d.%d' % (s, b), blk, key, 2000 + len(seen), 8, ' small'))
                if key[:3] == BIG[0]:
                    rows.append(_block_row(ssd, 'stage.%d.%d' % (s, b), blk, key, 2100, 32, ' small 32x32'))
    for an in ('search-XS', 'search-L'):
        arch = arch_zoo.get(an)
        sd = _sd(arch)
        d = spec.derive(arch)
        x = _tap(3, 77, 128, 128)
        ref, B, ref32 = fu.stem_fn(sd)(x)
        row = {'kind': 'stem', 'name': 'stem %s 3->32->%d' % (an, d['c0']), 'emul': fu.measure(stem_emul(x, sd), ref, B, ref32)}
        for mid, mut in sorted(MUTANTS.items()):
            got = stem_emul(x, sd, mut=mut)
            row[mid + '.1x1'] = fu.measure(got, ref, B, ref32) + (old_criterion(got, ref32),)
        for mid, kw in (('d', dict(halo=True)), ('e', dict(pixel=True))):
            got = stem_emul(x, sd, **kw)
            row[mid] = fu.measure(got, ref, B, ref32) + (old_criterion(got, ref32),)
        rows.append(row)
        for i, h in enumerate(d['heads']):
            a, b = _tap(h['refined_in'], 78 + i, 128, 128, positive=True), _tap(h['raw_in'], 88 + i, 128, 128)
            ref, B, ref32 = fu.head_fn(sd, i)(a, b)
            row = {'kind': 'head', 'name': 'final.%d %s %d+%d->%d' % (i, an, h['refined_in'], h['raw_in'], h['oup']),
                   'emul': fu.measure(head_emul(a, b, sd, i), ref, B, ref32)}
            for mid, mut in sorted(MUTANTS.items()):
                got = head_emul(a, b, sd, i, mut=mut)
                row[mid + '.1x1'] = fu.measure(got, ref, B, ref32) + (old_criterion(got, ref32),)
            for mid, kw in (('d', dict(halo=True)), ('e', dict(pixel=True))):
                got = head_emul(a, b, sd, i, **kw)
                row[mid] = fu.measure(got, ref, B, ref32) + (old_criterion(got, ref32),)
            rows.append(row)
    # a single convolution as a 1x1 over its K = Cin x taps products (B = A), mixed-sign weights, inputs in [0, 6] as
    # behind a relu6.  'conv': K = 16, 720 and the longest transposed convolution (four live taps per output);
    # 'dense': the k x k convolutions of pose_resnet, the shortest and the longest of tests/test_gpu_resnet_census.py
    kd = conv_lengths()
    for kind, K, O in (('conv', 16, 96), ('conv', 720, 120), ('conv', kd['deconv'], 64),
                       ('dense', kd['dense'][0], 32), ('dense', kd['dense'][1], 32)):
        g = torch.Generator().manual_seed(5 + K)
        w = torch.randn(O, K, 1, 1, generator=g) * (2.0 / K) ** 0.5
        b = torch.randn(O, generator=g) * 0.1
        side = 32 if K <= 1024 else 16
        x = torch.clamp(torch.randn(1, K, side, side, generator=g) * 2.0, 0.0, 6.0)
        ref, B = fu.conv_unit(x, w, b)
        ref32 = torch.nn.functional.conv2d(x, w, b)
        row = {'kind': kind, 'name': '1x1 K=%d' % K, 'emul': fu.measure(pw_emul(x, w, b), ref, B, ref32)}
        for mid, mut in sorted(MUTANTS.items()):
            got = pw_emul(x, w, b, **mut)
            row[mid + '.1x1'] = fu.measure(got, ref, B, ref32) + (old_criterion(got, ref32),)
        rows.append(row)
    _CACHE['rows'] = rows
    return rows


def _class_mutants(row):
    return {k: v for k, v in row.items() if k[0] in 'abc' and '.' in k}


def table():
    lines = ['  %-34s %-5s  emul P     R   | weakest (a)-(c): R, its P, old crit | (d) P   (e) P' % ('unit', 'kind')]
    for r in measured():
        cm = _class_mutants(r)
        wk = min(cm, key=lambda k: cm[k][1])
        lines.append('  %-34s %-5s %7.2f %5.2f | %-9s %6.1f %7.2f %5.2f | %s %s'
                     % (r['name'], r['kind'], r['emul'][0], r['emul'][1], wk, cm[wk][1], cm[wk][0], cm[wk][2],
                        '%8.3g' % r['d'][0] if 'd' in r else '       -', '%8.3g' % r['e'][0] if 'e' in r else '       -'))
    return '\n'.join(lines)


def test_units_cover_the_issue_minimum():
    keys = set(block_shapes())
    for want in ((16, 96, 16), (24, 144, 32), (120, 720, 120)):
        assert any(k[:3] == want for k in keys), want
    assert len(keys) >= 20


def test_m_is_half_the_weakest_mutant_and_twice_the_emulation():
    """M: one value for the stem, block, head and single-convolution units; M_KIND['dense'] for the dense k x k class,
    where the window of the sequential model closes: its emulation has to pass R, the factor 2 below is not there."""
    rows = measured()
    print('\n' + table())
    for kinds, m, headroom in ((('block', 'stem', 'head', 'conv'), fu.M, 2.0), (('dense',), fu.M_KIND['dense'], 1.0)):
        rs = [r for r in rows if r['kind'] in kinds]
        weakest = min(min(v[1] for v in _class_mutants(r).values()) for r in rs)
        emul = max(r['emul'][1] for r in rs)
        print('%s: weakest product-class mutant R %.2f; pessimistic emulation R at most %.2f; m = %.2f'
              % ('/'.join(kinds), weakest, emul, m))
        assert all(fu.m_of(k) == m for k in kinds)
        assert 0.8 * weakest / 2.0 <= m <= weakest / 2.0, ('m is half of the weakest mutant', m, weakest)
        assert emul <= m / headroom, (emul, m)


def test_every_product_class_mutant_fails_r():
    """Not asked of 'block_small': with the project's BatchNorm weight at 2^-8 its products are 2^-8 of the output, below
    the rounding of the final add -- no criterion on the output can see a product class missing there.  That class is
    in the table for its c_max, and its mutants (d) and (e) have to fail P like everywhere."""
    for r in measured():
        if r['kind'] == 'block_small':
            continue
        for k, v in _class_mutants(r).items():
            assert v[1] > fu.m_of(r['kind']), (r['name'], k, v)


def test_c_max_is_twice_the_emulation_per_kind():
    rows = measured()
    for kind, c in sorted(fu.C_MAX.items()):
        worst = max(r['emul'][0] for r in rows if r['kind'] == kind)
        print('%-5s emulation P at most %.3f, C_MAX %.2f' % (kind, worst, c))
        assert 2.0 * worst <= c <= 2.6 * worst, (kind, worst, c)


def test_halo_and_pixel_mutants_fail_p():
    for r in measured():
        for k in ('d', 'e'):
            if k in r:
                assert r[k][0] > fu.C_MAX[r['kind']], (r['name'], k, r[k])


def test_the_old_criterion_accepts_a_product_class_mutant():
    """The gap being closed: 2e-5 * max(1, max |ref|) passes kernels that lose a whole product class."""
    accepted = [(r['name'], k) for r in measured() for k, v in _class_mutants(r).items() if v[2] <= 1.0]
    print('%d mutants of (a)-(c) pass the old criterion, e.g. %s' % (len(accepted), accepted[:4]))
    assert accepted


def test_power_of_two_scaling_commutes_with_the_split():
    """The small-magnitude device row rests on this: scaling the input by 2^-12 scales the emulated output exactly."""
    g = torch.Generator().manual_seed(9)
    w = torch.randn(24, 48, 1, 1, generator=g)
    x = torch.randn(1, 48, 8, 8, generator=g)
    assert torch.equal(pw_emul(x * 2.0 ** -12, w, None), pw_emul(x, w, None) * 2.0 ** -12)


if __name__ == '__main__':
    print(table())
