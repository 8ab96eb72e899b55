"""The supernet's sub-network space and the table of sub-networks the census runs (tests/test_subnet_census_cpu.py,
tests/test_gpu_subnet_census.py).  Importable without a GPU.

The space is what ``ArchManager.random_sample()`` can return: every width is ``_make_divisible(c * m, 8)`` of a supernet
width ``c`` and a multiplier ``m`` of ``width_mult``; the layer shapes of an architecture are what ``oracle.spec.derive``
builds from it.  A width VECTOR is ``(input_channel, deconv 0, deconv 1, deconv 2, stage 1, stage 2, stage 3, stage 4)``.

``ROWS`` is a literal table, ``(id, width vector, H, W, N, flip)``:
  * sixteen TRUNK rows (t00-t15) that together contain every block, head and stem key of the space (107).  Sixteen is
    the minimum: each stage transition has 4 x 4 width pairs and an architecture holds one of them.  They run at the
    production sizes (``img_size`` 256 ... 512, square), every stage-4 width on the 16 x 16 deepest plane of 256 and on
    a deepest plane that is no multiple of the 16-pixel tile (20 / 24 / 28 of 320 / 384 / 448), every stage-1 width on
    a 64-wide and on an 80- or 112-wide plane; N = 3 with flip = 0 on three rows (odd grids), N = 1 with flip = 2 on the
    others;
  * forty-eight DECONV rows (d00-d47): with the trunk rows, the 64 architectures that hold all 4 x 4 x 4 (refined_in,
    raw_in, out) triples of each of the three deconv layers (192).  The table is an affine design over Z_4^3: each of
    the three triples is a bijection of the design's point.  They run at N = 1 on the smallest square input at which
    every deconv layer launches the kernel form it launches at 256 x 256 in every storage -- the GPU test asserts that
    equality.  That is 160 x 160: at 64, 96 and 128 deconv.1 (planes of at most 16 x 16) takes deconv4_kernel where
    256 x 256 takes deconv4x3_kernel (``h * w > 256``), and 144 x 144 has 9 x 9 planes, which 16-bit storage refuses
    (odd pixel count);
  * sixty-four SECOND-SIZE rows (e00-e63), so that every launch key of real draws is produced by a row: the form of
    a layer depends on its plane as well as on its shape -- deconv.0 is deconv4_kernel on the 16 x 16 plane of
    256 x 256 and deconv4x3_kernel on every larger one, the stage-3 / stage-4 depthwise is dw_pair16_kernel on
    16 x 16 planes only -- so every vector runs in both size classes: a trunk vector that ran at 256 again at 320, the
    others again at 256, and every deconv vector at 288 x 288 (18 x 18 deepest planes), N = 1, flip = 0.
``GATE_ROWS`` are the rows on both sides of the batch gate, ``OPTION_ROWS`` the rows of forms that an option selects (see
test_gpu_subnet_census.py)."""
import functools
import itertools

from oracle import spec

IMG_SIZES = (256, 320, 384, 448, 512)
FIELDS = ('input_channel', 'deconv.0', 'deconv.1', 'deconv.2', 'stage.0', 'stage.1', 'stage.2', 'stage.3')


def _cfg():
    from litepose_amd import config
    return config.get_cfg('crowd_pose')


@functools.lru_cache(maxsize=None)
def _manager():
    from litepose_amd.models import pose_supermobilenet as psm
    return psm.ArchManager(_cfg())


def widths():
    """The widths each position of a vector can take, in FIELDS order (sorted tuples), from the ArchManager's tables."""
    from litepose_amd.models.pose_supermobilenet import _make_divisible
    am = _manager()
    base = [am.input_channel] + list(am.deconv_setting)[:3] + [c for c, _, _ in am.arch_setting]
    return [tuple(sorted({_make_divisible(c * m, 8) for m in am.width_mult})) for c in base]


def arch_of(vec, img_size=256):
    """The cfg_arch dictionary ``random_sample()`` returns for the width vector ``vec``."""
    am = _manager()
    it = iter(vec)
    return am._sample(img_size, lambda c: next(it))


def vector_of(arch):
    return (arch['input_channel'],) + tuple(arch['deconv_setting'][:3]) + \
        tuple(st['channel'] for st in arch['backbone_setting'])


def archs():
    """Every width vector of the space (one architecture per vector at each img_size)."""
    return itertools.product(*widths())


def keys_of_derived(d):
    keys = {('stem', d['c0'])}
    for s, blocks in enumerate(d['stages']):
        for b in blocks:
            keys.add(('block', s, b['inp'], b['feat'], b['oup'], b['k'], b['stride'], bool(b['residual'])))
    for i, c in enumerate(d['deconv']):
        keys.add(('deconv', i, c['refined_in'], c['raw_in'], c['out']))
    for i, h in enumerate(d['heads']):
        keys.add(('head', i, h['refined_in'], h['raw_in'], h['oup']))
    return keys


def layer_keys(arch):
    """The layer shapes of ``arch``: ('block', stage, inp, feat, oup, k, stride, residual), ('deconv', index,
    refined_in, raw_in, out), ('head', index, refined_in, raw_in, oup), ('stem', c0)."""
    return keys_of_derived(spec.derive(arch))


def key_of_layer(arch, name):
    """The layer key of the layer a device error names ('stage.2.0', 'deconv.1', 'final.0', 'stem' ...)."""
    d = spec.derive(arch)
    parts = name.split('.')
    if parts[0] == 'stage':
        b = d['stages'][int(parts[1])][int(parts[2].split('-')[0])]
        return ('block', int(parts[1]), b['inp'], b['feat'], b['oup'], b['k'], b['stride'], bool(b['residual']))
    if parts[0] == 'deconv':
        c = d['deconv'][int(parts[1])]
        return ('deconv', int(parts[1]), c['refined_in'], c['raw_in'], c['out'])
    if parts[0].startswith('final'):
        h = d['heads'][int(parts[1])]
        return ('head', int(parts[1]), h['refined_in'], h['raw_in'], h['oup'])
    return ('stem', d['c0'])


# (id, (c0, deconv 0, 1, 2, stage 1, 2, 3, 4), H, W, N, flip)
ROWS = [
    # ---- trunk rows: every block, head and stem key; production sizes
    ('t00', (16, 16, 48, 32, 8, 16, 24, 40), 256, 256, 3, 0),
    ('t01', (16, 32, 24, 24, 32, 48, 48, 40), 320, 320, 1, 2),
    ('t02', (16, 48, 48, 16, 24, 16, 72, 40), 384, 384, 1, 2),
    ('t03', (16, 64, 24, 8, 16, 48, 96, 40), 512, 512, 1, 2),
    ('t04', (8, 16, 40, 24, 16, 32, 24, 80), 256, 256, 1, 2),
    ('t05', (24, 32, 16, 16, 8, 64, 48, 80), 448, 448, 1, 2),
    ('t06', (24, 48, 40, 8, 32, 32, 72, 80), 384, 384, 3, 0),
    ('t07', (24, 64, 16, 32, 24, 64, 96, 80), 512, 512, 1, 2),
    ('t08', (24, 16, 24, 16, 24, 48, 24, 120), 256, 256, 1, 2),
    ('t09', (16, 32, 48, 8, 16, 16, 48, 120), 320, 320, 3, 0),
    ('t10', (16, 48, 24, 32, 8, 48, 72, 120), 384, 384, 1, 2),
    ('t11', (24, 64, 48, 24, 32, 16, 96, 120), 320, 320, 1, 2),
    ('t12', (8, 16, 16, 8, 32, 64, 24, 160), 256, 256, 1, 2),
    ('t13', (8, 32, 40, 32, 24, 32, 48, 160), 448, 448, 1, 2),
    ('t14', (24, 48, 16, 24, 16, 64, 72, 160), 384, 384, 1, 2),
    ('t15', (8, 64, 40, 16, 8, 32, 96, 160), 512, 512, 1, 2),
    # ---- deconv rows: the other 48 points of the design
    ('d00', (8, 32, 40, 32, 32, 48, 24, 40), 160, 160, 1, 2),
    ('d01', (16, 48, 24, 32, 24, 16, 24, 40), 160, 160, 1, 2),
    ('d02', (24, 64, 16, 32, 16, 48, 24, 40), 160, 160, 1, 2),
    ('d03', (8, 16, 40, 24, 8, 16, 48, 40), 160, 160, 1, 2),
    ('d04', (16, 48, 16, 24, 24, 16, 48, 40), 160, 160, 1, 2),
    ('d05', (24, 64, 48, 24, 16, 48, 48, 40), 160, 160, 1, 2),
    ('d06', (8, 16, 24, 16, 8, 16, 72, 40), 160, 160, 1, 2),
    ('d07', (16, 32, 16, 16, 32, 48, 72, 40), 160, 160, 1, 2),
    ('d08', (24, 64, 40, 16, 16, 48, 72, 40), 160, 160, 1, 2),
    ('d09', (8, 16, 16, 8, 8, 16, 96, 40), 160, 160, 1, 2),
    ('d10', (16, 32, 48, 8, 32, 48, 96, 40), 160, 160, 1, 2),
    ('d11', (24, 48, 40, 8, 24, 16, 96, 40), 160, 160, 1, 2),
    ('d12', (8, 32, 24, 24, 8, 64, 24, 80), 160, 160, 1, 2),
    ('d13', (16, 48, 16, 24, 32, 32, 24, 80), 160, 160, 1, 2),
    ('d14', (24, 64, 48, 24, 24, 64, 24, 80), 160, 160, 1, 2),
    ('d15', (8, 16, 24, 16, 16, 32, 48, 80), 160, 160, 1, 2),
    ('d16', (16, 48, 48, 16, 32, 32, 48, 80), 160, 160, 1, 2),
    ('d17', (24, 64, 40, 16, 24, 64, 48, 80), 160, 160, 1, 2),
    ('d18', (8, 16, 16, 8, 16, 32, 72, 80), 160, 160, 1, 2),
    ('d19', (16, 32, 48, 8, 8, 64, 72, 80), 160, 160, 1, 2),
    ('d20', (24, 64, 24, 8, 24, 64, 72, 80), 160, 160, 1, 2),
    ('d21', (8, 16, 48, 32, 16, 32, 96, 80), 160, 160, 1, 2),
    ('d22', (16, 32, 40, 32, 8, 64, 96, 80), 160, 160, 1, 2),
    ('d23', (24, 48, 24, 32, 32, 32, 96, 80), 160, 160, 1, 2),
    ('d24', (8, 32, 16, 16, 16, 16, 24, 120), 160, 160, 1, 2),
    ('d25', (16, 48, 48, 16, 8, 48, 24, 120), 160, 160, 1, 2),
    ('d26', (24, 64, 40, 16, 32, 16, 24, 120), 160, 160, 1, 2),
    ('d27', (8, 16, 16, 8, 24, 48, 48, 120), 160, 160, 1, 2),
    ('d28', (16, 48, 40, 8, 8, 48, 48, 120), 160, 160, 1, 2),
    ('d29', (24, 64, 24, 8, 32, 16, 48, 120), 160, 160, 1, 2),
    ('d30', (8, 16, 48, 32, 24, 48, 72, 120), 160, 160, 1, 2),
    ('d31', (16, 32, 40, 32, 16, 16, 72, 120), 160, 160, 1, 2),
    ('d32', (24, 64, 16, 32, 32, 16, 72, 120), 160, 160, 1, 2),
    ('d33', (8, 16, 40, 24, 24, 48, 96, 120), 160, 160, 1, 2),
    ('d34', (16, 32, 24, 24, 16, 16, 96, 120), 160, 160, 1, 2),
    ('d35', (24, 48, 16, 24, 8, 48, 96, 120), 160, 160, 1, 2),
    ('d36', (8, 32, 48, 8, 24, 32, 24, 160), 160, 160, 1, 2),
    ('d37', (16, 48, 40, 8, 16, 64, 24, 160), 160, 160, 1, 2),
    ('d38', (24, 64, 24, 8, 8, 32, 24, 160), 160, 160, 1, 2),
    ('d39', (8, 16, 48, 32, 32, 64, 48, 160), 160, 160, 1, 2),
    ('d40', (16, 48, 24, 32, 16, 64, 48, 160), 160, 160, 1, 2),
    ('d41', (24, 64, 16, 32, 8, 32, 48, 160), 160, 160, 1, 2),
    ('d42', (8, 16, 40, 24, 32, 64, 72, 160), 160, 160, 1, 2),
    ('d43', (16, 32, 24, 24, 24, 32, 72, 160), 160, 160, 1, 2),
    ('d44', (24, 64, 48, 24, 8, 32, 72, 160), 160, 160, 1, 2),
    ('d45', (8, 16, 24, 16, 32, 64, 96, 160), 160, 160, 1, 2),
    ('d46', (16, 32, 16, 16, 24, 32, 96, 160), 160, 160, 1, 2),
    ('d47', (24, 48, 48, 16, 16, 64, 96, 160), 160, 160, 1, 2),
    # ---- second-size rows: e00-e15 the trunk vectors in the other size class, e16-e63 the deconv vectors at 288
    ('e00', (16, 16, 48, 32, 8, 16, 24, 40), 320, 320, 1, 0),
    ('e01', (16, 32, 24, 24, 32, 48, 48, 40), 256, 256, 1, 0),
    ('e02', (16, 48, 48, 16, 24, 16, 72, 40), 256, 256, 1, 0),
    ('e03', (16, 64, 24, 8, 16, 48, 96, 40), 256, 256, 1, 0),
    ('e04', (8, 16, 40, 24, 16, 32, 24, 80), 320, 320, 1, 0),
    ('e05', (24, 32, 16, 16, 8, 64, 48, 80), 256, 256, 1, 0),
    ('e06', (24, 48, 40, 8, 32, 32, 72, 80), 256, 256, 1, 0),
    ('e07', (24, 64, 16, 32, 24, 64, 96, 80), 256, 256, 1, 0),
    ('e08', (24, 16, 24, 16, 24, 48, 24, 120), 320, 320, 1, 0),
    ('e09', (16, 32, 48, 8, 16, 16, 48, 120), 256, 256, 1, 0),
    ('e10', (16, 48, 24, 32, 8, 48, 72, 120), 256, 256, 1, 0),
    ('e11', (24, 64, 48, 24, 32, 16, 96, 120), 256, 256, 1, 0),
    ('e12', (8, 16, 16, 8, 32, 64, 24, 160), 320, 320, 1, 0),
    ('e13', (8, 32, 40, 32, 24, 32, 48, 160), 256, 256, 1, 0),
    ('e14', (24, 48, 16, 24, 16, 64, 72, 160), 256, 256, 1, 0),
    ('e15', (8, 64, 40, 16, 8, 32, 96, 160), 256, 256, 1, 0),
    ('e16', (8, 32, 40, 32, 32, 48, 24, 40), 288, 288, 1, 0),
    ('e17', (16, 48, 24, 32, 24, 16, 24, 40), 288, 288, 1, 0),
    ('e18', (24, 64, 16, 32, 16, 48, 24, 40), 288, 288, 1, 0),
    ('e19', (8, 16, 40, 24, 8, 16, 48, 40), 288, 288, 1, 0),
    ('e20', (16, 48, 16, 24, 24, 16, 48, 40), 288, 288, 1, 0),
    ('e21', (24, 64, 48, 24, 16, 48, 48, 40), 288, 288, 1, 0),
    ('e22', (8, 16, 24, 16, 8, 16, 72, 40), 288, 288, 1, 0),
    ('e23', (16, 32, 16, 16, 32, 48, 72, 40), 288, 288, 1, 0),
    ('e24', (24, 64, 40, 16, 16, 48, 72, 40), 288, 288, 1, 0),
    ('e25', (8, 16, 16, 8, 8, 16, 96, 40), 288, 288, 1, 0),
    ('e26', (16, 32, 48, 8, 32, 48, 96, 40), 288, 288, 1, 0),
    ('e27', (24, 48, 40, 8, 24, 16, 96, 40), 288, 288, 1, 0),
    ('e28', (8, 32, 24, 24, 8, 64, 24, 80), 288, 288, 1, 0),
    ('e29', (16, 48, 16, 24, 32, 32, 24, 80), 288, 288, 1, 0),
    ('e30', (24, 64, 48, 24, 24, 64, 24, 80), 288, 288, 1, 0),
    ('e31', (8, 16, 24, 16, 16, 32, 48, 80), 288, 288, 1, 0),
    ('e32', (16, 48, 48, 16, 32, 32, 48, 80), 288, 288, 1, 0),
    ('e33', (24, 64, 40, 16, 24, 64, 48, 80), 288, 288, 1, 0),
    ('e34', (8, 16, 16, 8, 16, 32, 72, 80), 288, 288, 1, 0),
    ('e35', (16, 32, 48, 8, 8, 64, 72, 80), 288, 288, 1, 0),
    ('e36', (24, 64, 24, 8, 24, 64, 72, 80), 288, 288, 1, 0),
    ('e37', (8, 16, 48, 32, 16, 32, 96, 80), 288, 288, 1, 0),
    ('e38', (16, 32, 40, 32, 8, 64, 96, 80), 288, 288, 1, 0),
    ('e39', (24, 48, 24, 32, 32, 32, 96, 80), 288, 288, 1, 0),
    ('e40', (8, 32, 16, 16, 16, 16, 24, 120), 288, 288, 1, 0),
    ('e41', (16, 48, 48, 16, 8, 48, 24, 120), 288, 288, 1, 0),
    ('e42', (24, 64, 40, 16, 32, 16, 24, 120), 288, 288, 1, 0),
    ('e43', (8, 16, 16, 8, 24, 48, 48, 120), 288, 288, 1, 0),
    ('e44', (16, 48, 40, 8, 8, 48, 48, 120), 288, 288, 1, 0),
    ('e45', (24, 64, 24, 8, 32, 16, 48, 120), 288, 288, 1, 0),
    ('e46', (8, 16, 48, 32, 24, 48, 72, 120), 288, 288, 1, 0),
    ('e47', (16, 32, 40, 32, 16, 16, 72, 120), 288, 288, 1, 0),
    ('e48', (24, 64, 16, 32, 32, 16, 72, 120), 288, 288, 1, 0),
    ('e49', (8, 16, 40, 24, 24, 48, 96, 120), 288, 288, 1, 0),
    ('e50', (16, 32, 24, 24, 16, 16, 96, 120), 288, 288, 1, 0),
    ('e51', (24, 48, 16, 24, 8, 48, 96, 120), 288, 288, 1, 0),
    ('e52', (8, 32, 48, 8, 24, 32, 24, 160), 288, 288, 1, 0),
    ('e53', (16, 48, 40, 8, 16, 64, 24, 160), 288, 288, 1, 0),
    ('e54', (24, 64, 24, 8, 8, 32, 24, 160), 288, 288, 1, 0),
    ('e55', (8, 16, 48, 32, 32, 64, 48, 160), 288, 288, 1, 0),
    ('e56', (16, 48, 24, 32, 16, 64, 48, 160), 288, 288, 1, 0),
    ('e57', (24, 64, 16, 32, 8, 32, 48, 160), 288, 288, 1, 0),
    ('e58', (8, 16, 40, 24, 32, 64, 72, 160), 288, 288, 1, 0),
    ('e59', (16, 32, 24, 24, 24, 32, 72, 160), 288, 288, 1, 0),
    ('e60', (24, 64, 48, 24, 8, 32, 72, 160), 288, 288, 1, 0),
    ('e61', (8, 16, 24, 16, 32, 64, 96, 160), 288, 288, 1, 0),
    ('e62', (16, 32, 16, 16, 24, 32, 96, 160), 288, 288, 1, 0),
    ('e63', (24, 48, 48, 16, 16, 64, 96, 160), 288, 288, 1, 0),
]
TRUNK = [r for r in ROWS if r[0].startswith('t')]
DECONV = [r for r in ROWS if r[0].startswith('d')]
SECOND = [r for r in ROWS if r[0].startswith('e')]

# (id, vector, storage, H, W, N, flip, options, the gated tag, whether this side launches it): the batch gate on a
# search-space shape no published architecture has (see test_gpu_subnet_census.py: test_batch_gate_both_sides)
GATE_ROWS = [
    # mb16_kernel<3, 2>: the 48 -> 40 channel stage-4 entry block on 16 x 16 planes, a launch of >= 48 images
    ('mb16_c48_40_nb46', (16, 48, 16, 24, 24, 16, 48, 40), 'f32', 256, 256, 23, 2, {}, 'mb16_kernel', False),
    ('mb16_c48_40_nb48', (16, 48, 16, 24, 24, 16, 48, 40), 'f32', 256, 256, 24, 2, {}, 'mb16_kernel', True),
]

# the same layout, the last field always True: a form that only an option selects, on a search-space shape no published
# architecture has (test_gpu_subnet_census.py: test_option_row_launches_its_form)
OPTION_ROWS = [
    # mbtb_kernel<1, 1, true>: the 8-channel residual blocks of stage 1 (Cexp = 48: half a 16-channel MFMA group), which
    # mbtd_kernel takes by default; 32 x 32 planes = 2 x 2 tiles per image
    ('mbtb_c8_mbtd0', (16, 16, 48, 32, 8, 16, 24, 40), 'bf16', 128, 128, 3, 2, {'mbtd': 0}, 'mbtb_kernel', True),
]


def row_arch(row):
    """cfg_arch of a ROWS / GATE_ROWS row: img_size is the row's size where that is a production size."""
    H = row[2] if isinstance(row[2], int) else row[3]
    return arch_of(row[1], H if H in IMG_SIZES else IMG_SIZES[0])
