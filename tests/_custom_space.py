"""The architectures only a custom ``cfg_arch`` selects, and the table of rows the custom census runs
(tests/test_custom_census_cpu.py, tests/test_gpu_custom_census.py, tests/golden/gen_golden_custom.py).  Importable
without a GPU.

``lp_net_create`` takes any ``lp_arch`` and ``get_pose_net(cfg_arch=...)`` any dictionary; the plan checks the depthwise
kernel (3 / 5 / 7), the stride (1 / 2), three deconv layers and the stage count.  The rows below are the architectures
that reach the kernel forms no published architecture and no supernet draw launches (``NOT_REACHED`` of
tests/test_gpu_kernel_census.py), each at the smallest input at which the gate in question can still be passed.

A row is ``(id, arch, H, W, N, flip, options, expect_f32, expect_16, why)``: ``arch`` names an entry of ``ARCHS`` (a
``cfg_arch`` dictionary from the small builder below); ``options`` are ``lp_net_set_option`` switches, and the keys that
start with '_' modify the row: ``_joints`` (17: the COCO cfg, head widths 34 and 17), ``_plain`` (pose_simplenet: no raw
branches), ``_storages`` (the storages the row runs in; default all of f32, bf16, and f16 where F16_ROWS lists it).
``expect_f32`` / ``expect_16`` are the ``last_kernel_tag`` values the forward must launch in fp32 and in bf16 / f16
storage.  ``TARGET`` names, per row, the layer shapes the row is there for as launch keys
``(tag or None, Cin, Cexp, Cout, K, stride, residual)`` (tests/_net_check.py: launch_key; a deconv is
``(Ca + Cb, 0, Cout, 4, 2, False)``, a head ``(Ca + Cb, 0, Cout, 5, 1, False)``): the shape must be in
``spec.derive(arch)`` and, with a tag, the fp32 forward must launch that tag on that shape.  ``FORBID`` names, per row,
tags that launches of a layer (a launch-name prefix) must NOT carry: the far side of a gate.

Which strides an architecture may have is fixed by the Fusion Deconv Head, which reads two sources on ONE plane: a
deconv reads the refined tensor and ``x_list[-i-2]``, a head the deconv's output and ``x_list[-i-3]``; so the last stage
has stride 1 and the three before it stride 2 (four stages: 2, 2, 2, 1; five: the first is free).  The plan does not check
this for family 0 (the reference module fails on such a net where it adds the two branches), and no row violates it."""
import copy

from oracle import spec

# every fused block kernel built for 7x7 depthwise blocks only
FUSED_K7 = {'mb16_kernel', 'mbt_kernel', 'mbt_s2_kernel', 'mbconv_kernel', 'mbconv2_kernel', 'mbconv_s2_kernel',
            'mbtb_kernel', 'mbtb_s2_kernel', 'mbtd_kernel'}


def _st(channel, stride, blocks):
    return {'num_blocks': len(blocks), 'stride': stride, 'channel': channel, 'block_setting': [list(b) for b in blocks]}


def build(input_channel, stages, deconv, img_size=256):
    """A ``cfg_arch`` dictionary in the scheme of mobile_configs/*.json; ``stages`` = [(channel, stride, [[t, k] ...])]."""
    return {'img_size': img_size, 'input_channel': input_channel, 'deconv_setting': list(deconv),
            'backbone_setting': [_st(*s) for s in stages]}


def _mini(c0=16, s0=16, deconv=(16, 24, 24)):
    """search-XS with two blocks per stage: the trunk every deconv / head row shares."""
    return build(c0, [(s0, 2, [[6, 7]] * 2), (32, 2, [[6, 7]] * 2), (48, 2, [[6, 7]] * 2), (80, 1, [[6, 7]] * 2)], deconv)


ARCHS = {
    # 24-channel blocks that expand to 96 channels (Cexp % 32 == 0: launch_mbconv / launch_mbconv_s2 admit them; the
    # published 24-channel blocks expand to 144).  stage 0: the stride-2 entry and two residual blocks at 1/4; stage 1: the
    # same pair at 1/8, where a plane's width can be 2 mod 4 (W = 272 -> 34)
    'mb24': build(24, [(24, 2, [[4, 7]] * 3), (24, 2, [[4, 7]] * 2), (48, 2, [[6, 7]]), (80, 1, [[6, 7]])], (16, 24, 24)),
    # five stages, the first at stride 1: the NON-residual stride-1 24 -> 32 block (mbconv_kernel<false>) at 1/2, a
    # 32 -> 24 stride-2 entry with expand 3, stride-2 entries with 5x5 and 3x3 depthwise
    'five': build(24, [(32, 1, [[4, 7]]), (24, 2, [[3, 7], [4, 7]]), (32, 2, [[6, 5]]), (48, 2, [[6, 3]]), (80, 1, [[3, 5]])],
                  (16, 24, 24)),
    # three stages: the head's second raw source (x_list[-5]) does not exist
    'three': build(16, [(16, 2, [[6, 7]]), (32, 2, [[6, 7]]), (48, 1, [[6, 7]])], (16, 24, 24)),
    'mini': _mini(),
    # odd deconv filters: deconv.1 reads 18 + 32 channels (Ct & 3), deconv.2 17 + 24, the heads 17 + 24 and 9 + 24
    'odd': _mini(24, 24, (18, 17, 9)),
    # deconv.1 reads 34 + 32 = 66 channels (Ct & 3) into 40 filters (> 32: no fp32-MFMA form)
    'pair66': _mini(deconv=(34, 40, 24)),
    # deconv.0 has 72 filters (> 64: three channel blocks)
    'wide72': _mini(deconv=(72, 24, 24)),
    # even filters that are no multiple of 8: deconv.1 / deconv.2 read 12 + 32 and 20 + 16 channels (w3 without w4)
    'd4': _mini(deconv=(12, 20, 24)),
    # depthwise 3x3 / 5x5 inside blocks, expand ratios 1, 3, 6, 8; as the stride-2 entry and at stride 1
    'ksize': build(16, [(16, 2, [[6, 3], [6, 3], [1, 5]]), (32, 2, [[6, 5], [6, 5], [3, 3]]),
                        (48, 2, [[3, 3], [8, 7], [6, 5]]), (80, 1, [[6, 5], [6, 5], [6, 3], [8, 7]])], (16, 24, 24)),
    # 5x5 blocks of mb16_kernel's channel shapes (48 -> 80 entry, 80-channel residual) on the 16 x 16 plane of 256 x 256,
    # and one 7x7 residual block that shows the batch gate passed
    'gate5': build(16, [(16, 2, [[1, 3]]), (32, 2, [[3, 3]]), (48, 2, [[3, 5]]),
                        (80, 1, [[6, 5], [6, 5], [6, 5], [6, 7]])], (16, 24, 24)),
    # 5x5 / 3x3 residual blocks of 16 channels at 1/2 (five stages, the first at stride 1): mbtd_kernel's channel
    # shape; one 7x7 residual block shows that kernel launched in the same forward
    'gateq': build(16, [(16, 1, [[6, 5], [6, 5], [6, 3], [6, 7]]), (24, 2, [[3, 5]]), (32, 2, [[3, 3]]), (48, 2, [[3, 3]]),
                        (80, 1, [[1, 5]])], (16, 24, 24)),
}

_ODD16 = {'pw2_kernel', 'deconv_mfma_kernel', 'dw_pair_kernel<5>'}

# (id, arch, H, W, N, flip, options, expect_f32, expect_16, why)
ROWS = [
    # ---- 24-channel fused blocks
    ('mb24_128', 'mb24', 128, 128, 3, 2, {}, {'mbconv_s2_kernel', 'mbconv_kernel'}, {'mbtb_s2_kernel', 'mbtd_kernel'},
     'stage 0 on a 32 x 32 plane: exactly at the 1024-pixel gate of launch_mbconv / launch_mbconv_s2'),
    ('mb24_144x160', 'mb24', 144, 160, 3, 2, {}, {'mbconv_s2_kernel', 'mbconv_kernel'}, {'mbtb_s2_kernel', 'mbtd_kernel'},
     'a 36 x 40 plane: ragged 16 x 16 (mbconv_kernel) and 8 x 8 (mbconv_s2_kernel) tiles'),
    ('mb24_96x128', 'mb24', 96, 128, 3, 2, {}, {'dw_kernel<7,2>', 'dw_pair_kernel<7>'}, {'mbtb_s2_kernel'},
     'a 24 x 32 plane, below the gate: the unfused chain'),
    ('mb24_w34', 'mb24', 256, 272, 3, 2, {}, {'mbconv_s2_kernel', 'mbconv_kernel', 'dw_pair_kernel<7>'},
     {'mbtb_s2_kernel', 'mbtd_kernel'},
     'stage 1 on a 32 x 34 plane: mbconv_s2_kernel stores a width of 34, launch_mbconv refuses the residual block '
     '(W & 3) and it runs as the chain; no legal input gives stage 0 such a width (H, W are multiples of 16)'),
    ('five_128', 'five', 128, 128, 3, 2, {}, {'mbconv_kernel', 'mbt_s2_kernel', 'dw_kernel<5,2>', 'dw_kernel<3,2>'},
     {'dwb_kernel<5,2>', 'dwb_kernel<3,2>'},
     'five stages; the non-residual stride-1 24 -> 32 block on a 64 x 64 plane'),
    ('three_64', 'three', 64, 64, 1, 0, {}, set(), set(), 'three stages: refused at lp_net_create'),
    ('mbconv2_0', 'mini', 128, 128, 3, 2, {'mbconv2': 0}, {'dw_pair_kernel<7>', 'pw2_kernel'}, set(),
     'option "mbconv2" = 0 on 16-channel blocks: the unfused chain, NOT mbconv_kernel'),
    # ---- deconv fallbacks and heads fed by odd channel counts
    ('odd_64', 'odd', 64, 64, 3, 2, {'_joints': 17}, _ODD16 | {'deconv4_kernel', 'dw_pair16_kernel<5>'}, set(),
     'deconv_mfma_kernel<true> on 18 + 32 and on 17 + 24 channels; heads of 17 + 24 and 9 + 24 channels into 34 / 17 '
     'maps (two channel blocks), final.0 on a 16 x 16 plane'),
    ('odd_96x160', 'odd', 96, 160, 3, 2, {'_joints': 17}, _ODD16, set(), 'the same on non-square planes'),
    ('pair66_64', 'pair66', 64, 64, 3, 2, {}, {'deconv_pair_kernel', 'deconv4_kernel'}, set(),
     'deconv_pair_kernel<true> on 34 + 32 channels, 40 filters'),
    ('pair66_96x160', 'pair66', 96, 160, 3, 2, {}, {'deconv_pair_kernel'}, set(), 'the same on non-square planes'),
    ('wide72_64', 'wide72', 64, 64, 3, 2, {}, {'deconv_pair_kernel'}, set(),
     'deconv_pair_kernel on 80 + 48 = 128 channels, 72 filters; 16-bit storage refuses > 64 filters at finalize'),
    ('d4_256', 'd4', 256, 256, 3, 2, {}, {'deconv4_kernel', 'headfuse_kernel'}, set(),
     'deconv4_kernel on 32 x 32 and 64 x 64 planes (h * w > 256), where channel counts in eights take deconv4x3_kernel'),
    ('plain_mfma_64', 'odd', 64, 64, 3, 2, {'_plain': 1}, {'deconv_mfma_kernel', 'pw2_kernel'}, set(),
     'pose_simplenet: deconv_mfma_kernel<false> on 18 and on 17 channels, one-source heads of 17 and 9 channels'),
    ('plain_pair_64', 'pair66', 64, 64, 3, 2, {'_plain': 1}, {'deconv_pair_kernel'}, set(),
     'pose_simplenet: deconv_pair_kernel<false> on 34 channels, 40 filters'),
    # ---- depthwise kernel sizes and expand ratios inside blocks
    ('ksize_256', 'ksize', 256, 256, 3, 2, {},
     {'dw_kernel<3,2>', 'dw_kernel<5,2>', 'dw_pair_kernel<3>', 'dw_pair_kernel<5>', 'dw_pair16_kernel<3>',
      'dw_pair16_kernel<5>', 'dwpw_kernel'},
     {'dwb_kernel<3,2>', 'dwb_kernel<5,2>', 'dwb_kernel<3,1>', 'dwb_kernel<5,1>'},
     '3x3 / 5x5 blocks on 64 x 64 and 32 x 32 planes and on the 16 x 16 planes of stages 3 and 4'),
    ('ksize_128', 'ksize', 128, 128, 3, 2, {},
     {'dw_kernel<3,2>', 'dw_kernel<5,2>', 'dw_pair_kernel<3>', 'dw_pair_kernel<5>', 'dw_pair16_kernel<3>',
      'dw_pair16_kernel<5>'},
     {'dwb_kernel<3,2>', 'dwb_kernel<5,2>', 'dwb_kernel<3,1>', 'dwb_kernel<5,1>'},
     'the same blocks one plane class down: stage 2 on 16 x 16 planes (a stride-2 5x5 INTO a 16 x 16 plane), 8 x 8 below'),
    # ---- a batch gate passed in front of a block that is not 7x7
    ('gate5_nb48', 'gate5', 256, 256, 24, 2, {'_storages': ('f32',)}, {'mb16_kernel', 'dw_pair16_kernel<5>'}, set(),
     'a launch of 48 images (opt_mb16_min) on 16 x 16 planes: mb16_kernel takes the 7x7 block, never the 5x5 ones'),
    ('gateq_1024', 'gateq', 128, 128, 32, 2, {'_storages': ('bf16',)}, set(), {'mbtd_kernel', 'dwb_kernel<5,1>', 'dwb_kernel<3,1>'},
     '64 images x 16 tiles = 1024 tiles, a full-size launch: mbtd_kernel takes the 7x7 block, never the 5x5 / 3x3 ones'),
]

# row id -> the shapes it is there for: (tag the fp32 forward must launch on the shape, or None) + launch_key's shape
TARGET = {
    'mb24_128': [('mbconv_s2_kernel', 24, 96, 24, 7, 2, False), ('mbconv_kernel', 24, 96, 24, 7, 1, True)],
    'mb24_144x160': [('mbconv_s2_kernel', 24, 96, 24, 7, 2, False), ('mbconv_kernel', 24, 96, 24, 7, 1, True)],
    'mb24_96x128': [('dw_kernel<7,2>', 24, 96, 24, 7, 2, False), ('dw_pair_kernel<7>', 24, 96, 24, 7, 1, True)],
    'mb24_w34': [('mbconv_s2_kernel', 24, 96, 24, 7, 2, False), ('dw_pair_kernel<7>', 24, 96, 24, 7, 1, True)],
    'five_128': [('mbconv_kernel', 24, 96, 32, 7, 1, False), ('mbconv_kernel', 24, 96, 24, 7, 1, True),
                 ('mbt_s2_kernel', 32, 96, 24, 7, 2, False), ('dw_kernel<5,2>', 24, 144, 32, 5, 2, False),
                 ('dw_kernel<3,2>', 32, 192, 48, 3, 2, False), ('dw_pair_kernel<5>', 48, 144, 80, 5, 1, False)],
    'three_64': [],                  # refused: spec.derive has no such net either (x_list[-5] does not exist)
    'mbconv2_0': [('dw_pair_kernel<7>', 16, 96, 16, 7, 1, True)],
    'odd_64': [('deconv_mfma_kernel', 50, 0, 17, 4, 2, False), ('deconv_mfma_kernel', 41, 0, 9, 4, 2, False),
               ('pw2_kernel', 41, 0, 34, 5, 1, False), ('pw2_kernel', 33, 0, 17, 5, 1, False),
               ('dw_pair16_kernel<5>', 41, 0, 34, 5, 1, False), ('dw_pair_kernel<5>', 33, 0, 17, 5, 1, False)],
    'odd_96x160': [('deconv_mfma_kernel', 50, 0, 17, 4, 2, False), ('deconv_mfma_kernel', 41, 0, 9, 4, 2, False),
                   ('pw2_kernel', 41, 0, 34, 5, 1, False), ('pw2_kernel', 33, 0, 17, 5, 1, False)],
    'pair66_64': [('deconv_pair_kernel', 66, 0, 40, 4, 2, False), ('deconv4_kernel', 128, 0, 34, 4, 2, False)],
    'pair66_96x160': [('deconv_pair_kernel', 66, 0, 40, 4, 2, False)],
    'wide72_64': [('deconv_pair_kernel', 128, 0, 72, 4, 2, False)],
    'd4_256': [('deconv4_kernel', 44, 0, 20, 4, 2, False), ('deconv4_kernel', 36, 0, 24, 4, 2, False),
               ('headfuse_kernel', 36, 0, 28, 5, 1, False)],
    # a plain head's layers have no raw channels: spec.derive (the fusion head's bookkeeping) lists them with theirs
    'plain_mfma_64': [('deconv_mfma_kernel', 50, 0, 17, 4, 2, False), ('deconv_mfma_kernel', 41, 0, 9, 4, 2, False),
                      ('pw2_kernel', 41, 0, 28, 5, 1, False), ('pw2_kernel', 33, 0, 14, 5, 1, False)],
    'plain_pair_64': [('deconv_pair_kernel', 66, 0, 40, 4, 2, False)],
    # the 3x3 residual block of stage 1 (96 expanded channels, 16 filters, a 64 x 64 plane) passes launch_dwpw's gates
    # for the stem's dw3 + 1x1 and runs in dwpw_kernel<3, 1, 1, RES = true>
    'ksize_256': [('dw_kernel<3,2>', 16, 96, 16, 3, 2, False), ('dwpw_kernel', 16, 96, 16, 3, 1, True),
                  ('dw_pair_kernel<5>', 16, 16, 16, 5, 1, True), ('dw_kernel<5,2>', 16, 96, 32, 5, 2, False),
                  ('dw_pair_kernel<5>', 32, 192, 32, 5, 1, True), ('dw_pair_kernel<3>', 32, 96, 32, 3, 1, True),
                  ('dw_kernel<3,2>', 32, 96, 48, 3, 2, False), ('dw_pair16_kernel<7>', 48, 384, 48, 7, 1, True),
                  ('dw_pair16_kernel<5>', 48, 288, 48, 5, 1, True), ('dw_pair16_kernel<5>', 48, 288, 80, 5, 1, False),
                  ('dw_pair16_kernel<5>', 80, 480, 80, 5, 1, True), ('dw_pair16_kernel<3>', 80, 480, 80, 3, 1, True),
                  ('dw_pair16_kernel<7>', 80, 640, 80, 7, 1, True)],
    'ksize_128': [('dw_kernel<5,2>', 16, 96, 32, 5, 2, False), ('dw_pair16_kernel<5>', 32, 192, 32, 5, 1, True),
                  ('dw_pair16_kernel<3>', 32, 96, 32, 3, 1, True), ('dw_pair_kernel<3>', 16, 96, 16, 3, 1, True),
                  ('dw_pair_kernel<5>', 48, 288, 48, 5, 1, True), ('dw_pair_kernel<3>', 80, 480, 80, 3, 1, True)],
    'gate5_nb48': [('dw_pair16_kernel<5>', 48, 288, 80, 5, 1, False), ('dw_pair16_kernel<5>', 80, 480, 80, 5, 1, True),
                   ('mb16_kernel', 80, 480, 80, 7, 1, True)],
    'gateq_1024': [(None, 16, 96, 16, 5, 1, True), (None, 16, 96, 16, 3, 1, True), (None, 16, 96, 16, 7, 1, True)],
}

# row id -> {launch-name prefix: tags none of its launches may carry}: the far side of a gate
FORBID = {
    'mb24_96x128': {'stage.0.': {'mbconv_kernel', 'mbconv_s2_kernel'}},
    'mb24_w34': {'stage.1.1': {'mbconv_kernel'}},
    'mbconv2_0': {'stage.0.': {'mbconv_kernel', 'mbconv2_kernel'}},
}

# rows that also run in f16 storage: the rows that add a 16-bit form (dwb_kernel<5,2>, <3,2>, and <5,1> / <3,1> inside
# blocks; the 24-channel blocks of 96 expanded channels) and the deconv rows, whose f16 outcome is a refusal
F16_ROWS = ('mb24_128', 'five_128', 'ksize_256', 'ksize_128', 'odd_64', 'pair66_64', 'wide72_64', 'd4_256', 'plain_mfma_64',
            'plain_pair_64')

# (storage, row id) -> text the refusal (a LitePoseNativeError) must contain.  fp32 refuses only the three-stage net.
# 16-bit storage keeps its tensors in channel octets: deconv filters that are no multiple of 8 are refused at the
# forward by the first layer that has them, more than 64 filters at lp_net_finalize
_NO_OCTETS = {'odd_64': 'deconv.0', 'odd_96x160': 'deconv.0', 'pair66_64': 'deconv.0', 'pair66_96x160': 'deconv.0',
              'd4_256': 'deconv.0', 'plain_mfma_64': 'deconv.0', 'plain_pair_64': 'deconv.0'}
REFUSED = {('f32', 'three_64'): 'too few stages'}
for _s in ('bf16', 'f16'):
    REFUSED[(_s, 'three_64')] = 'too few stages'
    REFUSED[(_s, 'wide72_64')] = '%s storage: deconv filters > 64 are not supported' % _s
    for _r, _layer in _NO_OCTETS.items():
        REFUSED[(_s, _r)] = '%s storage: unsupported layer shape at %s' % (_s, _layer)

# NOT_REACHED tags (tests/test_gpu_kernel_census.py) that no lp_arch and no option select at a size a test may run
UNREACHABLE = {
    'dw_kernel<7,1>': 'launch_dw sends every stride-1 depthwise to dw_pair_kernel while (N + 1) / 2 <= 65535 (the image '
                      'pair is grid.y): only a launch of 131071 images or more falls back to it, whatever the arch',
    'dw_kernel<5,1>': 'as dw_kernel<7,1>: stride-1 5x5 planes take dw_pair_kernel<5> below 131071 images',
    'dw_kernel<3,1>': 'as dw_kernel<7,1>: stride-1 3x3 planes take dw_pair_kernel<3> below 131071 images',
}

# the two rows of the bitwise batched == per-image / flip-mode test: one mbconv row, one odd-filter deconv row
INVARIANCE_ROWS = ('mb24_144x160', 'odd_96x160')


def row(rid):
    return {r[0]: r for r in ROWS}[rid]


def arch_of(r):
    return copy.deepcopy(ARCHS[r[1]])


def head_of(r):
    """oracle.spec.HeadCfg of the row (``_joints``)."""
    return spec.HeadCfg(num_joints=r[6].get('_joints', 14))


def golden_id(r):
    """The row whose golden record this row reads: the first row with the same net and input size."""
    key = lambda q: (q[1], q[2], q[3], q[6].get('_joints', 14), bool(q[6].get('_plain')))
    return next(q[0] for q in ROWS if key(q) == key(r))


def storages_of(r):
    return r[6].get('_storages', ('f32', 'bf16') + (('f16',) if r[0] in F16_ROWS else ()))


def device_options(r):
    return {k: v for k, v in r[6].items() if not k.startswith('_')}


def shape_keys(arch, head=None):
    """Every layer shape of ``arch`` as launch_key's shape tuple."""
    d = spec.derive(arch, head)
    keys = set()
    for blocks in d['stages']:
        for b in blocks:
            keys.add((b['inp'], b['feat'], b['oup'], b['k'], b['stride'], bool(b['residual'])))
    for c in d['deconv']:
        keys.add((c['refined_in'] + c['raw_in'], 0, c['out'], 4, 2, False))
    for h in d['heads']:
        keys.add((h['refined_in'] + h['raw_in'], 0, h['oup'], 5, 1, False))
    return keys
