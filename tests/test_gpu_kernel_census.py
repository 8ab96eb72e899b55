"""Kernel census: every form the network dispatcher can choose (engine.cpp forward loops; each launcher names its form in
``last_kernel_tag``) against the reference, at the shapes, batches and options that select it.

``CASES`` is one table, importable without a GPU (tests/test_kernel_census_cpu.py reads it): a row is
``(id, arch, storage, H, W, N, flip, options, expect)``.  ``expect`` is the set of kernel tags the row's forward must
launch; every tag in the sources is either expected by some row or listed in ``NOT_REACHED`` with the reason.

Per row, one profiled forward (the whole batch in one launch per op) and then the comparison of EVERY image of the
batch (flip=2: the mirrored half against the oracle on torch.flip(x, [3])):
  * fp32: the block taps scaled by their magnitude (< 2e-5) and both outputs at 2e-5 against net_ref.forward; then, on
    three images, every unit of the net in float64 on the device's own input taps, per element (P) and per tap (R):
    tests/_fp32_units.py.  Measured over the fp32 rows: P at most 0.732 of c_max (prune_s_native_f32), R at most 0.142
    of m; the unit check costs a row 0.1 to 1.5 s (the three slowest: m512_b2_f32_flip 0.2 -> 1.7 s, s448_b4_f32_flip
    0.1 -> 1.2 s of comparison time, xs256_b64_f32_flip 0.6 -> 1.3 s);
  * bf16: every launch against net_ref.bf16_plan fed the device's own inputs (<= 1 bf16 ulp, < 2 % of the elements
    differing, heads within 2e-5); the output of a fused launch against the emulation chained through the tensors it
    never stores (tests/_net_check.py: check_bf16).
test_census_covers_production_launches keys every launch of the published archs and the BASELINE configs by
(tag, Cin, Cexp, Cout, K, stride, residual) and requires each key to be produced by some row."""
import pytest
import torch

from oracle import spec, synth

# (id, arch, storage, H, W, N, flip, options, expect)
CASES = [
    # ---- bench shapes at full batch (BASELINE configs 2/3, 4, 5) and the fp32 trunk of S / M (120-channel stage 4)
    ('xs256_b64_f32_flip', 'search-XS', 'f32', 256, 256, 64, 2, {},
     {'stem4_kernel', 'mbconv2_kernel', 'mbt_s2_kernel', 'mbt_kernel', 'mb16_kernel', 'headfuse_kernel'}),
    ('s448_b32_bf16_flip', 'search-S', 'bf16', 448, 448, 32, 2, {},
     {'stem4_kernel', 'mbtd_kernel', 'mbtb_s2_kernel', 'mbtb_kernel', 'headb_kernel', 'deconvb_kernel'}),
    ('m512_b32_bf16_flip', 'search-M', 'bf16', 512, 512, 32, 2, {},
     {'stem4_kernel', 'mbtd_kernel', 'mbtb_s2_kernel', 'mbtb_kernel', 'headb_kernel', 'deconvb_kernel'}),
    ('s448_b4_f32_flip', 'search-S', 'f32', 448, 448, 4, 2, {}, {'mbt_kernel', 'pw3d_kernel', 'dw_pair_kernel<7>'}),
    ('m512_b2_f32_flip', 'search-M', 'f32', 512, 512, 2, 2, {}, {'pw3d_kernel', 'pw3_kernel', 'dw_pair_kernel<7>', 'dw_kernel<7,2>'}),
    # ---- the seven published archs at their native img_size, both storages
    ('xs_native_f32', 'search-XS', 'f32', 256, 256, 3, 0, {}, {'deconv4_kernel', 'deconv4x3_kernel'}),
    ('s_native_f32', 'search-S', 'f32', 448, 448, 1, 0, {}, set()),
    ('m_native_f32', 'search-M', 'f32', 448, 448, 1, 0, {}, set()),
    ('l_native_f32', 'search-L', 'f32', 512, 512, 1, 0, {}, {'dwpw_kernel'}),
    ('prune_s_native_f32', 'prune-S', 'f32', 512, 512, 1, 0, {}, set()),
    ('prune_m_native_f32', 'prune-M', 'f32', 512, 512, 1, 0, {}, set()),
    ('prune_l_native_f32', 'prune-L', 'f32', 512, 512, 1, 0, {}, set()),
    ('xs_native_bf16', 'search-XS', 'bf16', 256, 256, 3, 0, {}, {'mbtd_kernel', 'mbtb_s2_kernel'}),
    ('s_native_bf16', 'search-S', 'bf16', 448, 448, 1, 0, {}, set()),
    ('m_native_bf16', 'search-M', 'bf16', 448, 448, 1, 0, {}, set()),
    # search-L's 160-channel blocks: mbtb_kernel<10, 5> would spill and is not built -> the pwb / dwt / pwb chain
    ('l_native_bf16', 'search-L', 'bf16', 512, 512, 1, 0, {}, {'pwb_kernel', 'dwt_kernel<7>', 'mbtb_kernel'}),
    ('prune_s_native_bf16', 'prune-S', 'bf16', 512, 512, 1, 0, {}, set()),
    ('prune_m_native_bf16', 'prune-M', 'bf16', 512, 512, 1, 0, {}, set()),
    ('prune_l_native_bf16', 'prune-L', 'bf16', 512, 512, 1, 0, {}, {'pwb_kernel'}),
    # ---- both sides of the gates
    # mb16_kernel: a launch of >= opt_mb16_min (48) images; flip=2 doubles the launch
    ('mb16_nb46_flip', 'search-XS', 'f32', 256, 256, 23, 2, {}, set()),
    ('mb16_nb48_flip', 'search-XS', 'f32', 256, 256, 24, 2, {}, {'mb16_kernel'}),
    ('mb16_nb47', 'search-XS', 'f32', 256, 256, 47, 0, {}, {'dw_pair16_kernel<7>'}),
    ('mb16_nb48', 'search-XS', 'f32', 256, 256, 48, 0, {}, {'mb16_kernel'}),
    # the residual blocks of <= 32 channels (bf16) have no batch gate: mbtd_kernel by default, mbtb_kernel with option
    # "mbtd" = 0, on either side of 1024 16x16 tiles per launch (where a form since removed used to take over from
    # mbtb_kernel).  XS@512: stage 1 on 128x128 planes = 64 tiles per image
    ('mbtd_960_default', 'search-XS', 'bf16', 512, 512, 15, 0, {}, {'mbtd_kernel'}),
    ('mbtd_1024_default', 'search-XS', 'bf16', 512, 512, 8, 2, {}, {'mbtd_kernel'}),
    ('mbtb_960_mbtd0', 'search-XS', 'bf16', 512, 512, 15, 0, {'mbtd': 0}, {'mbtb_kernel'}),
    # mbconv_s2_kernel's gate (24-channel stride-2 entry block, output plane >= 1024 pixels) on both sides: search-L's
    # entry block expands to 144 channels, which the kernel refuses (Cexp % 32), so both sides take the unfused chain
    ('mbconv_s2_896', 'search-L', 'f32', 112, 128, 2, 0, {}, {'dw_kernel<7,2>'}),
    ('mbconv_s2_1024', 'search-L', 'f32', 128, 128, 2, 0, {}, {'dw_kernel<7,2>'}),
    # ---- edge planes: the smallest legal input, extreme aspect ratios, a ragged plane, odd batches (grids that are not
    # a multiple of the 8 XCDs)
    ('xs16_f32', 'search-XS', 'f32', 16, 16, 3, 2, {}, {'dw_pair_kernel<5>', 'pw2_kernel'}),
    # bf16 storage needs an even pixel count on every plane (pwb_kernel): its smallest square input is 32 x 32 (2 x 2
    # planes); 16 x 16 is refused loudly (test_bf16_refuses_odd_planes_loudly)
    ('xs32_bf16', 'search-XS', 'bf16', 32, 32, 3, 2, {}, set()),
    ('xs16x32_bf16', 'search-XS', 'bf16', 16, 32, 3, 0, {}, set()),
    ('xs16x1024_f32', 'search-XS', 'f32', 16, 1024, 1, 0, {}, set()),
    ('xs16x1024_bf16', 'search-XS', 'bf16', 16, 1024, 1, 0, {}, set()),
    ('xs64x1024_bf16', 'search-XS', 'bf16', 64, 1024, 1, 2, {}, set()),
    ('xs1024x64_f32', 'search-XS', 'f32', 1024, 64, 1, 2, {}, set()),
    ('s208x336_f32', 'search-S', 'f32', 208, 336, 3, 2, {}, {'dw_pair_kernel<5>', 'pw2_kernel'}),
    ('m208x336_bf16', 'search-M', 'bf16', 208, 336, 3, 2, {}, set()),
    ('l208x336_f32', 'search-L', 'f32', 208, 336, 1, 0, {}, set()),
    # ---- option values that select a distinct form
    ('opt_mbt0', 'search-XS', 'f32', 256, 256, 2, 0, {'mbt': 0}, {'dwpw_kernel', 'dw_pair_kernel<7>'}),
    ('opt_mbt2', 'search-XS', 'f32', 256, 256, 2, 0, {'mbt': 2}, {'mbt_kernel'}),
    ('opt_mbt3', 'search-XS', 'f32', 256, 256, 2, 0, {'mbt': 3}, {'mbt_s2_kernel'}),
    ('opt_mbt_s2_0', 'search-XS', 'f32', 256, 256, 2, 0, {'mbt_s2': 0}, {'dw_kernel<7,2>'}),
    ('opt_mbconv2_0', 'search-XS', 'f32', 256, 256, 2, 0, {'mbconv2': 0}, set()),
    ('opt_mb16_run0', 'search-XS', 'f32', 256, 256, 24, 2, {'mb16_run': 0}, {'mb16_kernel'}),
    ('opt_pw3d0', 'search-XS', 'f32', 256, 256, 2, 0, {'pw3d': 0}, {'pw3_kernel'}),
    ('opt_pw3d2', 'search-M', 'f32', 256, 256, 2, 0, {'pw3d': 2}, {'pw3d_kernel'}),
    ('opt_stem0_f32', 'search-XS', 'f32', 128, 192, 2, 2, {'stem': 0}, {'stem_kernel', 'dwpw_kernel'}),
    ('opt_stem0_bf16', 'search-XS', 'bf16', 128, 192, 2, 2, {'stem': 0}, {'stemb_kernel', 'dwb_kernel<3,1>'}),
    ('opt_headb0', 'search-S', 'bf16', 224, 224, 2, 2, {'headb': 0}, {'dwt_kernel<5>', 'pwb_kernel'}),
    ('opt_dwt0', 'search-M', 'bf16', 256, 256, 2, 0, {'dwt': 0, 'mbtb': 0},
     {'dwb_kernel<7,1>', 'dwb_kernel<5,1>', 'dwb_kernel<7,2>'}),
    ('opt_dwt1', 'search-M', 'bf16', 256, 256, 2, 0, {'dwt': 1, 'mbtb': 0}, {'dwt_kernel<7>', 'dwb_kernel<5,1>'}),
    ('opt_mbtb0', 'search-S', 'bf16', 224, 224, 3, 0, {'mbtb': 0}, {'pwb_kernel', 'dwb_kernel<7,2>'}),
    ('opt_mbtb_s2_0', 'search-S', 'bf16', 224, 224, 3, 0, {'mbtb_s2': 0}, {'dwb_kernel<7,2>'}),
]

# kernel tag -> why no CASES row reaches it (the option value or shape that would).  CASES holds published architectures
# only; the forms a custom ``cfg_arch`` selects are launched and compared by the rows of tests/_custom_space.py
# (tests/test_gpu_custom_census.py), named here; tests/test_custom_census_cpu.py requires every entry to be expected by
# such a row or listed in its UNREACHABLE
NOT_REACHED = {
    'dw_kernel<7,1>': 'launch_dw takes dw_pair_kernel for every stride-1 plane up to 131070 images (grid.y <= 65535 '
                      'image pairs); only a larger launch would fall back to it',
    'dw_kernel<5,1>': 'as dw_kernel<7,1>: stride-1 5x5 planes take dw_pair_kernel<5> below 131071 images',
    'dw_kernel<3,1>': 'as dw_kernel<7,1>: stride-1 3x3 planes take dw_pair_kernel<3> below 131071 images',
    'dw_kernel<5,2>': 'no published arch has a stride-2 5x5 depthwise (heads are stride 1); a custom stage whose entry '
                      'block is 5x5 does: custom rows five_128, ksize_256, ksize_128',
    'dw_kernel<3,2>': 'no published arch has a stride-2 3x3 depthwise (the stem depthwise is stride 1); a custom stage '
                      'whose entry block is 3x3 does: custom rows five_128, ksize_256, ksize_128',
    'dw_pair_kernel<3>': 'the fp32 stem depthwise runs in stem4_kernel (option "stem" = 1) or dwpw_kernel<3> ("stem" = 0); '
                         'a custom 3x3 residual block runs it: custom rows ksize_256, ksize_128',
    'dw_pair16_kernel<5>': 'a 16x16 head plane alone; headfuse_kernel takes every 16x16 head plane of the published archs '
                           '(the heads fall back to dw_pair_kernel<5> + pw2_kernel only on planes it refuses: xs16_f32, '
                           's208x336_f32); custom 5x5 blocks on 16x16 planes and the odd-filter head of odd_64 run it',
    'dw_pair16_kernel<3>': 'as dw_pair_kernel<3>: the stem depthwise never runs alone; custom 3x3 blocks on 16x16 planes '
                           'run it: custom rows ksize_256, ksize_128',
    'dwb_kernel<5,2>': 'no published arch has a stride-2 5x5 depthwise; custom rows five_128, ksize_256, ksize_128 (bf16, f16)',
    'dwb_kernel<3,2>': 'no published arch has a stride-2 3x3 depthwise; custom rows five_128, ksize_256, ksize_128 (bf16, f16)',
    'mbconv_kernel': 'needs a 24-channel stride-1 block whose expansion is a multiple of 32 channels; the published archs '
                     'expand 24 channels to 144 (Cexp % 32 != 0); custom rows mb24_128, mb24_144x160, five_128 (expand 4)',
    'mbconv_s2_kernel': 'needs a 24-channel stride-2 entry block with <= 32 filters and an expansion that is a multiple '
                        'of 32; search-L / prune-M / prune-L expand to 144 (the gate cases mbconv_s2_896 / _1024 show the '
                        'chain taken on both sides); custom rows mb24_128, mb24_144x160, mb24_w34',
    'deconv_mfma_kernel': 'deconv layers whose channel counts leave no four-parity packing (odd inputs, or a total that is '
                          'no multiple of 4) and <= 32 filters; every published arch has even inputs and <= 64 filters '
                          '(deconv4 / deconv4x3); custom rows odd_64, odd_96x160, plain_mfma_64',
    'deconv_pair_kernel': 'scalar deconv fallback for shapes without an MFMA packing (> 64 filters, or > 32 with channel '
                          'counts that have no four-parity packing); custom rows pair66_64, wide72_64, plain_pair_64',
}


def _case_by_id():
    return {c[0]: c for c in CASES}


_MODELS = {}
RESULTS = {}              # case id -> (tags, worst criterion): the table of test_census_covers_production_launches
UNITS = {}                # fp32 case id -> (worst P as a fraction of c_max, worst R as a fraction of m): tests/_fp32_units.py


def _net(arch_name, storage):
    from _net_check import _model
    key = (arch_name, storage)
    if key not in _MODELS:
        _MODELS[key] = _model(arch_name, storage=storage)
    return _MODELS[key]


def _run_case(case, compare):
    from _net_check import check_bf16, check_fp32, profiled_forward, set_options
    cid, arch_name, storage, H, W, N, flip, options, expect = case
    m, arch, sd = _net(arch_name, storage)
    old = set_options(m, options)
    try:
        x = synth.make_images(N, H, seed=101 + N, w=W)
        outs, launches = profiled_forward(m, x.cuda(), flip)
        if not compare:
            return launches, None
        if storage == 'f32':
            # bench-size batches: the taps of the first chunk of each half, every image's outputs
            worst = check_fp32(m, arch, sd, x, flip, outs, chunk=8, tap_images=8 if N > 16 else None)
            crit = worst[0] / 2e-5
            UNITS[cid] = worst[3:5]
        else:
            rows = check_bf16(m, arch, sd, x, flip, outs, [n for n, _ in launches], chunk=8)
            crit = max(r[2] for r in rows.values())
        return launches, crit
    finally:
        set_options(m, old)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_kernel_form_vs_reference(cid):
    case = _case_by_id()[cid]
    launches, crit = _run_case(case, compare=True)
    tags = {t for _, t in launches}
    RESULTS[cid] = (tags, crit)
    units = '; units P %.3f of c_max, R %.3f of m' % UNITS[cid] if cid in UNITS else ''
    print('%s: %d launches, worst criterion %.3f of its bound%s; tags %s' % (cid, len(launches), crit, units, sorted(tags)))
    missing = set(case[8]) - tags
    assert not missing, ('expected forms not launched', sorted(missing), sorted(tags))


def _keys(launches, arch_name):
    from _net_check import launch_key
    from litepose_amd import arch_zoo
    d = spec.derive(arch_zoo.get(arch_name))
    return {launch_key(n, t, d) for n, t in launches}


# the launches production makes: the published archs at their native size (flip-TTA, one image) and the BASELINE
# configs at their bench batch with flip=2, plus the half batch the engine's pipelined halves launch
PRODUCTION = [(a, s, None, 1, 2) for a in ('search-XS', 'search-S', 'search-M', 'search-L', 'prune-S', 'prune-M',
                                            'prune-L') for s in ('f32', 'bf16')] + [
    ('search-XS', 'f32', 256, 1, 2), ('search-XS', 'f32', 256, 64, 2), ('search-XS', 'f32', 256, 32, 2),
    ('search-S', 'bf16', 448, 32, 2), ('search-S', 'bf16', 448, 16, 2),
    ('search-M', 'bf16', 512, 32, 2), ('search-M', 'bf16', 512, 16, 2)]


@pytest.mark.gpu
def test_census_covers_production_launches():
    from litepose_amd import arch_zoo
    covered, by_tag = {}, {}
    for case in CASES:
        launches, _ = _run_case(case, compare=False)
        for k in _keys(launches, case[1]):
            covered.setdefault(k, []).append(case[0])
            by_tag.setdefault(k[0], set()).add(case[0])
    unreached = {}
    for arch_name, storage, R, N, flip in PRODUCTION:
        R = R or arch_zoo.get(arch_name)['img_size']
        case = ('prod', arch_name, storage, R, R, N, flip, {}, set())
        launches, _ = _run_case(case, compare=False)
        for k in _keys(launches, arch_name):
            if k not in covered:
                unreached.setdefault(k, []).append('%s/%s@%d N=%d' % (arch_name, storage, R, N))
    print('\nkernel census: tag -> cases -> worst criterion (fraction of its bound; "-" = not compared in this run)')
    for tag in sorted(by_tag):
        ids = sorted(by_tag[tag])
        crits = [RESULTS[i][1] for i in ids if i in RESULTS]
        print('  %-22s %3d cases  worst %s  %s' % (tag, len(ids), '%.3f' % max(crits) if crits else '-',
                                                   ' '.join(ids[:6]) + (' ...' if len(ids) > 6 else '')))
    from test_kernel_census_cpu import source_tags
    never = sorted(t for t in source_tags() if t not in NOT_REACHED and t not in by_tag)
    assert not unreached, ('production launch keys no CASES row produces', sorted(unreached.items())[:12])
    assert not never, ('tags neither launched by a CASES row nor listed in NOT_REACHED', never)


@pytest.mark.gpu
def test_bf16_refuses_odd_planes_loudly():
    """bf16 storage needs an even pixel count on every plane; a 16 x 16 input (1 x 1 deepest planes) is an error that
    names the layer, never a silent fallback."""
    from litepose_amd import _native as nv
    m, _, _ = _net('search-XS', 'bf16')
    x = synth.make_images(1, 16, seed=3).cuda()
    with pytest.raises(nv.LitePoseNativeError, match='unsupported layer shape at stage'):
        m.forward_native(x, 0)
