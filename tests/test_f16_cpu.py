"""CPU checks of the fp16-storage path (LP_STORAGE_F16): the storage switch, the host rounding of the folded weights,
and the fp16 emulation (tests/_f16_ref.py) that the GPU tests of tests/test_gpu_f16.py lean on, against the reference's
own half mode (tests/golden/golden_f16.npz) and against the bf16 emulation."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _f16_ref
from oracle import net_ref, synth

GOLDEN_F16_CASES = [('search-XS', 128, 2), ('search-XS', 256, 1), ('search-S', 224, 1), ('search-M', 256, 1)]
GOLDEN_F16_STRIDE = 7
LP_STORAGE_BF16, LP_STORAGE_F16 = 1, 2


def _rms(d):
    return float(np.sqrt((np.asarray(d, np.float64) ** 2).mean()))


def test_storage_argument_mapping():
    from litepose_amd import arch_zoo, config
    from litepose_amd.models import pose_mobilenet
    cfg = config.get_cfg()
    arch = arch_zoo.get('search-XS')
    for name in ('f16', 'fp16', 'float16'):
        assert pose_mobilenet.LitePose(cfg, cfg_arch=arch, storage=name).storage == 'f16'
        assert pose_mobilenet.get_pose_net(cfg, is_train=False, cfg_arch=arch, storage=name).storage == 'f16'
    assert pose_mobilenet.LitePose(cfg, cfg_arch=arch, storage='bf16').storage == 'bf16'
    assert pose_mobilenet.LitePose(cfg, cfg_arch=arch).storage == 'f32'
    cfg.FP16.ENABLED = True                          # the reference's switch keeps meaning bf16 storage
    assert pose_mobilenet.get_pose_net(cfg, is_train=False, cfg_arch=arch).storage == 'bf16'
    with pytest.raises(ValueError):
        pose_mobilenet.LitePose(cfg, cfg_arch=arch, storage='half')


def _host_round(x, storage):
    from litepose_amd import _native as nv
    lib = nv.lib()
    src = np.ascontiguousarray(x, np.float32)
    dst = np.empty_like(src)
    rc = lib.lp_round16(src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), src.size, storage)
    assert rc == 0, lib.lp_last_error()
    return dst


def test_host_rounding_matches_torch_and_keeps_fp16_subnormals():
    """lp_round16 = the rounding lp_net_finalize applies to the folded weights.  fp16: RNE, overflow to +-inf and
    SUBNORMALS KEPT (about 0.1 % of the synthetic raw conv weights lie below the smallest normal half, 6.1e-5)."""
    rng = np.random.default_rng(7)
    tiny = np.float32(2.0 ** -24)                                    # smallest fp16 subnormal
    special = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 65504.0, 65520.0, 70000.0,
                        -1e6, 6.0e-5, 6.1e-5, 3.0e-5, 1.0e-6, tiny, 0.5 * tiny, 0.75 * tiny, 0.25 * tiny, 3.0 * tiny,
                        2.5 * tiny, 0.0, -0.0, 0.1], np.float32)
    x = np.concatenate([special, rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.uniform(-9, 4, 4096)])
    x = x.astype(np.float32)
    got = _host_round(x, LP_STORAGE_F16)
    want = torch.from_numpy(x).to(torch.float16).to(torch.float32).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    sub = (np.abs(want) > 0) & (np.abs(want) < 2.0 ** -14)
    assert sub.sum() > 100 and np.all(got[sub] != 0.0)               # the subnormal range survives
    assert got[2] == 1.0 + 2 * 2.0 ** -10 and got[1] == 1.0           # ties to even
    assert np.isinf(got[6]) and np.isinf(got[7]) and got[5] == np.inf  # overflow -> inf (65520 rounds up)
    assert got[13] == 0.0 and got[14] == tiny and got[16] == 3 * tiny and got[17] == 2 * tiny
    # bf16: the existing rounding, unchanged
    gb = _host_round(x, LP_STORAGE_BF16)
    assert np.array_equal(gb.view(np.uint32), net_ref._rb(torch.from_numpy(x)).numpy().view(np.uint32))
    from litepose_amd import _native as nv
    assert nv.lib().lp_round16(x.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), 1, 0) != 0


def test_library_host_code_rounds_to_half_only_from_float():
    """The folded weights are rounded double -> float -> half, like the emulation's ``w.float().to(float16)``.  A direct
    double -> half conversion (__truncdfhf2, what clang folds the two steps into without a barrier) rounds the weights
    that are exact fp16 ties as floats the other way -- 1 to 8 per layer of the synthetic nets, one fp16 ulp each, seen
    on the device as wrong depthwise outputs.  engine.cpp must not contain it."""
    from litepose_amd import _native as nv
    nv.lib()
    with open(nv.LIB_PATH, 'rb') as f:
        image = f.read()
    assert b'__truncsfhf2' in image                  # the float -> half conversion: symbol names are in the image
    assert b'__truncdfhf2' not in image


FAMILIES_16 = ('stemb_kernel', 'dwb_kernel', 'dwt_kernel', 'pwb_kernel', 'deconvb_kernel', 'headb_kernel',
               'octet_to_planar_kernel', 'mbtb_kernel', 'mbtb_s2_kernel', 'mbtd_kernel')


def _check_format_census(res):
    """Every kernel of the 16-bit path is one template with the format leading (csrc/fmt16.h): the instances of a family
    under lp::Bf16 and under lp::F16 have the same template lists, stem4_kernel has the same C0 under lp::F32 as well."""
    forms = {}                                        # family -> format -> set of template lists after the format
    for name in res:
        base, _, args = name.partition('<')
        if base.startswith('lp::') and base[4:] in FAMILIES_16 + ('stem4_kernel',):
            fmt, _, rest = args.rstrip('>').partition(', ')
            assert fmt in ('lp::F32', 'lp::Bf16', 'lp::F16'), '%s: no leading format argument' % name
            forms.setdefault(base[4:], {}).setdefault(fmt, set()).add(rest)
    for fam in FAMILIES_16:
        by = forms.get(fam, {})
        assert set(by) == {'lp::Bf16', 'lp::F16'}, (fam, sorted(by))
        assert by['lp::Bf16'] == by['lp::F16'] and by['lp::Bf16'], (fam, sorted(by['lp::Bf16'] ^ by['lp::F16']))
    stem = forms.get('stem4_kernel', {})
    assert set(stem) == {'lp::F32', 'lp::Bf16', 'lp::F16'}, sorted(stem)
    assert stem['lp::F32'] == stem['lp::Bf16'] == stem['lp::F16'] and stem['lp::F32'], stem
    for fmt in ('lp::Bf16', 'lp::F16'):
        n = sum(len(by[fmt]) for by in forms.values())
        assert n == 51, (fmt, n)


def test_every_16bit_kernel_is_built_in_both_formats_with_the_same_template_list():
    import json
    from litepose_amd import build as _b
    path = os.path.join(_b.LIBDIR, 'kernel_resources.json')
    if not os.path.exists(path):
        pytest.skip('no kernel resource report (written by `python -m litepose_amd.build`)')
    res = json.load(open(path))
    _check_format_census(res)
    # the check can fail: a form missing in one format, a stem missing in fp32, an instance without a format
    for gone in ('lp::pwb_kernel<lp::F16, 1, 2, false, false>', 'lp::mbtd_kernel<lp::Bf16, 2, 1, true>',
                 'lp::stem4_kernel<lp::F32, 24>', 'lp::headb_kernel<lp::F16, false>'):
        less = dict(res)
        del less[gone]
        with pytest.raises(AssertionError):
            _check_format_census(less)
    with pytest.raises(AssertionError, match='no leading format'):
        _check_format_census(dict(res, **{'lp::dwb_kernel<7, 1>': {}}))


def test_f16_plan_names_match_the_bf16_plan_and_stored_tensors_are_half():
    from litepose_amd import arch_zoo
    arch = arch_zoo.get('search-XS')
    sd = synth.make_state_dict(arch, seed=3)
    assert [n for n, _, _ in _f16_ref.plan(sd, arch)] == [n for n, _, _ in net_ref.bf16_plan(sd, arch)]
    assert [i for _, i, _ in _f16_ref.plan(sd, arch)] == [i for _, i, _ in net_ref.bf16_plan(sd, arch)]
    x = synth.make_images(1, 64, seed=2)
    with torch.no_grad():
        taps = {}
        o16 = _f16_ref.forward(x, sd, arch, taps=taps)
        ob = _f16_ref.forward(x, sd, arch, rnd=net_ref._rb)
        ob_ref = net_ref.forward_bf16(x, sd, arch)
    for a, b in zip(ob, ob_ref):                     # the restatement with bf16 rounding IS the bf16 emulation
        assert torch.equal(a, b)
    for k, v in taps.items():
        if k.startswith('final.') and k.endswith('.pw'):
            continue
        assert torch.equal(v, _f16_ref.rh(v)), k
    assert not torch.equal(o16[0], _f16_ref.rh(o16[0]))


@pytest.mark.parametrize('arch_name,R,N', GOLDEN_F16_CASES)
def test_f16_emulation_within_twice_the_reference_half_modes_distance(arch_name, R, N):
    """tests/_f16_ref.py against the REAL reference run in its own half recipe (network_to_half, torch.float16; fixture
    tests/golden/golden_f16.npz): the emulation's distance from the reference's fp32 outputs is at most 2x the reference
    half mode's own distance, max and rms (measured at fixture time: 0.6-0.75x)."""
    from litepose_amd import arch_zoo
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_f16.npz'))
    arch = arch_zoo.get(arch_name)
    sd = synth.make_state_dict(arch, seed=1234)
    x = synth.make_images(N, R, seed=21)
    with torch.no_grad():
        outs = _f16_ref.forward(x, sd, arch)
    for k in range(2):
        key = '%s_%d_out%d' % (arch_name, R, k)
        a = outs[k].numpy()
        assert tuple(a.shape) == tuple(g[key + '_shape'])
        s = a.reshape(-1)[::GOLDEN_F16_STRIDE]
        r32, rh = g[key + '_ref32'], g[key + '_reff16']
        d_ref, d_us = rh - r32, s - r32
        assert _rms(d_us) <= 2.0 * _rms(d_ref), (key, _rms(d_us), _rms(d_ref))
        assert np.abs(d_us).max() <= 2.0 * np.abs(d_ref).max(), (key, np.abs(d_us).max(), np.abs(d_ref).max())


@pytest.mark.parametrize('arch_name,R,N', GOLDEN_F16_CASES)
def test_f16_emulation_is_several_times_closer_to_fp32_than_bf16(arch_name, R, N):
    """The point of the format: 3 more mantissa bits.  On every fixture case the fp16 emulation's max and rms distance
    from fp32 is <= 0.25x the bf16 emulation's (measured 0.10-0.14x)."""
    from litepose_amd import arch_zoo
    arch = arch_zoo.get(arch_name)
    sd = synth.make_state_dict(arch, seed=1234)
    x = synth.make_images(N, R, seed=21)
    with torch.no_grad():
        o32 = net_ref.forward(x, sd, arch)
        oh = _f16_ref.forward(x, sd, arch)
        ob = net_ref.forward_bf16(x, sd, arch)
    for k in range(2):
        dh, db = (oh[k] - o32[k]).numpy(), (ob[k] - o32[k]).numpy()
        assert np.abs(dh).max() <= 0.25 * np.abs(db).max(), (k, np.abs(dh).max(), np.abs(db).max())
        assert _rms(dh) <= 0.25 * _rms(db), (k, _rms(dh), _rms(db))
