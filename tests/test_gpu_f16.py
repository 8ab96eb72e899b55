"""fp16-storage network path (LP_STORAGE_F16: the bf16 path's layout and kernels in IEEE half, the format the reference's
network_to_half uses, valid.py:152-153 -> lib/fp16_utils/fp16util.py:87-91).  Needs a real MI355X.

The protocol of tests/test_gpu_bf16.py at fp16 ulps (2^-10 relative), against tests/_f16_ref.py:
  (1) every launch against the emulation fed the device's own inputs (one launch per op);
  (2) the output of every fused launch against the emulation chained through the tensors it never stores;
  (3) network outputs against the fp32 oracle: within 2x the emulation's own distance, and strictly closer than the
      device's bf16 path on the same input;
  (4) batched == per-image, flip=2 == flip=0 + flip=1, bitwise;
  (5) the AE stage on the device's fp16-path maps bit-exact against the reference-semantics parser;
  (6) the kernel census rows of bf16 storage again under fp16: the same forms, the same checks;
  (7) folded weights in the fp16 SUBNORMAL range survive one 1x1 and one 7x7 depthwise, one launch per op;
  (8) the range edges through EVERY 16-bit kernel form, the fused ones included -- subnormal weights, inputs and inner
      tensors, and stores past 65504 -- with a derived bound: tests/_f16_range.py (the rows and the bound),
      tests/test_f16_range_cpu.py (coverage and preconditions), tests/test_gpu_f16_range.py (the device);
  (9) the engine end to end at BASELINE config 4's shape: records at least as close to the fp32 pipeline as bf16's.
"""
import numpy as np
import pytest
import torch

import _f16_ref
from _f16_range import ACC_REL, F16_ULP_REL, ulp16          # noqa: F401  (the unit of every bound here)
from _net_check import HEAD_ATOL, _model, _with_option, fused_inner, profiled_forward, set_options
from oracle import group_ref, inference_ref, net_ref, synth

pytestmark = pytest.mark.gpu

def layerwise_report(m, arch, sd, x):
    """tests/_net_check.py's layerwise_report at fp16: one launch per op ("mbtb" = "stem" = "headb" = 0), every launch
    against the emulated op on the device's own inputs, in units of ulp16.  [(name, max |d|, worst units, fraction
    differing, is_head)]."""
    outs = _with_option(m, 'headb', 0, lambda: _with_option(m, 'stem', 0, lambda: _with_option(
        m, 'mbtb', 0, lambda: [o.cpu() for o in m.forward_native(x.cuda(), 0)])))
    torch.cuda.synchronize()
    dev, rows, k_out = {'x': x}, [], 0
    mags = {n: fn for n, _, fn in _f16_ref.plan(sd, arch, absolute=True)}
    with torch.no_grad():
        for name, ins, fn in _f16_ref.plan(sd, arch):
            exp = fn(*[dev[k] for k in ins])
            head = name.startswith('final.') and name.endswith('.pw')
            if head:
                got = outs[k_out]
                k_out += 1
            else:
                got = m.tap(name).cpu().view(exp.shape)
            assert got.shape == exp.shape, (name, got.shape, exp.shape)
            dev[name] = got
            d = (got - exp).abs()
            ulp = ulp16(exp, mags[name](*[dev[k] for k in ins]))
            rows.append((name, float(d.max()), float((d / ulp).max()), float((d > 0).float().mean()), head))
    return rows


def check_f16(m, arch, sd, x, flip, outs, launch_names, chunk=8):
    """tests/_net_check.py's check_bf16 protocol at fp16 ulps against tests/_f16_ref.py: a launch that stores its own op
    <= 1 ulp16 on all but 1e-4 of the elements, <= 2 everywhere, < 2 % differing; a fused launch's output (inner tensors
    chained through the emulation) <= 1.5 ulp of the tensor's largest value with mean |d| <= 0.35 ulp of its mean
    magnitude (one inner tensor: also <= 2 own-ulp on all but 1e-3, < 5 % differing); heads within HEAD_ATOL.
    Returns {op name: (kind, max |d|, criterion value)}."""
    U = F16_ULP_REL
    mags = {n: fn for n, _, fn in _f16_ref.plan(sd, arch, absolute=True)}
    fused = fused_inner(launch_names)
    inner = {t for v in fused.values() for t in v}
    xin = x if flip == 0 else (torch.flip(x, [3]) if flip == 1 else torch.cat([x, torch.flip(x, [3])]))
    NB = xin.shape[0]
    plan = _f16_ref.plan(sd, arch)
    dev_full, k_out = {}, 0
    for name, _, _ in plan:
        if name in inner:
            continue
        if name.startswith('final.') and name.endswith('.pw'):
            dev_full[name] = outs[k_out]
            k_out += 1
        else:
            dev_full[name] = m.tap(name)
    rows, bad = {}, []
    for c0 in range(0, NB, chunk):
        c1 = min(NB, c0 + chunk)
        dev = {'x': xin[c0:c1]}
        with torch.no_grad():
            for name, ins, fn in plan:
                exp = fn(*[dev[k] for k in ins])
                if name in inner:
                    dev[name] = exp
                    continue
                got = dev_full[name].view((NB,) + tuple(exp.shape[1:]))[c0:c1].cpu()
                dev[name] = got
                d = (got - exp).abs()
                head = name.startswith('final.') and name.endswith('.pw')
                frac = float((d > 0).float().mean())
                if name in fused:
                    cap = 1.5 * U * float(exp.abs().max())
                    mean_rel = float(d.mean()) / (U * float(exp.abs().mean()) + 1e-12)
                    crit = max(float(d.max()) / cap, mean_rel / 0.35)
                    if float(d.max()) > cap or mean_rel > 0.35:
                        bad.append((name, c0, float(d.max()), cap, mean_rel))
                    elif len([t for t in fused[name] if t in inner]) == 1:
                        over = float((d > 2.0 * (exp.abs() * U + 1e-6)).float().mean())
                        if over > 1e-3 or frac > 0.05:
                            bad.append((name, c0, float(d.max()), over, frac))
                    kind = 'fused'
                elif head:
                    crit = float(d.max()) / HEAD_ATOL
                    if float(d.max()) > HEAD_ATOL:
                        bad.append((name, c0, float(d.max())))
                    kind = 'head'
                else:
                    r = d / ulp16(exp, mags[name](*[dev[k] for k in ins]))
                    ulps = float(r.max())
                    over1 = float((r > 1.0).float().mean())
                    crit = max(min(ulps, 1.0) if over1 <= 1e-4 else ulps, frac / 0.02)
                    if ulps > 2.0 or over1 > 1e-4 or frac > 0.02:
                        bad.append((name, c0, float(d.max()), ulps, over1, frac))
                    kind = 'op'
                prev = rows.get(name)
                if prev is None or crit > prev[2]:
                    rows[name] = (kind, float(d.max()), crit)
        assert not bad, bad[:8]
    return rows


# ------------------------------------------------------------------ (1) every launch
@pytest.mark.parametrize('arch_name,R,N', [('search-XS', 128, 3), ('search-XS', 256, 2), ('search-S', 448, 2),
                                           ('search-M', 256, 2), ('search-L', 128, 1)])
def test_f16_every_launch_vs_emulation_on_device_inputs(arch_name, R, N):
    m, arch, sd = _model(arch_name, storage='f16')
    assert m.storage == 'f16'
    x = synth.make_images(N, R, seed=41)
    rows = layerwise_report(m, arch, sd, x)
    bad = [r for r in rows if (r[1] > HEAD_ATOL if r[4] else (r[2] > 1.0 or r[3] > 0.02))]
    worst = max(rows, key=lambda r: r[2] if not r[4] else 0)
    print('f16 %s@%d: %d launches, worst %s: %.3g abs = %.2f ulp16, %.4f of elements differ'
          % (arch_name, R, len(rows), worst[0], worst[1], worst[2], worst[3]))
    assert not bad, bad[:8]


# ------------------------------------------------------------------ (2) fused launches, chained emulation
@pytest.mark.parametrize('arch_name,R,N', [('search-XS', 256, 2), ('search-S', 448, 2), ('search-M', 512, 1),
                                           ('search-L', 128, 1), ('search-XS', 128, 3)])
def test_f16_fused_launches_vs_chained_emulation(arch_name, R, N):
    m, arch, sd = _model(arch_name, storage='f16')
    x = synth.make_images(N, R, seed=41)
    outs, launches = profiled_forward(m, x.cuda(), 0)
    tags = {t for _, t in launches}
    assert {'stem4_kernel', 'mbtb_s2_kernel', 'mbtd_kernel'} <= tags, sorted(tags)
    rows = check_f16(m, arch, sd, x, 0, outs, [n for n, _ in launches])
    worst = max(rows.items(), key=lambda kv: kv[1][2])
    print('f16 %s@%d: %d launches (%s), worst criterion %.3f of its bound at %s'
          % (arch_name, R, len(launches), sorted(tags), worst[1][2], worst[0]))


# ------------------------------------------------------------------ (3) against fp32, and against bf16
@pytest.mark.parametrize('arch_name,R,N', [('search-XS', 256, 2), ('search-S', 448, 2), ('search-M', 512, 1)])
def test_f16_outputs_vs_fp32_oracle_and_closer_than_bf16(arch_name, R, N):
    m, arch, sd = _model(arch_name, storage='f16')
    mb, _, _ = _model(arch_name, storage='bf16')
    x = synth.make_images(N, R, seed=43)
    outs = [o.cpu() for o in m.forward_native(x.cuda(), 2)]
    outb = [o.cpu() for o in mb.forward_native(x.cuda(), 2)]
    with torch.no_grad():
        ref = net_ref.forward(x, sd, arch)
        ref_f = net_ref.forward(torch.flip(x, [3]), sd, arch)
        emu = _f16_ref.forward(x, sd, arch)
    for k in range(2):
        full = torch.cat([ref[k], ref_f[k]])
        scale = float(full.abs().max())
        d, db = (outs[k] - full).abs(), (outb[k] - full).abs()
        err, rms = float(d.max()), float(d.pow(2).mean().sqrt())
        errb, rmsb = float(db.max()), float(db.pow(2).mean().sqrt())
        emu_err = float((emu[k] - ref[k]).abs().max())
        err_plain = float((outs[k][:N] - ref[k]).abs().max())
        print('%s@%d out%d: |ref|max %.3f  f16 device-vs-fp32 max %.2e rms %.2e | bf16 device max %.2e rms %.2e | '
              'f16 emulation max %.2e' % (arch_name, R, k, scale, err, rms, errb, rmsb, emu_err))
        assert err_plain <= 2.0 * emu_err + 1e-3 * scale, (k, err_plain, emu_err)
        assert err < errb and rms < rmsb, (k, err, errb, rms, rmsb)


# ------------------------------------------------------------------ (4) batching and flip modes
def test_f16_batched_equals_per_image_and_flip_modes_bitwise():
    m, arch, sd = _model('search-S', storage='f16')
    N, R = 3, 192
    x = synth.make_images(N, R, seed=47).cuda()
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


# ------------------------------------------------------------------ (5) the AE stage on fp16-path maps
@pytest.mark.parametrize('arch_name,N,R', [('search-XS', 6, 256), ('search-S', 4, 448)])
def test_f16_engine_records_bit_exact_on_device_maps(arch_name, N, R):
    from litepose_amd import arch_zoo, config, engine
    arch = arch_zoo.get(arch_name)
    cfg = config.apply_arch(config.get_cfg(), arch)
    sd = synth.make_state_dict(arch, seed=1234, head_gain=0.25)
    eng = engine.PoseEngine(cfg, arch, sd, storage='f16')
    assert eng.model.storage == 'f16'
    x = synth.make_images(N, R, seed=5)
    off0, off1 = synth.lowres_offsets(8, N, 14, R, people=[4, 2, 7, 1, 3, 5][:N])
    f0, f1 = synth.flip_offsets(off0, off1, inference_ref.FLIP_CONFIG['CROWDPOSE'])
    offs = (torch.from_numpy(np.concatenate([off0, f0])).cuda(), torch.from_numpy(np.concatenate([off1, f1])).cuda())
    ans, count, scores = eng.infer_batch(x.cuda(), offsets=offs)
    torch.cuda.synchronize()
    det, tag = [t.cpu().numpy() for t in eng.last_maps()]
    with torch.no_grad():
        o = net_ref.forward(x, sd, arch)
        of = net_ref.forward(torch.flip(x, [3]), sd, arch)
        o = [o[0] + torch.from_numpy(off0), o[1] + torch.from_numpy(off1)]
        of = [of[0] + torch.from_numpy(f0), of[1] + torch.from_numpy(f1)]
        fh, tg = inference_ref.merge(o, of, inference_ref.TestCfg(), (R, R))
    err = float(np.abs(det - fh.numpy()).max())
    print('f16 engine: merged heatmap error vs the fp32 CPU pipeline %.2e' % err)
    assert err < 1e-2
    ora = group_ref.HeatmapParser(group_ref.Params())
    cnt, a_dev, s_dev = count.cpu().numpy(), ans.cpu().numpy(), scores.cpu().numpy()
    people = 0
    for n in range(N):
        a, sc = ora.parse_image(det[n], tag[n])
        assert cnt[n] == a.shape[0]
        assert np.array_equal(a_dev[n, :cnt[n]], a)
        assert np.array_equal(s_dev[n, :cnt[n]], sc)
        people += a.shape[0]
    assert people >= 15


# ------------------------------------------------------------------ (6) the kernel census under fp16
def _census_rows():
    from test_gpu_kernel_census import CASES
    return [c for c in CASES if c[2] == 'bf16']


_NETS = {}


def _net(arch_name, storage):
    if (arch_name, storage) not in _NETS:
        _NETS.clear()                    # one arch at a time: host memory of the bench-size rows
        _NETS[(arch_name, storage)] = _model(arch_name, storage=storage)
    return _NETS[(arch_name, storage)]


@pytest.mark.parametrize('cid', [c[0] for c in _census_rows()])
def test_f16_census_row_same_forms_as_bf16(cid):
    """Every bf16 row of tests/test_gpu_kernel_census.py's CASES again with storage 'f16': the forward launches exactly
    the kernel forms (tags) of the bf16 run of the row -- so every bf16 form of the census is reached under fp16 -- and
    passes check_f16.  fp16 storage shares bf16's dispatcher, gates and options."""
    case = {c[0]: c for c in _census_rows()}[cid]
    _, arch_name, _, H, W, N, flip, options, expect = case
    x = synth.make_images(N, H, seed=101 + N, w=W)
    tags = {}
    for storage in ('bf16', 'f16'):
        m, arch, sd = _net(arch_name, storage)
        old = set_options(m, options)
        try:
            outs, launches = profiled_forward(m, x.cuda(), flip)
            tags[storage] = {t for _, t in launches}
            if storage == 'f16':
                rows = check_f16(m, arch, sd, x, flip, outs, [n for n, _ in launches], chunk=8)
        finally:
            set_options(m, old)
    crit = max(r[2] for r in rows.values())
    print('%s f16: %d forms, worst criterion %.3f of its bound' % (cid, len(tags['f16']), crit))
    assert tags['f16'] == tags['bf16'], (sorted(tags['f16'] ^ tags['bf16']))
    assert set(expect) <= tags['f16']


def test_f16_refuses_odd_planes_loudly():
    from litepose_amd import _native as nv
    m, _, _ = _model('search-XS', storage='f16')
    x = synth.make_images(1, 16, seed=3).cuda()
    with pytest.raises(nv.LitePoseNativeError, match='f16 storage: unsupported layer shape at stage'):
        m.forward_native(x, 0)


# ------------------------------------------------------------------ (7) subnormal weights
def test_f16_subnormal_folded_weights_are_kept():
    """One 1x1 (the expand of stage.1.0: matrix-core A fragments) and one 7x7 stride-1 depthwise (banded MFMA fragments)
    get folded weights entirely in the fp16 subnormal range [2^-24, 2^-14); their outputs land in that range too.  A flush
    anywhere (host rounding, MFMA inputs, the f32 -> f16 store conversion, the f16 -> f32 unpack) zeroes them.  One
    launch per op, each against the emulation on the device's own inputs: every value within one fp16 ulp OF ITSELF
    (max(|v| 2^-10, 2^-24): the format's own spacing, no extra absolute floor) and nonzero wherever the emulation is."""
    from litepose_amd import arch_zoo
    from oracle import spec
    arch = arch_zoo.get('search-XS')
    d = spec.derive(arch)
    dw = next('stage.%d.%d.depth_conv' % (s, b) for s, blocks in enumerate(d['stages']) for b, blk in enumerate(blocks)
              if s >= 1 and blk['stride'] == 1 and blk['k'] == 7)
    targets = ('stage.1.0.inv', dw)
    sd = synth.make_state_dict(arch, seed=1234)
    g = torch.Generator().manual_seed(5)
    for key in targets:
        w = sd[key + '.0.weight']
        mag = 2.0 ** (-23.5 + 9.0 * torch.rand(w.shape, generator=g))             # 2^-23.5 .. 2^-14.5
        sd[key + '.0.weight'] = (mag * torch.sign(torch.randn(w.shape, generator=g))).float()
        for p, v in (('.1.weight', 1.0), ('.1.bias', 0.0), ('.1.running_mean', 0.0), ('.1.running_var', 1.0)):
            sd[key + p] = torch.full_like(sd[key + p], v)
    from _net_check import _cfg
    from litepose_amd.models import pose_mobilenet
    m = pose_mobilenet.get_pose_net(_cfg(), is_train=False, cfg_arch=arch, storage='f16')
    m.load_state_dict(sd, strict=True)
    x = synth.make_images(2, 256, seed=41)
    m.set_profiling(True)
    _with_option(m, 'headb', 0, lambda: _with_option(m, 'stem', 0, lambda: _with_option(
        m, 'mbtb', 0, lambda: m.forward_native(x.cuda(), 0))))
    torch.cuda.synchronize()
    kern = {n.split('|')[0]: n.split('|')[1] for n, _, _, _ in m.profile()}
    m.set_profiling(False)
    dev = {'x': x}
    with torch.no_grad():
        for name, ins, fn in _f16_ref.plan(sd, arch):
            if name.startswith('final.'):
                break
            exp = fn(*[dev[k] for k in ins])
            got = m.tap(name).cpu().view(exp.shape)
            dev[name] = got
            if name not in targets:
                continue
            nz = exp != 0
            sub = float(((exp.abs() < 2.0 ** -14) & nz).float().mean())
            ulp = torch.maximum(exp.abs() * F16_ULP_REL, torch.full_like(exp, 2.0 ** -24))
            worst = float(((got - exp).abs() / ulp).max())
            print('%s (%s): %.3f of the values nonzero, %.3f subnormal, worst %.2f ulp of the value'
                  % (name, kern.get(name), float(nz.float().mean()), sub, worst))
            assert float(nz.float().mean()) > 0.1 and sub > 0.1, (name, float(nz.float().mean()), sub)
            assert bool((got[nz] != 0).all()), (name, int((got[nz] == 0).sum()))
            assert worst <= 1.0, (name, worst)
    assert kern.get(dw) == 'dwt_kernel<7>' and kern.get('stage.1.0.inv') == 'pwb_kernel', kern


# ------------------------------------------------------------------ (9) end to end at BASELINE config 4's shape
def s448_parity(storage, B=8):
    """bench.py's config-4 workload (search-S 448x448, seeded synthetic scenes, head_gain 0.25) at a reduced batch through
    PoseEngine(storage=...), then bench.parity_check on every image: the records against the reference-semantics parser
    on the device maps and, reported, against the PURE fp32 CPU pipeline (joints identical, OKS)."""
    import bench
    from litepose_amd import arch_zoo, config, engine
    arch = arch_zoo.get('search-S')
    R = 448
    cfg = config.apply_arch(config.get_cfg(), arch)
    J = cfg.DATASET.NUM_JOINTS
    sd = synth.make_state_dict(arch, seed=1234, head_gain=0.25)
    eng = engine.PoseEngine(cfg, arch, sd, person_capacity=30, storage=storage)
    x = synth.make_images(B, R, seed=100).cuda()
    off0, off1 = synth.lowres_offsets(200, B, J, R)
    f0, f1 = synth.flip_offsets(off0, off1, inference_ref.FLIP_CONFIG['CROWDPOSE'])
    offs = (torch.from_numpy(np.concatenate([off0, f0])).cuda(), torch.from_numpy(np.concatenate([off1, f1])).cuda())
    rec = eng.infer_batch(x, offsets=offs)
    torch.cuda.synchronize()
    return bench.parity_check(eng, arch, sd, cfg, R, x, (off0, off1, f0, f1), rec, sample=range(B), tol=3e-2)


def test_f16_engine_parity_at_s448_at_least_as_close_as_bf16():
    res = {s: s448_parity(s) for s in ('bf16', 'f16')}
    p3 = {s: r['p3_vs_pure_cpu_pipeline'] for s, r in res.items()}
    for s in ('bf16', 'f16'):
        print(s, 'map error %.2e' % res[s]['heatmap_tag_max_abs_err'], p3[s])
        assert res[s]['ok'], res[s]
    b, h = p3['bf16'], p3['f16']
    assert h['joints_identical_position_and_presence'] >= b['joints_identical_position_and_presence'], (h, b)
    assert h['images_same_person_count'] >= b['images_same_person_count'], (h, b)
    assert h['oks_vs_cpu_persons']['min'] >= b['oks_vs_cpu_persons']['min'], (h, b)
    assert h['oks_vs_cpu_persons']['mean'] >= b['oks_vs_cpu_persons']['mean'], (h, b)
    assert res['f16']['heatmap_tag_max_abs_err'] < res['bf16']['heatmap_tag_max_abs_err']
