"""pose_simplenet on the device (lp_arch.plain_head = 1: LitePose without the Fusion Deconv Head, reference
lib/models/pose_simplenet.py).  Needs a real MI355X.

  * fp32: outputs against the REAL reference module's samples (tests/golden/gen_golden_simplenet.py) at NET_ATOL, block
    and deconv taps against tests/_simplenet_ref.py;
  * bf16 / fp16: every launch against the 16-bit emulation of tests/_simplenet_ref.py fed the device's own inputs, the
    fused block launches against the emulation chained through the tensors they never store (the protocol of
    tests/_net_check.py: check_bf16);
  * the one-source head forms (headfuse_kernel fp32, headb_kernel bf16 / fp16) bitwise against the unfused chain, one
    launch per output stage, and no dual-source deconv / head launch anywhere;
  * batched == per-image and flip=2 == an explicit flip, bitwise;
  * the engine on a simplenet.yaml cfg: records against the oracle parser on the device maps, and ``evaluate`` on mixed
    sizes against the reference-shaped batch-1 loop."""
import os

import numpy as np
import pytest
import torch

import _simplenet_ref as snr
from _net_check import HEAD_ATOL, NET_ATOL, TAP_REL, _with_option, fp32_tap_names, fused_inner, profiled_forward
from conftest import ROOT
from oracle import group_ref, inference_ref, net_ref, spec, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_simplenet.npz')
YAML = os.path.join(ROOT, 'tests', 'golden', 'simplenet.yaml')
ULP_REL = {'bf16': 2.0 ** -7, 'f16': 2.0 ** -10}


def _cfg():
    from litepose_amd import config
    return config.get_cfg('crowd_pose')


def _model(arch_name, storage='f32', seed=1234, head_gain=1.0):
    from litepose_amd import arch_zoo
    import litepose_amd.models as models
    arch = arch_zoo.get(arch_name)
    sd = snr.make_state_dict(arch, seed=seed, head_gain=head_gain)
    m = models.pose_simplenet.get_pose_net(_cfg(), is_train=False, cfg_arch=arch, storage=storage)
    m.load_state_dict(sd, strict=True)
    return m, arch, sd


def _rnd(storage):
    import _f16_ref
    return net_ref._rb if storage == 'bf16' else _f16_ref.rh


def _unit(storage, exp, mag):
    """One ulp of the emulated value; fp16 adds 2^-20 of the element's term-magnitude sum (tests/test_gpu_f16.py: ulp16)."""
    if storage == 'bf16':
        return exp.abs() * ULP_REL['bf16'] + 1e-6
    return torch.clamp(exp.abs() * ULP_REL['f16'], min=2.0 ** -24) + 2.0 ** -20 * mag


# ------------------------------------------------------------------ fp32
@pytest.mark.parametrize('arch_name,hw', [('search-XS', (64, 64)), ('search-S', (64, 64)), ('search-M', (96, 160))])
def test_fp32_vs_reference_samples_and_taps(arch_name, hw):
    golden = np.load(GOLDEN)
    m, arch, sd = _model(arch_name)
    H, W = hw
    x = synth.make_images(1, H, seed=11, w=W)
    out = m(x.cuda())
    taps = {}
    with torch.no_grad():
        ref = snr.forward(x, sd, arch, taps=taps)
    for k, t in enumerate(out):
        key = '%s_%dx%d_out%d' % (arch_name, H, W, k)
        assert tuple(t.shape) == tuple(golden[key + '_shape'])
        np.testing.assert_allclose(t.cpu().numpy().reshape(-1)[::13], golden[key + '_sample'], rtol=0, atol=NET_ATOL)
        assert float((t.cpu() - ref[k]).abs().max()) <= NET_ATOL
    for nm in fp32_tap_names(spec.derive(arch)):
        r = taps[nm]
        got = m.tap(nm).view(r.shape).cpu()
        assert float((got - r).abs().max()) / max(1.0, float(r.abs().max())) < TAP_REL, nm
    # a tap named for a raw-branch op does not exist on this net
    from litepose_amd import _native as nv
    with pytest.raises(nv.LitePoseNativeError):
        m.tap('final_raw.0.dw5')


# ------------------------------------------------------------------ 16-bit storage
def _check16(m, arch, sd, x, storage, outs, launch_names, chunk=4):
    """check_bf16's protocol against the plain-head emulation (flip=0): a launch that stores its own op <= 1 ulp on all
    but 1e-4 of the elements, <= 2 everywhere, < 2 % differing; heads within HEAD_ATOL; the output of a fused block
    launch, its inner tensors chained through the emulation, <= 1.5 ulp of the tensor's largest value with mean |d| <=
    0.35 ulp of its mean magnitude.  Returns the number of ops compared."""
    U = ULP_REL[storage]
    rnd = _rnd(storage)
    plan = snr.plan(sd, arch, rnd=rnd)
    mags = {n: fn for n, _, fn in snr.plan(sd, arch, rnd=rnd, absolute=True)}
    fused = fused_inner(launch_names)
    inner = {t for v in fused.values() for t in v}
    NB = x.shape[0]
    dev_full, k_out = {}, 0
    for name, _, _ in plan:
        if name in inner:
            continue
        if snr.is_head(name):
            dev_full[name] = outs[k_out]
            k_out += 1
        else:
            dev_full[name] = m.tap(name)
    bad, seen = [], 0
    for c0 in range(0, NB, chunk):
        c1 = min(NB, c0 + chunk)
        dev = {'x': x[c0:c1]}
        with torch.no_grad():
            for name, ins, fn in plan:
                exp = fn(*[dev[k] for k in ins])
                if name in inner:
                    dev[name] = exp
                    continue
                got = dev_full[name].view((NB,) + tuple(exp.shape[1:]))[c0:c1].cpu()
                dev[name] = got
                d = (got - exp).abs()
                seen += 1
                if name in fused:
                    cap = 1.5 * U * float(exp.abs().max())
                    mean_rel = float(d.mean()) / (U * float(exp.abs().mean()) + 1e-12)
                    if float(d.max()) > cap or mean_rel > 0.35:
                        bad.append((name, c0, float(d.max()), cap, mean_rel))
                elif snr.is_head(name):
                    if float(d.max()) > HEAD_ATOL:
                        bad.append((name, c0, float(d.max())))
                else:
                    r = d / _unit(storage, exp, mags[name](*[dev[k] for k in ins]))
                    ulps, over1, frac = float(r.max()), float((r > 1.0).float().mean()), float((d > 0).float().mean())
                    if ulps > 2.0 or over1 > 1e-4 or frac > 0.02:
                        bad.append((name, c0, float(d.max()), ulps, over1, frac))
    assert not bad, bad[:8]
    return seen


@pytest.mark.parametrize('storage', ['bf16', 'f16'])
def test_16bit_every_launch_vs_emulation(storage):
    """One launch per op ("mbtb" = "stem" = "headb" = 0): every launch against the emulation on the device's inputs."""
    m, arch, sd = _model('search-XS', storage)
    x = synth.make_images(2, 128, seed=5)
    opts = {'mbtb': 0, 'stem': 0, 'headb': 0}
    old = {k: m.set_option(k, v) for k, v in opts.items()}
    try:
        outs, prof = profiled_forward(m, x.cuda(), 0)
    finally:
        for k, v in old.items():
            m.set_option(k, v)
    names = [a for a, _ in prof]
    assert not fused_inner(names), names
    n = _check16(m, arch, sd, x, storage, outs, names)
    assert n == len(snr.plan(sd, arch))


@pytest.mark.parametrize('storage', ['bf16', 'f16'])
def test_16bit_default_forward_vs_chained_emulation(storage):
    """The default forms (fused blocks and stem; the head unfused, its one-source fused form is bitwise below)."""
    m, arch, sd = _model('search-XS', storage)
    x = synth.make_images(2, 256, seed=6)
    outs, prof = _with_option(m, 'headb', 0, lambda: profiled_forward(m, x.cuda(), 0))
    names = [a for a, _ in prof]
    assert fused_inner(names), names                      # the fused forms really ran
    _check16(m, arch, sd, x, storage, outs, names)


# ------------------------------------------------------------------ the one-source head and deconv forms
def _deconv_bytes(storage, NB, taps, d, i):
    """The profile's algorithmic bytes of deconv.i with ONE source (a dual-source launch counts Ca + Cb input planes)."""
    src = taps['deconv.%d' % (i - 1)] if i else taps['stage.%d.%d' % (len(d['stages']) - 1, len(d['stages'][-1]) - 1)]
    ih, iw = src.shape[2], src.shape[3]
    e = 4 if storage == 'f32' else 2
    return e * NB * (d['deconv'][i]['refined_in'] * ih * iw + d['deconv'][i]['out'] * 4 * ih * iw)


@pytest.mark.parametrize('storage', ['f32', 'bf16', 'f16'])
def test_one_source_head_bitwise_vs_unfused_chain(storage):
    """Default forward: each output head in ONE launch under the existing tag (headfuse_kernel / headb_kernel), every
    deconv a one-source launch; its outputs bitwise equal to the unfused chain (option headfuse = 0 / headb = 0), plain
    and mirrored."""
    m, arch, sd = _model('search-XS', storage)
    d = spec.derive(arch)
    x = synth.make_images(2, 256, seed=8).cuda()
    key, tag = ('headfuse', 'headfuse_kernel') if storage == 'f32' else ('headb', 'headb_kernel')
    m.set_profiling(True)
    try:
        fused = [o.clone() for o in m.forward_native(x, 2)]
        torch.cuda.synchronize()
        prof_full = m.profile()
    finally:
        m.set_profiling(False)
    prof1 = [tuple(n.rsplit('|', 1)) for n, _, _, _ in prof_full]
    chain, prof0 = _with_option(m, key, 0, lambda: profiled_forward(m, x, 2))
    heads1 = [(a, b) for a, b in prof1 if a.startswith('final')]
    assert heads1 == [('final.0.dw5+pw', tag), ('final.1.dw5+pw', tag)], prof1[-8:]
    prof0 = [tuple(p) for p in prof0]
    assert [a for a, _ in prof0 if a.startswith('final')] == ['final_refined.0.dw5', 'final.0.pw',
                                                              'final_refined.1.dw5', 'final.1.pw'], prof0[-8:]
    assert not any('raw' in a or 'dw5+dw5' in a for a, _ in prof1 + prof0)
    with torch.no_grad():
        taps = {}
        snr.forward(torch.zeros(1, 3, 256, 256), sd, arch, taps=taps)
    dec = [(n.rsplit('|', 1)[0], by) for n, _, by, _ in prof_full if n.startswith('deconv.')]
    assert [n for n, _ in dec] == ['deconv.0', 'deconv.1', 'deconv.2'], dec
    for i, (_, by) in enumerate(dec):
        assert by == _deconv_bytes(storage, 4, taps, d, i), (i, by)
    for a, b in zip(fused, chain):
        assert torch.equal(a, b)
    # the fp32 result also holds against the oracle
    if storage == 'f32':
        with torch.no_grad():
            ref = snr.forward(x.cpu(), sd, arch)
            ref_f = snr.forward(torch.flip(x.cpu(), [3]), sd, arch)
        for k in range(2):
            assert float((fused[k][:2].cpu() - ref[k]).abs().max()) <= NET_ATOL
            assert float((fused[k][2:].cpu() - ref_f[k]).abs().max()) <= NET_ATOL


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
def test_batched_and_flip_bitwise(storage):
    m, arch, sd = _model('search-XS', storage)
    x = synth.make_images(3, 256, seed=9).cuda()
    both = [o.clone() for o in m.forward_native(x, 2)]
    plain = [o.clone() for o in m.forward_native(x, 0)]
    flipped = [o.clone() for o in m.forward_native(torch.flip(x, [3]).contiguous(), 0)]
    only_f = [o.clone() for o in m.forward_native(x, 1)]
    for k in range(2):
        assert torch.equal(both[k][:3], plain[k])
        assert torch.equal(both[k][3:], flipped[k])
        assert torch.equal(only_f[k], flipped[k])
        for n in range(3):
            one = m.forward_native(x[n:n + 1].contiguous(), 0)[k]
            assert torch.equal(one[0], plain[k][n]), (k, n)


# ------------------------------------------------------------------ the engine
def _simplenet_cfg(arch):
    from litepose_amd import config

    class Args(object):
        cfg = YAML
        opts = []
    return config.apply_arch(config.update_config(config.get_cfg('crowd_pose'), Args()), arch)


def test_engine_simplenet_yaml_device_maps_vs_oracle_parser():
    from litepose_amd import arch_zoo, engine
    from litepose_amd.models import pose_simplenet
    arch = arch_zoo.get('search-XS')
    cfg = _simplenet_cfg(arch)
    assert cfg.MODEL.NAME == 'pose_simplenet'
    sd = snr.make_state_dict(arch, seed=1234)
    eng = engine.PoseEngine(cfg, arch, sd)
    assert isinstance(eng.model, pose_simplenet.LitePose)
    N, R = 4, 256
    x = synth.make_images(N, R, seed=21).cuda()
    off0, off1 = synth.lowres_offsets(33, N, 14, R, people=[3, 0, 7, 12])
    f0, f1 = synth.flip_offsets(off0, off1, inference_ref.FLIP_CONFIG['CROWDPOSE'])
    offs = (torch.from_numpy(np.concatenate([off0, f0])).cuda(), torch.from_numpy(np.concatenate([off1, f1])).cuda())
    ans, count, scores = eng.infer_batch(x, offsets=offs)
    det, tag = [t.cpu().numpy() for t in eng.last_maps()]
    ans, count, scores = ans.cpu().numpy(), count.cpu().numpy(), scores.cpu().numpy()
    ora = group_ref.HeatmapParser(group_ref.Params())
    total = 0
    for n in range(N):
        a, s = ora.parse_image(det[n], tag[n])
        assert count[n] == a.shape[0], (n, count[n], a.shape)
        assert np.array_equal(ans[n, :count[n]], a)
        assert np.array_equal(scores[n, :count[n]], s)
        total += a.shape[0]
    assert total >= 10
    with torch.no_grad():
        outs = snr.forward(x.cpu(), sd, arch)
        outs_f = snr.forward(torch.flip(x.cpu(), [3]), sd, arch)
        outs = [outs[0] + torch.from_numpy(off0), outs[1] + torch.from_numpy(off1)]
        outs_f = [outs_f[0] + torch.from_numpy(f0), outs_f[1] + torch.from_numpy(f1)]
        fh, tg = inference_ref.merge(outs, outs_f, inference_ref.TestCfg(), (R, R))
    assert float(np.abs(det - fh.numpy()).max()) < NET_ATOL
    assert float(np.abs(tag - tg.numpy()).max()) < NET_ATOL


def test_evaluate_simplenet_equals_the_batch1_loop():
    """PoseEngine.evaluate on 27 mixed-size images == the reference-shaped batch-1 loop (valid.py:195-233) on the
    drop-in pose_simplenet model, record for record."""
    from litepose_amd import arch_zoo, engine, results
    import litepose_amd.models as models
    from test_gpu_eval_batched import SAME_BUCKET, _batch1_loop, _images
    arch = arch_zoo.get('search-XS')
    cfg = _simplenet_cfg(arch)
    sd = snr.make_state_dict(arch, seed=1234, head_gain=6.0)       # noise peaks above the threshold
    model = eval('models.' + cfg.MODEL.NAME + '.get_pose_net')(cfg, is_train=False, cfg_arch=arch)
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    model.eval()
    eng = engine.PoseEngine(cfg, arch, sd)
    shapes = SAME_BUCKET * 4 + [(640, 427)] * 4 + [(612, 612)] * 3 + [(200, 600)] * 2 + [(360, 640)] * 2
    rng = np.random.default_rng(23)
    shapes = [shapes[i] for i in rng.permutation(len(shapes))]
    assert len(shapes) >= 24
    images = _images(shapes, 24)
    ids = [500 + 7 * i for i in range(len(images))]
    got = eng.evaluate(images, image_ids=ids, batch_size=4)
    all_preds, all_scores, _ = _batch1_loop(cfg, model, images)
    ref = results.preds_to_results(all_preds, all_scores, ids)
    assert sum(len(p) for p in all_preds) > 0, 'no persons: vacuous'
    assert got == ref
