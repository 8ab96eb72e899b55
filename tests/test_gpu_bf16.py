"""bf16-storage network path (SURVEY.md section 8 row g, BASELINE configs 4/5; the reference's reduced-precision
switch is valid.py:152-153 -> lib/fp16_utils/fp16util.py:87-91).  Needs a real MI355X.

Parity protocol for this path:
  (i)   every kernel launch against oracle.net_ref.bf16_plan fed the DEVICE's own inputs of that launch: the
        only difference left is the fp32 summation order inside ONE layer, which can flip a bf16 rounding --
        asserted: every element within one bf16 ulp (2^-7 relative) of the emulation, < 2 % of the elements
        differing at all; the two fp32 head outputs within 2e-5;
  (ii)  network outputs against the fp32 oracle with an explicit BUDGET (reported; 40 layers of bf16 rounding:
        ~2-3 % of the output range) -- never index identity end to end;
  (iii) batched == per-image and flip=2 == flip=0 + flip=1, bitwise;
  (iv)  the AE stage on the device's own merged maps stays bit-exact against the reference-semantics parser.
"""
import numpy as np
import pytest
import torch

from _net_check import BF16_ULP_REL, HEAD_ATOL, _model, _with_option, layerwise_report
from oracle import group_ref, inference_ref, net_ref, synth

pytestmark = pytest.mark.gpu

BUDGET_FRAC = 0.05           # of max|fp32 output| (hard cap); measured 0.015-0.025; per case additionally <= 2x the
                             # CPU emulation's own distance from fp32 (test_bf16_outputs_vs_fp32_oracle_within_budget)


@pytest.mark.parametrize('arch_name,R,N', [
    ('search-XS', 128, 3),      # 64/32/16/8/8 planes, odd batch, ragged 8x8 planes
    ('search-XS', 256, 2),      # headline shape
    ('search-S', 448, 2),       # BASELINE config 4: 224/112/56/28 planes (28, 56 are not multiples of 16)
    ('search-M', 256, 2),       # 144-wide expansions (4.5 channel blocks), 64/40-filter deconvs (two blocks)
    ('search-L', 128, 1),       # 24-channel stem output, 160-channel trunk
])
def test_bf16_every_launch_vs_emulation_on_device_inputs(arch_name, R, N):
    m, arch, sd = _model(arch_name)
    x = synth.make_images(N, R, seed=41)
    rows = layerwise_report(m, arch, sd, x)
    bad = []
    for name, dmax, ulps, frac, head in rows:
        if head:
            if dmax > HEAD_ATOL:
                bad.append((name, dmax))
        elif ulps > 1.0 or frac > 0.02:
            bad.append((name, dmax, ulps, frac))
    worst = max(rows, key=lambda r: r[2] if not r[4] else 0)
    print('%s@%d: %d launches, worst %s: %.3g abs = %.2f bf16 ulp, %.4f of elements differ'
          % (arch_name, R, len(rows), worst[0], worst[1], worst[2], worst[3]))
    assert not bad, bad[:8]


@pytest.mark.parametrize('arch_name,R,N', [('search-XS', 256, 2), ('search-S', 448, 2), ('search-M', 512, 1)])
def test_bf16_outputs_vs_fp32_oracle_within_budget(arch_name, R, N):
    m, arch, sd = _model(arch_name)
    x = synth.make_images(N, R, seed=43)
    outs = [o.cpu() for o in m.forward_native(x.cuda(), 2)]
    with torch.no_grad():
        ref = net_ref.forward(x, sd, arch)
        ref_f = net_ref.forward(torch.flip(x, [3]), sd, arch)
        emu = net_ref.forward_bf16(x, sd, arch)
    for k in range(2):
        full = torch.cat([ref[k], ref_f[k]])
        scale = float(full.abs().max())
        err = float((outs[k] - full).abs().max())
        rms = float((outs[k] - full).pow(2).mean().sqrt())
        emu_err = float((emu[k] - ref[k]).abs().max())
        print('%s@%d out%d: |ref|max %.3f  device-vs-fp32 max %.2e rms %.2e  (CPU emulation-vs-fp32 max %.2e)'
              % (arch_name, R, k, scale, err, rms, emu_err))
        assert err <= BUDGET_FRAC * scale, (k, err, scale)
        assert rms <= 0.01 * scale
        # the yardstick is the emulation's own distance from fp32 (same roundings, other summation order): the
        # device may not be further away than twice that on the plain pass
        err_plain = float((outs[k][:N] - ref[k]).abs().max())
        assert err_plain <= 2.0 * emu_err + 1e-3 * scale, (k, err_plain, emu_err)


def test_bf16_batched_equals_per_image_and_flip_modes_bitwise():
    m, arch, sd = _model('search-S')
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
    # mirror-on-read == the network on the flipped image
    fl = m.forward_native(torch.flip(x, [3]).contiguous(), 0)
    for k in range(2):
        assert torch.equal(fl[k], mirr[k])


@pytest.mark.parametrize('arch_name,N,R', [('search-XS', 6, 256), ('search-S', 4, 448)])
def test_bf16_engine_end_to_end_records_bit_exact_on_device_maps(arch_name, N, R):
    """bf16 storage through the whole engine (network, merge, AE stage), XS@256 and BASELINE config 4's S@448: the
    merged heatmaps within the stated budget of the fp32 CPU pipeline, the records BIT-EXACT against the
    reference-semantics parser fed the device's own maps."""
    from litepose_amd import arch_zoo, config, engine
    arch = arch_zoo.get(arch_name)
    cfg = config.apply_arch(config.get_cfg(), arch)
    sd = synth.make_state_dict(arch, seed=1234, head_gain=0.25)
    eng = engine.PoseEngine(cfg, arch, sd, storage='bf16')
    assert eng.model.storage == 'bf16'
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
    print('bf16 engine: merged heatmap error vs the fp32 CPU pipeline %.2e (budget 3e-2)' % err)
    assert err < 3e-2
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


def test_storage_switch_refinalizes_and_f32_is_unchanged():
    """One handle, both storages: bf16 -> f32 -> the fp32 result equals a net that was never bf16."""
    from litepose_amd import _native as nv
    m, arch, sd = _model('search-XS', storage='bf16')
    x = synth.make_images(2, 128, seed=3).cuda()
    ob = [o.clone() for o in m(x)]
    m.storage = 'f32'
    m.load_state_dict(sd, strict=True)
    assert nv.lib().lp_net_get_storage(m._h) == 0
    of = [o.clone() for o in m(x)]
    m2, _, _ = _model('search-XS', storage='f32')
    o2 = m2(x)
    for k in range(2):
        assert torch.equal(of[k], o2[k])
        assert not torch.equal(ob[k], of[k])
        assert float((ob[k] - of[k]).abs().max()) < 0.06 * float(of[k].abs().max())


# ------------------------------------------------------------------ the matrix-core depthwise kernels
@pytest.mark.parametrize('dwt', [0, 2])
@pytest.mark.parametrize('arch_name,R,N', [('search-XS', 128, 3), ('search-XS', 256, 2), ('search-S', 448, 2),
                                           ('search-M', 256, 2), ('search-M', 512, 1), ('search-L', 128, 1)])
def test_dwt_and_dwb_every_launch_vs_emulation(arch_name, R, N, dwt):
    """The two forms of the bf16 stride-1 depthwise -- option "dwt" = 2 (default since round 3): every 7x7 / 5x5 plane the
    shape rule admits runs as banded matrix products on the matrix cores (dwt_kernel); "dwt" = 0: dwb_kernel's packed
    FMAs everywhere -- both against the same criteria: every launch within 1 bf16 ulp of the emulation on the
    device's own inputs, M@512 (BASELINE config 5's shape) included."""
    m, arch, sd = _model(arch_name)
    x = synth.make_images(N, R, seed=41)
    m.set_profiling(True)
    rows = _with_option(m, 'dwt', dwt, lambda: layerwise_report(m, arch, sd, x))
    ran = [n for n, _, _, _ in m.profile() if 'dwt_kernel' in n]
    m.set_profiling(False)
    bad = [(n, d, u, f) for n, d, u, f, head in rows if (d > HEAD_ATOL if head else (u > 1.0 or f > 0.02))]
    print('%s@%d: %d launches on dwt_kernel' % (arch_name, R, len(ran)))
    assert not bad, bad[:8]
    assert (dwt == 0) == (not ran) or R < 96, 'dwt_kernel launches: %d with option dwt = %d' % (len(ran), dwt)


@pytest.mark.parametrize('arch_name,R,N', [
    ('search-XS', 256, 2), ('search-S', 448, 2), ('search-M', 256, 2),
    ('search-M', 512, 1), ('search-L', 128, 1), ('search-XS', 128, 3)])
def test_fused_bf16_block_vs_chained_emulation(arch_name, R, N):
    """The fused bf16 block kernels (option "mbtb", default on since round 3) against the emulation CHAINED through
    the tensors they never store: mbtb_kernel / mbtb_s2_kernel, the whole 7x7 InvBottleneck (stride 1 / 2) in one
    launch (expand, depthwise and project; both expanded tensors stay on the CU) -- every block of XS / S / M and all
    but the 160-channel ones of L (that variant would spill and is not built).
    A 1-ulp flip of one inner bf16 value (other summation order than the emulation's) reaches the block output
    through the following weights, so the per-element ulp count is not the yardstick where the output cancels.
    Required of a fused block's output:
      (i)   every difference <= 1.5 bf16 ulp OF THE TENSOR'S LARGEST VALUE;
      (ii)  mean |difference| <= 0.35 bf16 ulp of the tensor's MEAN magnitude (one inner tensor: measured 0.01-0.05;
            two inner tensors: see the printed numbers);
      (iii) one inner tensor only: <= 2 own-ulp on all but 1e-3 of the elements, < 5 % of the elements differing.
    Every other launch keeps the per-launch criterion (<= 1 bf16 ulp, < 2 % differing)."""
    m, arch, sd = _model(arch_name)
    x = synth.make_images(N, R, seed=41)

    def run():
        m.set_profiling(True)
        outs = [o.cpu() for o in m.forward_native(x.cuda(), 0)]
        torch.cuda.synchronize()
        prof = [n for n, _, _, _ in m.profile()]
        m.set_profiling(False)
        return outs, prof
    hook = 'mbtb'
    # the heads one launch per op here ("headb" = 0: the fused head is bit-identical to them and has its own test)
    outs, prof = _with_option(m, 'headb', 0, lambda: _with_option(m, 'mbtb', 1, run))
    fused = [n.split('|')[0] for n in prof if '+point_conv' in n]
    assert fused, 'mbtb_kernel took no launch'
    # round 6: the residual blocks with up to 32 channels run as mbtd_kernel (bf16 expanded tile, v_dot2 depthwise, two
    # workgroups per CU) -- stages 1-2 of every published architecture; they are held to the same yardstick below
    took_d = [n.split('|')[0] for n in prof if n.endswith('|mbtd_kernel')]
    assert len(took_d) >= 5, ('mbtd_kernel took %d launches' % len(took_d), prof[:12])
    n_blocks = sum(st['num_blocks'] for st in arch['backbone_setting'])
    if arch_name != 'search-L':
        assert len(fused) == n_blocks, 'mbtb / mbtb_s2 ran %d of the %d blocks' % (len(fused), n_blocks)
    inner = set()
    for n in fused:                                   # "stage.s.b.depth_conv+point_conv" or "stage.s.b.inv+dw+point_conv"
        pfx = n.split('.inv')[0].split('.depth_conv')[0]
        inner.add(pfx + '.depth_conv')
        if '.inv+' in n:
            inner.add(pfx + '.inv')
    whole = {f.split('.inv')[0] + '.point_conv' for f in fused if '.inv+' in f}
    # round 6: the stem in one launch (conv3x3 s2 + dw3 + 1x1): its two inner tensors are never stored either; 'stem.pw' is
    # then a fused output with two inner tensors, held to the same yardstick as a whole block
    stem_fused = any(n.startswith('stem.conv3x3s2+dw3+pw') for n in prof)
    assert stem_fused, 'the fused bf16 stem took no launch'
    inner |= {'stem.conv3x3s2', 'stem.dw3'}
    whole.add('stem.pw')
    dev, bad, k_out, worst = {'x': x}, [], 0, (0.0, 0.0, '')
    with torch.no_grad():
        for name, ins, fn in net_ref.bf16_plan(sd, arch):
            exp = fn(*[dev[k] for k in ins])
            head = name.startswith('final.') and name.endswith('.pw')
            if name in inner:
                dev[name] = exp                       # never stored on the device: chain the emulation
                continue
            got = outs[k_out] if head else m.tap(name).cpu().view(exp.shape)
            k_out += 1 if head else 0
            dev[name] = got
            d = (got - exp).abs()
            ulps = float((d / (exp.abs() * BF16_ULP_REL + 1e-6)).max())
            frac = float((d > 0).float().mean())
            fused_out = name == 'stem.pw' or any(name == f.split('.inv')[0].split('.depth_conv')[0] + '.point_conv' for f in fused)
            if head:
                if float(d.max()) > HEAD_ATOL:
                    bad.append((name, float(d.max())))
            elif fused_out:
                cap = 1.5 * BF16_ULP_REL * float(exp.abs().max())
                mean_rel = float(d.mean()) / (BF16_ULP_REL * float(exp.abs().mean()) + 1e-12)
                worst = max(worst, (mean_rel, float(d.max()) / cap, name))
                if float(d.max()) > cap or mean_rel > 0.35:
                    bad.append((name, float(d.max()), cap, mean_rel))
                elif name not in whole:
                    over = float((d > 2.0 * (exp.abs() * BF16_ULP_REL + 1e-6)).float().mean())
                    if over > 1e-3 or frac > 0.05:
                        bad.append((name, float(d.max()), cap, over, frac))
            elif ulps > 1.0 or frac > 0.02:
                bad.append((name, float(d.max()), ulps, frac))
    print('%s %s@%d: %d fused launches; worst block output: mean |d| = %.3f ulp of the mean magnitude, max |d| = %.2f of '
          'the cap (%s)' % (hook, arch_name, R, len(fused), worst[0], worst[1], worst[2]))
    assert not bad, bad[:8]


@pytest.mark.parametrize('arch_name,R,N', [('search-XS', 128, 2), ('search-XS', 256, 1), ('search-S', 224, 1),
                                           ('search-M', 256, 1)])
def test_device_bf16_outputs_within_the_reference_half_modes_own_distance(arch_name, R, N):
    """Round 5: a yardstick of the bf16 path that the REFERENCE holds.  tests/golden/golden_bf16.npz
    = outputs of the real reference module in fp32 and in its own reduced-precision recipe (valid.py:152-153 ->
    fp16util.py:87-91 network_to_half, with bfloat16) on seeded inputs.  The device's bf16-storage network (default
    kernels: fused blocks) must be no further from the reference's fp32 outputs than 1.1x (rms) / 1.5x (max) the
    reference's own bf16 mode, and within 1.6x of that rms from the reference's bf16 outputs themselves
    (tests/test_bf16_cpu.py: bf16_budget_vs_reference_half_mode, which the CPU emulation passes with 0.7x)."""
    from test_bf16_cpu import bf16_budget_vs_reference_half_mode
    m, arch, sd = _model(arch_name)
    x = synth.make_images(N, R, seed=21)
    outs = [o.cpu() for o in m.forward_native(x.cuda(), 0)]
    torch.cuda.synchronize()
    rep = bf16_budget_vs_reference_half_mode(arch_name, R, outs)
    print('device bf16 vs reference (rms ratio to fp32, max ratio, rms ratio to ref-bf16):', rep)


@pytest.mark.parametrize('arch_name,H,W', [('search-S', 448, 448), ('search-XS', 96, 160), ('search-L', 128, 128),
                                           ('search-XS', 160, 96)])
def test_bf16_fused_stem_vs_unfused_chain(arch_name, H, W):
    """Round 6: the stem of the bf16-storage network in ONE launch (stem4_kernel<lp::Bf16, C0>: image -> conv3x3 s2 -> dw3x3 ->
    1x1 with the two 32-channel tensors in LDS, rounded to bf16 where stemb_kernel / dwb_kernel<3,1> / pwb_kernel store
    them; pose_mobilenet.py:36-41 under valid.py:152-153) against those three launches (option "stem" = 0) on the stem
    output: plain and mirrored pass (flip-TTA read), ragged tiles and image borders.  Same roundings, other fp32 summation
    orders inside the conv / depthwise: a flipped bf16 rounding of an inner value reaches the output through the 1x1's
    weights -- every difference <= 1.5 bf16 ulp of the tensor's largest value, < 2 % of the elements differ at all, and the
    mean difference <= 0.05 ulp of the mean magnitude (the chained-emulation test holds it to the oracle)."""
    m, arch, sd = _model(arch_name)
    x = synth.make_images(3, H, seed=41, w=W).cuda()
    res = {}
    for mode in (1, 0):
        def run():
            m.set_profiling(True)
            outs = [o.clone() for o in m.forward_native(x, 2)]
            torch.cuda.synchronize()
            kern = [n.split('|')[1] for n, _, _, _ in m.profile()]
            m.set_profiling(False)
            return outs, m.tap('first').clone(), kern
        res[mode] = _with_option(m, 'stem', mode, run)
    assert 'stem4_kernel' in res[1][2] and 'stemb_kernel' not in res[1][2]
    assert 'stem4_kernel' not in res[0][2] and 'stemb_kernel' in res[0][2]
    a, b = res[1][1], res[0][1]
    d = (a - b).abs()
    cap = 1.5 * BF16_ULP_REL * float(b.abs().max())
    frac = float((d > 0).float().mean())
    mean_rel = float(d.mean()) / (BF16_ULP_REL * float(b.abs().mean()) + 1e-12)
    print('%s %dx%d bf16 stem, fused vs chain: max |d| %.3g (cap %.3g), %.4f of the elements differ, mean |d| = %.4f ulp of the '
          'mean magnitude' % (arch_name, H, W, float(d.max()), cap, frac, mean_rel))
    assert float(d.max()) <= cap and frac < 0.02 and mean_rel <= 0.05, (float(d.max()), cap, frac, mean_rel)


@pytest.mark.parametrize('arch_name,H,W,N', [('search-S', 448, 448, 2), ('search-M', 256, 256, 3), ('search-XS', 256, 192, 2),
                                             ('search-S', 224, 224, 3)])
def test_bf16_fused_head_bitwise_vs_three_launches(arch_name, H, W, N):
    """Round 6: headb_kernel -- an output head of the bf16-storage network in ONE launch (both 5x5 depthwise convs as
    dwt_kernel<5>'s banded MFMAs, their records handed to the dual-source 1x1's MFMAs through LDS; layers.py:120-133,
    pose_mobilenet.py:150-153 under valid.py:152-153) -- runs dwt_kernel's MFMA sequence and pwb_kernel's accumulation order:
    both network outputs must be BIT-IDENTICAL to the three launches per head (option "headb" = 0), plain and mirrored, on
    ragged regions (112 x 112, 56 x 56, 96 x 128 planes)."""
    m, arch, sd = _model(arch_name)
    x = synth.make_images(N, H, seed=47, w=W).cuda()
    res = {}
    for mode in (1, 0):
        def run():
            m.set_profiling(True)
            outs = [o.clone() for o in m.forward_native(x, 2)]
            torch.cuda.synchronize()
            kern = [n.split('|')[1] for n, _, _, _ in m.profile()]
            m.set_profiling(False)
            return outs, kern
        res[mode] = _with_option(m, 'headb', mode, run)
    assert 'headb_kernel' in res[1][1] and 'headb_kernel' not in res[0][1], (res[1][1][-8:], res[0][1][-8:])
    for a, b in zip(res[1][0], res[0][0]):
        assert torch.equal(a, b), float((a - b).abs().max())
