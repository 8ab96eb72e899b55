"""BatchNorm calibration of supernet sub-networks on the device (lp_calib_*, csrc/calib_kernels.hip) against the real
reference (tests/golden/golden_supernet.npz) and the float64 restatement (tests/_supernet_ref.py).

Tolerance of a running pair.  The yardstick of a layer is the reference's OWN distance from the float64 restatement for
that layer, step and architecture, stored in the golden (``dist``), and never less than one float32 spacing of the
layer's largest value (2^-23 * max|pair|: the pair is stored in float32, and where the reference happens to round every
channel of a small layer like float64 its distance is 0).  The test counts how many (layer, step, pair) comparisons
were judged against the floor and reports the worst ratio of the others separately (FLOOR_SPLIT below).  The device may be MARGIN times that far from
float64: its input to a layer carries the rounding of the convolutions before it, which sum in another order than the
reference's (bf16x3 matrix-core 1x1s, packed depthwise rows).  Every layer, every channel, every step of all three
architectures in fixture order is held to it; the sampled channels of the golden are compared directly as well
(|device - reference| <= (MARGIN + 1) yardsticks, by the triangle inequality).
Measured on an MI355X (worst ratio device distance / yardstick over all layers, channels and steps): see MEASURED below --
at most 2.38; MARGIN = 4, the next power of two, leaves room for another box or compiler summing in another order.

Tolerance of the eval outputs after calibration: the project's network tolerance 2e-5 * max(1, |out|_inf) plus the
statistic tolerance propagated: the oracle network is run twice on the reference's calibrated state dict, as it is and
with every running mean and variance moved by its layer's tolerance above, all in one direction (the coherent shift is
the first-order worst case of a sum); the largest output difference of the two runs is added.  The eval outputs
BEFORE a calibration are held to the golden's samples too: for the first architecture at the network tolerance alone, for
the later ones (they start from statistics the device moved) plus the largest propagated tolerance of the calibrations
before them.  The whole-layer sums of the golden bound the channels its samples leave out: |sum over all channels of
(device - reference)| <= C * (MARGIN + 1) yardsticks.
"""
import os

import numpy as np
import pytest
import torch

import _supernet_ref as sr
from conftest import ROOT
from oracle import group_ref, inference_ref, net_ref, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_supernet.npz')
MARGIN = 4.0
# worst device-distance / yardstick ratio per (size, architecture), running mean and variance, MI355X:
MEASURED = {'64x64_half': (2.38, 2.25), '64x64_full': (2.25, 1.95), '64x64_mixed': (2.02, 1.80),
            '96x160_half': (2.16, 1.81), '96x160_full': (1.63, 1.64), '96x160_mixed': (1.63, 1.86)}
# eval outputs after calibration and the floor split, at MARGIN = 4: see RECORDED below
NET_RTOL = 2e-5


def _cfg():
    from litepose_amd import config
    return config.get_cfg('crowd_pose')


def _super():
    from litepose_amd.models import pose_supermobilenet as psm
    m = psm.get_pose_net(_cfg())
    m.load_state_dict(sr.make_state_dict(sr.SEED), strict=True)
    return m


def _device_net(arch, sd):
    import litepose_amd.models as models
    net = models.pose_mobilenet.get_pose_net(_cfg(), cfg_arch=arch, storage='f32')
    net.load_state_dict(sd, strict=True)
    return net


def _calibrate(m, arch, H, W, ai, steps_out=None):
    layers = sr.bn_layers(arch)

    def on_step(i, cal):
        if steps_out is not None:
            got = {}
            for p, c in layers:
                mean, var = cal.read(p, c, 'cuda')
                got[p] = (mean.cpu().double().numpy(), var.cpu().double().numpy())
            steps_out.append(got)
    batches = [sr.step_images(H, W, ai, s).cuda() for s in range(sr.STEPS)]
    return m.calibrate(arch, batches, momentum=0.1, on_step=on_step)


@pytest.mark.parametrize('hw', sr.CASES, ids=['%dx%d' % c for c in sr.CASES])
def test_running_pairs_and_eval_outputs_vs_reference(hw):
    """Items 1 and 2 (see the module docstring), three architectures in fixture order on one supernet."""
    golden = np.load(GOLDEN)
    H, W = hw
    m = _super()
    sd32 = sr.make_state_dict(sr.SEED)
    sd64 = sr.to_double(sr.make_state_dict(sr.SEED))
    xe = synth.make_images(2, H, seed=11, w=W)
    worst_all = {}
    prop_before = 0.0          # largest propagated statistic tolerance of the calibrations so far
    split = [0, 0]             # comparisons judged against the golden's dist / against the float32 floor
    for ai, (name, arch) in enumerate(sr.golden_archs()):
        tag = '%dx%d_%s' % (H, W, name)
        layers = sr.bn_layers(arch)
        sub32, sub64 = sr.sub_state_dict(sd32, arch), sr.sub_state_dict(sd64, arch)
        # pre-calibration eval outputs of the device network on the slices the supernet holds NOW
        pre = _device_net(arch, m.sub_state_dict(arch)).forward_native(xe.cuda())
        for k, t in enumerate(pre):
            ref = golden['%s_pre%d_sample' % (tag, k)]
            assert tuple(t.shape) == tuple(golden['%s_pre%d_shape' % (tag, k)])
            got = t.cpu().numpy().reshape(-1)[::13]
            bound = NET_RTOL * max(1.0, float(np.abs(ref).max())) + prop_before
            err = float(np.abs(got - ref).max())
            print('%s pre out%d |dev-ref| %.3g bound %.3g' % (tag, k, err, bound))
            assert err <= bound, (tag, k, err, bound)
        dev_steps = []
        out_sd = _calibrate(m, arch, H, W, ai, dev_steps)
        assert len(dev_steps) == sr.STEPS
        tol = {}
        worst = [0.0, 0.0]
        worst_real = 0.0       # worst ratio among the comparisons whose yardstick is the reference's own distance
        failures = []
        for step in range(sr.STEPS):
            x = sr.step_images(H, W, ai, step)
            with torch.no_grad():
                sr.train_forward(x, sub32, arch)
                sr.train_forward(x.double(), sub64, arch)
            p64 = sr.pairs_of(sub64, arch)
            gp = golden[tag + '_pairs'][step].astype(np.float64)
            gd = golden[tag + '_dist'][step]
            gs = golden[tag + '_sums'][step]
            off = 0
            for li, (p, c) in enumerate(layers):
                idx = sr.sample_index(c)
                for q in range(2):
                    floor = 2.0 ** -23 * float(np.abs(p64[p][q]).max())
                    yard = max(float(gd[q][li]), floor)
                    d64 = float(np.abs(dev_steps[step][p][q] - p64[p][q]).max())
                    dref = float(np.abs(dev_steps[step][p][q][idx] - gp[q][off:off + len(idx)]).max())
                    dsum = abs(float(dev_steps[step][p][q].sum()) - float(gs[q][li]))
                    worst[q] = max(worst[q], d64 / yard)
                    split[0 if float(gd[q][li]) >= floor else 1] += 1
                    if float(gd[q][li]) >= floor:
                        worst_real = max(worst_real, d64 / yard)
                    tol[(p, q)] = MARGIN * yard
                    if not (d64 <= MARGIN * yard and dref <= (MARGIN + 1.0) * yard and dsum <= c * (MARGIN + 1.0) * yard):
                        failures.append((step, p, 'mean var'.split()[q], d64, dref, dsum, yard))
                off += len(idx)
        print('%s worst device-distance / yardstick: mean %.2f var %.2f; among those judged by the reference distance %.2f'
              % (tag, worst[0], worst[1], worst_real))
        worst_all[tag] = worst
        assert not failures, (tag, len(failures), failures[:6])
        # num_batches_tracked as the reference leaves it
        nbt = [int(out_sd[p + '.num_batches_tracked']) for p, _ in layers]
        assert nbt == [int(v) for v in golden[tag + '_nbt']]
        # ---- item 2: eval outputs of the calibrated handle vs the oracle on the reference's calibrated state dict
        with torch.no_grad():
            ora = net_ref.forward(xe, sub32, arch)
            moved = {k: v.clone() for k, v in sub32.items()}
            for p, c in layers:
                moved[p + '.running_mean'] += tol[(p, 0)]
                moved[p + '.running_var'] += tol[(p, 1)]
            ora_moved = net_ref.forward(xe, moved, arch)
        dev = m.calibrated_net.forward_native(xe.cuda())
        post_prop = 0.0
        for k in range(2):
            # the restatement's calibrated dict IS the reference's (pinned bit for bit at one thread by the generator)
            np.testing.assert_allclose(ora[k].numpy().reshape(-1)[::13], golden['%s_post%d_sample' % (tag, k)],
                                       rtol=0, atol=1e-6)
            prop = float((ora[k] - ora_moved[k]).abs().max())
            bound = NET_RTOL * max(1.0, float(ora[k].abs().max())) + prop
            err = float((dev[k].cpu() - ora[k]).abs().max())
            print('%s post out%d |dev-oracle| %.3g bound %.3g (propagated %.3g)' % (tag, k, err, bound, prop))
            assert err <= bound, (tag, k, err, bound)
            post_prop = max(post_prop, prop)
        prop_before = max(prop_before, post_prop)
        # the supernet's own tensors received the moved prefixes (view semantics)
        full = m.state_dict()
        for p, c in layers:
            assert torch.equal(full[p + '.running_mean'][:c], out_sd[p + '.running_mean'])
            assert torch.equal(full[p + '.running_var'][:c], out_sd[p + '.running_var'])
    print('MEASURED', worst_all)
    print('FLOOR_SPLIT %dx%d: %d comparisons judged by the reference distance, %d by the float32 floor' % (H, W, split[0], split[1]))


def test_two_calibrations_from_the_same_start_are_bitwise_equal():
    H, W = sr.CASES[1]
    outs = []
    for _ in range(2):
        m = _super()
        a = _calibrate(m, sr.golden_archs()[0][1], H, W, 0)
        b = _calibrate(m, sr.golden_archs()[2][1], H, W, 2)
        outs.append((a, b, m.state_dict()))
    for x, y in zip(outs[0], outs[1]):
        assert list(x) == list(y)
        for k in x:
            assert torch.equal(x[k], y[k]), k
    # and calibration moved something
    fresh = sr.make_state_dict(sr.SEED)
    assert not torch.equal(outs[0][2]['stage.1.2.inv.1.running_var'], fresh['stage.1.2.inv.1.running_var'])


def test_hand_over_a_fresh_pose_mobilenet_gives_the_calibrated_handles_outputs():
    H, W = sr.CASES[1]
    name, arch = sr.golden_archs()[2]
    m = _super()
    out_sd = _calibrate(m, arch, H, W, 2)
    x = synth.make_images(3, H, seed=5, w=W).cuda()
    a = m.calibrated_net.forward_native(x, 2)
    b = _device_net(arch, out_sd).forward_native(x, 2)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # and differs from the uncalibrated sub-network
    c = _device_net(arch, _super().sub_state_dict(arch)).forward_native(x, 2)
    assert not torch.equal(a[1], c[1])


def test_engine_on_the_calibrated_state_dict_records_vs_oracle_parser():
    """PoseEngine on calibrate()'s state dict and cfg_arch: records bit-exact with the reference-shaped parser on the same
    device maps, maps within the network tolerance of the oracle network on that state dict."""
    from litepose_amd import config, engine
    from litepose_amd.models import pose_mobilenet
    name, arch = sr.golden_archs()[0]
    m = _super()
    N, R = 4, 256
    g = torch.Generator().manual_seed(3)
    out_sd = m.calibrate(arch, [torch.randn(8, 3, R, R, generator=g).cuda() for _ in range(2)])
    cfg = config.apply_arch(_cfg(), arch)
    eng = engine.PoseEngine(cfg, arch, out_sd)
    assert type(eng.model) is pose_mobilenet.LitePose
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
        outs = net_ref.forward(x.cpu(), out_sd, arch)
        outs_f = net_ref.forward(torch.flip(x.cpu(), [3]), out_sd, arch)
        outs = [outs[0] + torch.from_numpy(off0), outs[1] + torch.from_numpy(off1)]
        outs_f = [outs_f[0] + torch.from_numpy(f0), outs_f[1] + torch.from_numpy(f1)]
        fh, tg = inference_ref.merge(outs, outs_f, inference_ref.TestCfg(), (R, R))
    assert float(np.abs(det - fh.numpy()).max()) < NET_RTOL * max(1.0, float(fh.abs().max()))
    assert float(np.abs(tag - tg.numpy()).max()) < NET_RTOL * max(1.0, float(tg.abs().max()))
