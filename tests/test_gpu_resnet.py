"""pose_resnet on the device (lp_arch.family = 1: LitePose built from dense FusedMBConv blocks, reference
lib/models/pose_resnet.py).  Needs a real MI355X.

  * fp32 outputs against the REAL reference module's samples (tests/golden/gen_golden_resnet.py) and against
    tests/_resnet_ref.py at NET_ATOL, plain and flip = 2, at 64x64, 96x160 and 256x256; the taps ``first``, every
    ``stage.s.b.inv``, every ``stage.s.b`` and every ``deconv.i`` against the restatement at TAP_REL;
  * batched == per-image and flip = 2 == an explicit flip, bitwise;
  * the engine on the resnet.yaml cfg: device maps against the restatement, records bit-exact against the oracle parser
    fed the device's own maps, ``evaluate`` on mixed sizes against the reference-shaped batch-1 loop, graph replay;
  * the profile of a forward names only the dense-conv family and the 1x1 kernels.
No fused block form is built (the two-launch FusedMBConv is the only one), so there is nothing to compare it with.
This file runs the ONE reference table; the tables ``lp_net_create`` accepts beyond it (other r/k/c/n/s, filters,
UpConv kernels 5 / 7, a deepest plane of 1/32) and the kernel forms only they reach are tests/test_gpu_resnet_census.py."""
import os

import numpy as np
import pytest
import torch

import _resnet_ref as rr
from _net_check import NET_ATOL, TAP_REL, profiled_forward
from conftest import ROOT
from oracle import group_ref, inference_ref, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_resnet.npz')
YAML = os.path.join(ROOT, 'tests', 'golden', 'resnet.yaml')
SIZES = [(64, 64), (96, 160), (256, 256)]


def _cfg():
    from litepose_amd import config
    return config.update_config(config.get_cfg('crowd_pose'), YAML)


def _model(seed=1234, head_gain=1.0):
    import litepose_amd.models as models
    cfg = _cfg()
    sd = rr.make_state_dict(cfg, seed=seed, head_gain=head_gain)
    m = models.pose_resnet.get_pose_net(cfg, is_train=False)
    m.load_state_dict(sd, strict=True)
    return m, cfg, sd


@pytest.mark.parametrize('hw', SIZES)
def test_fp32_vs_reference_samples_restatement_and_taps(hw):
    golden = np.load(GOLDEN)
    m, cfg, sd = _model()
    H, W = hw
    x = synth.make_images(1, H, seed=11, w=W)
    xf = torch.flip(x, [3])
    taps, taps_f = {}, {}
    with torch.no_grad():
        ref = rr.forward(x, sd, cfg, taps=taps)
        ref_f = rr.forward(xf, sd, cfg, taps=taps_f)
    # plain
    out = [o.cpu() for o in m(x.cuda())]
    for k, t in enumerate(out):
        key = '%dx%d_out%d' % (H, W, k)
        assert tuple(t.shape) == tuple(golden[key + '_shape'])
        err_g = float(np.abs(t.numpy().reshape(-1)[::13] - golden[key + '_sample']).max())
        err_r = float((t - ref[k]).abs().max())
        print('out%d %dx%d: vs golden %.3g, vs restatement %.3g' % (k, H, W, err_g, err_r))
        assert err_g <= NET_ATOL and err_r <= NET_ATOL
    worst = (0.0, '')
    for nm in rr.tap_names(cfg):
        r = taps[nm]
        got = m.tap(nm).view(r.shape).cpu()
        rel = float((got - r).abs().max()) / max(1.0, float(r.abs().max()))
        worst = max(worst, (rel, nm))
        assert rel < TAP_REL, (nm, rel)
    print('worst tap (plain) %.3g at %s' % worst)
    # flip = 2: images [0, N) plain, [N, 2N) mirrored
    both = [o.cpu() for o in m.forward_native(x.cuda(), 2)]
    for k in range(2):
        key = '%dx%d_out%d' % (H, W, k)
        assert both[k].shape[0] == 2
        assert float(np.abs(both[k][0].numpy().reshape(-1)[::13] - golden[key + '_sample']).max()) <= NET_ATOL
        assert float((both[k][:1] - ref[k]).abs().max()) <= NET_ATOL
        assert float((both[k][1:] - ref_f[k]).abs().max()) <= NET_ATOL
    for nm in rr.tap_names(cfg):
        r = torch.cat([taps[nm], taps_f[nm]])
        got = m.tap(nm).view(r.shape).cpu()
        rel = float((got - r).abs().max()) / max(1.0, float(r.abs().max()))
        assert rel < TAP_REL, (nm, rel)
    from litepose_amd import _native as nv
    with pytest.raises(nv.LitePoseNativeError):
        m.tap('stage.0.0.depth_conv')


def test_batched_and_flip_bitwise():
    m, cfg, sd = _model()
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
    # a non-square, non-256 plane as well (tiles that hang over the plane's edge)
    y = synth.make_images(2, 96, seed=10, w=160).cuda()
    both = [o.clone() for o in m.forward_native(y, 2)]
    flipped = [o.clone() for o in m.forward_native(torch.flip(y, [3]).contiguous(), 0)]
    for k in range(2):
        assert torch.equal(both[k][2:], flipped[k])
        assert torch.equal(m.forward_native(y[1:2].contiguous(), 0)[k][0], both[k][1])


def test_profile_names_only_the_dense_conv_family_and_the_1x1():
    m, cfg, sd = _model()
    d = rr.derive(cfg)
    nblocks = sum(len(b) for b in d['stages'])
    x = synth.make_images(2, 256, seed=3).cuda()
    _, prof = profiled_forward(m, x, 2)
    names = [a for a, _ in prof]
    tags = [b for _, b in prof]
    assert len(prof) == 2 + 2 * nblocks + 3 + 2, names
    assert names[:2] == ['first.0', 'first.1'] and names[-1] == 'final.1'
    assert sum(1 for t in tags if t.startswith('convk3_kernel<')) == 2 + nblocks + 3 + 2
    for (a, t) in prof:
        assert t.startswith('convk3_kernel<') or t in ('pw3_kernel', 'pw3d_kernel', 'pw2_kernel'), (a, t)
        assert not any(s in t for s in ('dw', 'deconv', 'mb', 'stem', 'headfuse')), (a, t)
        if a.endswith('.point_conv'):
            assert t.startswith('pw'), (a, t)
    assert set(tags) >= {'convk3_kernel<7,2>', 'convk3_kernel<7,1>', 'convk3_kernel<5,2>', 'convk3_kernel<5,1>',
                         'convk3_kernel<3,1>'}
    # FLOPs of the profile == the shapes' MACs (3.70 GMAC per image at 256^2), 4 images through the net
    m.set_profiling(True)
    try:
        m.forward_native(x, 2)
        torch.cuda.synchronize()
        fl = sum(f for _, _, _, f in m.profile())
    finally:
        m.set_profiling(False)
    assert fl / (2.0 * 4) == pytest.approx(3.70e9, rel=0.01)


def test_engine_resnet_yaml_device_maps_vs_oracle_parser():
    from litepose_amd import engine
    from litepose_amd.models import pose_resnet
    cfg = _cfg()
    assert cfg.MODEL.NAME == 'pose_resnet'
    sd = rr.make_state_dict(cfg, seed=1234)
    eng = engine.PoseEngine(cfg, None, sd)
    assert isinstance(eng.model, pose_resnet.LitePose)
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
        outs = rr.forward(x.cpu(), sd, cfg)
        outs_f = rr.forward(torch.flip(x.cpu(), [3]), sd, cfg)
        outs = [outs[0] + torch.from_numpy(off0), outs[1] + torch.from_numpy(off1)]
        outs_f = [outs_f[0] + torch.from_numpy(f0), outs_f[1] + torch.from_numpy(f1)]
        fh, tg = inference_ref.merge(outs, outs_f, inference_ref.TestCfg(), (R, R))
    assert float(np.abs(det - fh.numpy()).max()) < NET_ATOL
    assert float(np.abs(tag - tg.numpy()).max()) < NET_ATOL
    # the serving path replays captured graphs: same records, and replays really happen
    ref = None
    for it in range(16):                                   # 4 buffer sets: eager, capture, then replay on each
        with eng.submit(x, offsets=offs) as (a, c, s):
            torch.cuda.synchronize()
            if ref is None:
                ref = (a.clone(), c.clone(), s.clone())
            assert torch.equal(c, ref[1]) and torch.equal(a, ref[0]) and torch.equal(s, ref[2]), it
    assert np.array_equal(ref[1].cpu().numpy(), count)
    st = eng.graph_stats()
    assert st['graph_replays'] >= 1 and st['capture_failures'] == 0, st


def test_evaluate_resnet_equals_the_batch1_loop():
    """PoseEngine.evaluate on mixed-size images == the reference-shaped batch-1 loop (valid.py:195-233) on the drop-in
    pose_resnet model, record for record."""
    from litepose_amd import engine, results
    import litepose_amd.models as models
    from test_gpu_eval_batched import SAME_BUCKET, _batch1_loop, _images
    cfg = _cfg()
    sd = rr.make_state_dict(cfg, seed=1234, head_gain=6.0)         # noise peaks above the threshold
    model = eval('models.' + cfg.MODEL.NAME + '.get_pose_net')(cfg, is_train=False)
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    model.eval()
    eng = engine.PoseEngine(cfg, None, sd)
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
