"""lp_pose_loss on the device (csrc/loss_kernels.hip; litepose_amd.core.loss / core.trainer) against the real reference's
losses and their plain fp64 restatement (tests/golden/golden_targets.npz, tests/_loss_ref.py).

The rule, with f the fp64 restatement, r the reference's fp32 value and d the device value: |d - f| <= one fp32 ulp of f
(the device rounds an fp64 result once), and |d - r| <= |r - f| + one ulp (the device is no further from the reference
than the reference's own rounding error allows).  No other tolerance."""
import random

import numpy as np
import pytest
import torch

import _loss_ref as LR
import _poison as po
import _train_case as tc

pytestmark = pytest.mark.gpu

CFGS = [dict(heat=(True, True), ae=(True, False)), dict(heat=(False, True), ae=(True, True))]
FACTORS = (1.0, 0.001, 0.001)


@pytest.fixture(scope='module')
def g():
    g = tc.load()
    for k in ('out_16', 'out_32', 'out_32_tags', 'heat_16', 'heat_32', 'mask_t_16', 'mask_t_32', 'jt_16', 'jt_32'):
        g['d_' + k] = tc.dev(g[k])
    return g


def _stage(g, c, s):
    """(output, J, tag_offset, heat, mask, joints) device tensors of stage s under loss configuration c."""
    R = (16, 32)[s]
    out = g['d_out_16'] if s == 0 else (g['d_out_32'] if c == 0 else g['d_out_32_tags'])
    J = int(g['J'])
    heat = g['d_heat_%d' % R] if CFGS[c]['heat'][s] else None
    off = (J if CFGS[c]['heat'][s] else 0) if CFGS[c]['ae'][s] else -1
    return out, J, off, heat, g['d_mask_t_%d' % R], g['d_jt_%d' % R]


def _run(out, J, off, heat, mask, joints, lt, factors=FACTORS, fill='N'):
    N, R = out.shape[0], out.shape[2]
    hl, push, pull = [po.fill(torch.empty(N, dtype=torch.float32, device='cuda'), fill) for _ in range(3)]
    ws = po.fill(torch.empty(tc.loss_ws(N, J, R), dtype=torch.uint8, device='cuda'), fill)
    # every output and the workspace are handed over whatever the terms: one that is off must leave them alone
    tc.call_loss(out, J, off, heat, mask if heat is not None else None, joints if off >= 0 else None, lt, factors,
                 hl, push, pull, ws)
    if heat is None:
        assert (ws == po.pattern_byte(fill)).all()
    return hl, push, pull


def _hold(d, f, r, what):
    d, f, r = float(d), float(f), float(r)
    print('%s: device %.9g  fp64 %.17g  reference %.9g  ulp %.3g' % (what, d, f, r, LR.ulp32(f)))
    assert abs(d - f) <= LR.ulp32(f), what
    assert abs(d - r) <= abs(r - f) + LR.ulp32(f), what


@pytest.mark.parametrize('lt', ['exp', 'max'])
@pytest.mark.parametrize('c', [0, 1])
def test_losses_hold_to_the_reference(g, c, lt):
    """Both stages of both configurations: images with 0, 1, 2 and 4 persons, a mask with a zero block and a border."""
    ref, f64 = g['loss%d_%s_ref' % (c, lt)], g['loss%d_%s_f64' % (c, lt)]
    seen = 0
    for s in range(2):
        out, J, off, heat, mask, joints = _stage(g, c, s)
        hl, push, pull = _run(out, J, off, heat, mask, joints, LR_TYPES[lt])
        torch.cuda.synchronize()
        for n in range(g['N']):
            if heat is not None:
                _hold(hl[n], f64[s, 0, n], ref[s, 0, n], 'cfg %d %s stage %d image %d heat' % (c, lt, s, n))
                seen += 1
            if off >= 0:
                _hold(push[n], f64[s, 1, n], ref[s, 1, n], 'cfg %d %s stage %d image %d push' % (c, lt, s, n))
                _hold(pull[n], f64[s, 2, n], ref[s, 2, n], 'cfg %d %s stage %d image %d pull' % (c, lt, s, n))
                seen += 2
        if heat is None:
            assert (po.as_bits(hl) == -1).all()                 # a term that is off leaves its output alone
        if off < 0:
            assert (po.as_bits(push) == -1).all() and (po.as_bits(pull) == -1).all()
    assert seen == (16, 20)[c]


LR_TYPES = {'exp': 0, 'max': 1}


@pytest.mark.parametrize('R, shift', [(66, 0), (65, 0), (66, 1)])
def test_heat_strips_and_load_forms(R, shift):
    """Planes above one 4096-float strip: R = 66 (two strips, the second short, 16-byte loads), R = 65 (an odd plane:
    scalar loads) and R = 66 on a base one float off a 16-byte boundary (scalar loads).  The output has more channels
    than joints.  One rounding of the restatement."""
    rng = np.random.RandomState(R + shift)
    N, J, Cc = 2, 3, 5
    out = rng.standard_normal((N, Cc, R, R)).astype(np.float32)
    heat = rng.uniform(0, 1, (N, J, R, R)).astype(np.float32)
    mask = (rng.uniform(0, 1, (N, R, R)) > 0.3).astype(np.float32)

    def put(a):
        t = torch.empty(a.size + shift, dtype=torch.float32, device='cuda')
        v = t[shift:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 * shift
        return v
    hl, _, _ = _run(put(out), J, -1, put(heat), put(mask), None, 0, (0.5, 1.0, 1.0))
    torch.cuda.synchronize()
    assert tc.loss_ws(N, J, R) == N * J * 2 * 8
    for n in range(N):
        f = LR.heat_loss(out[n, :J], heat[n], mask[n], 0.5)
        assert abs(float(hl[n]) - f) <= LR.ulp32(f), (n, float(hl[n]), f)


def test_two_calls_give_identical_bits(g):
    for c, s in ((0, 0), (1, 1)):
        a = _run(*_stage(g, c, s), 0, fill='N')
        b = _run(*_stage(g, c, s), 0, fill='H')
        torch.cuda.synchronize()
        assert all(po.bitwise_equal(x, y) for x, y in zip(a, b))      # both stages have every term on


def test_replayed_from_a_captured_graph(g):
    out, J, off, heat, mask, joints = _stage(g, 0, 0)
    eager = [t.clone() for t in _run(out, J, off, heat, mask, joints, 0)]
    N, R = out.shape[0], out.shape[2]
    hl, push, pull = [torch.empty(N, dtype=torch.float32, device='cuda') for _ in range(3)]
    ws = torch.empty(tc.loss_ws(N, J, R), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # two launches in a row, no branches
        tc.call_loss(out, J, off, heat, mask, joints, 0, FACTORS, hl, push, pull, ws)
    for pat in ('N', 'H'):
        for t in (hl, push, pull, ws):
            po.fill(t, pat)
        graph.replay()
        torch.cuda.synchronize()
        assert all(po.bitwise_equal(a, b) for a, b in zip((hl, push, pull), eager))


def test_out_of_range_index_counts_as_not_visible(g):
    """An index at or beyond (C - tag_offset) * R * R, or negative, with the visible flag set: the result is that of the
    same joints with the flag cleared.  The output tensor sits between guards of NaN, so a read beyond it would show."""
    out, J, off, heat, mask, joints = _stage(g, 0, 0)
    R, Cc = out.shape[2], out.shape[1]
    arena = po.Arena('N')
    guarded = arena.inp(out, what='d_out')
    bad, cleared = joints.clone(), joints.clone()
    vis = np.argwhere(g['jt_16'][:, :, :, 1] == 1)
    in3, in2 = vis[vis[:, 0] == 3], vis[vis[:, 0] == 2]
    picks = [tuple(in3[0]), tuple(in3[-1]), tuple(in2[0])]       # two slots of the four-person image, one of the two-person one
    assert len(set(picks)) == 3 and picks[0][1] != picks[1][1]
    for (n, p, k), index in zip(picks, ((Cc - off) * R * R, -5, 2 ** 31 - 1)):
        bad[n, p, k, 0] = index
        cleared[n, p, k] = 0
    a = _run(guarded, J, off, heat, mask, bad, 0)
    b = _run(out, J, off, heat, mask, cleared, 0)
    arena.check()
    assert all(po.bitwise_equal(x, y) for x, y in zip(a, b))
    assert torch.isfinite(a[1]).all() and torch.isfinite(a[2]).all()
    want = [LR.tag_loss(g['out_16'][n, off:], cleared[n].cpu().numpy(), 'exp', 0.001, 0.001) for n in range(g['N'])]
    for n, (push, pull) in enumerate(want):
        assert abs(float(a[1][n]) - push) <= LR.ulp32(push) and abs(float(a[2][n]) - pull) <= LR.ulp32(pull), n


def _cfg(g, c, lt=None):
    from litepose_amd import config
    cfg = config.get_cfg()
    cfg.MODEL.NUM_JOINTS = cfg.DATASET.NUM_JOINTS = int(g['J'])
    cfg.DATASET.MAX_NUM_PEOPLE, cfg.DATASET.OUTPUT_SIZE = int(g['M']), [16, 32]
    cfg.LOSS.WITH_HEATMAPS_LOSS, cfg.LOSS.WITH_AE_LOSS = list(CFGS[c]['heat']), list(CFGS[c]['ae'])
    if lt is not None:
        cfg.LOSS.AE_LOSS_TYPE = lt
    return cfg


@pytest.mark.parametrize('c', [0, 1])
def test_multi_loss_factory_has_the_reference_structure(g, c):
    """Lists per stage: an [N] tensor, a scalar, a scalar, None where a term is off; the factors and the loss type from
    cfg.LOSS where present and the reference's defaults ('max', 1.0, 0.001, 0.001) otherwise."""
    from litepose_amd.core.loss import AELoss, HeatmapLoss, MultiLossFactory
    for lt in (None, 'exp'):
        fac = MultiLossFactory(_cfg(g, c, lt))
        assert fac.loss_type == (lt or 'max') and fac.push_loss_factor == (0.001, 0.001)
        outs = [g['d_out_16'], g['d_out_32'] if c == 0 else g['d_out_32_tags']]
        res = fac(outs, [g['d_heat_16'], g['d_heat_32']], [g['d_mask_t_16'], g['d_mask_t_32']], [g['d_jt_16'], g['d_jt_32']])
        hl, push, pull = res
        per = fac.per_image(outs, [g['d_heat_16'], g['d_heat_32']], [g['d_mask_t_16'], g['d_mask_t_32']],
                            [g['d_jt_16'], g['d_jt_32']])
        ref, f64 = g['loss%d_%s_ref' % (c, lt or 'max')], g['loss%d_%s_f64' % (c, lt or 'max')]
        for s in range(2):
            if CFGS[c]['heat'][s]:
                assert tuple(hl[s].shape) == (g['N'],) and hl[s].is_cuda
                for n in range(g['N']):
                    _hold(hl[s][n], f64[s, 0, n], ref[s, 0, n], 'factory heat')
            else:
                assert hl[s] is None
            if CFGS[c]['ae'][s]:
                # a scalar: torch's mean over the batch of the per-image terms, which hold to the reference one by one
                for got, k in ((push[s], 1), (pull[s], 2)):
                    assert got.dim() == 0 and po.bitwise_equal(got, per[k][s].mean())
                    for n in range(g['N']):
                        _hold(per[k][s][n], f64[s, k, n], ref[s, k, n], 'factory tags')
            else:
                assert push[s] is None and pull[s] is None
    # the two single losses with the reference's signatures
    J = int(g['J'])
    one = HeatmapLoss()(g['d_out_32'], g['d_heat_32'], g['d_mask_t_32'])
    assert tuple(one.shape) == (g['N'],)
    for n in range(g['N']):
        assert abs(float(one[n]) - g['loss0_exp_f64'][1, 0, n]) <= LR.ulp32(g['loss0_exp_f64'][1, 0, n])
    tags = g['d_out_16'][:, J:].contiguous().view(g['N'], -1, 1)
    push, pull = AELoss('exp', int(g['M']), 16)(tags, g['d_jt_16'].long())
    per = AELoss('exp', int(g['M']), 16).per_image(tags, g['d_jt_16'])
    assert push.dim() == 0 and float(push) == float(per[0].mean()) and float(pull) == float(per[1].mean())
    for n in range(g['N']):                              # factor 1 here: the fixture's values carry 0.001
        f = LR.tag_loss(g['out_16'][n, J:], g['jt_16'][n], 'exp', 1.0, 1.0)
        assert abs(float(per[0][n]) - f[0]) <= LR.ulp32(f[0]) and abs(float(per[1][n]) - f[1]) <= LR.ulp32(f[1])


def test_a_stage_without_a_loss_gives_nones(g):
    """WITH_HEATMAPS_LOSS and WITH_AE_LOSS both off on a stage: (None, None, None) for it, as the reference appends,
    and the other stage as ever."""
    from litepose_amd.core.loss import MultiLossFactory
    cfg = _cfg(g, 0, 'exp')
    cfg.LOSS.WITH_HEATMAPS_LOSS = [True, False]
    args = ([g['d_out_16'], g['d_out_32']], [g['d_heat_16'], g['d_heat_32']], [g['d_mask_t_16'], g['d_mask_t_32']],
            [g['d_jt_16'], g['d_jt_32']])
    hl, push, pull = MultiLossFactory(cfg)(*args)
    assert hl[1] is None and push[1] is None and pull[1] is None
    want = MultiLossFactory(_cfg(g, 0, 'exp'))(*args)
    assert po.bitwise_equal(hl[0], want[0][0]) and po.bitwise_equal(push[0], want[1][0])
    assert po.bitwise_equal(pull[0], want[2][0])


def test_pose_loss_into_kept_buffers_replays_from_a_graph(g):
    """``pose_loss`` with ``buffers``: no allocation in the call, so the wrapper itself is capturable; the replay gives
    the eager bits."""
    from litepose_amd.core.loss import loss_buffers, pose_loss
    out, J, off, heat, mask, joints = _stage(g, 0, 0)
    eager = [t.clone() for t in pose_loss(out, J, off, heat, mask, joints, 'exp', *FACTORS)]
    buf = loss_buffers(out.shape[0], J, out.shape[2], out.device)
    with pytest.raises(ValueError):
        pose_loss(g['d_out_32'], J, -1, g['d_heat_32'], g['d_mask_t_32'], buffers=buf)      # made for another shape
    got = pose_loss(out, J, off, heat, mask, joints, 'exp', *FACTORS, buffers=buf)
    assert got[0] is buf['heat'] and got[1] is buf['push'] and got[2] is buf['pull']
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pose_loss(out, J, off, heat, mask, joints, 'exp', *FACTORS, buffers=buf)
    for k in ('heat', 'push', 'pull', 'workspace'):
        po.fill(buf[k], 'N')
    graph.replay()
    torch.cuda.synchronize()
    assert all(po.bitwise_equal(buf[k], e) for k, e in zip(('heat', 'push', 'pull'), eager))


def test_loss_epoch_is_the_batch_weighted_average():
    """loss_epoch over five labelled images in batches of 2, 2, 1 equals the AverageMeter arithmetic done by hand on the
    per-batch values of the same loader, model and factory."""
    import _net_check as nc
    from litepose_amd.core import inference
    from litepose_amd.core.loss import MultiLossFactory
    from litepose_amd.core.trainer import loss_epoch
    from litepose_amd.dataset import LabelledSet
    model, _, _ = nc._model('search-XS', storage='f32')
    cfg = nc._cfg()
    cfg.DATASET.INPUT_SIZE, cfg.DATASET.OUTPUT_SIZE, cfg.DATASET.MAX_NUM_PEOPLE = 64, [16, 32], 6
    J = cfg.DATASET.NUM_JOINTS
    rng = np.random.RandomState(3)
    sizes = [(40, 56), (33, 47), (64, 64), (25, 30), (48, 36)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    joints = []
    for (h, w), people in zip(sizes, (2, 0, 3, 1, 6)):
        j = np.zeros((people, J, 3))
        j[:, :, 0], j[:, :, 1] = rng.uniform(0, w, (people, J)), rng.uniform(0, h, (people, J))
        j[:, :, 2] = rng.choice([0, 1, 2], (people, J))
        joints.append(j)
    ls = LabelledSet(images, joints, inference.flip_index_for(cfg)[:J], max_num_people=6, sigma=cfg.DATASET.SIGMA)
    got = loss_epoch(model, ls, cfg, 2, np.random.RandomState(8), random.Random(8))
    fac = MultiLossFactory(cfg)
    sums, count = {}, 0
    for images_b, heats, masks, jts in ls.batches(64, [16, 32], 2, np.random.RandomState(8), random.Random(8)):
        hl, push, pull = fac(model.forward(images_b), heats, masks, jts)
        n = images_b.shape[0]
        for key, vals in (('heatmaps', hl), ('push', push), ('pull', pull)):
            for s, v in enumerate(vals):
                if v is not None:
                    sums[key, s] = sums.get((key, s), 0.0) + float(v.mean()) * n
        count += n
    assert count == 5 and sorted(got) == ['heatmaps', 'pull', 'push']
    assert got['push'][1] is None and got['pull'][1] is None and got['heatmaps'][0] is not None
    for (key, s), v in sums.items():
        assert got[key][s] == pytest.approx(v / count, rel=1e-12, abs=0), (key, s)
        assert np.isfinite(got[key][s]) and got[key][s] >= 0
    assert got['heatmaps'][1] > 0 and got['pull'][0] > 0
