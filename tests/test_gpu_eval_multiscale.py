"""Multi-scale batch evaluation on the device: lp_tta_merge_scales against the batch-1 chain it replaces (tta_project
per scale + aggregate_results + the division of valid.py:224) bit for bit, against the real reference's multi-scale
outputs, and ``evaluate`` with several scales / without PROJECT2IMAGE against the batch-1 loop.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

from test_gpu_eval_batched import _batch1_loop, _images, _setup
from test_oracle_pinning import MS_CASES, _ms_case, _ms_center, _ms_p2i

pytestmark = pytest.mark.gpu


def _cfg(scales, p2i, dataset='crowd_pose'):
    from litepose_amd import config
    cfg = config.get_cfg(dataset)
    cfg.TEST.SCALE_FACTOR = list(scales)
    cfg.TEST.PROJECT2IMAGE = p2i
    return cfg


def _mid(rng, N, J, h1, w1):
    """A seeded mid buffer (lp_tta_workspace_bytes, uint8) and its float view [N,4,J,h1,w1]; some cells -0.0."""
    from litepose_amd import _native as nv
    need = int(nv.lib().lp_tta_workspace_bytes(N, J, h1, w1))
    buf = torch.empty(need, dtype=torch.uint8, device='cuda')
    v = buf[:N * 4 * J * h1 * w1 * 4].view(torch.float32).view(N, 4, J, h1, w1)
    a = rng.normal(size=(N, 4, J, h1, w1)).astype(np.float32)
    a[rng.random(a.shape) < 0.05] = -0.0
    a[rng.random(a.shape) < 0.05] = 0.0
    v.copy_(torch.from_numpy(a))
    return buf, v


def _chain(cfg, mids, N, J, T, base):
    """The batch-1 sequence on the same mids: tta_project per scale (to the base size with PROJECT2IMAGE, else at the
    scale's own size), aggregate_results, / len(SCALE_FACTOR), torch.cat of the tags."""
    from litepose_amd.core import inference
    order, _ = inference.scale_order(cfg)
    final, tags_list = None, []
    for sc, (_, v, h1, w1) in zip(order, mids):
        size = base if cfg.TEST.PROJECT2IMAGE else (w1, h1)
        det, tag = inference.tta_project(v, N, J, h1, w1, size, T)
        final, tags_list = inference.aggregate_results(cfg, sc, final, tags_list, inference._Merged([det]),
                                                       inference._Merged([tag]))
    final = final / float(len(order))
    return final, torch.cat(tags_list, dim=4)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


# (scale factors, T, PROJECT2IMAGE, N, J, stage-1 (h1, w1) per scale in visiting order, base (W, H))
KERNEL_CASES = [
    ([1], 2, True, 2, 5, [(13, 21)], (42, 26)),
    ([1], 1, False, 2, 5, [(13, 21)], None),
    ([1], 2, False, 3, 4, [(7, 9)], None),
    ([1, 2], 2, True, 2, 3, [(26, 42), (13, 21)], (42, 26)),
    ([1, 2], 1, True, 2, 3, [(26, 42), (13, 21)], (42, 26)),
    ([1, 2], 2, False, 2, 3, [(26, 42), (13, 21)], None),          # scale 1 not first: its tags are resized
    ([0.5, 1, 2], 2, True, 2, 4, [(32, 24), (16, 12), (8, 6)], (24, 32)),
    ([0.5, 1, 2], 1, False, 2, 4, [(32, 24), (16, 12), (8, 6)], None),
    ([0.5, 1, 2], 2, False, 1, 6, [(33, 19), (17, 10), (9, 5)], None),
    ([1, 0.5], 2, False, 2, 3, [(17, 9), (9, 5)], None),            # scale 1 first, odd sizes
    ([1, 0.5], 1, False, 2, 3, [(17, 9), (9, 5)], None),
    ([1, 0.75], 2, True, 2, 3, [(12, 16), (9, 12)], (32, 24)),
    ([0.75, 1], 2, False, 2, 3, [(12, 16), (9, 12)], None),
    ([1, 2], 2, True, 2200, 30, [(4, 6), (2, 3)], (6, 4)),           # N * J > 65535
    ([0.5, 1, 2], 2, False, 2200, 30, [(4, 6), (2, 3), (1, 2)], None),
]


@pytest.mark.parametrize('case', range(len(KERNEL_CASES)))
def test_merge_scales_equals_the_batch1_chain_bitwise(case):
    from litepose_amd.core import inference
    scales, T, p2i, N, J, hw, base = KERNEL_CASES[case]
    cfg = _cfg(scales, p2i)
    rng = np.random.default_rng(100 + case)
    mids = [_mid(rng, N, J, h1, w1) + (h1, w1) for h1, w1 in hw]
    det, tag = inference.tta_merge_scales(cfg, [(buf, h1, w1) for buf, _, h1, w1 in mids], N, J, T, base)
    ref_det, ref_tag = _chain(cfg, mids, N, J, T, base)
    assert det.shape == ref_det.shape and tag.shape == ref_tag.shape
    assert torch.equal(_bits(det), _bits(ref_det)), case
    assert torch.equal(_bits(tag), _bits(ref_tag)), case
    if len(scales) > 1:          # not the first scale's maps alone
        only, _ = _chain(_cfg([1], p2i), mids[:1], N, J, T, base)
        assert not torch.equal(det, only)


@pytest.mark.parametrize('name', MS_CASES)
def test_merge_scales_against_the_reference(golden_ms, name):
    """The real reference's per-scale network outputs through tta_stage + lp_tta_merge_scales == its final maps and
    tags (the budget of the existing multi-scale goldens)."""
    from litepose_amd import _native as nv
    from litepose_amd.core import inference
    J, base, flip, per = _ms_case(golden_ms, name)
    cfg = _cfg([sc for sc, _, _ in per], _ms_p2i(golden_ms, name), 'coco' if J in (17, 18) else 'crowd_pose')
    cfg.TEST.FLIP_TEST = flip
    cfg.DATASET.WITH_CENTER, cfg.TEST.IGNORE_CENTER = _ms_center(golden_ms, name)
    cfg.DATASET.NUM_JOINTS = cfg.MODEL.NUM_JOINTS = J
    Ju = inference.used_joints(cfg)
    mids = []
    for sc, outs, outs_f in per:                       # stored in descending-scale order
        N, _, h1, w1 = outs[1].shape
        mid = torch.empty(int(nv.lib().lp_tta_workspace_bytes(N, Ju, h1, w1)), dtype=torch.uint8, device='cuda')
        n, j, h1, w1, T = inference.tta_stage(cfg, [o.cuda() for o in outs],
                                              [o.cuda() for o in outs_f] if flip else None, mid)
        mids.append((mid, h1, w1))
    final, tags = inference.tta_merge_scales(cfg, mids, n, j, T, base)
    np.testing.assert_allclose(final.cpu().numpy(), golden_ms[name + '_final'], rtol=0, atol=2e-6)
    np.testing.assert_allclose(tags.cpu().numpy(), golden_ms[name + '_tags'], rtol=0, atol=2e-6)


def _eval_shapes(seed):
    # 36 images of one bucket at every configuration below (9 batches of 4: every buffer set captures and replays),
    # four more buckets in both orientations, buckets ending on padded batches, shuffled so that they interleave
    shapes = [(427, 640), (480, 640), (375, 500)] * 12 + [(640, 427)] * 5 + [(612, 612)] * 3 + [(360, 640)] * 2 + \
        [(200, 600)] * 2
    rng = np.random.default_rng(seed)
    return [shapes[i] for i in rng.permutation(len(shapes))]


def _evaluate_vs_loop(storage, scales, p2i, shapes, batch, replays):
    from litepose_amd import evaluate as ev
    from litepose_amd import results
    cfg, model, eng = _setup(storage)
    cfg.DATASET.INPUT_SIZE = 128
    cfg.TEST.SCALE_FACTOR = list(scales)
    cfg.TEST.PROJECT2IMAGE = p2i
    images = _images(shapes, 7 + len(scales))
    order = sorted(scales, reverse=True)
    batches = ev.plan(shapes, 128, min(scales), batch, order)
    assert any(b.real < batch for b in batches)
    keys = [b.size for b in batches]
    ids = [500 + 2 * i for i in range(len(images))]
    stats = {}
    got = eng.evaluate(images, image_ids=ids, batch_size=batch, stats=stats)
    all_preds, all_scores, _ = _batch1_loop(cfg, model, images)
    ref = results.preds_to_results(all_preds, all_scores, ids)
    assert sum(len(p) for p in all_preds) > 0, 'no persons: vacuous'
    assert len(got) == len(ref)
    assert got == ref
    st = eng.graph_stats()
    assert st['capture_failures'] == 0, st
    if replays:
        assert len(ev.bucket_histogram(batches)) >= 4
        assert max(keys.count(k) for k in set(keys)) >= 9
        assert st['graph_replays'] > 0, st
    assert stats['batches'] == len(batches)


@pytest.mark.parametrize('scales,p2i', [([0.5, 1, 2], True), ([1, 2], True), ([1], False), ([2, 1, 0.5], False)])
def test_evaluate_multiscale_equals_the_batch1_loop(scales, p2i):
    _evaluate_vs_loop(None, scales, p2i, _eval_shapes(31), 4, True)


def test_evaluate_multiscale_bf16_equals_the_batch1_loop():
    shapes = [(427, 640), (640, 427), (612, 612)] * 3 + [(480, 640)] * 3
    _evaluate_vs_loop('bf16', [1, 2], True, shapes, 4, False)


def test_release_scales_frees_every_scale():
    """A finished multi-scale bucket leaves no buffers or graphs of its shapes behind."""
    from litepose_amd.utils import transforms as T
    cfg, _, eng = _setup()
    cfg.TEST.SCALE_FACTOR = [1, 2]
    N = 2
    xs = (torch.randn(N, 3, 256, 256, device='cuda'), torch.randn(N, 3, 128, 128, device='cuda'))
    coef = torch.from_numpy(np.stack([T.final_preds_coef((64, 64), (1.28, 1.28), (128, 128))] * N)).cuda()
    for _ in range(2 * eng.buffer_sets() + 1):
        with eng.submit(xs, preds_coef=coef):
            pass
    torch.cuda.synchronize()
    lanes = eng._lanes
    assert any(ln['graphs'] for ln in lanes)
    eng.release_scales(N, [(256, 256), (128, 128)])
    for ln in lanes:
        assert not ln['graphs'] and not ln['seen']
        assert not [k for k in ln['eng']._bufs if k in ((N, 256, 256), (N, 128, 128)) or k[0] == 'ms']
