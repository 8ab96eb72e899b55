"""Batch evaluation of variable-size images (litepose_amd.evaluate): the per-image pre-processing and back-projection
kernels against their one-transform forms and the oracle, and ``evaluate`` against the reference-shaped batch-1 loop
(valid.py:195-233) over the same images.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

from oracle import group_ref, preprocess_ref, synth, transforms_ref

pytestmark = pytest.mark.gpu

# H x W of COCO / CrowdPose-like images; the first four share the (384, 256) bucket at 256
SAME_BUCKET = [(427, 640), (480, 640), (333, 500), (375, 500)]


def _images(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]


def test_preprocess_batch_v_bitwise_and_bounds():
    """Mixed source sizes of one bucket in ONE launch == resize_align_multi_scale + ToTensor/Normalize of the oracle
    per image, bit for bit, and == lp_preprocess per image; descriptors outside the source buffer give zeros."""
    from litepose_amd.utils import transforms as T
    shapes = SAME_BUCKET + [(427, 640), (400, 600)]
    imgs = _images(shapes, 11)
    size = T.get_multi_scale_size(imgs[0], 256, 1.0, 1.0)[0]
    assert all(tuple(T.get_multi_scale_size(im, 256, 1.0, 1.0)[0]) == tuple(size) for im in imgs)
    Wd, Hd = size
    # packed with gaps, not in input order
    order = [3, 0, 5, 1, 4, 2]
    offs, off = [0] * len(imgs), 0
    for n in order:
        off += 37
        offs[n] = off
        off += imgs[n].size
    buf = np.zeros(off + 100, np.uint8)
    for n, im in enumerate(imgs):
        buf[offs[n]:offs[n] + im.size] = im.reshape(-1)
    N = len(imgs) + 3
    desc = np.zeros(N, T.WARP_DESC_DTYPE)
    for n, im in enumerate(imgs):
        _, center, scale = T.get_multi_scale_size(im, 256, 1.0, 1.0)
        desc[n] = (offs[n], im.shape[0], im.shape[1], T.warp_invert(T.get_affine_transform(center, scale, 0, size)))
    # out of bounds: one byte past the buffer, an offset past its end, a zero height
    desc[len(imgs)] = (buf.size - imgs[0].size + 1, imgs[0].shape[0], imgs[0].shape[1], desc[0]['minv'])
    desc[len(imgs) + 1] = (buf.size + 4096, 10, 10, desc[0]['minv'])
    desc[len(imgs) + 2] = (0, 0, 640, desc[0]['minv'])
    src = torch.from_numpy(buf).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8).reshape(N, 64).copy()).cuda()
    out = torch.full((N, 3, Hd, Wd), 7.0, dtype=torch.float32, device='cuda')
    out_u8 = torch.full((N, Hd, Wd, 3), 7, dtype=torch.uint8, device='cuda')
    T.preprocess_batch_v_device(src, d_desc, size, out=out, out_u8=out_u8)
    torch.cuda.synchronize()
    got, got_u8 = out.cpu().numpy(), out_u8.cpu().numpy()
    for n, im in enumerate(imgs):
        ref_u8, _, _ = preprocess_ref.resize_align_multi_scale(im, 256, 1.0, 1.0)
        assert np.array_equal(got_u8[n], ref_u8), n
        assert np.array_equal(got[n], preprocess_ref.to_tensor_normalize(ref_u8)), n
        one_u8 = T.resize_align_multi_scale(im, 256, 1.0, 1.0)[0]
        one = T.ToTensorNormalize()(one_u8)
        assert np.array_equal(one_u8.cpu().numpy(), got_u8[n]) and np.array_equal(one.cpu().numpy(), got[n]), n
    for n in range(len(imgs), N):
        assert not got_u8[n].any() and not got[n].any(), n
    # the table is read when the launch runs: refilled in place, the same launch gives the new images
    desc2 = desc.copy()
    desc2[0], desc2[1] = desc[1], desc[0]
    d_desc.copy_(torch.from_numpy(desc2.view(np.uint8).reshape(N, 64).copy()))
    T.preprocess_batch_v_device(src, d_desc, size, out=out)
    assert torch.equal(out[0].cpu(), torch.from_numpy(got[1])) and torch.equal(out[1].cpu(), torch.from_numpy(got[0]))


def test_final_preds_v_bitwise_per_image():
    """lp_final_preds_v with a centre / scale per image == lp_final_preds on each image alone, bitwise, including a
    count of 0, a count above the capacity and a negative count."""
    from litepose_amd.utils import transforms as T
    rng = np.random.default_rng(3)
    N, pcap, J, D = 6, 8, 14, 5
    ans0 = torch.from_numpy(rng.uniform(-5, 300, size=(N, pcap, J, D)).astype(np.float32)).cuda()
    count = torch.tensor([3, 0, pcap, pcap + 5, -1, 1], dtype=torch.int32, device='cuda')
    hws = [(427, 640), (640, 427), (612, 612), (640, 360), (200, 600), (333, 500)]
    ref = ans0.clone()
    coef = np.zeros((N, 4), np.float64)
    for n, hw in enumerate(hws):
        size, center, scale = T.get_multi_scale_size(hw, 256, 1.0, 1.0)
        T.final_preds_device(ref[n:n + 1], count[n:n + 1], center, scale, size)
        coef[n] = T.final_preds_coef(center, scale, size)
    got = ans0.clone()
    T.final_preds_device_v(got, count, torch.from_numpy(coef).cuda())
    assert torch.equal(got, ref)
    assert not torch.equal(got, ans0)


def _batch1_loop(cfg, model, images):
    """valid.py:195-233 on the drop-in modules, batch 1: resize_align_multi_scale -> ToTensorNormalize ->
    get_multi_stage_outputs -> aggregate_results -> HeatmapParser.parse -> get_final_preds (imports as
    INTEGRATION.md section 3).  Returns (all_preds, all_scores, per-image (maps, centre, scale))."""
    from litepose_amd.core.group import HeatmapParser
    from litepose_amd.core.inference import aggregate_results, get_multi_stage_outputs
    from litepose_amd.utils.transforms import (ToTensorNormalize, get_final_preds, get_multi_scale_size,
                                               resize_align_multi_scale)
    parser = HeatmapParser(cfg)
    transforms = ToTensorNormalize()
    all_preds, all_scores, extra = [], [], []
    sf = cfg.TEST.SCALE_FACTOR
    for image in images:
        base_size, center, scale = get_multi_scale_size(image, cfg.DATASET.INPUT_SIZE, 1.0, min(sf))
        final_heatmaps, tags_list = None, []
        for s in sorted(sf, reverse=True):
            image_resized, center, scale = resize_align_multi_scale(image, cfg.DATASET.INPUT_SIZE, s, min(sf))
            image_resized = transforms(image_resized).unsqueeze(0).cuda()
            outputs, heatmaps, tags = get_multi_stage_outputs(cfg, model, image_resized, cfg.TEST.FLIP_TEST,
                                                              cfg.TEST.PROJECT2IMAGE, base_size)
            final_heatmaps, tags_list = aggregate_results(cfg, s, final_heatmaps, tags_list, heatmaps, tags)
        final_heatmaps = final_heatmaps / float(len(sf))
        tags = torch.cat(tags_list, dim=4)
        grouped, scores = parser.parse(final_heatmaps, tags, cfg.TEST.ADJUST, cfg.TEST.REFINE)
        final_results = get_final_preds(grouped, center, scale, [final_heatmaps.size(3), final_heatmaps.size(2)])
        all_preds.append(final_results)
        all_scores.append(scores)
        extra.append((final_heatmaps, tags, center, scale))
    return all_preds, all_scores, extra


def _setup(storage=None):
    from litepose_amd import arch_zoo, config, engine
    import litepose_amd.models as models
    arch = arch_zoo.get('search-XS')
    cfg = config.apply_arch(config.get_cfg('crowd_pose'), arch)
    sd = synth.make_state_dict(arch, seed=1234, head_gain=6.0)       # noise peaks above the threshold
    model = models.pose_mobilenet.get_pose_net(cfg, is_train=False, cfg_arch=arch, storage=storage)
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    model.eval()
    eng = engine.PoseEngine(cfg, arch, sd, storage=storage)
    return cfg, model, eng


def _mixed_shapes(seed):
    # 40 images of the (384, 256) bucket (10 batches of 4: every buffer set captures and replays), six buckets in
    # all, both orientations, buckets ending on padded batches, shuffled so that buckets interleave in input order
    shapes = SAME_BUCKET * 10 + [(640, 427)] * 6 + [(612, 612)] * 5 + [(640, 360)] * 3 + [(200, 600)] * 2 + \
        [(360, 640)] * 2
    rng = np.random.default_rng(seed)
    return [shapes[i] for i in rng.permutation(len(shapes))]


def test_evaluate_equals_the_batch1_loop():
    from litepose_amd import evaluate as ev
    from litepose_amd import results
    cfg, model, eng = _setup()
    shapes = _mixed_shapes(21)
    images = _images(shapes, 22)
    batches = ev.plan(shapes, cfg.DATASET.INPUT_SIZE, 1.0, 4)
    assert len(ev.bucket_histogram(batches)) == 6 and len(shapes) >= 48
    assert any(b.real < 4 for b in batches)
    ids = [1000 + 3 * i for i in range(len(images))]
    stats = {}
    got = eng.evaluate(images, image_ids=ids, batch_size=4, stats=stats)
    all_preds, all_scores, _ = _batch1_loop(cfg, model, images)
    ref = results.preds_to_results(all_preds, all_scores, ids)
    assert sum(len(p) for p in all_preds) > 0, 'no persons: vacuous'
    assert len(got) == len(ref)
    assert got == ref
    st = eng.graph_stats()
    assert st['graph_replays'] > 0 and st['capture_failures'] == 0, st
    assert stats['batches'] == len(batches)
    # a second call on the same engine (fresh staging buffers) gives the same list
    assert eng.evaluate(images, image_ids=ids, batch_size=4) == ref


def test_batch1_chain_non_square_against_the_oracle():
    """The batch-1 chain evaluate is compared with, checked itself at non-square sizes: the oracle parser and the
    oracle back-projection on the device's maps, with the image's own centre and scale."""
    cfg, model, _ = _setup()
    images = _images([(427, 640), (640, 427)], 31)
    all_preds, all_scores, extra = _batch1_loop(cfg, model, images)
    ora = group_ref.HeatmapParser(group_ref.Params())
    for preds, scores, (fh, tags, center, scale) in zip(all_preds, all_scores, extra):
        assert fh.shape[2] != fh.shape[3]
        a, sc = ora.parse_image(fh[0].cpu().numpy(), tags[0].cpu().numpy())
        ref = transforms_ref.get_final_preds([a], center, scale, [fh.size(3), fh.size(2)])
        assert len(preds) == len(ref) and len(ref) > 0
        for p, q in zip(preds, ref):
            np.testing.assert_allclose(p, q, rtol=0, atol=1e-4)
        assert np.array_equal(np.asarray(scores, np.float32), sc)


def test_evaluate_bf16_equals_the_batch1_loop():
    from litepose_amd import results
    cfg, model, eng = _setup(storage='bf16')
    shapes = [(427, 640), (640, 427), (612, 612)] * 3 + [(480, 640)]
    images = _images(shapes, 41)
    got = eng.evaluate(images, batch_size=2)
    all_preds, all_scores, _ = _batch1_loop(cfg, model, images)
    ref = results.preds_to_results(all_preds, all_scores, list(range(len(images))))
    assert sum(len(p) for p in all_preds) > 0, 'no persons: vacuous'
    assert got == ref
