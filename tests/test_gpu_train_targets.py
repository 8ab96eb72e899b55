"""lp_target_maps and lp_target_masks on the device (csrc/target_kernels.hip; litepose_amd.dataset.targets) against the real
reference's targets (tests/golden/golden_targets.npz, written by tests/golden/gen_golden_targets.py) and against the numpy
restatement of tests/_loss_ref.py: joints tensors exactly, heatmaps bit for bit with the library's own Gaussian table and
to one fp32 ulp of the reference's, masks bit for bit against the oracle's fixed-point warp and against
lp_augment_batch_v; bad descriptors, run-to-run identity, a captured-graph replay, and LabelledSet."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _loss_ref as LR
import _poison as po
import _train_case as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    from litepose_amd.dataset.targets import gaussian_table
    g = tc.load()
    g['table'] = {s: gaussian_table(s) for s in (1, 2)}
    g['d_table'] = {s: tc.dev(t) for s, t in g['table'].items()}
    g['d_joints'], g['d_first'] = tc.dev(g['joints']), tc.dev(g['first'])
    return g


def _outs(g, N, R, fill='N', M=None):
    heat = po.fill(torch.empty((N, int(g['J']), R, R), dtype=torch.float32, device='cuda'), fill)
    jout = po.fill(torch.empty((N, int(g['M']) if M is None else M, int(g['J']), 2), dtype=torch.int32, device='cuda'), fill)
    return heat, jout


def _restated(g, desc, joints, first, R, sigma, tag_per_joint=True, M=None):
    """tests/_loss_ref.py on the host tables, with the library's own table."""
    M = int(g['M']) if M is None else M
    heat, jt = [], []
    for n in range(len(desc)):
        rows = joints[first[n]:first[n] + min(first[n + 1] - first[n], M)]
        cx, cy, ok = LR.cells(rows, desc[n]['mat'], desc[n]['flip'], g['flip_index'].tolist(), R)
        heat.append(LR.heatmaps(cx, cy, ok, g['table'][sigma], R))
        jt.append(LR.joints_tensor(cx, cy, ok, R, M, tag_per_joint))
    return np.stack(heat), np.stack(jt)


def _one_ulp(got, want):
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all())


@pytest.mark.parametrize('R', [16, 32])
def test_batch_equals_the_reference(g, R):
    desc = tc.batch_desc(g, R)
    heat, jout = _outs(g, g['N'], R)
    tc.call_maps(g['d_joints'], g['d_first'], tc.table(desc), R, g, g['d_table'][2], 2, heat, jout)
    torch.cuda.synchronize()
    assert np.array_equal(jout.cpu().numpy(), g['jt_%d' % R])
    want_heat, want_jt = _restated(g, desc, g['joints'], g['first'], R, 2)
    assert np.array_equal(want_jt, g['jt_%d' % R])
    assert po.bitwise_equal(heat.cpu(), torch.from_numpy(want_heat))
    assert _one_ulp(heat.cpu().numpy(), g['heat_%d' % R])
    assert float(heat[1:].max()) == 1.0 and not heat[0].any()           # row 0 has no person: a zero plane stack


def test_sigma_1_and_tag_per_joint_0(g):
    R, desc = 16, tc.batch_desc(g, 16)
    heat, jout = _outs(g, g['N'], R)
    tc.call_maps(g['d_joints'], g['d_first'], tc.table(desc), R, g, g['d_table'][1], 1, heat, jout, tag_per_joint=0)
    torch.cuda.synchronize()
    assert np.array_equal(jout.cpu().numpy(), g['jt_16_nt'])
    assert po.bitwise_equal(heat.cpu(), torch.from_numpy(_restated(g, desc, g['joints'], g['first'], R, 1)[0]))
    assert _one_ulp(heat.cpu().numpy(), g['heat_16_s1'])
    assert int(jout[:, :, :, 0].max()) < R * R


@pytest.mark.parametrize('R', [16, 32])
def test_identity_rows_place_the_exact_cells(g, R):
    """(-0.5, -0.9) -> cell (0, 0); (-1, 3) and (R, 0) out; (R - 0.5, 0) in; v = 0 skipped; a shared cell and two
    overlapping windows (max merge); both flip values."""
    src = g['ident_joints_%d' % R]
    joints, first = tc.dev(np.concatenate([src, src])), tc.dev(np.array([0, 4, 8], np.int32))
    desc = tc.target_desc([tc.IDENT, tc.IDENT], [0, 1])
    heat, jout = _outs(g, 2, R)
    tc.call_maps(joints, first, tc.table(desc), R, g, g['d_table'][2], 2, heat, jout)
    torch.cuda.synchronize()
    for f in (0, 1):
        assert np.array_equal(jout[f].cpu().numpy(), g['ident_jt_%d_f%d' % (R, f)]), f
        assert _one_ulp(heat[f].cpu().numpy(), g['ident_heat_%d_f%d' % (R, f)]), f
    assert jout[0, 0].tolist() == [[0, 1], [2 * R * R + R - 1, 1], [0, 0], [0, 0], [0, 0]]
    want, _ = _restated(g, desc, np.concatenate([src, src]), [0, 4, 8], R, 2)
    assert po.bitwise_equal(heat.cpu(), torch.from_numpy(want))
    # the max merge: between the two overlapping joints of plane 1 the map is the larger entry, not a sum
    assert float(heat[0, 1].max()) == 1.0


def test_row_strips_and_person_cap(g):
    """R = 48: two row strips per plane, the second one short.  M = 2 below a row's four persons: the kernel reads the
    first M (the table's owner refuses such a row; the call's documented condition)."""
    R, M = 48, 2
    desc = tc.batch_desc(g, 32, scale=1.5)
    heat, jout = _outs(g, g['N'], R, M=M)
    tc.call_maps(g['d_joints'], g['d_first'], tc.table(desc), R, g, g['d_table'][2], 2, heat, jout, M=M)
    torch.cuda.synchronize()
    want_heat, want_jt = _restated(g, desc, g['joints'], g['first'], R, 2, M=M)
    assert np.array_equal(jout.cpu().numpy(), want_jt) and want_jt[:, :, :, 1].sum() > 6
    assert po.bitwise_equal(heat.cpu(), torch.from_numpy(want_heat))
    assert heat[:, :, 32:].any() and heat[:, :, :32].any()


def test_bad_rows_yield_zeros(g):
    """reserved != 0, a decreasing, a negative and an overlong d_first range: zeros for that row, the other rows as ever."""
    R = 16
    good = tc.batch_desc(g, R)
    heat0, jout0 = _outs(g, g['N'], R)
    tc.call_maps(g['d_joints'], g['d_first'], tc.table(good), R, g, g['d_table'][2], 2, heat0, jout0)
    cases = []
    bad = good.copy()
    bad[3]['reserved'] = 1
    cases.append((bad, g['first'], 3))
    cases.append((good, np.array([0, 0, 1, 3, 2], np.int32), 3))            # decreasing
    cases.append((good, np.array([-1, 0, 1, 3, 7], np.int32), 0))           # negative start
    cases.append((good, np.array([0, 0, 1, 3, 8], np.int32), 3))            # ends beyond P_tot = 7
    for desc, first, row in cases:
        heat, jout = _outs(g, g['N'], R, 'H')
        tc.call_maps(g['d_joints'], tc.dev(first), tc.table(desc), R, g, g['d_table'][2], 2, heat, jout)
        torch.cuda.synchronize()
        assert not po.as_bits(heat[row]).any() and not jout[row].any(), first
        for n in range(g['N']):
            if n != row and first[n] == g['first'][n] and first[n + 1] == g['first'][n + 1]:
                assert po.bitwise_equal(heat[n], heat0[n]) and torch.equal(jout[n], jout0[n])


def test_each_output_alone_and_twice(g):
    R, desc = 32, tc.table(tc.batch_desc(g, 32))
    heat, jout = _outs(g, g['N'], R)
    tc.call_maps(g['d_joints'], g['d_first'], desc, R, g, g['d_table'][2], 2, heat, jout)
    h2, j2 = _outs(g, g['N'], R, 'H')
    tc.call_maps(g['d_joints'], g['d_first'], desc, R, g, g['d_table'][2], 2, h2, None)
    tc.call_maps(g['d_joints'], g['d_first'], desc, R, g, None, 2, None, j2)
    torch.cuda.synchronize()
    assert po.bitwise_equal(h2, heat) and po.bitwise_equal(j2, jout)


@pytest.mark.parametrize('R', [16, 32])
def test_masks_equal_the_oracle_warp(g, R):
    from oracle.preprocess_ref import warp_affine_u8
    s = g['outs'].tolist().index(R)
    buf, rows = tc.mask_inputs(g, R)
    out = po.fill(torch.empty((g['N'], R, R), dtype=torch.float32, device='cuda'), 'N')
    tc.call_masks(tc.dev(buf), tc.table(rows), R, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, g['mask_t_%d' % R])                         # the real transforms.py on the oracle's warp
    for n in range(g['N']):
        w = warp_affine_u8((g['mask%d' % n] * 255)[:, :, None], g['mat_output'][n, s], (R, R))[:, :, 0]
        want = (w >= 128).astype(np.float32)
        assert np.array_equal(got[n], want[:, ::-1] if g['flip'][n] else want), n
        assert set(np.unique(got[n]).tolist()) == {0.0, 1.0}              # the border shows in every row
    # the one-channel form of lp_augment_batch_v: the mask replicated to three channels, its warped bytes >= 128
    from litepose_amd import _native as nv
    from litepose_amd.dataset.calibration import AUG_DESC_DTYPE
    img, aug, off = np.zeros(0, np.uint8), np.zeros(g['N'], AUG_DESC_DTYPE), 0
    for n in range(g['N']):
        aug[n] = rows[n]
        aug[n]['src_offset'] = off
        rep = np.repeat((g['mask%d' % n] * 255)[:, :, None], 3, axis=2).reshape(-1)
        img, off = np.concatenate([img, rep]), off + rep.size
    u8 = torch.empty((g['N'], R, R, 3), dtype=torch.uint8, device='cuda')
    src = tc.dev(img)
    one = (C.c_float * 3)(1, 1, 1)
    nv.check(nv.lib().lp_augment_batch_v(nv.dptr(src), src.numel(), nv.dptr(tc.table(aug)), g['N'], R, R, one, one,
                                         nv.dptr(u8), None, nv.stream_ptr()), 'lp_augment_batch_v')
    torch.cuda.synchronize()
    assert torch.equal((u8[:, :, :, 0] >= 128).float(), out) and torch.equal(u8[..., 0], u8[..., 2])


def test_bad_mask_descriptors_yield_zeros(g):
    R = 16
    buf, rows = tc.mask_inputs(g, R)
    bad = rows.copy()
    bad[0]['H'] = 0
    bad[1]['src_offset'] = buf.size - rows[1]['H'] * rows[1]['W'] + 1       # ends one byte past the buffer
    bad[2]['src_offset'] = -2
    bad[3]['reserved'] = 1
    out = po.fill(torch.empty((g['N'], R, R), dtype=torch.float32, device='cuda'), 'N')
    tc.call_masks(tc.dev(buf), tc.table(bad), R, out)
    torch.cuda.synchronize()
    assert not po.as_bits(out).any()
    # no source buffer at all: the all-ones rows are served, the rows that name an offset are zeros
    tc.call_masks(None, tc.table(rows), R, po.fill(out, 'H'))
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), g['mask_t_16'][0]) and np.array_equal(out[3].cpu().numpy(), g['mask_t_16'][3])
    assert not po.as_bits(out[1:3]).any()


def test_replayed_from_a_captured_graph(g):
    R = 32
    desc, (buf, rows) = tc.table(tc.batch_desc(g, R)), tc.mask_inputs(g, R)
    src, mdesc = tc.dev(buf), tc.table(rows)
    heat, jout = _outs(g, g['N'], R)
    mask = po.fill(torch.empty((g['N'], R, R), dtype=torch.float32, device='cuda'), 'N')

    def run():
        tc.call_maps(g['d_joints'], g['d_first'], desc, R, g, g['d_table'][2], 2, heat, jout)
        tc.call_masks(src, mdesc, R, mask)
    run()
    torch.cuda.synchronize()
    eager = [heat.clone(), jout.clone(), mask.clone()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # two launches in a row, no branches
        run()
    for pat in ('N', 'H'):
        for t in (heat, jout, mask):
            po.fill(t, pat)
        graph.replay()
        torch.cuda.synchronize()
        assert all(po.bitwise_equal(a, b) for a, b in zip((heat, jout, mask), eager))


def test_labelled_set_is_the_reference_loader(g):
    """The fixture's images, joints and masks through LabelledSet with the fixture's seed: the images of CalibrationSet
    bit for bit, and the reference loader's heatmaps (one ulp: the table), masks and joints (exactly)."""
    from litepose_amd.dataset import CalibrationSet, LabelledSet
    seed, S, outs = int(g['seed']), int(g['input_size']), g['outs'].tolist()
    aug = {k[4:]: g[k].item() for k in g if k.startswith('aug_')}
    images = [g['image%d' % n] for n in range(g['N'])]
    joints = [g['joints'][g['first'][n]:g['first'][n + 1]] for n in range(g['N'])]
    masks = [None, g['mask1'], g['mask2'], None]
    ls = LabelledSet(images, joints, g['flip_index'].tolist(), max_num_people=int(g['M']), sigma=2, masks=masks)
    got = list(ls.batches(S, outs, 3, np.random.RandomState(seed), random.Random(seed), **aug))
    want_images = list(CalibrationSet(images).batches(S, 3, np.random.RandomState(seed), random.Random(seed), **aug))
    torch.cuda.synchronize()
    assert [b[0].shape[0] for b in got] == [3, 1]
    for (im, heats, mks, jts), ref in zip(got, want_images):
        assert po.bitwise_equal(im, ref)
        assert len(heats) == len(mks) == len(jts) == 2
    for s, R in enumerate(outs):
        heat = torch.cat([b[1][s] for b in got]).cpu().numpy()
        assert heat.shape == (g['N'], int(g['J']), R, R) and _one_ulp(heat, g['heat_%d' % R])
        assert np.array_equal(torch.cat([b[2][s] for b in got]).cpu().numpy(), g['mask_t_%d' % R])
        jt = torch.cat([b[3][s] for b in got])
        assert jt.dtype == torch.int32 and np.array_equal(jt.cpu().numpy(), g['jt_%d' % R])
    with pytest.raises(IndexError):
        LabelledSet(images, joints, g['flip_index'].tolist(), max_num_people=3)


def test_batches_without_persons_after_the_last_person(g):
    """Person-less images at the end of the set, alone in their batches (people = [1, 0] in batches of one, and a last
    short batch of two empty images): zero heatmaps, (0, 0) joints, masks as ever; and rows that are not consecutive
    images are refused."""
    from litepose_amd.dataset import LabelledSet
    J, M, fi = int(g['J']), int(g['M']), g['flip_index'].tolist()
    images = [g['image%d' % n] for n in range(g['N'])]
    one = g['joints'][g['first'][1]:g['first'][2]]
    empty = np.zeros((0, J, 3))
    for joints, batch, shapes in (([one, empty], 1, [1, 1]), ([one, one, empty, empty], 2, [2, 2]),
                                  ([one, one, one, empty], 3, [3, 1])):
        ls = LabelledSet(images[:len(joints)], joints, fi, max_num_people=M, sigma=2)
        got = list(ls.batches(int(g['input_size']), [16, 32], batch, np.random.RandomState(2), random.Random(2)))
        torch.cuda.synchronize()
        assert [b[0].shape[0] for b in got] == shapes
        im, heats, masks, jts = got[-1]
        for s, R in enumerate((16, 32)):
            assert tuple(heats[s].shape) == (shapes[-1], J, R, R) and not po.as_bits(heats[s]).any()
            assert tuple(jts[s].shape) == (shapes[-1], M, J, 2) and not jts[s].any()
            assert masks[s].any()
        assert got[0][3][0][:, :, :, 1].sum() > 0                 # the first batch has its person's joints
    img, tables, first = ls.describe_labelled([0, 2], int(g['input_size']), [16, 32], np.random.RandomState(2),
                                              random.Random(2))
    with pytest.raises(ValueError):
        ls.targets([0, 2], tables, first, [16, 32])
