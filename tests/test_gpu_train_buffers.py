"""Buffer contract of lp_target_maps, lp_target_masks and lp_pose_loss (include/litepose_amd.h) with poisoned and guarded
buffers (tests/_poison.py): every documented element written, nothing outside the outputs or beyond the workspace bytes,
inputs unmodified and not over-read, results independent of what the buffers held."""
import pytest
import torch

import _poison as po
import _train_case as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    from litepose_amd.dataset.targets import gaussian_table
    g = tc.load()
    g['d_gauss'] = tc.dev(gaussian_table(2))
    return g


def _agree(res):
    z = res['Z']
    for pat in ('N', 'H'):
        for k, v in res[pat].items():
            left = po.still_poisoned(v, z[k], pat)
            assert not left, (pat, k, len(left), left[0])
            assert po.bitwise_equal(v, z[k]), (pat, k, po.first_difference(v, z[k]))


@pytest.mark.parametrize('which', ['both', 'heat_out', 'joints_out'])
def test_target_maps_respects_its_buffers(g, which):
    R, N, J, M = 32, g['N'], int(g['J']), int(g['M'])
    desc = tc.table(tc.batch_desc(g, R))
    res = {}
    for pat in po.PATTERNS:
        ar = po.Arena(pat)
        heat = ar.out((N, J, R, R), what='heat_out') if which != 'joints_out' else None
        jout = ar.out((N, M, J, 2), torch.int32, what='joints_out') if which != 'heat_out' else None
        joints = ar.inp(tc.dev(g['joints']), what='d_joints')
        first = ar.inp(tc.dev(g['first']), what='d_first')
        dd = ar.inp(desc, what='d_desc')
        gauss = ar.inp(g['d_gauss'], what='d_gauss')
        tc.call_maps(joints, first, dd, R, g, gauss, 2, heat, jout)
        ar.check()
        res[pat] = {k: v.clone() for k, v in (('heat', heat), ('joints', jout)) if v is not None}
    _agree(res)
    if 'joints' in res['Z']:
        assert torch.equal(res['Z']['joints'].cpu(), torch.from_numpy(g['jt_32']))


def test_target_masks_respects_its_buffers(g):
    R, N = 32, g['N']
    buf, rows = tc.mask_inputs(g, R)
    res = {}
    for pat in po.PATTERNS:
        ar = po.Arena(pat)
        out = ar.out((N, R, R), what='mask_out')
        src = ar.inp(tc.dev(buf), what='d_src')
        dd = ar.inp(tc.table(rows), what='d_desc')
        tc.call_masks(src, dd, R, out)
        ar.check()
        res[pat] = dict(mask=out.clone())
    _agree(res)
    assert torch.equal(res['Z']['mask'].cpu(), torch.from_numpy(g['mask_t_32']))


@pytest.mark.parametrize('terms', ['both', 'heat', 'tags'])
def test_pose_loss_respects_its_buffers(g, terms):
    R, N, J = 16, g['N'], int(g['J'])
    need = tc.loss_ws(N, J, R)
    assert need == N * J * 8
    res = {}
    for pat in po.PATTERNS:
        ar = po.Arena(pat)
        hl, push, pull = (ar.out((N,), what=w) for w in ('heat_loss_out', 'push_out', 'pull_out'))
        ws = ar.ws(need, align=8)
        out = ar.inp(tc.dev(g['out_16']), what='d_out')
        heat = ar.inp(tc.dev(g['heat_16']), what='d_heat') if terms != 'tags' else None
        mask = ar.inp(tc.dev(g['mask_t_16']), what='d_mask') if terms != 'tags' else None
        joints = ar.inp(tc.dev(g['jt_16']), what='d_joints') if terms != 'heat' else None
        off = J if terms == 'both' else (-1 if terms == 'heat' else 0)
        tc.call_loss(out, J, off, heat, mask, joints, 0, (1.0, 0.001, 0.001), hl, push, pull, ws, need)
        ar.check()
        got = {}
        if terms != 'tags':
            got['heat'] = hl.clone()
        else:                                              # a term that is off: its output and the workspace untouched
            assert (hl.view(torch.uint8) == po.pattern_byte(pat)).all() and (ws == po.pattern_byte(pat)).all()
        if terms != 'heat':
            got['push'], got['pull'] = push.clone(), pull.clone()
        else:
            assert (push.view(torch.uint8) == po.pattern_byte(pat)).all()
            assert (pull.view(torch.uint8) == po.pattern_byte(pat)).all()
        res[pat] = got
    _agree(res)
