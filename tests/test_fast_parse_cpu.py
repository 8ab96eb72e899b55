"""The fast parser (lp_fast_peaks / lp_fast_assign / lp_fast_parse: the reference's nano_demo/fast_utils) without a GPU:
the exports, every refusal before a pointer is dereferenced, the goldens of tests/golden/gen_golden_fast.py, and the
grouping routine itself -- litepose_amd/csrc/fast_assign.h, the text the device kernel runs per lane, built for the host
(tests/fast_assign_host.cpp) and compared bitwise with the reference's records."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_fast.npz')
NAMES = ('lp_fast_peaks', 'lp_fast_assign', 'lp_fast_parse_workspace_bytes', 'lp_fast_parse')
INVALID, WORKSPACE, UNSUPPORTED = -1, -6, -8


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _lib():
    from litepose_amd import _native as nv
    return nv.lib()


def test_library_exports_the_fast_parser():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), 'missing export ' + name


def _order(vals):
    return (C.c_int32 * len(vals))(*vals)


def test_refusals_come_before_any_pointer_is_dereferenced():
    lib = _lib()
    fake = C.c_void_p(1 << 20)                  # never dereferenced: every call below is refused first
    J, M = 14, 4
    good = _order(range(J))

    def peaks(det=fake, tmap=fake, stride=1, N=1, J=J, H=16, W=16, window=3, M=M, outs=(fake, fake, fake, fake)):
        return lib.lp_fast_peaks(det, tmap, stride, N, J, H, W, 0.1, window, M, outs[0], outs[1], outs[2], outs[3], None)

    def assign(ins=(fake, fake, fake, fake), N=1, J=J, M=M, order=good, ans=fake, num=fake):
        return lib.lp_fast_assign(ins[0], ins[1], ins[2], ins[3], N, J, M, order, 1.0, ans, num, None)

    def parse(det=fake, tmap=fake, stride=1, N=1, J=J, H=16, W=16, window=3, M=M, order=good, ans=fake, num=fake,
              ws=fake, ws_bytes=1 << 30):
        return lib.lp_fast_parse(det, tmap, stride, N, J, H, W, 0.1, window, M, order, 1.0, ans, num, ws, ws_bytes, None)

    for call in (peaks, parse):
        for bad in (0, 11, -1):
            assert call(M=bad) == UNSUPPORTED, bad
        assert b'[10]' in lib.lp_last_error()
        for bad in (0, 33):
            assert call(J=bad) == UNSUPPORTED, bad
        for bad in (4, 9, 0, 2, -3):
            assert call(window=bad) == UNSUPPORTED, bad
        assert call(W=1025) == UNSUPPORTED
        assert call(N=0) == INVALID and call(N=-2) == INVALID
        assert call(H=0) == INVALID and call(W=0) == INVALID and call(stride=0) == INVALID
        assert call(det=None) == INVALID and call(tmap=None) == INVALID
    for k in range(4):
        assert peaks(outs=tuple(None if i == k else fake for i in range(4))) == INVALID
        assert assign(ins=tuple(None if i == k else fake for i in range(4))) == INVALID
    for call in (assign, parse):
        assert call(M=11) == UNSUPPORTED and call(M=0) == UNSUPPORTED and call(J=33) == UNSUPPORTED
        assert call(N=0) == INVALID
        assert call(order=None) == INVALID and call(ans=None) == INVALID and call(num=None) == INVALID
        assert call(order=_order([0] + list(range(J - 1)))) == INVALID            # 0 twice
        assert b'repeated' in lib.lp_last_error()
        assert call(order=_order(list(range(J - 1)) + [J])) == INVALID            # J itself
        assert call(order=_order([-1] + list(range(1, J)))) == INVALID
    need = lib.lp_fast_parse_workspace_bytes(1, J, M)
    assert need > 0 and need % 256 == 0 and need >= 4 * J * (1 + 4 * M)
    assert lib.lp_fast_parse_workspace_bytes(0, J, M) == 0
    assert lib.lp_fast_parse_workspace_bytes(64, 17, 10) > lib.lp_fast_parse_workspace_bytes(1, 17, 10)
    assert parse(ws=None) == INVALID
    assert parse(ws_bytes=need - 1) == WORKSPACE
    assert parse(ws=C.c_void_p((1 << 20) + 2)) == WORKSPACE


def test_goldens_hold_what_the_gpu_tests_need(golden):
    n = int(golden['n_scenes'])
    assert n >= 40
    shapes, joints, windows, people = set(), set(), set(), set()
    for i in range(n):
        k = 's%d_' % i
        det, tmap = golden[k + 'det'], golden[k + 'tmap']
        N, J, H, W = det.shape
        window, M, _ = [int(v) for v in golden[k + 'cfg']]
        assert det.dtype == tmap.dtype == np.float32 and tmap.shape == det.shape
        assert 1 <= M <= 10, (i, M)                               # beyond [10] the reference is undefined
        assert (golden[k + 'num'] >= 0).all(), i                  # no scene hits the round cap
        assert (golden[k + 'num'] <= M).all() and (golden[k + 'count'] <= M).all()
        assert golden[k + 'count'].shape == (N, J) and golden[k + 'ind'].shape == (N, J, M, 2)
        assert golden[k + 'ans'].shape == (N, M, J, 4) and golden[k + 'num'].shape == (N,)
        assert sorted(golden[k + 'order'].tolist()) == list(range(J))
        shapes.add((H, W)), joints.add(J), windows.add(window), people.add(M)
    assert shapes == {(16, 16), (24, 40), (64, 64)} and joints >= {14, 17} and windows == {3, 5} and people == {4, 10}
    assert int(golden['n_capped']) >= 1


def test_torch_restatement_of_find_peaks_matches_the_reference_bitwise(golden):
    """tests/_fast_ref.find_peaks, the oracle of tests/test_gpu_fast_parse.py for planes wider than 64 columns or taller
    than one LDS band (the goldens stop at 64x64), against the real reference on every golden scene."""
    import _fast_ref as fr
    for i in range(int(golden['n_scenes'])):
        k = 's%d_' % i
        window, M, _ = [int(v) for v in golden[k + 'cfg']]
        got = fr.find_peaks(golden[k + 'det'], golden[k + 'tmap'], golden[k + 'thr'][0], window, M)
        for a, name in zip(got, ('count', 'val', 'tag', 'ind')):
            want = golden[k + name]
            assert a.dtype == want.dtype and a.shape == want.shape, (i, name)
            assert np.array_equal(a.view(np.int32), want.view(np.int32)), (i, name)


@pytest.fixture(scope='module')
def host_port(tmp_path_factory):
    """fast_assign.h built for the host: with the interface's round cap, and with the cap lifted."""
    out = {}
    for name, flags in (('cap', []), ('nocap', ['-DLP_FAST_KM_ROUND_CAP=%d' % (1 << 30)])):
        so = str(tmp_path_factory.mktemp('fast') / ('libfast_%s.so' % name))
        r = subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + flags +
                           [os.path.join(ROOT, 'tests', 'fast_assign_host.cpp'), '-o', so],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        f = C.CDLL(so).fast_assign_host
        f.restype = C.c_int
        f.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_float, C.c_void_p]
        out[name] = f
    return out


def _run_port(f, golden, k, n=0):
    cnt, val, tag, ind, order = [np.ascontiguousarray(golden[k + x]) for x in ('count', 'val', 'tag', 'ind', 'order')]
    M = int(golden[k + 'cfg'][1])
    J = cnt.shape[1]
    ans = np.full((M, J, 4), 7.0, np.float32)                     # the routine zeroes its record itself
    num = f(cnt[n].ctypes.data, val[n].ctypes.data, tag[n].ctypes.data, ind[n].ctypes.data, order.ctypes.data, J, M,
            C.c_float(float(golden[k + 'thr'][1])), ans.ctypes.data)
    return num, ans


def test_host_build_of_the_grouping_routine_matches_the_reference_bitwise(golden, host_port):
    for i in range(int(golden['n_scenes'])):
        k = 's%d_' % i
        for n in range(golden[k + 'num'].shape[0]):
            num, ans = _run_port(host_port['cap'], golden, k, n)
            assert num == int(golden[k + 'num'][n]), i
            assert np.array_equal(ans.view(np.int32), golden[k + 'ans'][n].view(np.int32)), i


def test_round_cap_answers_minus_one_and_the_uncapped_routine_still_matches(golden, host_port):
    """Peak lists for which the reference needs more than 4096 match / update rounds in one joint: the routine answers
    num = -1 with an all-zero record; with the cap lifted it reproduces the reference's records."""
    for i in range(int(golden['n_capped'])):
        k = 'c%d_' % i
        num, ans = _run_port(host_port['cap'], golden, k)
        assert num == -1 and not ans.view(np.int32).any(), i
        num, ans = _run_port(host_port['nocap'], golden, k)
        assert num == int(golden[k + 'num'][0]) and num >= 0, i
        assert np.array_equal(ans.view(np.int32), golden[k + 'ans'][0].view(np.int32)), i


def test_params_refuse_more_than_ten_people():
    from litepose_amd import config
    from litepose_amd.fast_utils import group
    cfg = config.get_cfg('crowd_pose')
    cfg.DATASET.MAX_NUM_PEOPLE = 10
    p = group.Params(cfg)
    assert p.max_num_people == 10 and p.num_joints == 14 and p.window_size == cfg.TEST.NMS_KERNEL
    assert p.joint_order[:14] == [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13]
    cfg.DATASET.MAX_NUM_PEOPLE = 30
    with pytest.raises(NotImplementedError, match=r'\[10\]'):
        group.Params(cfg)
    with pytest.raises(NotImplementedError, match=r'\[10\]'):
        group.HeatmapParser(cfg)
