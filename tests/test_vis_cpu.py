"""utils.vis without a GPU: the exported symbols, the link tables against the reference's (tests/golden/vis_tables.json,
written by tests/golden/gen_golden_vis.py), every host refusal of lp_draw_poses / lp_draw_poses_v with fake pointers that
are never dereferenced, and hand-computed pixel sets held against the NumPy restatement of the raster rule
(tests/_vis_ref.py) that the GPU tests use as their reference."""
import ctypes as C
import json
import os

import numpy as np

import _vis_ref as vr
from conftest import ROOT
from litepose_amd import _native as nv

INVALID, UNSUPPORTED = -1, -8


def test_symbols_are_exported():
    lib = nv.lib()
    for name in ('lp_draw_poses', 'lp_draw_poses_v', 'lp_draw_pass_prims'):
        assert name in nv.EXPORTS and hasattr(lib, name), name
    c = lib.lp_draw_pass_prims()
    assert c == 0 or 64 <= c <= 4096                         # 16-byte entries: the list stays far below 64 KB of LDS
    assert C.sizeof(nv.LpImageDesc) == 16


def test_link_tables_equal_the_fixture():
    from litepose_amd.utils import vis
    with open(os.path.join(ROOT, 'tests', 'golden', 'vis_tables.json')) as f:
        g = json.load(f)
    assert sorted(g) == sorted(vis.VIS_CONFIG) == ['COCO', 'CROWDPOSE']
    for ds, n_links in (('COCO', 19), ('CROWDPOSE', 15)):
        cfg = vis.VIS_CONFIG[ds]
        assert list(cfg['part_labels']) == g[ds]['part_labels']
        assert [list(p) for p in cfg['part_orders']] == g[ds]['part_orders']
        assert cfg['part_idx'] == {b: a for a, b in enumerate(g[ds]['part_labels'])}
        idx = cfg['part_idx']
        assert cfg['links'] == [(idx[a], idx[b]) for a, b in g[ds]['part_orders']] and len(cfg['links']) == n_links
        assert all(isinstance(v, int) for ab in cfg['links'] for v in ab)


def _args(**kw):
    """Valid arguments of lp_draw_poses with fake device pointers; keyword overrides."""
    fake = C.c_void_p(1 << 20)                               # never dereferenced: every call below is refused first
    a = dict(images=fake, N=2, H=40, W=56, kpts=fake, count=fake, pcap=3, J=17, D=3,
             links=(C.c_int32 * 4)(0, 1, 1, 40), n_links=2, palette=(C.c_uint8 * 6)(0, 0, 255, 9, 9, 9), n_colors=2,
             Rj=2, Rl=1)
    a.update(kw)
    return a


def _plain(**kw):
    a = _args(**kw)
    return nv.lib().lp_draw_poses(a['images'], a['N'], a['H'], a['W'], a['kpts'], a['count'], a['pcap'], a['J'], a['D'],
                                  a['links'], a['n_links'], a['palette'], a['n_colors'], a['Rj'], a['Rl'], None)


def _packed(desc=C.c_void_p(1 << 20), nbytes=1 << 16, **kw):
    a = _args(**kw)
    return nv.lib().lp_draw_poses_v(a['images'], nbytes, desc, a['N'], a['kpts'], a['count'], a['pcap'], a['J'],
                                    a['D'], a['links'], a['n_links'], a['palette'], a['n_colors'], a['Rj'], a['Rl'], None)


def test_draw_abi_refusals():
    lib = nv.lib()
    no_links = C.POINTER(C.c_int32)()
    no_pal = C.POINTER(C.c_uint8)()
    for call in (_plain, _packed):
        for name in ('images', 'kpts', 'count'):
            assert call(**{name: None}) == INVALID and b'null' in lib.lp_last_error(), name
        assert call(links=no_links) == INVALID and call(palette=no_pal) == INVALID
        assert call(links=no_links, n_links=0) == INVALID        # a null table is refused even when it is empty
        for n in (0, -1):
            assert call(N=n) == INVALID and b'N must be positive' in lib.lp_last_error()
        for pcap in (0, -3):
            assert call(pcap=pcap) == INVALID and b'pcap' in lib.lp_last_error()
        for J in (0, 33, -1):
            assert call(J=J) == UNSUPPORTED and b'J must be 1..32' in lib.lp_last_error()
        for D in (2, 0, -1):
            assert call(D=D) == INVALID and b'D must be >= 3' in lib.lp_last_error()
        for n_links in (-1, 65):
            assert call(n_links=n_links) == UNSUPPORTED and b'n_links' in lib.lp_last_error()
        assert call(links=(C.c_int32 * 4)(0, 1, -1, 2)) == INVALID and b'link index' in lib.lp_last_error()
        assert call(links=(C.c_int32 * 4)(0, 1, 2, -7)) == INVALID
        for n_colors in (0, 33, -1):
            assert call(n_colors=n_colors) == UNSUPPORTED and b'n_colors' in lib.lp_last_error()
        for r in (-1, 9):
            assert call(Rj=r) == UNSUPPORTED and b'0..8' in lib.lp_last_error()
            assert call(Rl=r) == UNSUPPORTED and b'0..8' in lib.lp_last_error()
    for hw in (0, -1, 16385):
        assert _plain(H=hw) == INVALID and b'1..16384' in lib.lp_last_error()
        assert _plain(W=hw) == INVALID and b'1..16384' in lib.lp_last_error()
    assert _packed(desc=None) == INVALID and b'null' in lib.lp_last_error()
    assert _packed(nbytes=0) == INVALID and b'image_bytes' in lib.lp_last_error()


def _pixels(mask):
    return sorted((int(x), int(y)) for y, x in zip(*np.nonzero(mask)))


DISC2 = sorted((x, y) for x in range(-2, 3) for y in range(-2, 3) if x * x + y * y <= 4)


def test_hand_computed_discs():
    assert len(DISC2) == 13 and (2, 0) in DISC2 and (1, 1) in DISC2 and (2, 1) not in DISC2
    assert _pixels(vr.disc_mask(9, 11, (5, 4), 2)) == sorted((5 + x, 4 + y) for x, y in DISC2)
    assert _pixels(vr.disc_mask(9, 11, (5, 4), 1)) == [(4, 4), (5, 3), (5, 4), (5, 5), (6, 4)]
    assert _pixels(vr.disc_mask(9, 11, (5, 4), 0)) == [(5, 4)]
    # clipped at the corner: the quarter of the disc that lies inside
    assert _pixels(vr.disc_mask(9, 11, (0, 0), 2)) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)]


def test_hand_computed_capsules():
    # (2,2)-(5,2), radius 1: the rows y = 1 and y = 3 over x = 2..5, the row y = 2 over x = 1..6
    want = sorted([(x, y) for y in (1, 3) for x in range(2, 6)] + [(x, 2) for x in range(1, 7)])
    assert len(want) == 14
    assert _pixels(vr.capsule_mask(6, 9, (2, 2), (5, 2), 1)) == want
    assert _pixels(vr.capsule_mask(6, 9, (5, 2), (2, 2), 1)) == want
    # A == B is the disc of the link's radius
    for R in (0, 1, 2, 3):
        assert np.array_equal(vr.capsule_mask(12, 12, (6, 5), (6, 5), R), vr.disc_mask(12, 12, (6, 5), R))
    # a diagonal: (1,1)-(4,4), radius 1: the pixels at most 1 from the segment -- |x - y| <= 1 between the end caps
    diag = sorted((x, y) for x in range(0, 6) for y in range(0, 6) if abs(x - y) <= 1 and 2 <= x + y <= 8
                  or (x, y) in ((1, 0), (0, 1), (5, 4), (4, 5)))
    assert _pixels(vr.capsule_mask(7, 7, (1, 1), (4, 4), 1)) == diag


def test_truncation_and_visibility():
    assert vr.joint_pos([-0.5, 3.9, 1.0]) == (0, 3)
    assert vr.joint_pos([-1.5, -0.999, 0.1]) == (-1, 0)
    assert vr.joint_pos([16383.9, -16384.5, 1.0]) == (16383, -16384)
    for bad in ([16384.0, 0, 1], [0, -16385.0, 1], [float('nan'), 0, 1], [0, float('inf'), 1], [1e9, 0, 1],
                [3, 3, 0.0], [3, 3, -1.0], [3, 3, float('nan')]):
        assert vr.joint_pos(bad) is None, bad
    # one person, joints 0 and 1 linked, joint 2 invisible: its mark and its link are missing
    person = np.array([[2.9, 2.2, 1.0], [5.1, 2.0, 0.5], [8.0, 8.0, 0.0]], np.float32)
    m = vr.person_mask(12, 12, person, [(0, 1), (1, 2), (0, 7)])
    want = vr.disc_mask(12, 12, (2, 2), 2) | vr.disc_mask(12, 12, (5, 2), 2) | vr.capsule_mask(12, 12, (2, 2), (5, 2), 1)
    assert np.array_equal(m, want) and not m[6:].any()


def test_draw_paints_in_person_order_and_counts():
    img = np.full((10, 10, 3), 7, np.uint8)
    k = np.zeros((3, 1, 3), np.float32)
    k[:, 0] = [[4, 4, 1], [5, 4, 1], [20, 20, 1]]
    pal = [(1, 2, 3), (4, 5, 6)]
    out, mask = vr.draw(img, k, 2, [], pal)
    assert tuple(out[4, 5]) == (4, 5, 6) and tuple(out[4, 2]) == (1, 2, 3) and tuple(out[4, 7]) == (4, 5, 6)
    assert mask.sum() == 13 + 13 - 8 and (out[~mask] == 7).all() and (img == 7).all()
    for cnt in (0, -1):
        out, mask = vr.draw(img, k, cnt, [], pal)
        assert not mask.any() and np.array_equal(out, img)
    out5, _ = vr.draw(img, k, 8, [], pal)                    # clamped to pcap = 3; person 2 lies outside the image
    assert np.array_equal(out5, vr.draw(img, k, 3, [], pal)[0]) and np.array_equal(out5, vr.draw(img, k, 2, [], pal)[0])
