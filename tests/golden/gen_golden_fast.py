#!/usr/bin/env python
"""Peak lists and person records of the REAL reference's real-time parser (nano_demo/fast_utils: find_peaks + assign).

Run in the build container only (needs the reference checkout and a host g++, like gen_golden.py):

    python tests/golden/gen_golden_fast.py

Compiles the reference's parse/find_peaks.cpp and parse/assign.cpp (plain C++, no torch) with the host compiler into a
temporary directory -- nothing compiled and none of its text is kept -- and calls ``find_peaks_out_nchw`` and ``assign_out``
through ctypes with zero-initialised outputs, as fast_utils/plugins.cpp:55-58,101-102 allocates them.  Every ``assign_out``
runs in a child process under a time limit: the reference's Kuhn-Munkres loop has no termination proof, and a scene it
does not finish is dropped.  The project's own restatement of assign (litepose_amd/csrc/fast_assign.h, built for the
host) is asserted against the reference on every scene with its round cap lifted; a scene for which the reference needs
more than the interface's 4096 match / update rounds in one joint is no scene either: only its peak lists and the
reference's records are kept, as c{i}_* (n_capped of them; no maps).  Stored per surviving scene ``i`` in tests/golden/golden_fast.npz:
  s{i}_det, s{i}_tmap   [N,J,H,W] float32 inputs (tmap = the first tag map, fast_utils/group.py:40)
  s{i}_thr              float32 [threshold, tag_threshold]
  s{i}_cfg              int32 [window, M, group]   (scenes of one group share shape and parameters: they stack to a batch)
  s{i}_order            int32 [J]  joint_order (fast_utils/group.py:25-31 truncated to J, as the reference's loop reads it)
  s{i}_count [N,J], s{i}_val / s{i}_tag [N,J,M], s{i}_ind [N,J,M,2]      find_peaks
  s{i}_ans [N,M,J,4], s{i}_num [N]                                       assign
Scene kinds (five per group): people from the first joint on; an empty first joint and people who appear at a later
joint; more people than M with plateaus of equal values (raster cut-off, num == M saturation); peaks in corners and on
borders, values exactly at and one ulp below the threshold, tag distances on both sides of tag_threshold; a quantised
noise plane (far more than M peaks, ties everywhere).  M <= 10 throughout: the reference's arrays are [10].
"""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
SRC = [os.path.join(REF, 'nano_demo/fast_utils/parse', f) for f in ('find_peaks.cpp', 'assign.cpp')]
TIME_LIMIT = 10.0
KINDS = ('plain', 'late', 'crowd', 'edges', 'noise')

ORDER17 = [i - 1 for i in [1, 2, 3, 4, 5, 6, 7, 12, 13, 8, 9, 10, 11, 14, 15, 16, 17]]
ORDER18 = [i - 1 for i in [18, 1, 2, 3, 4, 5, 6, 7, 12, 13, 8, 9, 10, 11, 14, 15, 16, 17]]

# (H, W, J, window, M, joint_order table, threshold, tag_threshold)
GROUPS = [
    (16, 16, 14, 3, 4, ORDER17, 0.1, 1.0),
    (16, 16, 17, 5, 10, ORDER17, 0.1, 1.0),
    (16, 16, 17, 3, 4, ORDER17, 0.2, 0.5),
    (16, 16, 14, 5, 10, ORDER17, 0.1, 1.0),
    (24, 40, 17, 3, 10, ORDER17, 0.1, 1.0),
    (24, 40, 14, 5, 4, ORDER17, 0.3, 2.0),
    (24, 40, 17, 5, 4, ORDER17, 0.1, 1.0),
    (24, 40, 14, 3, 10, ORDER17, 0.1, 0.5),
    (64, 64, 17, 5, 10, ORDER17, 0.1, 1.0),
    (64, 64, 14, 3, 4, ORDER17, 0.1, 1.0),
    (24, 40, 18, 3, 10, ORDER18, 0.1, 1.0),
]


def joint_order(table, J):
    """The first J entries of the table, as the reference's loop reads it (assign.cpp:76-77).  The 17-entry table
    truncated to 14 is a permutation of the 14 CrowdPose joints.  The 18-entry table (WITH_CENTER, centre joint first)
    names joint 17 in its first entry, so any truncation of it indexes past the planes of a 14- or 17-joint input: it is
    used whole, with J = 18, in a group of its own."""
    o = list(table[:J])
    assert sorted(o) == list(range(J)), (table, J)
    return np.array(o, np.int32)


def compile_reference(tmp):
    lib = os.path.join(tmp, 'libfastref.so')
    subprocess.check_call(['g++', '-O2', '-fPIC', '-shared', '-ffp-contract=off'] + SRC + ['-o', lib])
    names = subprocess.check_output(['nm', '-D', '--defined-only', lib], text=True).split()
    sym = {k: [n for n in names if k in n] for k in ('find_peaks_out_nchw', 'assign_out')}
    assert all(len(v) == 1 for v in sym.values()), sym
    dll = C.CDLL(lib)
    fp = getattr(dll, sym['find_peaks_out_nchw'][0])
    fp.restype = None
    fp.argtypes = [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_float, C.c_int]
    ao = getattr(dll, sym['assign_out'][0])
    ao.restype = None
    ao.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_float]
    return fp, ao


def compile_port(tmp, cap=None):
    """The project's own grouping routine (litepose_amd/csrc/fast_assign.h, the text the device kernel runs per lane) built
    for the host by tests/fast_assign_host.cpp; ``cap``: its round cap (default: the interface's 4096)."""
    lib = os.path.join(tmp, 'libfastport_%s.so' % cap)
    flags = ['-DLP_FAST_KM_ROUND_CAP=%d' % cap] if cap else []
    subprocess.check_call(['g++', '-O2', '-fPIC', '-shared', '-ffp-contract=off'] + flags +
                          [os.path.join(os.path.dirname(HERE), 'fast_assign_host.cpp'), '-o', lib])
    f = C.CDLL(lib).fast_assign_host
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_float, C.c_void_p]
    return f


def port_assign(f, count, val, tag, ind, order, M, tag_thr):
    N, J = count.shape
    ans = np.zeros((N, M, J, 4), np.float32)
    num = np.zeros((N,), np.int32)
    for n in range(N):
        num[n] = f(ptr(count[n]), ptr(val[n]), ptr(tag[n]), ptr(ind[n]), ptr(order), J, M, C.c_float(tag_thr), ptr(ans[n]))
    return ans, num


def ptr(a):
    assert a.flags['C_CONTIGUOUS']
    return a.ctypes.data_as(C.c_void_p)


def find_peaks(fp, det, tmap, thr, window, M):
    N, J, H, W = det.shape
    count = np.zeros((N, J), np.int32)
    val = np.zeros((N, J, M), np.float32)
    tag = np.zeros((N, J, M), np.float32)
    ind = np.zeros((N, J, M, 2), np.int32)
    fp(ptr(count), ptr(val), ptr(tag), ptr(ind), ptr(det), ptr(tmap), N, J, H, W, M, C.c_float(thr), window)
    return count, val, tag, ind


def _assign_child(conn, ao, count, val, tag, ind, order, M, tag_thr):
    N, J = count.shape
    ans = np.zeros((N, M, J, 4), np.float32)
    num = np.zeros((N,), np.int32)
    for n in range(N):
        one = np.zeros((1,), np.int32)
        ao(ptr(one), ptr(ans[n]), ptr(count[n]), ptr(val[n]), ptr(tag[n]), ptr(ind[n]), ptr(order), J, M,
           C.c_float(tag_thr))
        num[n] = one[0]
    conn.send((ans, num))
    conn.close()


def assign(ao, count, val, tag, ind, order, M, tag_thr):
    """(ans, num) of the reference, or None when it does not finish within TIME_LIMIT seconds."""
    ctx = mp.get_context('fork')
    a, b = ctx.Pipe(duplex=False)
    p = ctx.Process(target=_assign_child, args=(b, ao, count, val, tag, ind, order, M, tag_thr))
    p.start()
    b.close()
    out = a.recv() if a.poll(TIME_LIMIT) else None
    if out is None:
        p.kill()
    p.join()
    return out


def blob(det, j, y, x, v):
    H, W = det.shape[2:]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W:
                det[0, j, yy, xx] = max(det[0, j, yy, xx], np.float32(v) * np.float32(0.5))
    det[0, j, y, x] = v


def make_scene(rng, kind, H, W, J, window, M, order, thr, tag_thr):
    thr32 = np.float32(thr)
    det = np.zeros((1, J, H, W), np.float32)
    # background tags: a coarse field, so that a peak the scene did not plan still reads a defined, non-zero tag
    coarse = rng.integers(-8, 9, (1, J, (H + 7) // 8, (W + 7) // 8)).astype(np.float32) / 4
    tmap = np.ascontiguousarray(np.repeat(np.repeat(coarse, 8, 2), 8, 3)[:, :, :H, :W])
    if kind == 'noise':
        P = 5
        ptags = (np.arange(P) * 2.5 * tag_thr).astype(np.float32)
        R = min(H, 12)                                           # the noise band: the first rows (keeps the file small)
        shape = (1, J, R, W)
        det[:, :, :R] = rng.integers(0, 8, shape).astype(np.float32) * np.float32(thr * 0.25)
        tmap[:, :, :R] = ptags[rng.integers(0, P, shape)] + rng.integers(-2, 3, shape).astype(np.float32) * np.float32(tag_thr / 8)
        det[0, order[0]] = 0                                     # an empty first joint on top
        return det, tmap
    P = {'plain': int(rng.integers(1, M + 1)), 'late': min(M, 4), 'crowd': M + 3, 'edges': min(M, 6)}[kind]
    if kind == 'edges':                                          # neighbouring tags 0.9 / 1.1 thresholds apart
        gaps = np.where(np.arange(P) % 2 == 0, 0.9, 1.1) * tag_thr
        ptags = np.cumsum(gaps).astype(np.float32)
    else:
        ptags = ((np.arange(P) - P // 2) * 2.5 * tag_thr + rng.normal(0, 0.2 * tag_thr, P)).astype(np.float32)
    start = np.zeros(P, np.int64)
    empty = set()
    if kind == 'late':
        start = rng.integers(0, J // 2, P)
        start[0] = 1
        empty = {int(order[0]), int(order[J // 2]), int(order[J - 1])}
    border = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)]
    for idx in range(J):
        j = int(order[idx])
        if j in empty:
            continue
        for p in range(P):
            if idx < start[p] or rng.random() < (0.1 if kind == 'crowd' else 0.25):
                continue
            if kind == 'edges' and rng.random() < 0.6:
                y, x = border[int(rng.integers(0, len(border)))]
            else:
                y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            v = np.float32(rng.uniform(thr + 0.05, 1.0))
            if kind == 'edges':
                r = rng.random()
                v = thr32 if r < 0.25 else (np.nextafter(thr32, np.float32(0)) if r < 0.4 else v)
            blob(det, j, y, x, v)
            t = ptags[p] + np.float32(rng.normal(0, 0.05 * tag_thr))
            tmap[0, j, y, x] = t
            if kind == 'crowd' and rng.random() < 0.3:           # plateaus: every cell of equal value is a peak
                for dy, dx in ((0, 1), (1, 0), (1, 1)) if rng.random() < 0.5 else ((0, 1), (0, 2)):
                    yy, xx = y + dy, x + dx
                    if yy < H and xx < W:
                        det[0, j, yy, xx] = v
                        tmap[0, j, yy, xx] = t + np.float32(0.01 * (dy + 2 * dx))
    return det, tmap


def main():
    rng = np.random.default_rng(20240607)
    out, kept, dropped, capped = {}, 0, [], 0
    with tempfile.TemporaryDirectory() as tmp:
        fp, ao = compile_reference(tmp)
        port, port_nocap = compile_port(tmp), compile_port(tmp, 1 << 30)
        for g, (H, W, J, window, M, table, thr, tag_thr) in enumerate(GROUPS):
            assert M <= 10
            order = joint_order(table, J)
            for kind in KINDS:
                det, tmap = make_scene(rng, kind, H, W, J, window, M, order, thr, tag_thr)
                count, val, tag, ind = find_peaks(fp, det, tmap, thr, window, M)
                res = assign(ao, count, val, tag, ind, order, M, tag_thr)
                if res is None:
                    dropped.append((g, kind))
                    continue
                ans, num = res
                # the restatement, asserted against the reference on EVERY scene with its round cap lifted
                pa, pn = port_assign(port_nocap, count, val, tag, ind, order, M, tag_thr)
                assert np.array_equal(pn, num) and np.array_equal(pa.view(np.int32), ans.view(np.int32)), (g, kind)
                if (port_assign(port, count, val, tag, ind, order, M, tag_thr)[1] < 0).any():
                    # the reference needs more than the interface's 4096 rounds for some joint: not a scene (no scene may
                    # hit the cap); its peak lists are kept as a capped list -- the device must answer num = -1, ans = 0,
                    # and the host build without the cap must still give the reference's records
                    k = 'c%d_' % capped
                    out.update({k + 'thr': np.array([thr, tag_thr], np.float32), k + 'cfg': np.array([window, M, g], np.int32),
                                k + 'order': order, k + 'count': count, k + 'val': val, k + 'tag': tag, k + 'ind': ind,
                                k + 'ans': ans, k + 'num': num})
                    capped += 1
                    continue
                k = 's%d_' % kept
                out.update({k + 'det': det, k + 'tmap': tmap, k + 'thr': np.array([thr, tag_thr], np.float32),
                            k + 'cfg': np.array([window, M, g], np.int32), k + 'order': order, k + 'count': count,
                            k + 'val': val, k + 'tag': tag, k + 'ind': ind, k + 'ans': ans, k + 'num': num,
                            k + 'kind': np.array(KINDS.index(kind), np.int32)})
                kept += 1
    out['n_scenes'] = np.array(kept, np.int32)
    out['n_capped'] = np.array(capped, np.int32)
    print('scenes kept', kept, 'dropped (reference did not finish)', dropped, 'capped lists', capped)
    assert kept >= 40, kept
    S = range(kept)
    cfg = [out['s%d_cfg' % i] for i in S]
    # what the scenes must cover
    assert {tuple(out['s%d_det' % i].shape[2:]) for i in S} == {(16, 16), (24, 40), (64, 64)}
    assert {out['s%d_det' % i].shape[1] for i in S} == {14, 17, 18}
    assert {int(c[0]) for c in cfg} == {3, 5} and {int(c[1]) for c in cfg} == {4, 10}
    assert any((out['s%d_count' % i] == c[1]).any() for i, c in zip(S, cfg)), 'no plane reaches M peaks'
    assert any((out['s%d_num' % i] == c[1]).any() for i, c in zip(S, cfg)), 'no scene saturates num == M'
    assert any((out['s%d_count' % i] == 0).any() for i in S)
    assert any(out['s%d_count' % i][0, out['s%d_order' % i][0]] == 0 and out['s%d_num' % i][0] > 0 for i in S), \
        'no scene with an empty first joint and people'
    late = 0
    for i in S:                              # a person whose first joint in joint_order is not the scene's first
        a, o = out['s%d_ans' % i][0], out['s%d_order' % i]
        first = [next((idx for idx in range(len(o)) if a[p, o[idx], 2] != 0 or a[p, o[idx], 0] != 0), None)
                 for p in range(int(out['s%d_num' % i][0]))]
        late += len({f for f in first if f is not None}) > 1
    assert late >= 5, late
    assert all((out['s%d_num' % i] >= 0).all() for i in S)
    # the value cases, read from what the reference KEPT (a scene moved to the capped lists takes its cases with it)
    at_thr = plateau = corner = border = below = above = 0
    for i, c in zip(S, cfg):
        cnt, val, tag, ind = [out['s%d_%s' % (i, n)][0] for n in ('count', 'val', 'tag', 'ind')]
        thr32, tag_thr = out['s%d_thr' % i]
        H, W = out['s%d_det' % i].shape[2:]
        tags = []
        for j in range(cnt.shape[0]):
            k = int(cnt[j])
            v, xy = val[j, :k], ind[j, :k].astype(np.int64)
            tags.append(tag[j, :k])
            at_thr += int((v == thr32).sum())                    # kept although not above the threshold (the test is <)
            onx, ony = (xy[:, 0] == 0) | (xy[:, 0] == W - 1), (xy[:, 1] == 0) | (xy[:, 1] == H - 1)
            corner += int((onx & ony).sum())
            border += int((onx ^ ony).sum())
            for a in range(k):                                   # two neighbouring cells of one value, both peaks
                for b in range(a + 1, k):
                    plateau += int(v[a] == v[b] and np.abs(xy[a] - xy[b]).max() == 1)
        d = np.abs(np.subtract.outer(np.concatenate(tags), np.concatenate(tags)))
        below += int(((d > 0.5 * tag_thr) & (d < tag_thr)).sum())
        above += int(((d > tag_thr) & (d < 1.5 * tag_thr)).sum())
    print('kept peaks: at the threshold', at_thr, 'plateau pairs', plateau, 'corner', corner, 'border', border,
          'tag distances in (0.5, 1) / (1, 1.5) thresholds', below, above)
    assert at_thr >= 3 and plateau >= 10 and corner >= 4 and border >= 10 and below >= 20 and above >= 20
    path = os.path.join(HERE, 'golden_fast.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 512 * 1024


if __name__ == '__main__':
    main()
