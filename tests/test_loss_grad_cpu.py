"""The gradient of the training loss without a GPU: the numpy restatement tests/_loss_grad_ref.py against the values stored
in tests/golden/golden_loss_grad.npz (tests/golden/gen_golden_loss_grad.py: autograd through the real lib/core/loss.py),
against central differences of the loss restatement tests/_loss_ref.py, and its support; the refusals of
lp_pose_loss_grad with dummy pointers (a refusal precedes any dereference and any launch)."""
import ctypes as C
import os

import numpy as np
import pytest

import _loss_grad_case as GC
import _loss_grad_ref as GR
import _loss_ref as LR

U = 2.0 ** -24               # unit roundoff of fp32
E = 2.0 ** -53               # unit roundoff of fp64


@pytest.fixture(scope='module')
def case():
    return GC.load()


def _stored(g, c, lt, s, which):
    """(heat part or None, tag part or None) of the stored gradient of (configuration, loss type, stage)."""
    return g.get('gheat%d_%d_%s' % (c, s, which)), g.get('gtag%d_%s_%d_%s' % (c, lt, s, which))


def _restated(b, g, c, lt, s):
    out, J, off, heat, mask, jts = GC.stage(b, c, s)
    hg = tg = None
    if heat is not None:
        hg = np.stack([GR.heat_grad(out[n, :J], heat[n], mask[n], GC.FACTORS[0], g['w_heat'][n]) for n in range(GC.N)])
    if off >= 0:
        tg = np.stack([GR.tag_grad(out[n, off:], jts[n], lt, GC.FACTORS[1], GC.FACTORS[2], g['w_push'][n], g['w_pull'][n])
                       for n in range(GC.N)])
    return hg, tg


def test_fixture_holds_what_the_tests_need(case):
    b, g = case
    assert os.path.getsize(GC.GOLDEN) < (1 << 20)
    for w in ('w_heat', 'w_push', 'w_pull'):
        assert g[w].dtype == np.float32 and len(set(g[w].tolist())) == GC.N and (g[w] == 0).sum() == 1
    people = [int((b['jt_16'][n, :, :, 1].sum(1) > 0).sum()) for n in range(GC.N)]
    assert people[:3] == [0, 1, 2] and people[3] >= 3 and people[4] >= 3      # persons with a joint inside the plane
    for R in GC.OUTS:
        pa, pb = g['x_shared_%d' % R]
        jt = b['jt_%d' % R][4]
        assert pa != pb and jt[pa, 0, 0] == jt[pb, 0, 0] and jt[pa, 0, 1] == 1 and jt[pb, 0, 1] == 1
    for c in range(2):
        for s in range(2):
            out, J, off, heat, mask, jts = GC.stage(b, c, s)
            if off >= 0:
                for n in range(GC.N):                # away from the kinks of 'max'
                    assert all(gap >= 1e-3 and abs(gap - 1.0) >= 1e-3 for gap in GR.push_gaps(out[n, off:], jts[n]))


@pytest.mark.parametrize('lt', ['exp', 'max'])
@pytest.mark.parametrize('c', [0, 1])
def test_restatement_equals_the_stored_values(case, c, lt):
    """heat_grad / tag_grad recomputed from the inputs: the stored fp64 values (1e-15 relative: another machine's exp)."""
    b, g = case
    seen = 0
    for s in range(2):
        for got, want in zip(_restated(b, g, c, lt, s), _stored(g, c, lt, s, 'f64')):
            assert (got is None) == (want is None)
            if got is not None:
                assert got.shape == want.shape and want.dtype == np.float64
                assert (np.abs(got - want) <= 1e-15 * np.abs(want)).all()
                seen += got.size
    assert seen == (5 * (5 * 256 + 5 * 1024 + 5 * 256), 5 * (10 * 256 + 5 * 1024 + 5 * 1024))[c]


def _ref_bounds(out, J, off, jts, n, g, lt):
    """Bounds on |autograd's fp32 gradient - exact gradient| from the arithmetic of loss.py and of its backward, U the fp32
    unit roundoff.

    heat (relative): backward of ``((p - g)^2 * m).mean(3).mean(2).mean(1) * factor * w`` -- w and the factor 1.0 are exact;
        each mean's backward is a division, or a product with a rounded reciprocal: two roundings at most, three times;
        the product with m; the difference p - g; the product 2 (p - g) * upstream.  Nine roundings: 9 U (1 + 9 U).

    tags (absolute, per cell), T = the largest |tag| of the image, P its persons, cnt >= 1 the joints of a person:
        a mean carries (J + 1) U T from its sum and division, a deviation t - mu one rounding of a value <= 2 T more:
        |err(t - mu)| <= (J + 3) U T.  The pull slope is A * 2 (t - mu) with A = |w_pull * factor| / (cnt * P) <= A1 (cnt = 1):
        the deviation's error, the path through mu -- analytically sum_k (t_k - mu) = 0, in fp32 a residual of at most
        (J + 3) U T per term plus (J - 1) U 2 T of summation, handed to every slot -- and eight roundings of the chain
        (factor, 1 / P, 1 / cnt, vis, the square's backward, the sums' expansions) on a value <= 4 A1 T:
        pull_err <= A1 U T (2 (J + 3) + 2 (3 J + 1) + 32).
        The push slope is B * 2 D_p / cnt, B = |w_push * factor| * 0.5 / den.  D_p sums P values f'(d): for 'exp' |f''| <= 2,
        so the error 2 (J + 3) U T of a difference of two means moves f' by at most 4 (J + 3) U T, plus five roundings of a
        value <= 0.86 (the square, the negation is free, exp's 2 U, the product with -2 d, the mask): e_f = 4 (J + 3) U T + 5 U;
        for 'max' f' is exactly -+1 or 0 away from the kinks, which the fixture keeps 1e-3 away: e_f = 0.  The sum of P terms
        adds P U per term, the chain to the slot six roundings of a value <= 2 B P:
        push_err <= 2 B (P e_f + P^2 U + 6 P U).
        A cell named by K slots adds their bounds and K - 1 roundings of the accumulated value."""
    heat_rel = 9 * U * (1 + 9 * U)
    if off < 0:
        return heat_rel, 0.0
    T = float(np.abs(out[n, off:]).max())
    vis = [[int(i) for i, v in person if v > 0] for person in jts[n]]
    P = sum(1 for v in vis if v)
    cells = [i for v in vis for i in v]
    K = max([cells.count(i) for i in cells] or [1])
    pc = max(P, 1)
    den = max((pc - 1) * pc, 1)
    A1 = abs(float(g['w_pull'][n])) * float(np.float32(GC.FACTORS[2])) / pc
    B = abs(float(g['w_push'][n])) * float(np.float32(GC.FACTORS[1])) * 0.5 / den if P >= 2 else 0.0
    e_f = 4 * (J + 3) * U * T + 5 * U if lt == 'exp' else 0.0
    pull_err = A1 * U * T * (2 * (J + 3) + 2 * (3 * J + 1) + 32)
    push_err = 2 * B * (P * e_f + P * P * U + 6 * P * U)
    value = 4 * A1 * T + 2 * B * P
    return heat_rel, K * (pull_err + push_err) + (K - 1) * U * K * value


@pytest.mark.parametrize('lt', ['exp', 'max'])
@pytest.mark.parametrize('c', [0, 1])
def test_restatement_lies_within_the_reference_error(case, c, lt):
    """|autograd through the real loss.py (fp32) - restatement| <= the reference's own error (``_ref_bounds``) plus the
    rounding of the stored fp32 value; where the restatement is exactly zero (outside the support, a zero weight, a masked
    pixel) the reference is zero too."""
    b, g = case
    seen = 0
    for s in range(2):
        out, J, off, heat, mask, jts = GC.stage(b, c, s)
        rh, rt = _stored(g, c, lt, s, 'ref')
        fh, ft = _restated(b, g, c, lt, s)
        for n in range(GC.N):
            heat_rel, tag_abs = _ref_bounds(out, J, off, jts, n, g, lt)
            if fh is not None:
                err = np.abs(rh[n].astype(np.float64) - fh[n])
                print('cfg %d %s stage %d image %d heat: worst %.3g of the bound' % (
                    c, lt, s, n, float((err / np.maximum((heat_rel + U) * np.abs(fh[n]), 1e-300)).max())))
                assert (err <= (heat_rel + U) * np.abs(fh[n])).all(), (s, n)
                seen += int((fh[n] != 0).sum())
            if ft is not None:
                err = np.abs(rt[n].astype(np.float64) - ft[n])
                print('cfg %d %s stage %d image %d tags: worst %.3g, bound %.3g' % (c, lt, s, n, float(err.max()), tag_abs))
                assert (err <= tag_abs + U * np.abs(ft[n])).all(), (s, n, float(err.max()), tag_abs)
                assert not rt[n][ft[n] == 0].any()
                seen += int((ft[n] != 0).sum())
    assert seen > 5000


@pytest.mark.parametrize('lt', ['exp', 'max'])
def test_restatement_agrees_with_central_differences(case, lt):
    """(L(x + h) - L(x - h)) / 2h of _loss_ref.heat_loss / tag_loss in fp64, L the weighted loss of one image, x one element.

    heat: L is quadratic in x, so the truncation is zero; an evaluation sums n = J R R rounded terms, |L| n E bounds its
    rounding, the quotient carries 2 |L| n E / 2h.  h = 2^-10.  A seeded sample of 48 elements per image and stage.
    tags: pull is quadratic; push moves through a person's mean by h / cnt, 'exp' has |f'''| <= 8 and den >= P (P - 1), so the
    third derivative of L is at most 16 |w_push * factor| (two persons may move on a shared cell) and the truncation
    h^2 / 6 * 16 |w_push * factor|; 'max' is piecewise linear and no pair comes within 1e-3 > h of a kink: truncation zero.
    An evaluation has at most ops = M J + M^2 + 8 rounded operations on terms that sum to at most
    S = |w_pull * factor| (2 T)^2 + |w_push * factor| (P + 1): rounding 2 ops E S / 2h.  h = 2^-14.  Every cell a counting slot
    names, and eight others per image, which must give exactly zero on both sides."""
    b, g = case
    rng = np.random.RandomState(5)
    seen = 0
    for c in range(2):
        for s in range(2):
            out, J, off, heat, mask, jts = GC.stage(b, c, s)
            fh, ft = _restated(b, g, c, lt, s)
            for n in range(GC.N):
                if heat is not None and lt == 'exp':
                    h = 2.0 ** -10
                    w = float(g['w_heat'][n])
                    x = out[n, :J].astype(np.float64)
                    tol = abs(w) * LR.heat_loss(x, heat[n], mask[n], GC.FACTORS[0]) * x.size * E / h
                    for i in rng.choice(x.size, 48, replace=False):
                        lo, hi = x.copy(), x.copy()
                        lo.reshape(-1)[i] -= h
                        hi.reshape(-1)[i] += h
                        cd = w * (LR.heat_loss(hi, heat[n], mask[n], GC.FACTORS[0]) -
                                  LR.heat_loss(lo, heat[n], mask[n], GC.FACTORS[0])) / (2 * h)
                        assert abs(cd - fh[n].reshape(-1)[i]) <= tol, (c, s, n, i, cd, fh[n].reshape(-1)[i], tol)
                        seen += 1
                if off >= 0:
                    h = 2.0 ** -14
                    wpu, wpl = float(g['w_push'][n]), float(g['w_pull'][n])
                    x = out[n, off:].astype(np.float64)
                    M = jts.shape[1]
                    T = float(np.abs(x).max())
                    named = sorted({int(i) for person in jts[n] for i, v in person if v > 0})
                    P = sum(1 for person in jts[n] if (person[:, 1] > 0).any())
                    kf = float(np.float32(GC.FACTORS[1]))
                    S = abs(wpl) * kf * (2 * T) ** 2 + abs(wpu) * kf * (P + 1)
                    tol = (h * h / 6 * 16 * abs(wpu) * kf if lt == 'exp' else 0.0) + (M * J + M * M + 8) * E * S / h
                    others = [int(i) for i in rng.choice(x.size, 8, replace=False) if int(i) not in named]
                    for i in named + others:
                        lo, hi = x.copy(), x.copy()
                        lo.reshape(-1)[i] -= h
                        hi.reshape(-1)[i] += h
                        a = LR.tag_loss(hi, jts[n], lt, GC.FACTORS[1], GC.FACTORS[2])
                        z = LR.tag_loss(lo, jts[n], lt, GC.FACTORS[1], GC.FACTORS[2])
                        cd = (wpu * (a[0] - z[0]) + wpl * (a[1] - z[1])) / (2 * h)
                        f = ft[n].reshape(-1)[i]
                        if i in named:
                            assert abs(cd - f) <= tol, (c, s, n, i, cd, f, tol)
                        else:
                            assert cd == 0 and f == 0
                        seen += 1
    assert seen > 100


def test_exactly_zero_outside_the_support(case):
    """Tag cells no counting slot names, an image without persons, an upstream that is None or zero, masked pixels."""
    b, g = case
    out, J, off, heat, mask, jts = GC.stage(b, 0, 0)
    for lt in ('exp', 'max'):
        for n in range(GC.N):
            t = GR.tag_grad(out[n, off:], jts[n], lt, 0.001, 0.001, g['w_push'][n], g['w_pull'][n])
            named = {int(i) for person in jts[n] for i, v in person if v > 0}
            flat = t.reshape(-1)
            assert not np.delete(flat, sorted(named)).any() and t.shape == out[n, off:].shape
            if n == 0:
                assert not named and not t.any()
            assert not GR.tag_grad(out[n, off:], jts[n], lt, 0.001, 0.001, None, None).any()
    h = GR.heat_grad(out[1, :J], heat[1], mask[1], 1.0, 1.5)
    assert (mask[1] == 0).any() and not h[:, mask[1] == 0].any() and h[:, mask[1] != 0].any()
    assert not GR.heat_grad(out[1, :J], heat[1], mask[1], 1.0, 0.0).any()
    # a push weight alone moves nothing below two persons; with two persons the push slopes of one pair cancel in the sum
    assert not GR.tag_grad(out[1, off:], jts[1], 'exp', 0.001, 0.001, 1.0, None).any()
    two = GR.tag_grad(out[2, off:], jts[2], 'exp', 0.001, 0.001, 1.0, None)
    assert two.any()


# ------------------------------------------------------------------ the C ABI without a device
OK, INVALID, UNSUPPORTED = 0, -1, -8
P = C.c_void_p(0x1000)        # a dummy device pointer: never dereferenced, every case below is refused before any launch


def _grad(**kw):
    from litepose_amd import _native as nv
    a = dict(out=P, N=2, C=10, R=16, J=5, off=5, heat=P, mask=P, joints=P, M=4, lt=0, gh=P, gpu=P, gpl=P, grad=P)
    a.update(kw)
    return nv.lib().lp_pose_loss_grad(a['out'], a['N'], a['C'], a['R'], a['J'], a['off'], a['heat'], a['mask'], a['joints'],
                                      a['M'], a['lt'], 1.0, 1.0, 1.0, a['gh'], a['gpu'], a['gpl'], a['grad'], None)


@pytest.mark.parametrize('kw, code', [
    (dict(J=0), UNSUPPORTED), (dict(J=33), UNSUPPORTED), (dict(R=0), UNSUPPORTED), (dict(R=1025), UNSUPPORTED),
    (dict(M=0), UNSUPPORTED), (dict(M=65), UNSUPPORTED), (dict(lt=2), UNSUPPORTED), (dict(lt=-1), UNSUPPORTED),
    (dict(out=None), INVALID), (dict(grad=None), INVALID), (dict(heat=None, off=-1), INVALID), (dict(mask=None), INVALID),
    (dict(joints=None), INVALID), (dict(N=0), INVALID), (dict(C=0), INVALID), (dict(C=4), INVALID), (dict(off=10), INVALID),
    (dict(off=4), INVALID), (dict(off=0), INVALID),            # the tag channels would overlap the heatmap channels
])
def test_pose_loss_grad_refusals(kw, code):
    from litepose_amd import _native as nv
    assert 'lp_pose_loss_grad' in nv.EXPORTS
    assert _grad(**kw) == code, (kw, nv.lib().lp_last_error())
    assert nv.lib().lp_last_error()
