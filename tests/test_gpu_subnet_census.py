"""Census of the supernet's sub-network space on the device: the rows of tests/_subnet_space.py (sixteen trunk rows that
hold every block, head and stem shape ``ArchManager.random_sample()`` can draw, forty-eight more that complete all 192
deconv triples, and sixty-four second-size rows that run every vector in the other plane class) against the oracle,
with synthetic weights (oracle.synth.make_state_dict).

Tests: every row in fp32 (check_fp32: all block taps and both outputs, every image and the mirrored half); every row in
bf16 and the trunk rows plus sixteen deconv rows in f16 (check_bf16 / check_f16, their own criteria); both sides of the
batch gate, and the form an option selects, on shapes no published architecture has; batched == per-image and flip
modes, bitwise; closure of the launch keys of 32 real draws over the rows; BatchNorm calibration on the two extreme
architectures.  Every row test prints its tags, its worst fraction of the bound and its wall time.

Measured on an MI355X, every test passing.  Columns: input size, N, flip; the worst fp32 block tap and the worst fp32
output as fractions of TAP_REL / NET_ATOL; the worst bf16 and f16 criterion as a fraction of its bound (check_bf16 /
check_f16: 1.000 is a difference of exactly one ulp of the storage where one ulp is allowed); the forms launched.
  * every fp32 row launches deconv4x3_kernel, headfuse_kernel and pw2_kernel; the letters are a = deconv4_kernel,
    b = dw_kernel<7,2>, c = dw_pair16_kernel<7>, d = dw_pair_kernel<5>, e = dw_pair_kernel<7>, f = dwpw_kernel,
    g = mbconv2_kernel, h = mbt_kernel, i = mbt_s2_kernel, j = pw3d_kernel, k = stem4_kernel, l = stem_kernel;
  * every 16-bit row launches deconvb_kernel, headb_kernel, mbtb_s2_kernel and mbtd_kernel; the letters are
    a = dwb_kernel<3,1>, b = dwb_kernel<5,1>, c = dwb_kernel<7,1>, d = dwb_kernel<7,2>, e = dwt_kernel<7>,
    f = mbtb_kernel, g = pwb_kernel, h = stem4_kernel, i = stemb_kernel; a row that runs in f16 launches the same
    forms there as in bf16.
  id   size N f   taps   outs   bf16    f16   fp32 forms    16-bit forms
  t00   256 3 0  0.101  0.030  0.984  0.971   abc-e-g-i-k-  --c--fgh-
  t01   320 1 2  0.168  0.044  0.990  0.987   -b--e--hijk-  ---defgh-
  t02   384 1 2  0.155  0.044  0.983  0.974   -b-de-g-ijk-  ---defgh-
  t03   512 1 2  0.193  0.080  0.999  0.987   -b--e-ghijk-  ---defgh-
  t04   256 1 2  0.158  0.038  0.992  0.995   abc--fghij-l  a-c--fg-i
  t05   448 1 2  0.165  0.042  0.977  0.992   -b--e--h-jk-  ---d-fgh-
  t06   384 3 0  0.215  0.055  0.983  0.992   -b-de--hijk-  ---defgh-
  t07   512 1 2  0.178  0.072  0.981  0.990   -b--ef---jk-  ----efgh-
  t08   256 1 2  0.129  0.052  0.992  0.981   abc-e--h-jk-  --cd-fgh-
  t09   320 3 0  0.111  0.030  0.983  0.985   ----e-ghijk-  ---d-fgh-
  t10   384 1 2  0.169  0.042  1.000  0.994   -b--e--hijk-  ---d-fgh-
  t11   320 1 2  0.212  0.059  0.984  0.990   -b-de-ghijk-  ---defgh-
  t12   256 1 2  0.151  0.058  0.999  0.995   abc-ef-hij-l  a-cd-fg-i
  t13   448 1 2  0.170  0.036  1.000  0.995   -b--ef-hij-l  a---efg-i
  t14   384 1 2  0.203  0.054  0.981  0.992   -b--e-g-ijk-  ---defgh-
  t15   512 1 2  0.193  0.055  1.000  0.992   -b--ef-h-j-l  a--defg-i
  d00   160 1 2  0.107  0.027  0.990  0.980   ab-def-hij-l  abcd-fg-i
  d01   160 1 2  0.108  0.030  0.983      -   ab-de---i-k-  -bc--fgh-
  d02   160 1 2  0.097  0.042  0.992      -   ab-de-ghijk-  -bcd-fgh-
  d03   160 1 2  0.091  0.020  0.968      -   ab-def--ij-l  abcd-fg-i
  d04   160 1 2  0.104  0.036  0.977  0.995   ab-de---ijk-  -bcd-fgh-
  d05   160 1 2  0.101  0.042  0.938      -   ab-de-ghijk-  -bcd-fgh-
  d06   160 1 2  0.085  0.033  0.984      -   ab-def---j-l  abcd-fg-i
  d07   160 1 2  0.133  0.036  0.775      -   ab-de--hijk-  -bc--fgh-
  d08   160 1 2  0.125  0.033  0.990  0.983   ab-de-ghijk-  -bcd-fgh-
  d09   160 1 2  0.134  0.024  0.968  0.967   ab-def---j-l  abcd-fg-i
  d10   160 1 2  0.105  0.032  0.760      -   ab-de--hijk-  -bc--fgh-
  d11   160 1 2  0.094  0.042  0.984      -   ab-de----jk-  -bcd-fgh-
  d12   160 1 2  0.109  0.024  0.977      -   ab-def---j-l  abcd-fg-i
  d13   160 1 2  0.096  0.042  0.711  0.963   a--de--hijk-  -bc--fgh-
  d14   160 1 2  0.086  0.046  0.970      -   ab-de----jk-  -bcd-fgh-
  d15   160 1 2  0.125  0.022  0.968      -   ab-defghij-l  ab---fg-i
  d16   160 1 2  0.103  0.029  0.955      -   a--de--hijk-  -b---fgh-
  d17   160 1 2  0.129  0.033  0.970  0.985   ab-de----jk-  -b-d-fgh-
  d18   160 1 2  0.112  0.023  0.968  0.970   ab-defghij-l  abcd-fg-i
  d19   160 1 2  0.092  0.029  0.901      -   ab-de---ijk-  -bcd-fgh-
  d20   160 1 2  0.151  0.035  0.815      -   ab-de----jk-  -bc--fgh-
  d21   160 1 2  0.108  0.042  0.968      -   ab-defghij-l  abcd-fg-i
  d22   160 1 2  0.123  0.036  0.920  0.991   ab-de---ijk-  -bcd-fgh-
  d23   160 1 2  0.140  0.041  0.955      -   ab-de--hijk-  -bcd-fgh-
  d24   160 1 2  0.104  0.025  0.968      -   ab-defg-ij-l  abc--fg-i
  d25   160 1 2  0.087  0.025  0.862      -   ab-de--hijk-  -bcd-fgh-
  d26   160 1 2  0.102  0.035  0.968  0.962   ab-de--hijk-  -bc--fgh-
  d27   160 1 2  0.111  0.046  0.983  0.967   ab-def-h-j-l  ab-d-fg-i
  d28   160 1 2  0.092  0.045  0.966      -   ab-de--hijk-  -b-d-fgh-
  d29   160 1 2  0.107  0.039  0.659      -   ab-de--hijk-  -b-d-fgh-
  d30   160 1 2  0.094  0.033  0.968      -   ab-def-h-j-l  ab---fg-i
  d31   160 1 2  0.091  0.025  0.983  0.973   ab-de-g-ijk-  -b-d-fgh-
  d32   160 1 2  0.184  0.046  0.941      -   ab-de--hijk-  -b-d-fgh-
  d33   160 1 2  0.117  0.031  0.968      -   ab-def-h-j-l  abc--fg-i
  d34   160 1 2  0.098  0.042  0.962      -   ab-de-g-ijk-  -bcd-fgh-
  d35   160 1 2  0.119  0.072  0.970  0.987   ab-de--h-jk-  -bcd-fgh-
  d36   160 1 2  0.103  0.030  0.992  0.983   ab-def-hij-l  abc---g-i
  d37   160 1 2  0.107  0.039  0.973      -   ab-de-g-ijk-  -bcd-fgh-
  d38   160 1 2  0.109  0.035  0.976      -   ab-de--hijk-  -bc---gh-
  d39   160 1 2  0.128  0.043  0.984      -   ab-def-hij-l  abcd-fg-i
  d40   160 1 2  0.104  0.032  0.988  0.994   ab-de-g-ijk-  -bcd-fgh-
  d41   160 1 2  0.098  0.048  0.977      -   ab-de--hijk-  -bc--fgh-
  d42   160 1 2  0.162  0.038  0.968      -   ab-def-hij-l  abc--fg-i
  d43   160 1 2  0.148  0.039  0.984      -   ab-de--hijk-  -bcd-fgh-
  d44   160 1 2  0.099  0.038  0.990  0.993   ab-de--h-jk-  -bcd-fgh-
  d45   160 1 2  0.115  0.053  0.968  0.982   ab-def-hij-l  abc--fg-i
  d46   160 1 2  0.109  0.054  0.908      -   ab-de--hijk-  -bcd-fgh-
  d47   160 1 2  0.129  0.032  0.992      -   ab-de-g-ijk-  -bcd-fgh-
  e00   320 1 0  0.104  0.033  0.905      -   -b--e-g-i-k-  ----efgh-
  e01   256 1 0  0.130  0.041  0.938      -   abc----hijk-  --cd-fgh-
  e02   256 1 0  0.118  0.036  0.831      -   abcde-g-ijk-  --cd-fgh-
  e03   256 1 0  0.143  0.063  0.962      -   abc---ghijk-  --cd-fgh-
  e04   320 1 0  0.144  0.040  0.991      -   -b--efghij-l  a---efg-i
  e05   256 1 0  0.134  0.034  0.894      -   abc-e----jk-  ---d-fgh-
  e06   256 1 0  0.194  0.059  0.983      -   abcd---hijk-  --cd-fgh-
  e07   256 1 0  0.118  0.047  0.933      -   abc-e----jk-  --c--fgh-
  e08   320 1 0  0.173  0.060  0.968      -   -b--e--h-jk-  ---defgh-
  e09   256 1 0  0.111  0.025  0.962      -   a-c---g-ijk-  ---d-fgh-
  e10   256 1 0  0.151  0.036  0.868      -   abc-e--hijk-  ---d-fgh-
  e11   256 1 0  0.169  0.053  0.895      -   abcd--ghijk-  --cd-fgh-
  e12   320 1 0  0.127  0.064  0.991      -   -b--ef-hij-l  a--defg-i
  e13   256 1 0  0.128  0.027  0.992      -   abc-ef-hij-l  a-c--fg-i
  e14   256 1 0  0.182  0.042  0.992      -   abc-e-g-ijk-  --cd-fgh-
  e15   256 1 0  0.148  0.039  0.992      -   abc-ef-h-j-l  a-cd-fg-i
  e16   288 1 0  0.135  0.033  0.968      -   -b-def-hij-l  a--defg-i
  e17   288 1 0  0.116  0.034  0.984      -   -b-de-g-i-k-  ----efgh-
  e18   288 1 0  0.154  0.055  0.999      -   -b-de-ghijk-  ---defgh-
  e19   288 1 0  0.078  0.026  0.926      -   -b-defghi--l  a--defg-i
  e20   288 1 0  0.130  0.040  0.954      -   -b-de-ghi-k-  ---defgh-
  e21   288 1 0  0.131  0.045  0.999      -   -b-de-ghijk-  ---defgh-
  e22   288 1 0  0.097  0.037  0.926      -   -b-defg--j-l  a--defg-i
  e23   288 1 0  0.189  0.041  0.927      -   -b-de--hijk-  ----efgh-
  e24   288 1 0  0.153  0.036  0.999      -   -b-de-ghijk-  ---defgh-
  e25   288 1 0  0.153  0.031  0.992      -   -b-defg--j-l  a--defg-i
  e26   288 1 0  0.112  0.042  0.883      -   -b-de--hijk-  ----efgh-
  e27   288 1 0  0.131  0.045  0.984      -   -b-de-g--jk-  ---defgh-
  e28   288 1 0  0.115  0.028  0.938      -   -b-def---j-l  a--defg-i
  e29   288 1 0  0.118  0.066  0.932      -   ---de--hijk-  ----efgh-
  e30   288 1 0  0.127  0.061  0.983      -   -b-de----jk-  ---defgh-
  e31   288 1 0  0.117  0.031  0.901      -   -b-defghij-l  a----fg-i
  e32   288 1 0  0.126  0.034  0.859      -   ---de--hijk-  -----f-h-
  e33   288 1 0  0.154  0.039  0.962      -   -b-de--h-jk-  ---d-fgh-
  e34   288 1 0  0.135  0.031  0.941      -   -b-defghij-l  a--defg-i
  e35   288 1 0  0.134  0.036  0.895      -   -b-de---ijk-  ---defgh-
  e36   288 1 0  0.161  0.044  0.999      -   -b-de----jk-  ----efgh-
  e37   288 1 0  0.122  0.055  0.941      -   -b-defghij-l  a--defg-i
  e38   288 1 0  0.118  0.036  0.926      -   -b-de---ijk-  ---defgh-
  e39   288 1 0  0.170  0.044  0.988      -   -b-de--hijk-  ---defgh-
  e40   288 1 0  0.156  0.035  0.895      -   -b-defg-ij-l  a---efg-i
  e41   288 1 0  0.115  0.030  0.977      -   -b-de--hijk-  ---defgh-
  e42   288 1 0  0.132  0.044  0.681      -   -b-de-ghijk-  ----efgh-
  e43   288 1 0  0.122  0.049  0.901      -   -b-def-h-j-l  a--d-fg-i
  e44   288 1 0  0.106  0.045  0.940      -   -b-de--hijk-  ---d-fgh-
  e45   288 1 0  0.140  0.048  0.914      -   -b-de-ghijk-  ---d-fgh-
  e46   288 1 0  0.119  0.039  0.977      -   -b-def-h-j-l  a----fg-i
  e47   288 1 0  0.089  0.031  0.969      -   -b-de-g-ijk-  ---d-fgh-
  e48   288 1 0  0.199  0.050  0.990      -   -b-de-ghijk-  ---d-fgh-
  e49   288 1 0  0.133  0.039  0.999      -   -b-def-h-j-l  a---efg-i
  e50   288 1 0  0.127  0.046  0.948      -   -b-de-g-ijk-  ---defgh-
  e51   288 1 0  0.145  0.072  0.865      -   -b-de--h-jk-  ---defgh-
  e52   288 1 0  0.109  0.038  0.969      -   -b-def-hij-l  a---e-g-i
  e53   288 1 0  0.128  0.046  0.998      -   -b-de-g-ijk-  ---defgh-
  e54   288 1 0  0.147  0.065  0.992      -   -b-de--hijk-  ----e-gh-
  e55   288 1 0  0.161  0.048  0.999      -   -b-def-hij-l  a--defg-i
  e56   288 1 0  0.149  0.045  0.992      -   -b-de-ghijk-  ---defgh-
  e57   288 1 0  0.117  0.060  0.968      -   -b-de--hijk-  ----efgh-
  e58   288 1 0  0.158  0.064  0.992      -   -b-def-hij-l  a---efg-i
  e59   288 1 0  0.165  0.036  0.988      -   -b-de--hijk-  ---defgh-
  e60   288 1 0  0.153  0.055  1.000      -   -b-de--h-jk-  ---defgh-
  e61   288 1 0  0.147  0.059  0.934      -   -b-def-hij-l  a---efg-i
  e62   288 1 0  0.131  0.063  0.961      -   -b-de--hijk-  ---defgh-
  e63   288 1 0  0.155  0.040  0.999      -   -b-de-g-ijk-  ---defgh-
Worst of all rows: taps 0.215 (t06), outputs 0.080 (t03), bf16 1.000 (t10, t13, t15, e60), f16 0.995 (t04, t12,
t13, d04).
  * REFUSED is empty: neither storage refuses a row or a draw.
  * Gate rows: mb16_c48_40_nb46 0.136 of the bound without mb16_kernel (the entry block runs as pw3_kernel +
    dw_pair16_kernel<7> + pw2_kernel), mb16_c48_40_nb48 0.137 with it.
  * The 32 draws produce 357 launch keys (storage included), 0 unreached, 0 refused builds; the rows produce 820.
  * Calibration: CALIB_MEASURED below.
  * No row launches a tag that NOT_REACHED in test_gpu_kernel_census.py lists (dw_pair16_kernel<5>, mbconv_kernel,
    mbconv_s2_kernel, deconv_mfma_kernel, deconv_pair_kernel among them): every head, those fed by 8 + 8 channels
    included, runs in headfuse_kernel or, on planes it refuses, as dw_pair_kernel<5> + pw2_kernel; 24-channel blocks
    expand to 144 here too; every deconv has even inputs and <= 64 filters.
  * Wall time: this file 37 s (303 tests in one process; the slowest row test 0.32 s, t00 in fp32 with N = 3; the
    closure test 2.9 s), next to test_gpu_kernel_census.py at 43 s (57 tests) on the same machine.  That file's
    native-size rows (N = 1 or 3, like the rows here) are none of them among its eight slowest tests, the eighth of
    which takes 0.71 s; their own times were not recorded, so the comparison stands as: every row here is under
    0.35 s per storage, and no N was shrunk.
"""
import random
import re
import time

import pytest
import torch

import _subnet_space as sp
import _supernet_ref as sr
from oracle import spec, synth

pytestmark = pytest.mark.gpu

# the deconv rows that also run in bf16 and f16 storage: one of every three consecutive rows, the position rotating, so
# that the sixteen span all stem widths and every width of each deconv layer
DECONV16 = [r for i, r in enumerate(sp.DECONV) if i % 3 == (i // 3) % 3]
ROWS16 = sp.TRUNK + DECONV16            # bf16 AND f16; bf16 runs every row (the closure test needs its deconv keys)

# (storage, layer key) -> the layer the refusal names: search-space shapes that 16-bit storage refuses with
# "unsupported layer shape at ..." (a LitePoseNativeError, never a silent fallback).  fp32 refuses nothing.
REFUSED = {
}

# the shape at which a GATE_ROWS / OPTION_ROWS row must launch its form: (Cin, Cexp, Cout, K, stride, residual)
GATE_SHAPE = {'mb16_kernel': (48, 288, 40, 7, 1, False), 'mbtb_kernel': (8, 48, 8, 7, 1, True)}

# stem 16, 24, 24, 24; stage widths (8, 16, 24, 40), (24, 64, 96, 80), (32, 16, 96, 120), (16, 64, 72, 160)
INVARIANCE_ROWS = ('t00', 't07', 't11', 't14')
DRAWS, DRAW_SEED = 32, 2024

_ROW = {r[0]: r for r in sp.ROWS}
_NETS = {}
LAUNCHES = {}              # (row id, storage) -> launches or ('refused', layer), filled by the row tests
_REFUSAL = re.compile(r'unsupported layer shape at ([\w.\-+]+)')


def _net(vec, storage):
    from _net_check import _model_for
    key = (tuple(vec), storage)
    if key not in _NETS:
        if len(_NETS) >= 6:
            _NETS.clear()
        arch = sp.arch_of(vec)          # img_size sets no layer shape: the input's own size does
        _NETS[key] = _model_for(arch, storage) + (arch,)
    return _NETS[key]


def _forward(vec, storage, H, W, N, flip, options=None):
    """One profiled forward of the sub-network ``vec``: (net, arch, sd, x, outs, launches), or the layer name of a
    refusal ("unsupported layer shape at <layer>" raised as LitePoseNativeError)."""
    from _net_check import profiled_forward, set_options
    from litepose_amd import _native as nv
    try:
        m, sd, arch = _net(vec, storage)
        old = set_options(m, options or {})
        try:
            x = synth.make_images(N, H, seed=101 + N, w=W)
            outs, launches = profiled_forward(m, x.cuda(), flip)
        finally:
            set_options(m, old)
    except nv.LitePoseNativeError as e:
        mo = _REFUSAL.search(str(e))
        if mo is None:
            raise
        assert storage != 'f32', ('fp32 refuses nothing', str(e))
        assert ('%s storage' % storage) in str(e), str(e)
        return mo.group(1)
    return m, arch, sd, x, outs, launches


def _expected_refusals(vec, storage):
    keys = sp.layer_keys(sp.arch_of(vec))
    return {k: v for (s, k), v in REFUSED.items() if s == storage and k in keys}


def _check_refusal(rid, vec, storage, layer):
    key = sp.key_of_layer(sp.arch_of(vec), layer)
    print('%s %s: REFUSED at %s %s' % (rid, storage, layer, key))
    assert REFUSED.get((storage, key)) == layer, ('a refusal outside REFUSED', rid, storage, key, layer)


def _deconv_tags(launches):
    return {n.split('|')[0][:8]: t for n, t in launches if n.startswith('deconv.')}


def _same_deconv_forms_as_256(rid, vec, storage, launches):
    """The deconv rows run small: every deconv layer must launch the form it launches at 256 x 256 (device-only)."""
    big = _forward(vec, storage, 256, 256, 1, 2)
    assert not isinstance(big, str), (rid, storage, big)
    assert _deconv_tags(launches) == _deconv_tags(big[5]) and len(_deconv_tags(launches)) == 3, \
        (rid, storage, _deconv_tags(launches), _deconv_tags(big[5]))


@pytest.mark.parametrize('rid', [r[0] for r in sp.ROWS])
def test_row_fp32_vs_oracle(rid):
    """Every block tap and both outputs of every image (and of the mirrored half) against net_ref.forward at the
    project's TAP_REL and NET_ATOL (tests/_net_check.py: check_fp32)."""
    from _net_check import NET_ATOL, TAP_REL, check_fp32
    _, vec, H, W, N, flip = _ROW[rid]
    t0 = time.time()
    res = _forward(vec, 'f32', H, W, N, flip)
    assert not isinstance(res, str), ('fp32 refuses nothing', rid, res)
    m, arch, sd, x, outs, launches = res
    LAUNCHES[(rid, 'f32')] = launches
    worst_tap, name, worst_out, unit_p, unit_r = check_fp32(m, arch, sd, x, flip, outs)
    print('%s f32 %dx%d N=%d flip=%d: taps %.3f of the bound (%s), outputs %.3f; units P %.3f of c_max, R %.3f of m; %.1f s; '
          'tags %s' % (rid, H, W, N, flip, worst_tap / TAP_REL, name, worst_out / NET_ATOL, unit_p, unit_r, time.time() - t0,
                       ' '.join(sorted({t for _, t in launches}))))
    if rid.startswith('d'):
        _same_deconv_forms_as_256(rid, vec, 'f32', launches)


CASES16 = [(r[0], 'bf16') for r in sp.ROWS] + [(r[0], 'f16') for r in ROWS16]


@pytest.mark.parametrize('rid,storage', CASES16, ids=['%s-%s' % c for c in CASES16])
def test_row_16bit_vs_emulation(rid, storage):
    """check_bf16 (tests/_net_check.py) / check_f16 (tests/test_gpu_f16.py) with their own criteria; a refusal must be
    a LitePoseNativeError that names a layer whose shape REFUSED lists for this storage."""
    from _net_check import check_bf16
    from test_gpu_f16 import check_f16
    _, vec, H, W, N, flip = _ROW[rid]
    t0 = time.time()
    res = _forward(vec, storage, H, W, N, flip)
    if isinstance(res, str):
        LAUNCHES[(rid, storage)] = ('refused', res)
        _check_refusal(rid, vec, storage, res)
        return
    m, arch, sd, x, outs, launches = res
    LAUNCHES[(rid, storage)] = launches
    assert not _expected_refusals(vec, storage), ('REFUSED lists a shape of this row, the forward ran', rid, storage)
    check = check_bf16 if storage == 'bf16' else check_f16
    rows = check(m, arch, sd, x, flip, outs, [n for n, _ in launches])
    worst = max(rows.items(), key=lambda kv: kv[1][2])
    print('%s %s %dx%d N=%d flip=%d: worst criterion %.3f of its bound (%s); %.1f s; tags %s'
          % (rid, storage, H, W, N, flip, worst[1][2], worst[0], time.time() - t0,
             ' '.join(sorted({t for _, t in launches}))))
    if rid.startswith('d'):
        _same_deconv_forms_as_256(rid, vec, storage, launches)


def _keyed_row(row):
    """A GATE_ROWS / OPTION_ROWS row: the forward launches its tag at GATE_SHAPE exactly when the row says so, and every
    image is compared like a census row's."""
    from _net_check import NET_ATOL, TAP_REL, check_bf16, check_fp32, launch_key
    gid, vec, storage, H, W, N, flip, options, tag, launched = row
    t0 = time.time()
    res = _forward(vec, storage, H, W, N, flip, options)
    assert not isinstance(res, str), (gid, res)
    m, arch, sd, x, outs, launches = res
    LAUNCHES[(gid, storage)] = launches
    d = spec.derive(arch)
    keys = {launch_key(n, t, d) for n, t in launches}
    assert ((tag,) + GATE_SHAPE[tag] in keys) == launched, (gid, sorted(k for k in keys if k[0] == tag))
    if storage == 'f32':
        worst = check_fp32(m, arch, sd, x, flip, outs, chunk=8, tap_images=8)
        crit = max(worst[0] / TAP_REL, worst[2] / NET_ATOL)
    else:
        rows = check_bf16(m, arch, sd, x, flip, outs, [n for n, _ in launches], chunk=8)
        crit = max(r[2] for r in rows.values())
    units = '; units P %.3f of c_max, R %.3f of m' % worst[3:5] if storage == 'f32' else ''
    print('%s: worst criterion %.3f of its bound%s; %.1f s; tags %s'
          % (gid, crit, units, time.time() - t0, ' '.join(sorted({t for _, t in launches}))))


@pytest.mark.parametrize('gid', [g[0] for g in sp.GATE_ROWS])
def test_batch_gate_both_sides(gid):
    """The batch-gated form on a search-space shape no published architecture has, one row on each side.
      * mb16_kernel: ``NB >= opt_mb16_min`` (48) and ``mb16_supported``: ``H == 16 && W == 16 && K == 7 && S == 1``,
        ``!(Cout & 7) && !(res && Cin != Cout) && !(Cin & 15) && !(Cexp & 31)`` and (Cin / 16, ceil(Cout / 32)) one of
        (3, 2) (3, 3) (3, 4) (5, 3) (6, 3).  In the space that is stage 4 at 256 x 256: the 80-channel residual blocks and
        the 48 -> 80 entry (search-XS), the 48 -> 120 entry (search-S), and two shapes no published architecture has,
        the 48 -> 40 and the 96 -> 80 entry.  The rows take 48 -> 40 (mb16_kernel<3, 2>); N = 24 / 23 with flip = 2."""
    _keyed_row({g[0]: g for g in sp.GATE_ROWS}[gid])


@pytest.mark.parametrize('oid', [o[0] for o in sp.OPTION_ROWS])
def test_option_row_launches_its_form(oid):
    """mbtb_kernel<1, 1, true> on the 8-channel residual blocks of stage 1 (Cexp = 48: half a 16-channel MFMA group; no
    published architecture has them): mbtd_kernel is asked first and takes every residual block of up to 32 channels
    (``mode_d && wrow2 && res && ck <= 2 && nmt == 1``), so the row switches it off (option "mbtd" = 0).  No batch gate
    is involved: three images, mirrored, on 32 x 32 stage-1 planes."""
    _keyed_row({o[0]: o for o in sp.OPTION_ROWS}[oid])


@pytest.mark.parametrize('storage', ['bf16', 'f16'])
@pytest.mark.parametrize('rid', INVARIANCE_ROWS)
def test_batched_equals_per_image_and_flip_modes_bitwise(rid, storage):
    """test_bf16_batched_equals_per_image_and_flip_modes_bitwise on four trunk rows of different widths, at the row's
    size with three images."""
    _, vec, H, W, _, _ = _ROW[rid]
    m, sd, arch = _net(vec, storage)
    N = 3
    x = synth.make_images(N, H, seed=47, w=W).cuda()
    both = [o.clone() for o in m.forward_native(x, 2)]
    plain = [o.clone() for o in m.forward_native(x, 0)]
    mirr = [o.clone() for o in m.forward_native(x, 1)]
    for k in range(2):
        assert torch.equal(both[k][:N], plain[k])
        assert torch.equal(both[k][N:], mirr[k])
    for n in range(N):
        one = m.forward_native(x[n:n + 1], 0)
        for k in range(2):
            assert torch.equal(one[k][0], plain[k][n])
    fl = m.forward_native(torch.flip(x, [3]).contiguous(), 0)
    for k in range(2):
        assert torch.equal(fl[k], mirr[k])


def _row_launches(rid, vec, storage, H, W, N, flip, options=None):
    if (rid, storage) not in LAUNCHES:
        res = _forward(vec, storage, H, W, N, flip, options)
        LAUNCHES[(rid, storage)] = ('refused', res) if isinstance(res, str) else res[5]
    return LAUNCHES[(rid, storage)]


def test_rows_cover_the_launches_of_real_draws():
    """32 seeded draws of ``ArchManager.random_sample()``, each built in fp32 and in bf16 and run once at its own
    img_size (N = 1, flip = 2), no comparison: every launch key (storage, tag, Cin, Cexp, Cout, K, stride, residual) of
    those forwards is produced by some census row in that storage -- covering the layer shapes covers the kernel
    forms.  A failure is mended by a new row; the condition is zero unreached keys."""
    from _net_check import launch_key
    covered = {}
    for rid, vec, H, W, N, flip in sp.ROWS:
        d = spec.derive(sp.arch_of(vec))
        for storage in ('f32', 'bf16', 'f16'):
            if storage != 'f32' and (rid, storage) not in CASES16:
                continue
            got = _row_launches(rid, vec, storage, H, W, N, flip)
            if got and got[0] == 'refused':
                continue
            for n, t in got:
                covered.setdefault((storage,) + launch_key(n, t, d), []).append(rid)
    for gid, vec, storage, H, W, N, flip, options, _, _ in sp.GATE_ROWS:
        d = spec.derive(sp.arch_of(vec))
        for n, t in _row_launches(gid, vec, storage, H, W, N, flip, options):
            covered.setdefault((storage,) + launch_key(n, t, d), []).append(gid)
    random.seed(DRAW_SEED)
    am = sp._manager()
    drawn, unreached, refused = set(), {}, 0
    for i in range(DRAWS):
        arch = am.random_sample()
        vec, R = sp.vector_of(arch), arch['img_size']
        d = spec.derive(arch)
        for storage in ('f32', 'bf16'):
            res = _forward(vec, storage, R, R, 1, 2)
            if isinstance(res, str):
                _check_refusal('draw%d' % i, vec, storage, res)
                refused += 1
                continue
            for n, t in res[5]:
                k = (storage,) + launch_key(n, t, d)
                drawn.add(k)
                if k not in covered:
                    unreached.setdefault(k, []).append('draw%d %s@%d' % (i, vec, R))
    print('%d draws: %d launch keys, %d unreached, %d refused builds; the rows produce %d keys'
          % (DRAWS, len(drawn), len(unreached), refused, len(covered)))
    assert not unreached, ('launch keys of real draws that no census row produces', sorted(unreached.items())[:12])


# ------------------------------------------------------------------ calibration on the extremes
# (name, width vector): the all-minimum architecture, and one that mixes the minima and maxima of adjacent layers
CALIB = [('all_min', (8, 16, 16, 8, 8, 16, 24, 40)), ('min_max', (24, 64, 16, 32, 8, 64, 24, 160))]
CALIB_HW, CALIB_STEPS = (96, 160), 2
# worst device-distance / yardstick ratio (running mean, running var) over all layers and both steps, MI355X
CALIB_MEASURED = {'all_min': (1.87, 1.91), 'min_max': (1.77, 1.76)}


@pytest.mark.parametrize('ci', range(len(CALIB)), ids=[c[0] for c in CALIB])
def test_calibration_on_the_extreme_widths(ci):
    """``calibrate`` (the unfused launches, stem_raw_kernel, deconv_raw_kernel, bn_stats_kernel, bn_apply_kernel) on
    8-channel layers and an 8-filter deconv, 96 x 160 (15-pixel deepest planes: the scalar path), two steps of N = 4:
    every running pair of every layer against sr.train_forward in float64.  The reference golden has no ``dist`` for
    these architectures, so the yardstick of a layer is the float32 restatement's own distance from float64
    (sr.train_forward in float32, which the golden generator pins bit for bit to the real reference), never less than
    2^-23 max|pair|; the device may be MARGIN = 4 (tests/test_gpu_supernet.py, not retuned) yardsticks from float64.
    Measured: CALIB_MEASURED above (the 8-channel layers and the 8-filter deconv stay below half of MARGIN)."""
    import numpy as np
    from litepose_amd.models import pose_supermobilenet as psm
    from test_gpu_supernet import MARGIN
    name, vec = CALIB[ci]
    H, W = CALIB_HW
    arch = sp.arch_of(vec)
    layers = sr.bn_layers(arch)
    assert min(c for _, c in layers) == 8
    m = psm.get_pose_net(sp._cfg())
    m.load_state_dict(sr.make_state_dict(sr.SEED), strict=True)
    dev_steps = []

    def on_step(i, cal):
        got = {}
        for p, c in layers:
            mean, var = cal.read(p, c, 'cuda')
            got[p] = (mean.cpu().double().numpy(), var.cpu().double().numpy())
        dev_steps.append(got)
    xs = [sr.step_images(H, W, ci, s) for s in range(CALIB_STEPS)]
    m.calibrate(arch, [x.cuda() for x in xs], momentum=0.1, on_step=on_step)
    assert len(dev_steps) == CALIB_STEPS
    sub32 = sr.sub_state_dict(sr.make_state_dict(sr.SEED), arch)
    sub64 = sr.sub_state_dict(sr.to_double(sr.make_state_dict(sr.SEED)), arch)
    worst, failures = [0.0, 0.0], []
    for step in range(CALIB_STEPS):
        with torch.no_grad():
            sr.train_forward(xs[step], sub32, arch)
            sr.train_forward(xs[step].double(), sub64, arch)
        p32, p64 = sr.pairs_of(sub32, arch), sr.pairs_of(sub64, arch)
        for p, c in layers:
            for q in range(2):
                floor = 2.0 ** -23 * float(np.abs(p64[p][q]).max())
                yard = max(float(np.abs(p32[p][q] - p64[p][q]).max()), floor)
                d64 = float(np.abs(dev_steps[step][p][q] - p64[p][q]).max())
                worst[q] = max(worst[q], d64 / yard)
                if not d64 <= MARGIN * yard:
                    failures.append((step, p, 'mean var'.split()[q], d64, yard))
    print('calibration %s %dx%d: worst device-distance / yardstick: mean %.2f var %.2f (MARGIN %g)'
          % (name, H, W, worst[0], worst[1], MARGIN))
    assert not failures, (name, len(failures), failures[:6])
