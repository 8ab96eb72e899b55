"""Census of the kernel forms only a custom architecture selects: the rows of tests/_custom_space.py on the device
against the oracle, with synthetic weights (oracle.synth.make_state_dict).  These are the forms ``NOT_REACHED`` of
tests/test_gpu_kernel_census.py lists -- mbconv_kernel, mbconv_s2_kernel, deconv_mfma_kernel, deconv_pair_kernel,
deconv4_kernel on planes above 16 x 16, the 3x3 / 5x5 depthwise forms inside blocks -- and the refusals the fused 7x7
kernels must make for other kernel sizes.  They are also what a refused fast path falls back to.

Per row, one profiled forward (tests/_net_check.py: profiled_forward; the whole batch in one launch per op):
  * fp32: check_fp32 -- every block tap (TAP_REL, scaled by the tap's magnitude) and both outputs (NET_ATOL) of every
    image, the mirrored half (flip = 2) against the oracle on torch.flip; the outputs of image 0 against the samples of
    the REAL reference module (tests/golden/golden_custom.npz) at NET_ATOL; the launched tags a superset of
    ``expect_f32``; every ``TARGET`` shape launched under its tag; no ``FORBID`` tag on its layer;
  * bf16: check_bf16 with its own criteria, ``expect_16``;
  * f16: check_f16 (tests/test_gpu_f16.py) on ``F16_ROWS``: the rows that add a 16-bit form (dwb_kernel<5,2>, <3,2>,
    <5,1> and <3,1> inside blocks: ksize_256, ksize_128, five_128; the 24-channel blocks of 96 expanded channels:
    mb24_128) and the deconv rows (odd_64, pair66_64, wide72_64, d4_256, plain_mfma_64, plain_pair_64), whose outcome
    in 16-bit storage is a refusal;
  * in every storage: no launch of a block whose depthwise is not 7x7 carries a fused-7x7 tag (FUSED_K7);
  * a refusal is a LitePoseNativeError whose text ``REFUSED`` lists for (storage, row); one outside the table fails, and
    so does a listed one that does not happen.  16-bit storage keeps tensors in channel octets, so deconv filters that
    are no multiple of 8 are refused there (by the first layer that has them, at the forward), as are more than 64
    (at lp_net_finalize); fp32 refuses the three-stage net only, as the reference module does (IndexError);
  * two rows (INVARIANCE_ROWS: mb24_144x160, odd_96x160): batched == per-image and flip = 2 == an explicit flip, bitwise.
Tolerances are the project's own (NET_ATOL = TAP_REL = 2e-5, the criteria inside check_bf16 / check_f16).

What the rows exposed, and what was done (DESIGN.md, appendix "channel counts"):
  * pw2_kernel walked ``C >> 1`` k-pairs per source against a packing of ``(K + 1) / 2`` pairs over the concatenated
    channels: with the 17 + 24-channel head of odd_64 the last refined channel was never multiplied, the raw source and
    the second channel block read shifted weights.  deconv_mfma_kernel had the same walk (``nkp = C >> 1`` per tap and
    source against ``K index = tap * Ct + ci``).  MEASURED BEFORE the fix, fp32, max |device - oracle| (max |oracle|):
      odd_64         deconv.2 (17 + 24 ch) 3.53 (2.92)   final.0 (17 + 24 ch) 0.566 (0.382)   final.1 (9 + 24 ch) 1.05 (1.09)
      odd_96x160     deconv.2 3.98 (3.10)                final.0 0.523 (0.369)                final.1 1.36 (1.12)
      plain_mfma_64  deconv.2 (17 ch) 0.333 (0.494)      final.0 4.6e-8 (0.054)               final.1 (9 ch) 0.0170 (0.028)
    with deconv.0 / deconv.1 (even channel counts) within 2.4e-6: silently wrong maps, no error.  Both kernels now read
    k-pairs packed per source, an odd source ending in a pair whose absent channel is a zero weight and a zero operand
    that is never loaded; even channel counts pack and run bit for bit as before.
  * the 16-bit packer of depthwise weights (channel octets) wrote the channels beyond the last whole octet past the
    block it had reserved (deconv filters of 20: four floats per tap into the arena's spare capacity).  It packs whole
    octets only now; such a net is refused at the forward as before, and the plan's bytes are unchanged.
  * DESIGN.md said option "mbconv2" = 0 selects mbconv_kernel; it selects the unfused chain (row mbconv2_0).
  * no fused 7x7 kernel accepts another kernel size, with or without its batch gate passed.  launch_dwpw's
    ``KP = C >> 1`` stands behind ``C & 31``, the channel-pair depthwise arrays (``wpair``) behind an even channel
    count in the plan and in launch_headfuse; ``wdup`` is per channel.

Sensitivity (scratch builds of one wrong edit each, not committed; the fp32 row tests named failed at check_fp32's
output assertion, ``err <= NET_ATOL``, with the error given):
  mbconv_kernel       depthwise tap kx = 6 reads tap 5        mb24_128 0.199, mb24_144x160 0.186, five_128 0.121
  mbconv_s2_kernel    depthwise taps mirrored in x            mb24_128 0.292, mb24_144x160 0.294, mb24_w34 0.402
                      (tap 6 -> 5 as above made the kernel need scratch: its launcher refused it and the rows
                      failed on "expected forms not launched" instead)
  deconv_mfma_kernel  first k-pair of every tap dropped       odd_64 0.0341, plain_mfma_64 0.0314
  deconv_pair_kernel  one of the 16 taps reads its neighbour  pair66_64 0.103, wide72_64 0.0393, plain_pair_64 0.0308
  pw2_kernel          the odd source's tail pair dropped      odd_64 0.0969, odd_96x160 0.0854, plain_mfma_64 0.0015

Measured on an MI355X, every test passing.  Columns: input size, N, flip; the worst fp32 block tap and the worst fp32
output as fractions of TAP_REL / NET_ATOL; the worst bf16 and f16 criterion as a fraction of its bound ("ref": the
refusal REFUSED lists, "-": the row does not run in that storage); the forms launched in fp32 and in bf16 (a row that
runs in f16 launches the same forms there); the wall time of the row's tests, oracle included.
  fp32 forms: a = deconv4_kernel, b = deconv4x3_kernel, c = deconv_mfma_kernel, d = deconv_pair_kernel,
    e = dw_kernel<3,2>, f = dw_kernel<5,2>, g = dw_kernel<7,2>, h = dw_pair16_kernel<3>, i = dw_pair16_kernel<5>,
    j = dw_pair16_kernel<7>, k = dw_pair_kernel<3>, l = dw_pair_kernel<5>, m = dw_pair_kernel<7>, n = dwpw_kernel,
    o = headfuse_kernel, p = mb16_kernel, q = mbconv2_kernel, r = mbconv_kernel, s = mbconv_s2_kernel, t = mbt_kernel,
    u = mbt_s2_kernel, v = pw2_kernel, w = pw3_kernel, x = pw3d_kernel, y = stem4_kernel
  16-bit forms: a = deconvb_kernel, b = dwb_kernel<3,1>, c = dwb_kernel<3,2>, d = dwb_kernel<5,1>, e = dwb_kernel<5,2>,
    f = dwb_kernel<7,2>, g = dwt_kernel<7>, h = headb_kernel, i = mbtb_kernel, j = mbtb_s2_kernel, k = mbtd_kernel,
    l = pwb_kernel, m = stem4_kernel
  id                size     N f   taps   outs   bf16    f16   fp32 forms                16-bit forms    wall
  mb24_128          128x128   3 2  0.063  0.024  0.961  0.981   ab----g--j-lm-o--rs--v-xy a------hijk-m   0.3 s
  mb24_144x160      144x160   3 2  0.065  0.021  0.914      -   ab----g----lm----rs--v--y a--d---hijklm   0.1 s
  mb24_96x128       96x128    3 2  0.052  0.019  0.990      -   ab----g----lm--------v-xy a----f-hijklm   0.0 s
  mb24_w34          256x272   3 2  0.060  0.021  0.968      -   -b----g----lm----rs--v-xy a------hijk-m   0.2 s
  five_128          128x128   3 2  0.067  0.010  1.000  0.990   ab--ef-----l--o--r--uv-xy a-cde-gh-jklm   0.0 s
  three_64          64x64     1 0    ref    ref    ref      -   refused                   refused         0.0 s
  mbconv2_0         128x128   3 2  0.055  0.013  0.851      -   ab-------j-lm-o-----uv-xy a------hijk-m   0.0 s
  odd_64            64x64     3 2  0.056  0.022    ref    ref   a-c---g-ij-lm--------v-xy refused         0.0 s
  odd_96x160        96x160    3 2  0.061  0.027    ref      -   a-c---g----lm------t-v-xy refused         0.0 s
  pair66_64         64x64     3 2  0.050  0.021    ref    ref   a--d--g-ij-lm-------uv-xy refused         0.0 s
  pair66_96x160     96x160    3 2  0.057  0.024    ref      -   ab-d--g----lm------tuv-xy refused         0.0 s
  wide72_64         64x64     3 2  0.050  0.018    ref    ref   a--d--g-ij-lm-------uv-xy refused         0.0 s
  d4_256            256x256   3 2  0.067  0.018    ref    ref   a--------j----o-q--tu--xy refused         0.1 s
  plain_mfma_64     64x64     3 2  0.048  0.002    ref    ref   a-c---g-ij-lm--------v-xy refused         0.0 s
  plain_pair_64     64x64     3 2  0.050  0.002    ref    ref   a--d--g-ij-lm-------uv-xy refused         0.0 s
  ksize_256         256x256   3 2  0.075  0.027  0.984  0.996   ab--ef-hijkl-no------v-xy abcde--hi--lm   0.6 s
  ksize_128         128x128   3 2  0.063  0.021  1.000  0.995   ab--ef-hi-klm-o------v-xy abcde--hi--lm   0.0 s
  gate5_nb48        256x256  24 2  0.062  0.033      -      -   ab--ef--i-----op-----vw-y -               0.2 s
  gateq_1024        128x128  32 2      -      -  1.000      -   -                         abcde--h--klm   0.9 s
Worst of all rows: taps 0.075 (ksize_256), outputs 0.033 (gate5_nb48), bf16 1.000, f16 0.996 (1.000 is a difference of
exactly one ulp of the storage where one ulp is allowed).  The scalar deconv_pair_kernel (128 input channels in
wide72_64) stays at 0.018 of NET_ATOL: the reference-distance margin was not needed.
Wall time: this file 6.4 s (51 tests in one process, among them a second 64-image row that is gone with the form it
launched; the slowest of the others 0.9 s, gateq_1024 with 64 images in bf16),
next to test_gpu_kernel_census.py at 43 s (57 tests) on the same kind of machine."""
import os
import time

import numpy as np
import pytest
import torch

import _custom_space as cs
import _simplenet_ref as snr
from conftest import ROOT
from oracle import net_ref, spec, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'golden_custom.npz')

_NETS = {}
_GOLD = {}


def _golden():
    if 'z' not in _GOLD:
        _GOLD['z'] = np.load(GOLDEN)
    return _GOLD['z']


def _cfg(joints):
    from litepose_amd import config
    return config.get_cfg('coco' if joints == 17 else 'crowd_pose')


def _net(row, storage):
    """(net, arch, state dict, HeadCfg, plain) of the row in ``storage``; creation may raise the refusal."""
    import litepose_amd.models as models
    head, plain = cs.head_of(row), bool(row[6].get('_plain'))
    key = (row[1], storage, head.num_joints, plain)
    if key not in _NETS:
        if len(_NETS) >= 6:
            _NETS.clear()
        arch = cs.arch_of(row)
        mod = models.pose_simplenet if plain else models.pose_mobilenet
        m = mod.get_pose_net(_cfg(head.num_joints), is_train=False, cfg_arch=arch, storage=storage)
        sd = snr.make_state_dict(arch, head, seed=1234) if plain else synth.make_state_dict(arch, head, seed=1234)
        m.load_state_dict(sd, strict=True)
        _NETS[key] = (m, arch, sd, head, plain)
    return _NETS[key]


def _images(row):
    """N images at the row's size; image 0 is the golden generator's (seed 11)."""
    _, _, H, W, N = row[:5]
    x = synth.make_images(1, H, seed=11, w=W)
    return x if N == 1 else torch.cat([x, synth.make_images(N - 1, H, seed=101 + N, w=W)])


def _forward(row, storage):
    """One profiled forward of the row: (net, arch, sd, head, plain, x, outs, launches), or the refusal's text."""
    from _net_check import profiled_forward, set_options
    from litepose_amd import _native as nv
    try:
        m, arch, sd, head, plain = _net(row, storage)
        old = set_options(m, cs.device_options(row))
        try:
            x = _images(row)
            outs, launches = profiled_forward(m, x.cuda(), row[5])
        finally:
            set_options(m, old)
    except nv.LitePoseNativeError as e:
        return str(e)
    return m, arch, sd, head, plain, x, outs, launches


def _check_refusal(row, storage, text):
    want = cs.REFUSED.get((storage, row[0]))
    print('%s %s: REFUSED: %s' % (row[0], storage, text))
    assert want is not None, ('a refusal outside REFUSED', row[0], storage, text)
    assert want in text, ('the refusal does not name its rule or layer', row[0], storage, text, want)


def _check_launches(row, storage, arch, head, launches, expect):
    from _net_check import launch_key
    d = spec.derive(arch, head)
    tags = {t for _, t in launches}
    missing = set(expect) - tags
    assert not missing, ('expected forms not launched', row[0], storage, sorted(missing), sorted(tags))
    keys = {launch_key(n, t, d) for n, t in launches}
    for n, t in launches:
        k = launch_key(n, t, d)
        if n.startswith('stage.') and k[4] != 7:
            assert t not in cs.FUSED_K7, ('a fused 7x7 kernel took a block that is not 7x7', row[0], storage, n, t, k)
    if storage == 'f32':
        for tgt in cs.TARGET[row[0]]:
            if tgt[0] is not None:
                assert tuple(tgt) in keys, ('target shape not launched under its tag', row[0], tgt,
                                            sorted(k for k in keys if k[1:] == tuple(tgt[1:])))
        for prefix, bad in cs.FORBID.get(row[0], {}).items():
            hit = [(n, t) for n, t in launches if n.startswith(prefix) and t in bad]
            assert not hit, ('a form on the far side of its gate', row[0], hit)
    return tags


F32_ROWS = [r[0] for r in cs.ROWS if 'f32' in cs.storages_of(r)]
CASES16 = [(r[0], s) for r in cs.ROWS for s in cs.storages_of(r) if s != 'f32']


@pytest.mark.parametrize('rid', F32_ROWS)
def test_row_fp32_vs_oracle(rid):
    """check_fp32 at TAP_REL / NET_ATOL on every image and the mirrored half, image 0 against the reference module's
    samples at NET_ATOL, the launched tags, the target shapes under their tags, the far sides of the gates."""
    from _net_check import NET_ATOL, TAP_REL, check_fp32
    row = cs.row(rid)
    _, _, H, W, N, flip = row[:6]
    t0 = time.time()
    res = _forward(row, 'f32')
    if isinstance(res, str):
        _check_refusal(row, 'f32', res)
        return
    assert ('f32', rid) not in cs.REFUSED, ('REFUSED lists this row, the forward ran', rid)
    m, arch, sd, head, plain, x, outs, launches = res
    tags = _check_launches(row, 'f32', arch, head, launches, row[7])
    big = N > 16                                        # the gate rows: taps on the first chunk of each half
    worst_tap, name, worst_out, unit_p, unit_r = check_fp32(m, arch, sd, x, flip, outs, chunk=8, tap_images=8 if big else None,
                                                            head=head, forward=snr.forward if plain else net_ref.forward)
    g = _golden()
    gid = cs.golden_id(row)
    for k in range(2):
        key = '%s_out%d' % (gid, k)
        got = outs[k][0].cpu().numpy()
        assert tuple(got.shape) == tuple(g[key + '_shape'][1:]), (rid, k, got.shape)
        err = float(np.abs(got.reshape(-1)[::13] - g[key + '_sample']).max())
        assert err <= NET_ATOL, ('image 0 against the reference module', rid, k, err)
    print('%s f32 %dx%d N=%d flip=%d: taps %.3f of the bound (%s), outputs %.3f; units P %.3f of c_max, R %.3f of m; %.1f s; '
          'tags %s' % (rid, H, W, N, flip, worst_tap / TAP_REL, name, worst_out / NET_ATOL, unit_p, unit_r, time.time() - t0,
                       ' '.join(sorted(tags))))


@pytest.mark.parametrize('rid,storage', CASES16, ids=['%s-%s' % c for c in CASES16])
def test_row_16bit_vs_emulation(rid, storage):
    """check_bf16 / check_f16 with their own criteria and ``expect_16``; a refusal must be the LitePoseNativeError that
    REFUSED lists for (storage, row)."""
    from _net_check import check_bf16
    from test_gpu_f16 import check_f16
    row = cs.row(rid)
    _, _, H, W, N, flip = row[:6]
    t0 = time.time()
    res = _forward(row, storage)
    if isinstance(res, str):
        _check_refusal(row, storage, res)
        return
    assert (storage, rid) not in cs.REFUSED, ('REFUSED lists this row, the forward ran', rid, storage)
    m, arch, sd, head, plain, x, outs, launches = res
    assert not plain and head.num_joints == 14          # every such row is refused: check_bf16 has the fusion head only
    tags = _check_launches(row, storage, arch, head, launches, row[8])
    check = check_bf16 if storage == 'bf16' else check_f16
    rows = check(m, arch, sd, x, flip, outs, [n for n, _ in launches], chunk=8)
    worst = max(rows.items(), key=lambda kv: kv[1][2])
    print('%s %s %dx%d N=%d flip=%d: worst criterion %.3f of its bound (%s); %.1f s; tags %s'
          % (rid, storage, H, W, N, flip, worst[1][2], worst[0], time.time() - t0, ' '.join(sorted(tags))))


@pytest.mark.parametrize('rid', cs.INVARIANCE_ROWS)
def test_batched_equals_per_image_and_flip_modes_bitwise(rid):
    """test_batched_forward_is_bitwise_per_image (tests/test_gpu_parity.py) on an mbconv row and an odd-filter deconv row:
    the numerics of a form must not depend on the batch, and flip = 2 is the plain and the mirrored forward."""
    row = cs.row(rid)
    m = _net(row, 'f32')[0]
    N = 3
    x = _images(row)[:N].cuda()
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
