"""deconv4x3_kernel with the input tile staged in LDS (net_kernels.hip): a workgroup owns a 2-D tile of one image,
stages tile + halo once (split into bf16 hi / mid / lo records) and reads the nine shifted views from LDS.  Needs a real
MI355X.

  * the deconv taps and both outputs of search-XS / -S / -M against the oracle (net_ref.forward) at the project's
    tolerance TAP_REL * max(1, |tap|_inf) / NET_ATOL, plain + mirrored (flip=2), on shapes that exercise a narrow plane
    (32x32), ragged planes (28- and 56-wide at 448^2, 208x336), planes <= 16 wide with more than 256 cells (the 16-column
    tile: 608x256), NB = 2 (search-M's 64- and 40-filter deconvs, K = 136 in three slabs), and pose_simplenet (one source);
  * every case checks that the deconvs above 256 cells did run deconv4x3_kernel;
  * P4 on the deconv taps: batch 1 equals the same image inside a batch, bitwise.

Bit-identity with the previous body of the kernel (views fetched from global memory) was checked once against the parent
commit on the same seeded inputs: profiles/r09_deconv_bitwise.txt."""
import pytest
import torch

import _simplenet_ref as snr
from _net_check import NET_ATOL, TAP_REL, _model, check_fp32, profiled_forward
from oracle import spec, synth

pytestmark = pytest.mark.gpu

CASES = [('search-XS', 256, 256, 4), ('search-XS', 208, 336, 3), ('search-XS', 608, 256, 2),
         ('search-S', 448, 448, 3), ('search-S', 208, 336, 2),
         ('search-M', 448, 448, 2), ('search-M', 256, 256, 3), ('search-M', 608, 256, 2)]


def _deconv_tags(launches):
    return {n.split('|')[0]: t for n, t in launches if n.startswith('deconv.')}


def _expect_x3(arch, H, W, launches):
    """Every deconv whose input plane has more than 256 cells runs deconv4x3_kernel (the launcher's gate)."""
    d = spec.derive(arch)
    tags = _deconv_tags(launches)
    nd = len(d['deconv'])
    assert len(tags) >= nd, tags
    for i in range(nd):
        h, w = ((H + 15) // 16) << i, ((W + 15) // 16) << i     # the backbone ends at 1/16 of the input
        name = [n for n in tags if n.startswith('deconv.%d' % i)][0]
        assert tags[name] == ('deconv4x3_kernel' if h * w > 256 else 'deconv4_kernel'), (name, h, w, tags[name])


@pytest.mark.parametrize('arch_name,H,W,N', CASES)
def test_deconv_taps_and_outputs_vs_oracle(arch_name, H, W, N):
    m, arch, sd = _model(arch_name, storage='f32')
    x = synth.make_images(N, H, seed=31, w=W)
    _, launches = profiled_forward(m, x.cuda(), 2)
    _expect_x3(arch, H, W, launches)
    outs = [o.clone() for o in m.forward_native(x.cuda(), 2)]
    torch.cuda.synchronize()
    worst_tap, worst_name, worst_out, unit_p, unit_r = check_fp32(m, arch, sd, x, 2, outs, chunk=2)
    print('%s %dx%d b%d: worst tap %.3g (%s), worst output %.3g; units: P %.3f of c_max, R %.3f of m'
          % (arch_name, H, W, N, worst_tap, worst_name, worst_out, unit_p, unit_r))
    assert worst_tap < TAP_REL and worst_out <= NET_ATOL


@pytest.mark.parametrize('H,W', [(256, 256), (208, 336), (448, 448)])
def test_simplenet_one_source_deconv_vs_reference(H, W):
    from litepose_amd import arch_zoo
    import litepose_amd.models as models
    from litepose_amd import config
    arch = arch_zoo.get('search-XS')
    sd = snr.make_state_dict(arch, seed=1234)
    m = models.pose_simplenet.get_pose_net(config.get_cfg('crowd_pose'), is_train=False, cfg_arch=arch, storage='f32')
    m.load_state_dict(sd, strict=True)
    x = synth.make_images(2, H, seed=37, w=W)
    _, launches = profiled_forward(m, x.cuda(), 0)
    _expect_x3(arch, H, W, launches)
    out = [o.clone() for o in m.forward_native(x.cuda(), 0)]
    taps = {}
    with torch.no_grad():
        ref = snr.forward(x, sd, arch, taps=taps)
    for k in range(len(ref)):
        assert float((out[k].cpu() - ref[k]).abs().max()) <= NET_ATOL, k
    for i in range(len(spec.derive(arch)['deconv'])):
        r = taps['deconv.%d' % i]
        got = m.tap('deconv.%d' % i).view(r.shape).cpu()
        rel = float((got - r).abs().max()) / max(1.0, float(r.abs().max()))
        print('simplenet %dx%d deconv.%d: %.3g' % (H, W, i, rel))
        assert rel < TAP_REL, i


@pytest.mark.parametrize('arch_name,H,W', [('search-XS', 256, 256), ('search-XS', 208, 336), ('search-M', 448, 448),
                                           ('search-XS', 608, 256)])
def test_p4_deconv_taps_batch1_equals_batched_bitwise(arch_name, H, W):
    m, arch, sd = _model(arch_name, storage='f32')
    N = 5
    x = synth.make_images(N, H, seed=41, w=W).cuda()
    names = ['deconv.%d' % i for i in range(len(spec.derive(arch)['deconv']))]
    m.forward_native(x, 0)
    torch.cuda.synchronize()
    batched = {nm: m.tap(nm).clone() for nm in names}
    for n in (0, N - 1):
        m.forward_native(x[n:n + 1].contiguous(), 0)
        torch.cuda.synchronize()
        for nm in names:
            full = batched[nm].reshape(N, -1)
            one = m.tap(nm).reshape(-1)
            assert one.numel() == full.shape[1], (nm, one.numel(), full.shape)
            assert torch.equal(one, full[n]), (nm, n)
