"""Helpers shared by the network parity tests (test_gpu_bf16.py, test_gpu_kernel_census.py): build a net with synthetic
weights, switch kernel-family options, run a profiled forward, and compare the device network with the oracle --
fp32 against ``net_ref.forward`` (block taps and outputs), bf16 against ``net_ref.bf16_plan`` fed the device's own
inputs of every launch (the per-launch criterion), with the tensors a fused launch never stores chained through the
emulation (the fused-output yardstick).

A plain module, not a conftest: the tests import it by name (tests/ is on sys.path under pytest)."""
import re
import time

import torch

from oracle import net_ref, spec, synth

BF16_ULP_REL = 2.0 ** -7
HEAD_ATOL = 2e-5
NET_ATOL = 2e-5              # fp32 network outputs against the oracle (test_gpu_parity.py)
TAP_REL = 2e-5               # fp32 block taps, scaled by max(1, the tap's magnitude) (test_block_taps_tight_256)


def _cfg():
    from litepose_amd import config
    return config.get_cfg('crowd_pose')


def _model(arch_name, storage='bf16', seed=1234, head_gain=1.0):
    from litepose_amd import arch_zoo
    from litepose_amd.models import pose_mobilenet
    arch = arch_zoo.get(arch_name)
    sd = synth.make_state_dict(arch, seed=seed, head_gain=head_gain)
    m = pose_mobilenet.get_pose_net(_cfg(), is_train=False, cfg_arch=arch, storage=storage)
    m.load_state_dict(sd, strict=True)
    return m, arch, sd


def _model_for(arch, storage='f32', seed=1234):
    """_model for a cfg_arch dictionary that is in no zoo (a drawn sub-network): (net, state dict)."""
    from litepose_amd.models import pose_mobilenet
    sd = synth.make_state_dict(arch, seed=seed)
    m = pose_mobilenet.get_pose_net(_cfg(), is_train=False, cfg_arch=arch, storage=storage)
    m.load_state_dict(sd, strict=True)
    return m, sd


def _with_option(m, key, value, fn):
    """Run fn with a kernel-family switch of the net changed (lp_net_set_option), restore it afterwards."""
    old = m.set_option(key, value)
    try:
        return fn()
    finally:
        m.set_option(key, old)


def layerwise_report(m, arch, sd, x):
    """Run the device network on x (flip=0), ONE LAUNCH PER OP (option "mbtb" = 0: the fused block kernel keeps the two
    expanded tensors of a block on the CU, so there would be nothing to compare them with; it has its own test
    below), and compare every launch with the emulated op on the device's own inputs.
    Returns [(name, max_abs_diff, worst_ulp_ratio, mismatch_fraction, is_head)]."""
    # ... and option "stem" = 0: the fused stem (stem4_kernel<lp::Bf16, C0>, round 6) keeps the conv and depthwise outputs in LDS
    # ... and "headb" = 0: the fused head keeps both depthwise outputs in LDS (it is bit-identical to its three launches)
    outs = _with_option(m, 'headb', 0, lambda: _with_option(m, 'stem', 0, lambda: _with_option(
        m, 'mbtb', 0, lambda: [o.cpu() for o in m.forward_native(x.cuda(), 0)])))
    torch.cuda.synchronize()
    dev = {'x': x}
    rows = []
    k_out = 0
    with torch.no_grad():
        for name, ins, fn in net_ref.bf16_plan(sd, arch):
            exp = fn(*[dev[k] for k in ins])
            head = name.startswith('final.') and name.endswith('.pw')
            if head:
                got = outs[k_out]
                k_out += 1
            else:
                got = m.tap(name).cpu().view(exp.shape)
            assert got.shape == exp.shape, (name, got.shape, exp.shape)
            dev[name] = got
            d = (got - exp).abs()
            ulp = exp.abs() * BF16_ULP_REL + 1e-6
            rows.append((name, float(d.max()), float((d / ulp).max()), float((d > 0).float().mean()), head))
    return rows


# ------------------------------------------------------------------ profiled forwards and launch keys
def set_options(m, options):
    """Set every option of ``options``; returns the previous values (set them back with set_options)."""
    return {k: m.set_option(k, v) for k, v in options.items()}


def profiled_forward(m, x, flip):
    """One profiled forward: (outputs on the device, [(launch name, kernel tag)]).  Profiling runs the whole batch in one
    launch per op (the internal stream fan-out is off), so every launch sees the case's full image count."""
    m.set_profiling(True)
    try:
        outs = m.forward_native(x, flip)
        torch.cuda.synchronize()
        prof = [n.rsplit('|', 1) for n, _, _, _ in m.profile()]
    finally:
        m.set_profiling(False)
    return outs, [(a, b) for a, b in prof]


_STAGE = re.compile(r'^stage\.(\d+)\.(\d+)')
_DECONV = re.compile(r'^deconv\.(\d+)')
_HEAD = re.compile(r'^final\w*\.(\d+)')


def launch_key(name, tag, d):
    """(tag, Cin, Cexp, Cout, K, stride, residual) of a launch, the layer shape taken from oracle.spec by the launch name
    (``d`` = spec.derive(arch)).  A run of blocks in one launch ('stage.2.1-9...') keys by its first block: a run holds
    blocks of one shape only.  Profile names may be cut short to keep the tag; the layer prefix always survives."""
    mo = _STAGE.match(name)
    if mo:
        b = d['stages'][int(mo.group(1))][int(mo.group(2))]
        return (tag, b['inp'], b['feat'], b['oup'], b['k'], b['stride'], bool(b['residual']))
    mo = _DECONV.match(name)
    if mo:
        c = d['deconv'][int(mo.group(1))]
        return (tag, c['refined_in'] + c['raw_in'], 0, c['out'], 4, 2, False)
    mo = _HEAD.match(name)
    if mo:
        h = d['heads'][int(mo.group(1))]
        return (tag, h['refined_in'] + h['raw_in'], 0, h['oup'], 5, 1, False)
    if name.startswith('stem') or name.startswith('first'):
        return (tag, 3, 32, d['c0'], 3, 2, False)
    raise AssertionError('launch name with no layer: %r' % name)


# ------------------------------------------------------------------ fp32 against the oracle
def fp32_tap_names(d):
    return ['first'] + ['stage.%d.%d' % (s, b) for s, blocks in enumerate(d['stages']) for b in range(len(blocks))] \
        + ['deconv.%d' % i for i in range(len(d['deconv']))]


def check_fp32(m, arch, sd, x, flip, outs, chunk=8, tap_images=None, head=None, forward=net_ref.forward):
    """The device fp32 network (its last forward: ``outs`` and the block taps) against net_ref.forward on every image of
    the batch, the mirrored half (flip=2) against the oracle on torch.flip(x, [3]).  The oracle runs ``chunk`` images at a
    time so that the host memory of its taps stays bounded; taps are compared on the first ``tap_images`` images of each
    half (None: all).  ``head``: the oracle's HeadCfg when it is not the default; ``forward``: the oracle of another head
    form with net_ref.forward's signature (tests/_simplenet_ref.py).

    Then the unit check of tests/_fp32_units.py on at most three images of the device batch -- the first, the first of
    the mirrored half (flip=2) and the last: every unit in float64 on the DEVICE's own input taps, P (per element,
    ``e <= c_max u B``) and R (``rms(e / B) <= m rms(|ref32 - ref| / B)``) asserted per unit and image.  With another
    ``forward`` than net_ref.forward (pose_simplenet) the stem and the blocks are checked and the deconv and output-head
    units are skipped.

    Returns (worst scaled tap error, its name, worst output error, worst P as a fraction of c_max, worst R as a fraction
    of m)."""
    import _fp32_units as fu
    t_all = time.time()
    d = spec.derive(arch, head)
    N = x.shape[0]
    halves = [(0, x)] if flip == 0 else ([(0, torch.flip(x, [3]))] if flip == 1 else [(0, x), (N, torch.flip(x, [3]))])
    names = fp32_tap_names(d)
    dev_taps = {nm: m.tap(nm) for nm in names}          # on the device: sliced per chunk below
    worst_tap, worst_name, worst_out = 0.0, '', 0.0
    for base, xs in halves:
        for c0 in range(0, N, chunk):
            c1 = min(N, c0 + chunk)
            with_taps = tap_images is None or c0 < tap_images
            taps = {} if with_taps else None
            with torch.no_grad():
                ref = forward(xs[c0:c1], sd, arch, head, taps=taps)
            for k in range(2):
                got = outs[k][base + c0:base + c1].cpu()
                err = float((got - ref[k]).abs().max())
                worst_out = max(worst_out, err)
                assert err <= NET_ATOL, ('out%d' % k, base + c0, err)
            if not with_taps:
                continue
            for nm in names:
                r = taps[nm]
                full = dev_taps[nm].view((-1,) + tuple(r.shape[1:]))
                got = full[base + c0:base + c1].cpu()
                rel = float((got - r).abs().max()) / max(1.0, float(r.abs().max()))
                if rel > worst_tap:
                    worst_tap, worst_name = rel, nm
                assert rel < TAP_REL, (nm, base + c0, rel)
    xin = x if flip == 0 else (torch.flip(x, [3]) if flip == 1 else torch.cat([x, torch.flip(x, [3])]))
    images = sorted({0, xin.shape[0] - 1} | ({N} if flip == 2 else set()))
    t0 = time.time()
    rows = fu.check_device(m, sd, arch, xin, outs, images, head, heads=forward is net_ref.forward)
    worst_p, worst_r = max(v[0] for v in rows.values()), max(v[1] for v in rows.values())
    print('check_fp32 units: %d units x %d images of %d x %d in %.1f s (of %.1f s): P %.3f of c_max, R %.3f of m'
          % (len(rows), len(images), x.shape[2], x.shape[3], time.time() - t0, time.time() - t_all, worst_p, worst_r))
    return worst_tap, worst_name, worst_out, worst_p, worst_r


# ------------------------------------------------------------------ bf16 against the emulation
def fused_inner(launch_names):
    """{stored output: [tensors the launch keeps on the CU]} of the fused bf16 launches among ``launch_names``."""
    out = {}
    for nm in launch_names:
        if nm.endswith('.inv+dw+point_conv'):                     # mbtb / mbtb_s2 / mbtd: a whole block
            p = nm[:-len('.inv+dw+point_conv')]
            out[p + '.point_conv'] = [p + '.inv', p + '.depth_conv']
        elif nm == 'stem.conv3x3s2+dw3+pw':                       # stem4_kernel<lp::Bf16, C0>
            out['stem.pw'] = ['stem.conv3x3s2', 'stem.dw3']
        elif nm.endswith('.dw5+dw5+pw'):                          # headb_kernel
            h = nm.split('.')[1]
            out['final.%s.pw' % h] = ['final_refined.%s.dw5' % h, 'final_raw.%s.dw5' % h]
    return out


def check_bf16(m, arch, sd, x, flip, outs, launch_names, chunk=8):
    """The device bf16 network (its last forward) against net_ref.bf16_plan, every op fed the device's own inputs, on
    every image of the batch (flip=2: the emulation's input is cat(x, flip(x)); its ops are per image).
      * an op stored by its own launch: <= 1 bf16 ulp on all but 1e-4 of the elements and <= 2 ulp everywhere, < 2 % of
        the elements differing; a head output within HEAD_ATOL (layerwise_report's criterion, with the 2-ulp tail that
        bench-size batches of deconvb_kernel show);
      * the output of a fused launch, whose inner tensors are chained through the emulation: every difference <= 1.5 bf16
        ulp of the tensor's largest value, mean |difference| <= 0.35 ulp of its mean magnitude; with one inner tensor also
        <= 2 own-ulp on all but 1e-3 of the elements and < 5 % differing (test_fused_bf16_block_vs_chained_emulation).
    Returns {op name: (kind, max |d|, criterion value)}."""
    fused = fused_inner(launch_names)
    inner = {t for v in fused.values() for t in v}
    xin = x if flip == 0 else (torch.flip(x, [3]) if flip == 1 else torch.cat([x, torch.flip(x, [3])]))
    NB = xin.shape[0]
    plan = net_ref.bf16_plan(sd, arch)
    # every stored op, sliced per chunk on the device (host memory: one chunk of every tap at a time)
    dev_full = {}
    k_out = 0
    for name, _, _ in plan:
        if name in inner:
            continue
        if name.startswith('final.') and name.endswith('.pw'):
            dev_full[name] = outs[k_out]
            k_out += 1
        else:
            dev_full[name] = m.tap(name)
    rows, bad = {}, []
    for c0 in range(0, NB, chunk):
        c1 = min(NB, c0 + chunk)
        dev = {'x': xin[c0:c1]}
        with torch.no_grad():
            for name, ins, fn in plan:
                exp = fn(*[dev[k] for k in ins])
                if name in inner:
                    dev[name] = exp                               # never stored on the device: chain the emulation
                    continue
                got = dev_full[name].view((NB,) + tuple(exp.shape[1:]))[c0:c1].cpu()
                dev[name] = got
                d = (got - exp).abs()
                head = name.startswith('final.') and name.endswith('.pw')
                frac = float((d > 0).float().mean())
                if name in fused:
                    cap = 1.5 * BF16_ULP_REL * float(exp.abs().max())
                    mean_rel = float(d.mean()) / (BF16_ULP_REL * float(exp.abs().mean()) + 1e-12)
                    crit = max(float(d.max()) / cap, mean_rel / 0.35)
                    if float(d.max()) > cap or mean_rel > 0.35:
                        bad.append((name, c0, float(d.max()), cap, mean_rel))
                    elif len([t for t in fused[name] if t in inner]) == 1:
                        over = float((d > 2.0 * (exp.abs() * BF16_ULP_REL + 1e-6)).float().mean())
                        if over > 1e-3 or frac > 0.05:
                            bad.append((name, c0, float(d.max()), over, frac))
                    kind = 'fused'
                elif head:
                    crit = float(d.max()) / HEAD_ATOL
                    if float(d.max()) > HEAD_ATOL:
                        bad.append((name, c0, float(d.max())))
                    kind = 'head'
                else:
                    # <= 1 ulp; at bench batches a few deconv.0 elements (< 1e-4) differ by 2 ulp where the fp32 sum of
                    # the 4-tap x (Ca + Cb)-channel accumulation cancels: bounded, and reported in the census table
                    r = d / (exp.abs() * BF16_ULP_REL + 1e-6)
                    ulps = float(r.max())
                    over1 = float((r > 1.0).float().mean())
                    crit = max(min(ulps, 1.0) if over1 <= 1e-4 else ulps, frac / 0.02)
                    if ulps > 2.0 or over1 > 1e-4 or frac > 0.02:
                        bad.append((name, c0, float(d.max()), ulps, over1, frac))
                    kind = 'op'
                prev = rows.get(name)
                if prev is None or crit > prev[2]:
                    rows[name] = (kind, float(d.max()), crit)
        assert not bad, bad[:8]
    return rows
