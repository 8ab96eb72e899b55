#!/usr/bin/env python
"""Headline benchmark: images/sec end-to-end (backbone + deconv head + AE grouping),
LitePose-Auto-XS @ 256x256, batch 64 per GPU, fp32, flip-TTA, on N GPUs of one node.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one pass of the whole hot path over one synthetic batch already resident
in HBM (steps are software-pipelined over two HIP streams; K steps = K batches fully completed): network on the batch and on its mirror, flip-TTA merge + projection, NMS/top-k,
tag grouping, adjust/refine, back-projection, and (N > 1) one RCCL all-gather of the
per-image keypoint records.  Weak scaling: every rank owns 64 images.  Rank 0 prints
ONE JSON line.

A plain run does only what the headline needs: set-up, warm-up, the K timed steps, --dump-outputs, the line.
Everything else -- the 200-step region, the parity check against the CPU oracle, the I/O leg, the single- and
small-batch latencies, path / kernel rooflines, the CPU baseline and BASELINE configs 4 / 5 -- runs with --full.
See DESIGN.md "Measurement" for the definitions.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
FP32_PEAK_TFLOPS = 157.3        # dense fp32: matrix cores and packed vector FMAs alike (MI355X_MICROARCH.md)
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 matrix-core peak (no sparsity)


# BASELINE.json `configs` as presets (--config): 1 = the reference's own CPU-runnable case, 2 / 3 = the headline,
# 4 / 5 = the bf16 workloads (5 per GPU: 256 images over 8 GPUs = 32 each; search-M.json's img_size is 448, the
# config names 512, the net is fully convolutional: SURVEY.md 8a-0)
CONFIGS = {1: dict(arch='search-XS', size=256, batch=1, storage='f32'),
           2: dict(arch='search-XS', size=256, batch=64, storage='f32'),
           3: dict(arch='search-XS', size=256, batch=64, storage='f32'),
           4: dict(arch='search-S', size=448, batch=32, storage='bf16'),
           5: dict(arch='search-M', size=512, batch=32, storage='bf16')}


BF16X3_EQUIV_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 6.0   # an fp32-exact product as 6 bf16 MFMAs: what the bf16 pipe can deliver of them


N_CUS = 256                     # MI355X_MICROARCH.md


def cus_occupied(grid, wgs_per_cu):
    """CUs a launch can hold: its workgroups spread over the chip at `wgs_per_cu` (HIP occupancy query) per CU."""
    if grid <= 0:
        return float(N_CUS)
    return float(min(N_CUS, -(-grid // max(1, wgs_per_cu))))


def price_flops(flops, flops_valu, ms, storage, mfma_peak=None):
    """Roofline price of a launch (or a family of launches) whose algorithmic FLOPs fall into two classes with
    different peaks: the depthwise / stem-conv FMAs run on the vector pipe (fp32, 157.3 TF whatever the storage), the
    1x1 convolutions and deconvolutions on the matrix cores (fp32 storage: fp32-exact arithmetic, priced at the fp32
    peak, 157.3 TF -- the bf16x3 split is an implementation detail, not a lower precision; bf16 storage: dense bf16
    MFMA peak, 2.5 PF).  The floor of a kernel that overlapped both pipes perfectly would be the LARGER of the two
    times; a fused block on this chip runs them one after the other (profiles/r04_phase_mix.txt), so the SUM is the
    floor that can be approached.  frac = floor / measured: <= 1 as long as the two pipes do take turns -- a kernel
    that overlapped them would be bounded by floor_ms_max instead and could print a frac_flops above 1 (none does:
    profiles/r04_phase_mix.txt; floor_ms_max is in the line for that reason)."""
    if mfma_peak is None:
        mfma_peak = FP32_PEAK_TFLOPS if storage == 'f32' else BF16_MFMA_PEAK_TFLOPS
    t_valu = flops_valu / (FP32_PEAK_TFLOPS * 1e12)
    t_mfma = (flops - flops_valu) / (mfma_peak * 1e12)
    t = ms * 1e-3
    return {'flops_valu': int(flops_valu), 'flops_mfma': int(flops - flops_valu), 'mfma_peak_tflops': mfma_peak,
            'valu_peak_tflops': FP32_PEAK_TFLOPS, 'floor_ms_sum': round((t_valu + t_mfma) * 1e3, 5),
            'floor_ms_max': round(max(t_valu, t_mfma) * 1e3, 5),
            'frac_flops': round((t_valu + t_mfma) / t, 4) if t > 0 else None}


_T0 = time.time()


def _log(msg):
    """Progress on stderr (the JSON line is the only thing on stdout)."""
    if int(os.environ.get('RANK', '0')) == 0:
        sys.stderr.write('[bench %6.1f s] %s\n' % (time.time() - _T0, msg))
        sys.stderr.flush()


def algorithmic_bytes_per_image(arch, J, R, flip, act_bytes=4):
    """B_op (op-boundary activation bytes of one forward, weights
    excluded, BN/act/adds fused) and B_post (network outputs consumed by the AE stage).
    act_bytes = 2 for bf16 storage (the fp32 image and the two fp32 head outputs stay 4 bytes)."""
    from oracle import spec
    d = spec.derive(arch)
    e = 0                                     # elements
    h = R // 2
    e4 = 3 * R * R                            # elements that are fp32 in every storage mode
    e += 32 * h * h                           # stem conv (image counted in e4)
    e += 2 * 32 * h * h                       # dw3
    e += 32 * h * h + d['c0'] * h * h         # pw
    div = 2
    for blocks in d['stages']:
        for b in blocks:
            hi = R // div
            ho = hi // b['stride']
            e += (b['inp'] + b['feat']) * hi * hi
            e += b['feat'] * hi * hi + b['feat'] * ho * ho
            e += (b['feat'] + b['oup']) * ho * ho + (b['oup'] * ho * ho if b['residual'] else 0)
            div *= b['stride']
    hh = R // div
    raws = [hh, hh * 2, hh * 4]
    for i, dc in enumerate(d['deconv']):
        hi = raws[i]
        e += (dc['refined_in'] + dc['raw_in']) * hi * hi + dc['out'] * (2 * hi) ** 2
        if i > 0:
            hd = d['heads'][i - 1]
            ho = 2 * hi
            e += 2 * hd['refined_in'] * ho * ho + 2 * hd['raw_in'] * ho * ho       # two dw5
            e += (hd['refined_in'] + hd['raw_in']) * ho * ho                          # fused 1x1 pair
            e4 += hd['oup'] * ho * ho
    b_op = act_bytes * e + 4 * e4
    F = 2 if flip else 1
    b_post = 4 * F * (2 * J * (R // 4) ** 2 + J * (R // 2) ** 2)
    return b_op, b_post


def pmc_traffic(kernel, launches, cfgkey):
    """HBM bytes per launch of `kernel` from the newest committed PMC passes (profiles/rNN_traffic*.json, written by
    tools/pmc_traffic.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs; FETCH_SIZE doubled per the
    gfx950 correction) THAT WERE MEASURED ON THIS CONFIGURATION: the file's `config` {arch, size, batch, storage}
    must equal `cfgkey`, otherwise the answer is (None, None) -- a number of another workload is not evidence.
    NOT a counter of this run: the JSON line carries `traffic_source` (file + the commit it was measured on)."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_traffic*.json')), reverse=True):
        try:
            with open(path) as f:
                t = json.load(f)
            if t.get('config') != cfgkey:
                continue
            ks = t['kernels']
            if kernel in ks:
                tot = ks[kernel]['hbm_bytes_per_forward']
            else:       # the PMC summary keeps the template arguments of the dw* kernels (dwpw_kernel<3,1,1>)
                hits = [v['hbm_bytes_per_forward'] for k, v in ks.items() if k.split('<')[0] == kernel]
                if not hits:
                    raise KeyError(kernel)
                tot = sum(hits)
            return (int(tot / max(1, launches)),
                    '%s@%s' % (os.path.relpath(path, ROOT), t.get('commit', 'unknown')))
        except Exception:
            continue
    return None, None


def traffic_file(cfgkey):
    """(relative path @ commit, parsed JSON) of the newest committed PMC traffic file measured on `cfgkey`, or (None, None)."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_traffic*.json')), reverse=True):
        try:
            with open(path) as f:
                t = json.load(f)
            if t.get('config') == cfgkey and 'kernels' in t:
                return '%s@%s' % (os.path.relpath(path, ROOT), t.get('commit', 'unknown')), t
        except Exception:
            continue
    return None, None


def baseline_config_of(arch, size, batch, storage, asked=0):
    """Which BASELINE.json config a run IS (the default line is config 3 and said `null`): the preset that
    was asked for, else the highest-numbered preset whose {arch, size, batch, storage} equal the run's (2 and 3 share
    one workload; the default run executes the full path, which is config 3)."""
    if asked:
        return asked
    key = dict(arch=arch, size=size, batch=batch, storage=storage)
    hits = [k for k, v in CONFIGS.items() if v == key]
    return max(hits) if hits else None


def gpu_affinity(local_rank, world, slot=None):
    """8-GPU readiness (the reference's only multi-GPU evaluation line is valid.py:165): eight
    ranks on one host and nothing pinned was the one risk DESIGN section 5 named.  With world > 1 each rank binds
    itself to the cores of ITS GPU's NUMA node (PCI address of the HIP device -> /sys/bus/pci/devices/<addr>/numa_node
    and local_cpulist; the node's cores are dealt to the ranks that share it), so the launch threads, the RCCL proxy
    and the pinned staging buffers of a rank stay next to its GPU.  Best effort: anything unreadable leaves the
    process unpinned and says so.  world == 1 never pins (cpu_baseline wants the host's cores)."""
    info = {'pinned': False}
    if world <= 1 or os.environ.get('LP_BENCH_NO_AFFINITY'):
        info['why'] = 'single rank' if world <= 1 else 'LP_BENCH_NO_AFFINITY'
        return info
    try:
        def parse_cpulist(txt):
            cpus = []
            for part in txt.strip().split(','):
                if not part:
                    continue
                a, _, b = part.partition('-')
                cpus += list(range(int(a), int(b or a) + 1))
            return cpus

        def node_of(dev):
            pr = torch.cuda.get_device_properties(dev)
            addr = '%04x:%02x:%02x.0' % (getattr(pr, 'pci_domain_id', 0), pr.pci_bus_id, pr.pci_device_id)
            base = '/sys/bus/pci/devices/' + addr
            with open(base + '/numa_node') as f:
                node = int(f.read().strip())
            with open(base + '/local_cpulist') as f:
                cpus = parse_cpulist(f.read())
            return addr, node, cpus
        ndev = torch.cuda.device_count()
        one_gpu = bool(os.environ.get('LP_BENCH_ONE_GPU'))
        dev = 0 if one_gpu else local_rank
        addr, node, cpus = node_of(dev)
        allowed = sorted(os.sched_getaffinity(0))
        cpus = [c for c in cpus if c in allowed] or allowed
        # the ranks that share this node (same cpu list) split it
        peers = []
        for r in range(world):
            d = 0 if one_gpu else (r if r < ndev else r % max(1, ndev))
            try:
                if node_of(d)[2] == node_of(dev)[2]:
                    peers.append(r)
            except Exception:
                pass
        me = local_rank if slot is None else slot          # LP_BENCH_ONE_GPU: every rank sits on device 0 -- split by the rank
        peers = peers or [me]
        k = peers.index(me) if me in peers else 0
        per = max(1, len(cpus) // len(peers))
        mine = cpus[k * per:(k + 1) * per] or cpus
        global _AFF_ORIG
        _AFF_ORIG = set(allowed)
        os.sched_setaffinity(0, mine)
        info.update({'pinned': True, 'pci': addr, 'numa_node': node, 'cores': len(mine),
                     'first_core': mine[0], 'last_core': mine[-1], 'ranks_on_node': len(peers)})
    except Exception as e:                     # never a bench failure
        info['why'] = '%s: %s' % (type(e).__name__, e)
    return info


_AFF_ORIG = None


def release_affinity():
    """After the timed region: give the process its original cores back (rank 0 goes on to run the CPU oracle for the parity
    check; the pinning exists for the serving loop)."""
    global _AFF_ORIG
    if _AFF_ORIG:
        try:
            os.sched_setaffinity(0, _AFF_ORIG)
        except Exception:
            pass
        _AFF_ORIG = None


def run_extra_config(n, steps, warmup, timeout=240):
    """BASELINE configs 4 / 5 inside the `--full` run of the default workload (two of BASELINE.json's
    five configs were never on a record of the default command).  After the
    headline has been measured this process starts `bench.py --config N --full` as a child with the same steps / warm-up (own
    process: own engine, own hipGraphs; this process is idle and only keeps its buffers), and the child's whole JSON line
    is condensed to the fields a reviewer needs.  A failure is reported as such and never touches the headline."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), '--config', str(n), '--steps', str(steps), '--warmup', str(warmup),
           '--full', '--no-cpu-baseline', '--no-io-leg', '--no-extra-configs', '--no-small-batch', '--parity-images', '16']
    t0 = time.time()
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout,
                           env=dict(os.environ, RANK='0', LOCAL_RANK='0', WORLD_SIZE='1'))
        lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
        if r.returncode != 0 or not lines:
            return {'error': 'rc %d: %s' % (r.returncode, (r.stderr or r.stdout)[-400:])}
        d = json.loads(lines[-1])
    except Exception as e:
        return {'error': '%s: %s' % (type(e).__name__, e)}
    return condense_child_line(d, n, steps, warmup, round(time.time() - t0, 1))


def condense_child_line(d, n, steps, warmup, wall_s):
    """A child run's full JSON line -> the entry of `configs` in the parent's line (the fields a reviewer needs to judge a
    BASELINE config: time, value, both roofline fractions, the dominant kernel, parity incl. OKS)."""
    pr, rl, par = d.get('path_roofline', {}), d.get('roofline', {}), d.get('parity', {})
    p3 = par.get('p3_vs_pure_cpu_pipeline', {})
    return {'workload': d['metric'], 'dtype': d['dtype'], 'ms_per_step': d['ms_per_step'], 'value': d['value'],
            'unit': d['unit'], 'steps': d['steps'], 'warmup': d['warmup'], 'graph_replay': d.get('graph_replay'),
            'path_frac': pr.get('frac'), 'frac_flops': pr.get('frac_flops'),
            'roofline': {k: rl.get(k) for k in ('kernel', 'bound', 'frac', 'frac_flops', 'frac_alg_bytes', 'achieved', 'peak',
                                                'unit', 'launches', 'avg_launch_us', 'traffic', 'traffic_source',
                                                'cus_occupied', 'frac_flops_per_occupied_cu')},
            'kernels_ms': {k: v['ms_per_step'] for k, v in d.get('kernels', {}).items()},
            'network_ms_single_stream': d.get('network_ms_single_stream'),
            'latency_ms_single_batch': d.get('latency_ms_single_batch'),
            'latency_ms_single_batch_graph': d.get('latency_ms_single_batch_graph'),
            'parity': {'ok': par.get('ok'), 'images': par.get('images'), 'heatmap_err': par.get('heatmap_tag_max_abs_err'),
                       'tolerance': par.get('tolerance'),
                       'records_identical_to_oracle_parser': par.get('records_identical_to_oracle_parser'),
                       'persons': par.get('persons'), 'joints_compared': p3.get('joints_compared'),
                       'joints_identical': p3.get('joints_identical_position_and_presence'),
                       'oks': p3.get('oks_vs_cpu_persons')},
            'wall_s': wall_s,
            'ms_per_step_200': d.get('ms_per_step_200'),
            'command': 'python bench.py --config %d --steps %d --warmup %d --full --no-cpu-baseline --no-io-leg --parity-images 16'
                       % (n, steps, warmup)}


def cpu_baseline(arch, sd, cfg, R, n_img, offs_np, runs=3):
    """The oracle (CPU port of the reference path) timed on this box's host cores on a bounded sample:
    network+flip+merge at batch n_img, then the parser image by image (it is batch-1 by construction).  One
    warm-up, then the MEDIAN of `runs` timed passes with torch capped at 64 threads (`cores` = the threads used,
    `host_cores` = what the box has).  Why not all cores: oneDNN on these small convolutions does not
    scale to hundreds of threads -- round 3 measured 186.7 s against 6.5 s for the same 24 images on a 256-core
    box -- so an all-cores pass would neither fit the bench's time budget nor be the faster
    baseline; it is not re-measured here and no number of another run is put into this run's record."""
    from oracle import group_ref, inference_ref, net_ref, synth
    cores = os.cpu_count() or 1
    x = synth.make_images(n_img, R, seed=7)
    off0, off1, f0, f1 = [torch.from_numpy(a[:n_img]) for a in offs_np]
    tc = inference_ref.TestCfg()

    def run():
        with torch.no_grad():
            o = net_ref.forward(x, sd, arch)
            of = net_ref.forward(torch.flip(x, [3]), sd, arch)
            o = [o[0] + off0, o[1] + off1]
            of = [of[0] + f0, of[1] + f1]
            fh, tg = inference_ref.merge(o, of, tc, (R, R))
        ora = group_ref.HeatmapParser(group_ref.Params())
        fh, tg = fh.numpy(), tg.numpy()
        persons = 0
        for n in range(n_img):
            a, _ = ora.parse_image(fh[n], tg[n])
            persons += a.shape[0]
        return persons

    res = []
    threads = min(cores, 64)
    torch.set_num_threads(threads)
    t0 = time.time()
    persons = run()                         # warm-up (oneDNN primitive caches)
    warm = time.time() - t0
    ts = []
    for _ in range(runs):
        t0 = time.time()
        run()
        ts.append(time.time() - t0)
    res.append((sorted(ts)[len(ts) // 2], threads, ts))
    _log('cpu_baseline %d threads: warm-up %.1f s, runs %s' % (threads, warm, ['%.1f' % v for v in ts]))
    dt, threads, _ = min(res)
    return {'value': round(n_img / dt, 3), 'unit': 'images/s', 'cores': threads, 'host_cores': cores, 'kind': 'port',
            'runs': runs,
            'sample': '%d images XS@%d, %d persons: oracle net+flip+merge (torch fp32) + NumPy HeatmapParser per '
                      'image; median of %d runs after one warm-up: %s'
                      % (n_img, R, persons, runs,
                         '; '.join('%d threads of %d cores %.2f s (%.2f img/s)' % (t, cores, d, n_img / d)
                                   for d, t, _ in res))}


def respawn_under_torchrun(n):
    """`python bench.py --gpus N` without a launcher: re-exec as one process per GPU under
    torch.distributed.run (what the driver does itself for N > 1); rank 0 prints the JSON line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    raise SystemExit(subprocess.call(cmd, env=env))


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(dirname, records, pcap, seed=0):
    """--dump-outputs DIR: what the timed path handed its caller in its last step -- the (all-gathered) keypoint records
    (kpts [N, pcap, J, D], count [N], scores [N, pcap]) -- as float32 DIR/<name>.npy, so that two builds can be compared
    output for output.  Slots past an image's person count are not part of the result (the buffer set keeps whatever it
    held there) and are written as zeros.  Above 64 MB in all a fixed, seeded sample of images is written, and their
    indices as image_index.npy."""
    kpts, count, scores = [t.cpu() for t in records]
    N, P = kpts.shape[0], kpts.shape[1]
    valid = torch.arange(P)[None, :] < count.to(torch.int64).clamp(max=pcap)[:, None]
    kpts = torch.where(valid[:, :, None, None], kpts, torch.zeros((), dtype=kpts.dtype))
    scores = torch.where(valid, scores, torch.zeros((), dtype=scores.dtype))
    arrays = {'kpts': kpts.numpy().astype(np.float32), 'count': count.numpy().astype(np.float32),
              'scores': scores.numpy().astype(np.float32)}
    per_image = sum(a[0].nbytes for a in arrays.values()) + 4
    if N * per_image > DUMP_CAP_BYTES:
        keep = np.sort(np.random.default_rng(seed).choice(N, DUMP_CAP_BYTES // per_image, replace=False))
        arrays = {k: a[keep] for k, a in arrays.items()}
        arrays['image_index'] = keep.astype(np.float32)
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + '.npy'), np.ascontiguousarray(a))
    return sorted(arrays)


def parity_check(eng, arch, sd, cfg, R, x, offs_np, records, sample, tol=2e-5):
    """Outside the timed region: the last batch's device maps and records against the oracle on a
    sample of images.  (i) merged heatmaps / tags vs the full CPU pipeline, <= 2e-5; (ii) the
    reference-semantics parser fed the device maps must reproduce the records bit for bit."""
    from oracle import group_ref, inference_ref, net_ref, oks
    det, tag = eng.last_maps()
    ans, count, scores = records
    off0, off1, f0, f1 = offs_np
    idx = list(sample)
    xs = x[idx].cpu()
    with torch.no_grad():
        o = net_ref.forward(xs, sd, arch)
        of = net_ref.forward(torch.flip(xs, [3]), sd, arch)
        o = [o[0] + torch.from_numpy(off0[idx]), o[1] + torch.from_numpy(off1[idx])]
        of = [of[0] + torch.from_numpy(f0[idx]), of[1] + torch.from_numpy(f1[idx])]
        fh, tg = inference_ref.merge(o, of, inference_ref.TestCfg(), (R, R))
    dsel, tsel = det[idx].cpu().numpy(), tag[idx].cpu().numpy()
    err = max(float(np.abs(dsel - fh.numpy()).max()), float(np.abs(tsel - tg.numpy()).max()))
    ora = group_ref.HeatmapParser(group_ref.Params())
    ans, count, scores = ans.cpu().numpy(), count.cpu().numpy(), scores.cpu().numpy()
    same, persons = True, 0
    pcap = ans.shape[1]
    for k, n in enumerate(idx):
        a, sc = ora.parse_image(dsel[k], tsel[k])
        m = min(a.shape[0], pcap)
        same = same and int(count[n]) == a.shape[0] and np.array_equal(ans[n, :m], a[:m]) \
            and np.array_equal(scores[n, :m], sc[:m])
        persons += a.shape[0]
    # P3, reported not asserted: the GPU pipeline's records against the records of the PURE CPU pipeline
    # (CPU maps -> CPU parser) on the same sample -- persons matched by order, joints by position + presence
    joints = agree = same_cnt = 0
    oks_vals = []
    for k, n in enumerate(idx):
        a_cpu, _ = ora.parse_image(fh[k].numpy(), tg[k].numpy())
        m = min(int(count[n]), pcap)
        same_cnt += int(int(count[n]) == a_cpu.shape[0])
        # keypoint similarity in mAP's own unit: per CPU-pipeline person, OKS of its best one-to-one device match
        oks_vals += oks.image_oks([a_cpu[q] for q in range(a_cpu.shape[0])], [ans[n, q] for q in range(m)])
        for p_ in range(min(m, a_cpu.shape[0])):
            g, c = ans[n, p_], a_cpu[p_]
            joints += g.shape[0]
            agree += int(np.sum(np.all(g[:, :2] == c[:, :2], axis=1) & ((g[:, 2] > 0) == (c[:, 2] > 0))))
    return {'images': len(idx), 'heatmap_tag_max_abs_err': err, 'tolerance': tol,
            'records_identical_to_oracle_parser': bool(same), 'persons': persons,
            'p3_vs_pure_cpu_pipeline': {'images_same_person_count': same_cnt, 'joints_compared': joints,
                                        'joints_identical_position_and_presence': agree,
                                        'oks_vs_cpu_persons': oks.summary(oks_vals)},
            'ok': bool(same and err < tol)}


def arg_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', type=int, default=0, choices=[0, 1, 2, 3, 4, 5],
                    help='a BASELINE.json config as a preset of --arch / --size / --batch / --storage (5: search-M '
                         '512x512, 32 images per GPU, bf16 -- with --gpus 8 the 256-image workload of config 5)')
    ap.add_argument('--batch', type=int, default=None, help='images per GPU (default 64)')
    ap.add_argument('--arch', default=None, help='default search-XS')
    ap.add_argument('--size', type=int, default=0, help='input side (default: arch img_size)')
    ap.add_argument('--storage', default=None, choices=['f32', 'bf16'],
                    help='activation/weight storage (bf16: BASELINE configs 4/5; never the headline)')
    ap.add_argument('--parity-images', type=int, default=-1,
                    help='images of the last batch checked against the oracle outside the timed region: 0 = all, '
                         '-1 (default) = all when the CPU oracle is cheap (XS@256 b64: the headline), else 8 evenly spaced')
    ap.add_argument('--no-extra-configs', action='store_true',
                    help='default run only: do not attach BASELINE configs 4 / 5 (bench.py --config N in a child process)')
    ap.add_argument('--long-steps', type=int, default=200,
                    help='a second, longer timed run after the K-step one -> ms_per_step_200 (the driver\'s 20 steps are a '
                         '59 ms region: 2-3 % run-to-run; 0 = skip)')
    ap.add_argument('--no-small-batch', action='store_true',
                    help='skip the batch-1 / batch-8 latency legs (the reference\'s operating point, valid.py:195-196)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-kernel-profile', action='store_true')
    ap.add_argument("--cpu-images", type=int, default=24)
    ap.add_argument('--no-parity-check', action='store_true')
    ap.add_argument('--no-io-leg', action='store_true', help='skip the I/O-inclusive leg (value_with_io)')
    ap.add_argument('--shard-seed', type=int, default=-1, help='data seed offset (default: the rank)')
    ap.add_argument('--dump', default='', help='rank 0 saves the gathered records of the last step (npz)')
    ap.add_argument('--dump-outputs', default='', metavar='DIR',
                    help='rank 0 writes the records of the last timed step as float32 DIR/<name>.npy (dump_outputs)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline, also measure and check everything else: the --long-steps region, the parity '
                         'check, the I/O leg, single- and small-batch latencies, path / kernel rooflines, the CPU baseline '
                         'and (default workload, one rank) BASELINE configs 4 / 5; the --no-* options skip single legs')
    return ap


def main():
    ap = arg_parser()
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    default_run = not (args.config or args.arch or args.size or args.batch or args.storage)
    preset = CONFIGS.get(args.config, {})
    args.arch = args.arch or preset.get('arch', 'search-XS')
    args.size = args.size or preset.get('size', 0)
    args.batch = args.batch or preset.get('batch', 64)
    args.storage = args.storage or preset.get('storage', 'f32')

    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if args.gpus != world and world > 1:
        raise SystemExit('--gpus %d but WORLD_SIZE %d' % (args.gpus, world))
    if args.gpus > 1 and world == 1:
        respawn_under_torchrun(args.gpus)          # does not return
    # LP_BENCH_BACKEND=gloo + LP_BENCH_ONE_GPU=1: functional check of the N>1 code path on a 1-GPU box
    backend = os.environ.get('LP_BENCH_BACKEND', 'nccl')
    rank_slot = local_rank
    if os.environ.get('LP_BENCH_ONE_GPU'):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    affinity = gpu_affinity(local_rank, world, slot=rank_slot)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
        else:
            dist.init_process_group(backend)

    from litepose_amd import arch_zoo, config, engine, parallel
    from oracle import inference_ref, synth

    arch = arch_zoo.get(args.arch)
    R = args.size or arch['img_size']
    cfg = config.apply_arch(config.get_cfg(), arch)
    J = cfg.DATASET.NUM_JOINTS
    # head_gain 0.25: the random network's own heatmap noise stays below DETECTION_THRESHOLD,
    # so the people in the scene are the injected blobs (1..10 per image), as on real images
    sd = synth.make_state_dict(arch, seed=1234, head_gain=0.25)
    pcap = 30                                    # all-gather record capacity
    eng = engine.PoseEngine(cfg, arch, sd, person_capacity=pcap, storage=args.storage,
                            options=engine.options_from_env())     # LP_* experiment switches: read HERE, not in the engine
    B = args.batch
    # synthetic data, resident in HBM before the timed region; each rank gets its own shard
    shard = rank if args.shard_seed < 0 else args.shard_seed
    x = synth.make_images(B, R, seed=100 + shard).cuda()
    off0, off1 = synth.lowres_offsets(200 + shard, B, J, R)
    f0, f1 = synth.flip_offsets(off0, off1, inference_ref.FLIP_CONFIG['CROWDPOSE'])
    offs = (torch.from_numpy(np.concatenate([off0, f0])).cuda(),
            torch.from_numpy(np.concatenate([off1, f1])).cuda())

    # Software-pipelined serving loop (PoseEngine.submit): step k submits batch k and then collects + all-gathers
    # batch k - depth, so the AE stage of one batch runs under the convolutions of the next ones.  `run(K)` fully
    # completes K batches (last collects + gathers included).
    depth = eng.pipeline_depth()
    # the documented serving pattern: one staging buffer per buffer set, re-filled in place by the
    # loader; here they are filled once (same shard in each) and stay resident in HBM
    nset = eng.buffer_sets()
    xbuf = [x] + [x.clone() for _ in range(nset - 1)]
    obuf = [offs] + [tuple(o.clone() for o in offs) for _ in range(nset - 1)]
    turn = [0]

    def run(k):
        pending, out = [], None
        for _ in range(k):
            i = turn[0] % nset
            turn[0] += 1
            pending.append(eng.submit(xbuf[i], offsets=obuf[i]))
            if len(pending) > depth:
                h = pending.pop(0)
                out = parallel.all_gather_records(*h.result())
                h.release()
        for h in pending:
            out = parallel.all_gather_records(*h.result())
            h.release()
        return out

    # engine setup, not steps: buffer sets allocated and their hipGraphs captured for these staging buffers
    # (PoseEngine.prepare; submit would otherwise do it lazily during its first 8 calls)
    _log('engine built, preparing (graph capture)')
    eng.prepare(xbuf, offsets=obuf)
    _log('prepared: %s' % (eng.graph_stats(),))
    if args.warmup > 0:
        out = run(args.warmup)
    stats0 = eng.graph_stats()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(args.steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    stats1 = eng.graph_stats()
    # every timed step a pair of graph replays?  (a failed capture -- e.g. another thread's HIP call under
    # capture_error_mode='global' -- leaves a rank on eager launches for good: visible here, per rank)
    replayed = stats1['graph_replays'] - stats0['graph_replays']
    rank_info = [dt / args.steps * 1e3, float(replayed == args.steps and stats1['use_graphs']),
                 float(stats1['capture_failures'])]
    per_rank = [rank_info]
    if world > 1:
        dev_t = 'cuda' if backend == 'nccl' else 'cpu'
        t = torch.tensor(rank_info, dtype=torch.float64, device=dev_t)
        allr = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allr, t)
        per_rank = [[float(v) for v in r.tolist()] for r in allr]
        dt = max(r[0] for r in per_rank) * args.steps * 1e-3
    release_affinity()
    all_aff = [affinity]
    if world > 1:
        all_aff = [None] * world
        dist.all_gather_object(all_aff, affinity)
    ms_per_step = dt / args.steps * 1e3
    total_images = B * world * args.steps
    value = total_images / dt
    _log('timed run: %.4f ms/step' % ms_per_step)
    if rank == 0 and args.dump_outputs:
        # `out` is the last timed step's result: its buffer set is not written again before the next submit
        dumped = dump_outputs(args.dump_outputs, out, pcap)
        _log('outputs of the last timed step written to %s: %s' % (args.dump_outputs, ', '.join(dumped)))
    # a second, longer region: the same loop for --long-steps steps, bracketed the same way, max over
    # ranks -- a low-variance number beside the driver's K-step one, never instead of it
    ms_long = None
    if args.full and args.long_steps > args.steps:
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(args.long_steps)          # same content per buffer set: the records checked below are this run's last batch
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dl = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dl], dtype=torch.float64, device='cuda' if backend == 'nccl' else 'cpu')
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dl = float(t.item())
        ms_long = dl / args.long_steps * 1e3
        _log('long run: %.4f ms/step over %d steps' % (ms_long, args.long_steps))

    persons = int(out[1].clamp(max=pcap).sum().item())
    overflow = int((out[1] > pcap).sum().item())
    if rank == 0 and args.dump:
        np.savez(args.dump, kpts=out[0].cpu().numpy(), count=out[1].cpu().numpy(), scores=out[2].cpu().numpy())

    line = {
        'metric': 'images/sec end-to-end (backbone+deconv+AE-group), LitePose-%s@%d b%d'
                  % (args.arch.split('-')[-1], R, B),
        'value': round(value, 1), 'unit': 'images/s', 'n_gpus': world, 'steps': args.steps,
        'warmup': args.warmup, 'ms_per_step': round(ms_per_step, 4), 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': args.storage, 'data': 'synthetic',
        'config': {'baseline_config': baseline_config_of(args.arch, R, B, args.storage, args.config),
                   'workload': 'LitePose-Auto-%s %dx%d, batch %d per GPU, %s, flip-TTA, PROJECT2IMAGE, '
                               'NMS5 top-30, tag grouping, adjust+refine; random weights + synthetic blob scenes'
                               % (args.arch.split('-')[-1], R, R, B,
                                  'fp32 (1x1 convs / deconvs on the matrix cores either as fp32 MFMAs or as exact '
                                  'bf16x3-split products: 6 bf16 MFMAs accumulated in fp32, dropped terms <= 3*2^-24; '
                                  'depthwise convs and everything else fp32 FMAs)' if args.storage == 'f32' else
                                  'bf16 storage (activations + BN-folded weights bf16 in HBM; every stride-1 InvBottleneck '
                                  'as ONE launch that keeps its two expanded tensors on the CU: bf16 MFMA 1x1s, fp32 '
                                  'depthwise FMAs over the bf16-rounded values; bf16 MFMA deconvs and stride-2 blocks, '
                                  'head depthwise as banded bf16 MFMA products; fp32 accumulation / bias / activation / '
                                  'residual everywhere, every stored tensor rounded once; fp32 head outputs and fp32 '
                                  'AE stage)'),
                   'global_batch': B * world, 'parallelism': 'dp%d (shard images, all-gather records)' % world,
                   'persons_per_step': persons, 'records_overflowing_pcap': overflow,
                   'schedule': eng.options['sched'] + ': %d batches pending before the oldest is '
                               'collected (PoseEngine.submit: NET stages on two streams, AE stages on a third, '
                               '%d buffer sets each fed from its own staging buffer, one hipGraph per stage, captured '
                               'in PoseEngine.prepare() before the warm-up steps)' % (depth, nset)},
        # 8-GPU runs are the driver's: nothing in this line is a measured scaling claim
        'scaling_measured': world > 1,
        # did the serving loop run as hipGraph replays on EVERY rank (False = some rank fell back to eager launches)
        'graph_replay': all(r[1] == 1.0 for r in per_rank),
        'per_rank': {'ms_per_step': [round(r[0], 4) for r in per_rank],
                     'graph_replay': [bool(r[1]) for r in per_rank],
                     'capture_failures': [int(r[2]) for r in per_rank],
                     'affinity': all_aff},
        'graphs': stats1,
        'ms_per_step_200': None if ms_long is None else round(ms_long, 4),
        'long_steps': args.long_steps if ms_long is not None else 0,
    }
    if rank == 0 and args.full and not args.no_parity_check:
        _log('parity check')
        local = (out[0][:B], out[1][:B], out[2][:B])          # rank 0's own shard of the gathered records
        # bf16 storage: the heatmap error against the fp32 oracle is a BUDGET (reported, <= 3e-2 on maps of
        # range ~1; measured ~6e-3), the records must still be bit-exact on the device's own maps
        if args.parity_images < 0:       # auto: the headline keeps every image; the big shapes a bounded sample
            args.parity_images = 0 if B * R * R <= 64 * 256 * 256 else 8
        npar = B if args.parity_images <= 0 else min(B, args.parity_images)
        sample = range(B) if npar == B else sorted({int(round(i * (B - 1) / max(1, npar - 1))) for i in range(npar)})
        pc = parity_check(eng, arch, sd, cfg, R, x, (off0, off1, f0, f1), local, sample=sample,
                          tol=2e-5 if args.storage == 'f32' else 3e-2)
        line['parity_checked'] = pc['ok']
        line['parity'] = pc
    elif rank == 0:
        line['parity_checked'] = False
    # ---- I/O-inclusive leg (reported BESIDE the headline, never instead of it): what the reference loop body also
    # does around the path (valid.py:178-186,213: ToTensor + Normalize + H2D; :232-245: results on the host).  uint8
    # HWC images in pinned host memory -> H2D (12.5 MB per 64 images) -> lp_preprocess_batch -> the same serving loop
    # -> packed records D2H into pinned memory, pipelined over the same buffer sets on a loader stream.
    io = None
    if args.full and not args.no_io_leg:   # after the dump / parity check: this leg re-uses (overwrites) the engine's buffer sets
        loader = engine.StagedLoader(eng, B, R, R, own_stream=os.environ.get('LP_IO_OWN_STREAM') == '1')
        g = torch.Generator().manual_seed(300 + shard)
        u8 = torch.randint(0, 256, (B, R, R, 3), dtype=torch.uint8, generator=g)
        for hbuf in loader.host_u8:
            hbuf.copy_(u8)
        _log('I/O leg: preparing')
        eng.prepare(loader.x, offsets=obuf)
        _log('I/O leg: prepared')

        def run_io(k):
            # batch k+1's images cross PCIe and are normalised on the loader stream while batch k is submitted and
            # batch k - depth is collected
            pending, out = [], None
            i = turn[0] % nset
            loader.start(i)
            for _ in range(k):
                turn[0] += 1
                nxt = turn[0] % nset
                pending.append((i, eng.submit(loader.get(i), offsets=obuf[i])))
                loader.start(nxt)
                i = nxt
                if len(pending) > depth:
                    j, h = pending.pop(0)
                    out = parallel.all_gather_records(*h.result())
                    loader.store(j, *out)
                    h.release()
            for j, h in pending:
                out = parallel.all_gather_records(*h.result())
                loader.store(j, *out)
                h.release()
            for j in range(nset):
                loader.wait(j)
            return out
        turn[0] = 0
        run_io(max(args.warmup, nset))
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out_io = run_io(args.steps)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt_io = time.perf_counter() - t1
        _log('I/O leg: %.4f ms/step' % (dt_io / args.steps * 1e3))
        if world > 1:
            t = torch.tensor([dt_io], dtype=torch.float64, device='cuda' if backend == 'nccl' else 'cpu')
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_io = float(t.item())
        io = {'value_with_io': round(total_images / dt_io, 1), 'ms_per_step_with_io': round(dt_io / args.steps * 1e3, 4),
              'h2d_bytes_per_step': int(u8.numel()), 'd2h_bytes_per_step': int(loader.host_rec[0].numel() * 4),
              'persons_per_step': int(out_io[1].clamp(max=pcap).sum().item()),
              'what': 'uint8 HWC images pinned on the host -> H2D -> lp_preprocess_batch (ToTensor+Normalize, '
                      'valid.py:178-186,213) -> the same pipelined path -> packed records D2H to pinned host memory '
                      '(valid.py:232-245), own staging triple per buffer set, transfers of batch k+1 issued right after '
                      'batch k is submitted'}
    if io is not None:
        line['value_with_io'] = io['value_with_io']
        line['io'] = io
    if rank == 0 and args.full:
        # un-pipelined latency of ONE batch (infer_batch, nothing to hide the AE stage behind)
        lat = []
        for _ in range(7):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            eng.infer_batch(x, offsets=offs)
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t1) * 1e3)
        line['latency_ms_single_batch'] = round(sorted(lat)[len(lat) // 2], 4)
        # the same batch through the serving API with nothing else in flight: submit (the NET and AE graph replays the timed
        # loop uses) -> result -> host sync, median of 15.  infer_batch above launches ~180 kernels one by one in two halves.
        lat_g = []
        for _ in range(15):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            with eng.submit(x, offsets=offs) as _res:
                pass
            torch.cuda.synchronize()
            lat_g.append((time.perf_counter() - t1) * 1e3)
        line['latency_ms_single_batch_graph'] = round(sorted(lat_g)[len(lat_g) // 2], 4)
    if rank == 0 and args.full and not args.no_small_batch:
        # the reference's own operating point (valid.py:195-196 asserts batch 1; VERDICT r05 missing #2): one batch of 1 / 8
        # images through the whole path with nothing else in flight -- submit (two graph replays) -> result -> host sync,
        # median of 25 after the captures; `eager_ms` = the same batch through infer_batch (plain launches)
        line['latency_small_batch'] = {}
        for nb in (1, 8):
            xs = synth.make_images(nb, R, seed=400 + nb).cuda()
            o0, o1 = synth.lowres_offsets(500 + nb, nb, J, R)
            g0, g1 = synth.flip_offsets(o0, o1, inference_ref.FLIP_CONFIG['CROWDPOSE'])
            os_ = (torch.from_numpy(np.concatenate([o0, g0])).cuda(), torch.from_numpy(np.concatenate([o1, g1])).cuda())
            eng.prepare(xs, offsets=os_)
            lat, lat_e = [], []
            for _ in range(25):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                with eng.submit(xs, offsets=os_) as (ka, kc, ks_):
                    pass
                torch.cuda.synchronize()
                lat.append((time.perf_counter() - t1) * 1e3)
            persons_nb = int(kc.clamp(max=pcap).sum().item())
            for _ in range(9):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.infer_batch(xs, offsets=os_)
                torch.cuda.synchronize()
                lat_e.append((time.perf_counter() - t1) * 1e3)
            med = sorted(lat)[len(lat) // 2]
            line['latency_ms_batch%d' % nb] = round(med, 4)
            line['latency_small_batch'][str(nb)] = {
                'ms': round(med, 4), 'min_ms': round(min(lat), 4), 'eager_ms': round(sorted(lat_e)[len(lat_e) // 2], 4),
                'images_per_s': round(nb / (med * 1e-3), 1), 'persons': persons_nb, 'graph_replay': True,
                'what': 'LitePose-Auto-%s %dx%d, batch %d, %s, full path (flip-TTA, NMS, grouping, adjust+refine): submit '
                        '-> result -> synchronize, nothing else in flight, median of 25'
                        % (args.arch.split('-')[-1], R, R, nb, args.storage)}
            _log('latency batch %d: %.4f ms (eager %.4f)' % (nb, med, line['latency_small_batch'][str(nb)]['eager_ms']))
    if rank == 0 and args.full:
        b_op, b_post = algorithmic_bytes_per_image(arch, J, R, cfg.TEST.FLIP_TEST,
                                                   act_bytes=4 if args.storage == 'f32' else 2)
        F = 2 if cfg.TEST.FLIP_TEST else 1
        path_bytes = B * (F * b_op + b_post)
        cfgkey = {'arch': args.arch, 'size': R, 'batch': B, 'storage': args.storage}
        tsrc, tfile = traffic_file(cfgkey)
        real = None
        if tfile is not None:
            real = int(sum(v.get('hbm_bytes_per_forward', 0) for v in tfile['kernels'].values()))
        line['path_roofline'] = {
            'bound': 'hbm', 'bytes_per_step': path_bytes,
            'achieved': round(path_bytes / (ms_per_step * 1e-3) / 1e9, 1), 'peak': HBM_PEAK_GBS,
            'unit': 'GB/s', 'frac': round(path_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            'note': 'whole step incl. AE stage vs N*(F*B_op+B_post), SURVEY.md 8(d).  B_op-EQUIVALENT: the bytes the '
                    'reference ops would move op by op; the fused kernels keep most of them on the CU, so this is not '
                    'HBM utilisation (real HBM traffic of one step from the PMC passes of %s: %s) -- the honest fraction of '
                    'a fused path is frac_flops'
                    % (tsrc or 'no committed traffic file for this configuration',
                       '%.2f GB = %.2f of the HBM peak at this step time' % (real / 1e9, real / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS)
                       if real else 'n/a'),
            'hbm_traffic_bytes_per_step': real, 'traffic_source': tsrc}
        if not args.no_kernel_profile:
            _log('kernel profile')
            # per-kernel HIP-event timing of the network launches (own pass, outside the timed region)
            m = eng.model
            m.set_profiling(True)
            agg = {}
            reps = 3
            for rep in range(reps + 1):
                eng.forward_maps(x, offs)
                prof = m.profile(launches=True)
                if rep == 0:        # untimed: first launches on this stream (buffers of this engine instance are
                    continue        # allocated, a spilling kernel makes the runtime allocate the queue's scratch)
                for name, ms, by, fl, fv, (grid, _thr, _lds, per_cu) in prof:
                    fam = name.split('|')[1] if '|' in name else name      # the HIP kernel that ran
                    if fam.startswith('(fused'):
                        continue
                    a = agg.setdefault(fam, [0.0, 0, 0, 0, 0, 0.0])
                    a[0] += ms
                    a[1] += by
                    a[2] += fl
                    a[3] += 1
                    a[4] += fv
                    a[5] += ms * cus_occupied(grid, per_cu)         # time-weighted CUs the launch can hold
            m.set_profiling(False)
            dom = max(agg.items(), key=lambda kv: kv[1][0])
            fam, (ms, by, fl, cnt, fv, cu_ms) = dom
            gbs, tfs = by / (ms * 1e-3) / 1e9, fl / (ms * 1e-3) / 1e12
            # fused kernels move far fewer bytes than the B_op of the reference ops they replace, so both fractions
            # are reported: algorithmic B_op bytes vs 8 TB/s, and the FLOP floor -- the two FLOP classes of the launch
            # each at its own peak (price_flops) -- vs the measured time.  `frac` is the larger; neither can exceed 1
            # unless B_op-equivalent bytes exceed what HBM could move, which the byte fraction then says openly.
            pr = price_flops(fl, fv, ms, args.storage)
            frac_hbm, frac_fl = gbs / HBM_PEAK_GBS, pr['frac_flops']
            if frac_hbm >= frac_fl:
                rl = {'bound': 'hbm', 'achieved': round(gbs, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                      'frac': round(frac_hbm, 4)}
            else:       # time floor of the launch's FLOPs (vector-pipe FMAs + matrix-core products) / measured time
                eff_peak = fl / max(1e-30, pr['floor_ms_sum'] * 1e-3) / 1e12
                rl = {'bound': 'mfma', 'achieved': round(tfs, 2), 'peak': round(eff_peak, 1), 'unit': 'TFLOP/s',
                      'frac': round(frac_fl, 4),
                      'peak_note': 'FLOP-weighted peak of the launch: depthwise FMAs at %.1f TF (vector pipe), 1x1 / '
                                   'deconv products at %.1f TF (matrix cores, %s)'
                                   % (FP32_PEAK_TFLOPS, pr['mfma_peak_tflops'],
                                      'fp32-exact arithmetic' if args.storage == 'f32' else 'dense bf16')}
            tr, src = pmc_traffic(fam, cnt // reps, cfgkey)
            rl.update({'kernel': fam, 'traffic': tr, 'traffic_source': src, 'launches': cnt // reps,
                       'avg_launch_us': round(ms / cnt * 1e3, 2), 'alg_bytes_per_launch': by // cnt,
                       'alg_flops_per_launch': fl // cnt, 'alg_flops_valu_per_launch': fv // cnt,
                       'alg_gbps': round(gbs, 1), 'tflops': round(tfs, 2),
                       'hbm_gbps': round(tr / (ms / cnt * 1e-3) / 1e9, 1) if tr else None,
                       'frac_alg_bytes': round(frac_hbm, 4), 'frac_flops': round(frac_fl, 4),
                       'flop_floor_ms_per_launch': round(pr['floor_ms_sum'] / cnt, 6),
                       'timing': 'HIP events per launch on the launch stream, one stream, %d forwards' % reps})
            # how much of the chip the family's grids can hold at all (mb16_kernel is one workgroup per
            # image = 128 workgroups on 256 CUs, the other NET stream fills the rest): time-weighted over its launches
            occ = cu_ms / ms if ms > 0 else float(N_CUS)
            rl['cus_occupied'] = round(occ, 1)
            rl['cus_total'] = N_CUS
            rl['frac_flops_per_occupied_cu'] = round(frac_fl * N_CUS / max(occ, 1.0), 4)
            rl['cus_note'] = ('min(%d, grid workgroups / workgroups per CU by the HIP occupancy query), time-weighted over the '
                              'family\'s launches; frac_flops is a fraction of the whole chip' % N_CUS)
            line['roofline'] = rl
            # alg_gbps = B_op-EQUIVALENT bytes of the reference ops the launch replaces / time: may exceed the HBM peak for a
            # fused kernel (that is what fusion is for); hbm_gbps = the PMC-counted traffic / time, always below it
            def kernel_entry(k, v):
                hb = pmc_traffic(k, v[3] // reps, cfgkey)[0]
                return {'ms_per_step': round(v[0] / reps, 4), 'launches': v[3] // reps,
                        'cus_occupied': round(v[5] / v[0], 1) if v[0] > 0 else None,
                        'alg_gbps': round(v[1] / (v[0] * 1e-3) / 1e9, 1),
                        'tflops': round(v[2] / (v[0] * 1e-3) / 1e12, 2),
                        'hbm_traffic_per_launch': hb,
                        'hbm_gbps': round(hb * v[3] / (v[0] * 1e-3) / 1e9, 1) if hb else None}
            line['kernels'] = {k: kernel_entry(k, v) for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])}
            net_ms = sum(v[0] for v in agg.values()) / reps
            line['network_ms_single_stream'] = round(net_ms, 4)
            F2 = 2 if cfg.TEST.FLIP_TEST else 1
            # whole path: the FLOP floor of one step's network launches (both classes at their own peaks) / step time
            ppr = price_flops(sum(v[2] for v in agg.values()) / reps, sum(v[4] for v in agg.values()) / reps,
                              ms_per_step, args.storage)
            line['path_roofline']['frac_flops'] = ppr['frac_flops']
            line['path_roofline']['flop_floor'] = ppr
            if args.storage == 'f32':
                # the second legitimate yardstick: the 1x1 / deconv products of the fp32 path run on the
                # bf16 matrix pipe as 6 MFMAs each -- priced at what THAT pipe can deliver (2 500 / 6 = 417 TF fp32-equivalent)
                p3 = price_flops(sum(v[2] for v in agg.values()) / reps, sum(v[4] for v in agg.values()) / reps,
                                 ms_per_step, args.storage, mfma_peak=BF16X3_EQUIV_TFLOPS)
                line['path_roofline']['frac_flops_bf16x3'] = p3['frac_flops']
                line['path_roofline']['flop_floor_bf16x3'] = p3
        if world == 1 and not args.no_cpu_baseline:
            _log('cpu baseline')
            line['cpu_baseline'] = cpu_baseline(arch, sd, cfg, R, args.cpu_images, (off0, off1, f0, f1))
        if world == 1 and default_run and not args.no_extra_configs:
            # the children measure on an otherwise idle GPU: drop this process's engine, graphs and buffers first
            try:
                eng.reset_graphs()
                del loader
            except Exception:
                pass
            eng = None
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            # BASELINE configs 4 / 5 (per GPU) as child runs, attached to THIS line so the driver's record carries them
            line['configs'] = {}
            for n_cfg in (4, 5):
                _log('BASELINE config %d (child process)' % n_cfg)
                line['configs'][str(n_cfg)] = run_extra_config(n_cfg, args.steps, args.warmup)
    if rank == 0:
        _log('done')
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
