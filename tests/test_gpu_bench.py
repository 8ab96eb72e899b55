"""bench.py itself on the GPU: a plain run prints the headline and nothing it did not measure; `--full` runs every other leg
after it.  Each run is a child process, as the benchmark is always started."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only --full measures
FULL_ONLY = ('parity', 'path_roofline', 'roofline', 'kernels', 'network_ms_single_stream', 'cpu_baseline', 'configs',
             'io', 'value_with_io', 'latency_ms_single_batch', 'latency_ms_single_batch_graph', 'latency_small_batch',
             'latency_ms_batch1', 'latency_ms_batch8')


def _bench(args, timeout):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), wall


def test_plain_run_prints_the_headline_only(tmp_path):
    """The default workload (XS@256, 64 images): the contract keys, every timed step a graph replay, --dump-outputs
    written, and no figure of a leg that did not run."""
    steps, warmup = 4, 2
    line, wall = _bench(['--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                         '--dump-outputs', str(tmp_path / 'out')], timeout=300)
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'n_gpus'):
        assert k in line, k
    assert line['unit'] == 'images/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['steps'] == steps and line['warmup'] == warmup and line['config']['baseline_config'] == 3
    assert abs(line['value'] - 64e3 / line['ms_per_step']) < 0.01 * line['value']
    assert line['graph_replay'] is True and line['graphs']['capture_failures'] == 0
    assert line['parity_checked'] is False and line['ms_per_step_200'] is None and line['long_steps'] == 0
    assert not [k for k in FULL_ONLY if k in line], [k for k in FULL_ONLY if k in line]
    count = np.load(str(tmp_path / 'out' / 'count.npy'))
    assert count.shape == (64,) and np.minimum(count, 30).sum() == line['config']['persons_per_step']
    print('plain run: %.1f s wall, %.1f s outside the %d steps' % (wall, wall - (steps + warmup) * line['ms_per_step'] * 1e-3,
                                                                  steps + warmup))


def test_full_run_adds_every_other_leg():
    """--full on a small non-default workload (no config children): the --long-steps region, parity, I/O leg, latencies,
    rooflines, per-kernel times and the CPU baseline are all in the line, and the parity check passes."""
    line, _ = _bench(['--gpus', '1', '--steps', '3', '--warmup', '2', '--batch', '8', '--long-steps', '6',
                      '--cpu-images', '2', '--full'], timeout=600)
    assert line['graph_replay'] is True and line['config']['baseline_config'] is None
    assert line['long_steps'] == 6 and line['ms_per_step_200'] > 0
    assert line['parity_checked'] is True and line['parity']['images'] == 8
    assert line['value_with_io'] > 0 and line['latency_ms_single_batch'] > 0 and line['latency_ms_single_batch_graph'] > 0
    assert line['latency_ms_batch1'] > 0 and line['latency_ms_batch8'] > 0
    assert line['path_roofline']['bytes_per_step'] > 0 and 0 < line['path_roofline']['frac_flops'] < 1
    assert line['roofline']['kernel'] in line['kernels'] and line['network_ms_single_stream'] > 0
    assert line['cpu_baseline']['kind'] == 'port' and line['cpu_baseline']['value'] > 0
    assert 'configs' not in line
