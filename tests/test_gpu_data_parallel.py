"""Data-parallel training with two ranks on the one GPU under gloo (tests/_dp_worker.py is a rank): synchronised BatchNorm
through ``convert_sync_batchnorm``, ``GradBucket``, ``broadcast_state`` and ``do_train(group=...)``.

Gradient step: the case of tests/_train_net_case.py split one image per rank.  With synchronised BatchNorm the two ranks
together compute the golden step, so the concatenated outputs, every bucket gradient and the running tensors are held to
the rules of tests/test_gpu_train_net.py against the golden's fp64 -- four times the largest error the reference's own
fp32 shows in the pool (the pools are formed from the golden's fp32, so the reference is within them by construction);
and the same run WITHOUT the conversion must break the rule for the outputs (at 64 x 64 the deepest planes are 2 x 2: a
rank alone normalises four cells per channel).  The bucket gradients and the running buffers are the same bits on both ranks.

``do_train``: two steps of the library's SGD at lr = 0.25 on a four-image set sharded two and two, after rank 1 started
from other weights and ``broadcast_state`` made it equal: p == p_before - lr * (bucket mean) bitwise after each step, every
parameter and buffer equal across the ranks, and a second run gives the same bits.

Each rank is a fresh child under its own ``timeout -k 10``; the first child that fails ends its sibling; nothing is
retried, and after a failed pair no further pair is started.  Measured ratios: DESIGN.md 4h."""
import concurrent.futures
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _poison as po
import _train_net_case as TC
from conftest import ROOT

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LR = 0.25
WORKER = os.path.join(ROOT, 'tests', '_dp_worker.py')
LIMIT = 120          # seconds per child: torch's import, the library's load and a handful of steps
_failed = []


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _run_pair(mode, out, world=2):
    """-> the list of the ranks' results.  Ends the sibling as soon as one child fails."""
    if _failed:
        pytest.fail('rank pair %r failed earlier: no further process is started on the GPU' % _failed[0])
    out = str(out)
    port = _free_port()
    logs = [open(os.path.join(out, 'rank%d.log' % r), 'w') for r in range(world)]
    procs = [subprocess.Popen(['timeout', '-k', '10', str(LIMIT), sys.executable, WORKER, mode, str(r), str(world),
                               str(port), out], stdout=logs[r], stderr=subprocess.STDOUT, cwd=ROOT)
             for r in range(world)]
    try:
        with concurrent.futures.ThreadPoolExecutor(world) as pool:
            waits = [pool.submit(p.wait) for p in procs]
            for done in concurrent.futures.as_completed(waits):
                if done.result() != 0:
                    for q in procs:
                        if q.poll() is None:
                            q.terminate()                   # timeout passes the signal on to the rank
    finally:
        for f in logs:
            f.close()
    codes = [p.returncode for p in procs]
    if any(codes):
        _failed.append(mode)
        tails = [open(os.path.join(out, 'rank%d.log' % r)).read()[-1500:] for r in range(world)]
        pytest.fail('%s: exit codes %s\n%s' % (mode, codes, '\n-----\n'.join(tails)))
    return [torch.load(os.path.join(out, 'rank%d.pt' % r), weights_only=False) for r in range(world)]


@pytest.fixture(scope='module')
def case():
    return TC.load()


@pytest.fixture(scope='module')
def step_sync(tmp_path_factory):
    return _run_pair('step_sync', tmp_path_factory.mktemp('step_sync'))


@pytest.fixture(scope='module')
def step_plain(tmp_path_factory):
    return _run_pair('step_plain', tmp_path_factory.mktemp('step_plain'))


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    return _run_pair('train', tmp_path_factory.mktemp('train'))


def _rel(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _output_ratio(case, ranks):
    """the rule's unit for the outputs, concatenated in rank order: e / (largest e of the reference's fp32 outputs)"""
    pool = max(_rel(case['out%d_32' % s], case['out%d_64' % s]) for s in range(2))
    return max(_rel(torch.cat([r['outs'][s] for r in ranks]), case['out%d_64' % s]) for s in range(2)) / pool


def test_two_ranks_compute_the_golden_step(case, step_sync):
    """the 4-times rule of tests/test_gpu_train_net.py for the concatenated outputs and every bucket gradient"""
    pools, worst = {}, {}
    for k in case['params']:
        kind = TC.kind_of(k, case['shapes'][k])
        pools[kind] = max(pools.get(kind, 0.0), _rel(case['grad_32'][k], case['grad_64'][k]))
    assert sorted(pools) == ['beta', 'deconv', 'dw', 'gamma', 'pw', 'stem']
    grads = step_sync[0]['grads']
    assert sorted(grads) == sorted(case['params'])
    mine = {}
    for k in case['params']:
        kind = TC.kind_of(k, case['shapes'][k])
        mine[k] = (kind, _rel(grads[k], case['grad_64'][k]))
        worst[kind] = max(worst.get(kind, 0.0), mine[k][1] / pools[kind])
    worst['output'] = _output_ratio(case, step_sync)
    for kind in sorted(worst):
        print('%-7s largest e / (largest reference e of the kind) = %.3f' % (kind, worst[kind]))
    for k, (kind, e) in mine.items():
        assert e <= 4 * pools[kind], (k, kind, e / pools[kind])
    assert worst['output'] <= 4
    # a rank's own gradient is its share: the bucket mean is not it
    assert not all(po.bitwise_equal(step_sync[0]['own'][k], grads[k]) for k in grads)


def test_running_pairs_of_two_ranks_against_the_golden_step(case, step_sync):
    m = 0.1
    pools = {}
    for k in case['buffers']:
        kind = k.rsplit('.', 1)[1]
        pools[kind] = max(pools.get(kind, 0.0), _rel(case['run_32'][k], case['run_64'][k]))
    worst = 0.0
    sd = step_sync[0]['sd']
    for k in case['buffers']:
        f = np.asarray(case['run_64'][k], np.float64)
        r0 = (1 - m) * case['sd'][k].astype(np.float64)
        terms = np.abs(r0) + np.abs(f - r0)
        bound = 3 * U * np.linalg.norm(terms) + 4 * pools[k.rsplit('.', 1)[1]] * np.linalg.norm(f)
        err = np.linalg.norm(sd[k].double().numpy() - f)
        worst = max(worst, err / bound)
        assert err <= bound, (k, err / bound)
    print('running pairs: largest error / bound = %.3f' % worst)
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith('num_batches_tracked'))


def test_both_ranks_hold_the_same_gradients_and_buffers(step_sync):
    a, b = step_sync
    assert all(po.bitwise_equal(a['grads'][k], b['grads'][k]) for k in a['grads'])
    assert all(po.bitwise_equal(a['sd'][k], b['sd'][k]) for k in a['sd'])
    assert not all(po.bitwise_equal(a['own'][k], b['own'][k]) for k in a['own'])
    assert not po.bitwise_equal(a['outs'][0], b['outs'][0])


def test_without_the_conversion_the_outputs_break_the_rule(case, step_plain):
    """the power of the test above: per-rank BatchNorm is another function"""
    ratio = _output_ratio(case, step_plain)
    print('outputs without convert_sync_batchnorm: e / (largest reference e) = %.1f (the rule allows 4)' % ratio)
    assert ratio > 4
    a, b = step_plain
    assert not all(po.bitwise_equal(a['sd'][k], b['sd'][k]) for k in a['sd'] if k.endswith('running_mean'))
    assert all(po.bitwise_equal(a['grads'][k], b['grads'][k]) for k in a['grads'])      # the bucket still agrees


def test_broadcast_state_makes_rank_1_equal_to_rank_0(case, trained):
    a, b = (r['runs'][0] for r in trained)
    assert not any(po.bitwise_equal(a['before_broadcast'][k], b['before_broadcast'][k]) for k in a['start'])
    for k, v in a['start'].items():
        assert po.bitwise_equal(v, a['before_broadcast'][k]), k          # the source keeps its state
        assert po.bitwise_equal(v, b['start'][k]), k
        if not k.endswith('num_batches_tracked'):
            assert np.array_equal(v.numpy(), case['sd'][k]), k


def test_do_train_steps_with_the_mean_gradient_on_every_rank(trained):
    for r in trained:
        for run in r['runs']:
            assert run['images'] == [[2], [2]]                           # four images, two and two, one batch per epoch
            for st in run['steps']:
                assert np.isfinite(st['heat'])
                for k, p in st['p_after'].items():
                    assert bool(st['grad'][k].any()), k
                    assert po.bitwise_equal(p, st['p_before'][k] - LR * st['grad'][k]), k
            assert all(int(v) == 2 for k, v in run['steps'][1]['sd'].items() if k.endswith('num_batches_tracked'))
    a, b = (r['runs'][0] for r in trained)
    for sa, sb in zip(a['steps'], b['steps']):
        assert all(po.bitwise_equal(sa['grad'][k], sb['grad'][k]) for k in sa['grad'])
        assert all(po.bitwise_equal(sa['sd'][k], sb['sd'][k]) for k in sa['sd'])
        assert sa['heat'] != sb['heat']                                  # the meters are the rank's own
    assert not all(po.bitwise_equal(a['steps'][1]['sd'][k], a['start'][k]) for k in a['start'])


def test_a_second_run_gives_the_same_bits(trained):
    for r in trained:
        first, second = r['runs']
        for sa, sb in zip(first['steps'], second['steps']):
            assert all(po.bitwise_equal(sa['grad'][k], sb['grad'][k]) for k in sa['grad'])
            assert all(po.bitwise_equal(sa['sd'][k], sb['sd'][k]) for k in sa['sd'])
            assert sa['heat'] == sb['heat']
