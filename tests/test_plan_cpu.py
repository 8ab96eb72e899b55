"""The network plan, pinned on the CPU: tests/plan_digest.cpp links csrc/plan.cpp alone (no HIP), builds the plan of a
fixed list of nets from generated weights and prints, per net, digests of the packed weight arena, of the op list and of
the buffer plan -- or the refusal's message.  tests/golden/plan_digests.txt holds the lines the engine gave BEFORE plan.cpp
was cut out of it (the same program compiled around that engine.cpp, see the head of plan_digest.cpp): a line that
differs is a change of the bytes the kernels read, of buffer ids or of a refusal, never a reason to regenerate."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_bytes_ops_and_buffers_match_the_recorded_digests(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path / 'plan_digest')
    r = subprocess.run([hipcc, '-x', 'c++', '-O2', '-std=c++17', os.path.join(ROOT, 'tests', 'plan_digest.cpp'),
                        os.path.join(ROOT, 'litepose_amd', 'csrc', 'plan.cpp'), '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    with open(os.path.join(ROOT, 'tests', 'golden', 'plan_digests.txt')) as f:
        want = f.read().splitlines()
    got = r.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
