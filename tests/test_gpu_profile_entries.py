"""The profile of a forward, entry by entry: ``(name|kernel tag, bytes, flops, flops_valu)`` of every launch that
``lp_net_profile2`` reports, for a table of cases that reaches every fusion rule of ``lp_net_forward`` and every case of
its one-launch-per-op switches, in both storages.  bench.py prices its rooflines from these numbers.

  * Every case's entry list equals ``tests/golden/profile_entries.json`` exactly and in order.  THE GOLDEN FILE WAS RECORDED
    FROM THE PARENT OF THE COMMIT THAT ADDED THIS TEST (c69402e, the engine whose forwards computed each entry's cost and
    name inline), with this module's record mode on a checkout of that commit::

        python tests/test_gpu_profile_entries.py --record tests/golden/profile_entries.json

    It is never recorded from the code under test: an entry that differs is a change of what the profile reports.
  * The golden file covers every rule and every switch case: a hit count per rule, taken from the entry names and tags
    (``RULES``), is at least one.  This part needs no GPU.
  * Independent of the golden file: a fused entry costs the sum of the reference ops it replaces.  The same case runs
    again with every fusion option of its storage at 0 (``UNFUSED``; "headfuse" is a public option key, so the fp32 heads
    are included), and each fused entry's ``flops``, ``flops_valu`` and ``bytes`` must equal the sums over the unfused
    entries of the ops its name covers.  The bytes of a 16-bit whole-block entry (``launch_mbtb``) are the launch's own
    traffic by definition and are held by the golden file only.  The fp32 stem's ``dw3+pw`` entry (dwpw_kernel<3>) has no
    option that splits it; it is a term of the fused stem's sum and is held by the golden file.
Needs a real MI355X."""
import json
import os
import re
import sys

import pytest

from conftest import ROOT
from oracle import synth

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'profile_entries.json')
RECORDED_FROM = 'c69402e'

# (id, family, arch, storage, H, W, N, flip, options).  family: mobilenet = the Fusion Deconv Head nets of the zoo,
# simplenet = the plain-head net of tests/test_gpu_simplenet.py, resnet = the family-1 table of tests/test_gpu_resnet.py
CASES = [
    # ---- fp32
    ('f32_xs256_nb48', 'mobilenet', 'search-XS', 'f32', 256, 256, 24, 2, {}),          # mb16 run at the NB >= 48 gate, mbt,
    #                                                                       mbt_s2, mbconv2, stem4, two-source headfuse
    ('f32_xs256_nb48_run0', 'mobilenet', 'search-XS', 'f32', 256, 256, 24, 2, {'mb16_run': 0}),   # one block per mb16 launch
    ('f32_xs256_n2', 'mobilenet', 'search-XS', 'f32', 256, 256, 2, 0, {}),             # below the gate: pw3 / dw_pair16 / pw
    ('f32_xs256_n2_chain', 'mobilenet', 'search-XS', 'f32', 256, 256, 2, 0, {'mbt': 0, 'mbt_s2': 0, 'mbconv2': 0}),
    #                                                      dwpw_kernel and the unfused DWPW fallback with its two entries
    ('f32_xs128x192_stem0', 'mobilenet', 'search-XS', 'f32', 128, 192, 2, 2, {'stem': 0}),   # stem_kernel + dwpw<3>
    ('f32_xs16', 'mobilenet', 'search-XS', 'f32', 16, 16, 3, 2, {}),                   # heads headfuse refuses: dw + dw + pw
    ('f32_l128', 'mobilenet', 'search-L', 'f32', 128, 128, 2, 0, {}),                  # stride-2 chain, both deconv forms
    ('f32_plain64', 'simplenet', 'search-XS', 'f32', 64, 64, 2, 2, {}),                # one-source head chain and deconv
    ('f32_plain256', 'simplenet', 'search-XS', 'f32', 256, 256, 1, 0, {}),             # (added) one-source headfuse launch
    ('f32_resnet64', 'resnet', None, 'f32', 64, 64, 2, 2, {}),                         # OP_CONVK
    # ---- bf16
    ('bf16_s224', 'mobilenet', 'search-S', 'bf16', 224, 224, 3, 2, {}),                # mbtb, mbtb_s2, stem4, headb, deconvb
    ('bf16_s224_mbtb0', 'mobilenet', 'search-S', 'bf16', 224, 224, 3, 2, {'mbtb': 0}),       # per-op chain
    ('bf16_s224_stem0', 'mobilenet', 'search-S', 'bf16', 224, 224, 3, 2, {'stem': 0}),       # unfused stem
    ('bf16_s224_headb0', 'mobilenet', 'search-S', 'bf16', 224, 224, 3, 2, {'headb': 0}),     # unfused head
    ('bf16_s224_dwt0', 'mobilenet', 'search-S', 'bf16', 224, 224, 3, 2, {'dwt': 0}),   # dwb everywhere, no headb launch
    ('bf16_l128', 'mobilenet', 'search-L', 'bf16', 128, 128, 1, 0, {}),                # 160-channel blocks: pwb / dwt / pwb
    ('bf16_plain128', 'simplenet', 'search-XS', 'bf16', 128, 128, 2, 2, {}),           # one-source headb
    # ---- f16: the format flag reaches every launcher
    ('f16_s224', 'mobilenet', 'search-S', 'f16', 224, 224, 3, 2, {}),
]
CASE_IDS = [c[0] for c in CASES]

# every fusion option at 0 (the keys that exist for the storage): one launch per reference op
UNFUSED = {'f32': {'mbt': 0, 'mbt_s2': 0, 'mbconv2': 0, 'mb16': 0, 'headfuse': 0, 'stem': 0},
           'bf16': {'mbtb': 0, 'mbtb_s2': 0, 'headb': 0, 'stem': 0},
           'f16': {'mbtb': 0, 'mbtb_s2': 0, 'headb': 0, 'stem': 0}}

_RUN = re.compile(r'^stage\.\d+\.\d+-\d+\.')
_MBT16 = ('mbtb_kernel', 'mbtb_s2_kernel', 'mbtd_kernel')

# (rule or switch case of csrc/engine.cpp, fp32 storage?, predicate(name, tag)): what the golden file must reach
RULES = [
    ('rule_mb16: a run of blocks', True, lambda n, t: t == 'mb16_kernel' and bool(_RUN.match(n))),
    ('rule_mb16: one block', True, lambda n, t: t == 'mb16_kernel' and not _RUN.match(n)),
    ('rule_mbt: launch_mbt stride 1', True, lambda n, t: t == 'mbt_kernel'),
    ('rule_mbt: launch_mbt stride 2', True, lambda n, t: t == 'mbt_s2_kernel'),
    ('rule_mbt: launch_mbconv', True, lambda n, t: t.startswith('mbconv')),
    ('rule_stem3', True, lambda n, t: n == 'stem.conv3x3s2+dw3+pw'),
    ('rule_dwpw3', True, lambda n, t: n.endswith('+pw') and t.startswith('dwpw_kernel')),
    ('rule_head: two sources', True, lambda n, t: t == 'headfuse_kernel' and n.endswith('.dw5+dw5+pw')),
    ('rule_head: one source', True, lambda n, t: t == 'headfuse_kernel' and n.endswith('.dw5+pw')),
    ('f32 OP_STEM', True, lambda n, t: t == 'stem_kernel'),
    ('f32 OP_DW', True, lambda n, t: n.endswith('.dw5') and t.startswith('dw_')),
    ('f32 OP_PW', True, lambda n, t: n.endswith('.inv') and t.startswith('pw')),
    ('f32 OP_PW: a head', True, lambda n, t: n.startswith('final.') and n.endswith('.pw') and t.startswith('pw')),
    ('f32 OP_DECONV: deconv4', True, lambda n, t: t == 'deconv4_kernel'),
    ('f32 OP_DECONV: deconv4x3', True, lambda n, t: t == 'deconv4x3_kernel'),
    ('f32 OP_CONVK', True, lambda n, t: t.startswith('convk3_kernel')),
    ('f32 OP_DWPW: dwpw_kernel', True, lambda n, t: n.endswith('.depth_conv+point_conv') and t.startswith('dwpw_kernel')),
    ('f32 OP_DWPW: depthwise half', True, lambda n, t: n.endswith('.depth_conv') and t.startswith('dw_')),
    ('f32 OP_DWPW: 1x1 half', True, lambda n, t: n.endswith('.point_conv') and t.startswith('pw')),
    ('rule_mbtb: stride 1', False, lambda n, t: n.endswith('+dw+point_conv') and t in ('mbtb_kernel', 'mbtd_kernel')),
    ('rule_mbtb: stride 2', False, lambda n, t: n.endswith('+dw+point_conv') and t == 'mbtb_s2_kernel'),
    ('rule_stem3b', False, lambda n, t: n == 'stem.conv3x3s2+dw3+pw'),
    ('rule_headb: two sources', False, lambda n, t: t == 'headb_kernel' and n.endswith('.dw5+dw5+pw')),
    ('rule_headb: one source', False, lambda n, t: t == 'headb_kernel' and n.endswith('.dw5+pw')),
    ('16-bit OP_STEM', False, lambda n, t: t == 'stemb_kernel'),
    ('16-bit OP_DW: dwt_kernel', False, lambda n, t: t.startswith('dwt_kernel')),
    ('16-bit OP_DW: dwb_kernel', False, lambda n, t: t.startswith('dwb_kernel')),
    ('16-bit OP_PW', False, lambda n, t: t == 'pwb_kernel' and not n.startswith('final.')),
    ('16-bit OP_PW: a head', False, lambda n, t: t == 'pwb_kernel' and n.startswith('final.')),
    ('16-bit OP_DECONV', False, lambda n, t: t == 'deconvb_kernel'),
]

_MODELS = {}


def _net(family, arch_name, storage):
    key = (family, arch_name, storage)
    if key not in _MODELS:
        if family == 'mobilenet':
            from _net_check import _model
            _MODELS[key] = _model(arch_name, storage=storage)[0]
        elif family == 'simplenet':
            from test_gpu_simplenet import _model
            _MODELS[key] = _model(arch_name, storage=storage)[0]
        else:
            from test_gpu_resnet import _model
            _MODELS[key] = _model()[0]
    return _MODELS[key]


def _entries(case, extra=None):
    """One profiled forward of the case (``extra``: options on top of the case's): [[name|tag, bytes, flops, flops_valu]]."""
    import torch
    from _net_check import set_options
    cid, family, arch_name, storage, H, W, N, flip, options = case
    m = _net(family, arch_name, storage)
    old = set_options(m, dict(options, **(extra or {})))
    m.set_profiling(True)
    try:
        m.forward_native(synth.make_images(N, H, seed=7, w=W).cuda(), flip)
        torch.cuda.synchronize()
        return [[n, int(by), int(fl), int(fv)] for n, _, by, fl, fv in m.profile(split=True)]
    finally:
        m.set_profiling(False)
        set_options(m, old)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_reaches_every_rule_and_switch_case():
    g = _golden()
    assert g['recorded_from'] == RECORDED_FROM
    assert sorted(g['cases']) == sorted(CASE_IDS)
    hits = {label: 0 for label, _, _ in RULES}
    for case in CASES:
        for full, by, fl, fv in g['cases'][case[0]]:
            assert all(type(v) is int for v in (by, fl, fv)), full
            name, tag = full.rsplit('|', 1)
            for label, f32, pred in RULES:
                if f32 == (case[3] == 'f32') and pred(name, tag):
                    hits[label] += 1
    print(json.dumps(hits, indent=1))
    assert not [k for k, v in hits.items() if v == 0], hits
    names = {k: [e[0].rsplit('|', 1)[0] for e in g['cases'][k]] for k in ('f16_s224', 'bf16_s224')}
    assert names['f16_s224'] and names['f16_s224'] == names['bf16_s224']        # the same rules fire for both formats


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_entries_equal_the_parent_commits(case):
    want = _golden()['cases'][case[0]]
    got = _entries(case)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    assert len(got) == len(want)


def _covered(name):
    """Predicate over unfused entry names: the reference ops that the fused entry ``name`` replaces (None: not fused).
    Profile names may be cut short to keep the kernel tag; the layer prefix always survives."""
    mo = re.match(r'^stage\.(\d+)\.(\d+)(?:-(\d+))?\.inv\+', name)
    if mo:
        s, b0, b1 = mo.group(1), int(mo.group(2)), int(mo.group(3) or mo.group(2))
        prefixes = tuple('stage.%s.%d.' % (s, b) for b in range(b0, b1 + 1))
        return lambda n: n.startswith(prefixes)
    if name == 'stem.conv3x3s2+dw3+pw':
        return lambda n: n.startswith('stem.')
    mo = re.match(r'^final\.(\d+)\.dw5\+', name)
    if mo:
        head = re.compile(r'^final(_refined|_raw)?\.%s\.' % mo.group(1))
        return lambda n: bool(head.match(n))
    return None


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_a_fused_entry_costs_the_sum_of_the_ops_it_replaces(case):
    storage = case[3]
    fused = [(e, _covered(e[0].rsplit('|', 1)[0])) for e in _entries(case)]
    fused = [(e, cov) for e, cov in fused if cov]
    if not fused:
        return                                  # a row of single-op launches: nothing to sum
    chain = [(e[0].rsplit('|', 1)[0], e[1:]) for e in _entries(case, UNFUSED[storage])]
    assert not [n for n, _ in chain if _covered(n)], 'the unfused forward still fuses'
    for (full, by, fl, fv), cov in fused:
        parts = [c for n, c in chain if cov(n)]
        assert len(parts) >= 2, (full, parts)
        s_by, s_fl, s_fv = (sum(p[k] for p in parts) for k in range(3))
        print('%-48s bytes %d (sum %d) flops %d (sum %d) valu %d (sum %d)' % (full, by, s_by, fl, s_fl, fv, s_fv))
        assert (fl, fv) == (s_fl, s_fv), (full, fl, s_fl, fv, s_fv)
        if storage != 'f32' and full.rsplit('|', 1)[1] in _MBT16:
            assert by < s_by, (full, by, s_by)  # the launch's own traffic: held by the golden file
        else:
            assert by == s_by, (full, by, s_by)


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--record', 'usage: test_gpu_profile_entries.py --record OUT.json'
    out = {'recorded_from': RECORDED_FROM,
           'what': 'lp_net_profile2 entries [name|kernel tag, bytes, flops, flops_valu] per case of '
                   'tests/test_gpu_profile_entries.py, recorded with its --record mode on a checkout of the parent commit '
                   '(never from the code under test)',
           'cases': {c[0]: _entries(c) for c in CASES}}
    cases = out.pop('cases')                    # one case per line
    body = ',\n'.join('"%s":%s' % (k, json.dumps(v, separators=(',', ':'))) for k, v in cases.items())
    with open(sys.argv[2], 'w') as f:
        f.write(json.dumps(out, indent=0)[:-2] + ',\n"cases": {\n' + body + '\n}\n}\n')
    out['cases'] = cases
    print('recorded %d cases, %d entries' % (len(out['cases']), sum(len(v) for v in out['cases'].values())))
