"""The buffer-contract harness without a GPU: the helpers of tests/_poison.py on CPU tensors (guard detection,
unwritten-element detection, what every poison pattern decodes to), and the coverage of tests/test_gpu_buffer_contract.py:
every lp_* function of include/litepose_amd.h with a non-const device-pointer parameter is a key of its ``CALLS`` or
excused in ``EXCUSED`` with the reason; an ``EXCUSED`` entry for a function that no longer exists fails too."""
import os
import re

import pytest
import torch

import _poison as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'litepose_amd.h')

# writable-device-pointer entry points the contract test does not run, with the reason (none today)
EXCUSED = {}

_PROTO = re.compile(r'\b(lp_\w+)\s*\(([^;{]*?)\)\s*;', re.S)
_COMMENT = re.compile(r'/\*.*?\*/|//[^\n]*', re.S)


def writable_device_calls(path=HEADER):
    """lp_* functions declared in the header with a parameter ``d_*`` that is a pointer to non-const memory."""
    with open(path) as f:
        src = _COMMENT.sub(' ', f.read())
    out = set()
    for name, params in _PROTO.findall(src):
        for prm in params.split(','):
            prm = ' '.join(prm.split())
            m = re.match(r'(.*?)\*\s*(d_\w+)$', prm)
            if m and not re.search(r'\bconst\b', m.group(1)):
                out.add(name)
    return out


def coverage_gaps(calls, excused, header=HEADER):
    found = writable_device_calls(header)
    return (sorted(found - set(calls) - set(excused)), sorted(set(excused) - found), sorted(set(calls) - found),
            sorted(set(calls) & set(excused)))


def _calls():
    import test_gpu_buffer_contract as bc
    return bc.CALLS


# ------------------------------------------------------------------ helper controls
def test_guard_write_is_reported_with_its_offset():
    for align in (256, 16, 8):
        p = P.place(1000, align, 'N', device='cpu')
        assert p.bytes.data_ptr() % align == 0 and p.off >= P.GUARD
        assert p.base.numel() - p.off - p.nbytes >= P.GUARD
        p.view(torch.float32, (250,)).fill_(3.0)
        p.check_guards()
        p.base[p.off + p.nbytes] = 0                     # the byte right after the exact size
        with pytest.raises(AssertionError, match='offset 1000 '):
            p.check_guards('x')
        q = P.place(64, align, 'H', device='cpu')
        q.base[q.off - 1] = 7
        with pytest.raises(AssertionError, match='offset -1 '):
            q.check_guards('x')


def test_unwritten_elements_are_found():
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.uint8):
        for pat in ('N', 'H'):
            t = P.fill(torch.empty(10, dtype=dt), pat)
            ref = torch.zeros(10, dtype=dt)
            t[:7] = ref[:7]
            assert P.still_poisoned(t, ref, pat) == [7, 8, 9], (dt, pat)
            t[7:] = ref[7:]
            assert P.still_poisoned(t, ref, pat) == []
    # a legitimately written value equal to the poison (a count of -1 under N) is not reported
    t = P.fill(torch.empty(3, dtype=torch.int32), 'N')
    assert P.still_poisoned(t, torch.tensor([-1, -1, -1], dtype=torch.int32), 'N') == []


def test_patterns_decode_to_the_intended_values():
    import math
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        z = P.fill(torch.ones(4, dtype=dt), 'Z').float()
        assert torch.equal(z, torch.zeros(4)), dt
        n = P.fill(torch.ones(4, dtype=dt), 'N').float()
        assert torch.isnan(n).all(), dt
    h = {dt: float(P.fill(torch.ones(1, dtype=dt), 'H').float()) for dt in (torch.float32, torch.bfloat16, torch.float16)}
    assert math.isclose(h[torch.float32], 3.3961514e38, rel_tol=1e-6), h
    assert math.isclose(h[torch.bfloat16], 3.3895314e38, rel_tol=1e-6), h
    assert h[torch.float16] == 65504.0, h
    # f16 regions of a raw byte workspace: halfwords 0x7BFF
    w = P.fill(torch.empty(8, dtype=torch.uint8), 'H', half=True)
    assert torch.equal(w.view(torch.float16).float(), torch.full((4,), 65504.0))
    assert P.poison_bits(torch.int32, 'N') == -1 and P.poison_bits(torch.int32, 'H') == 0x7F7F7F7F
    # strided views are filled in place, NaN payload kept
    t = torch.zeros(4, 6)
    P.fill(t[:, 1], 'N')
    assert (P.as_bits(t[:, 1]) == -1).all() and not P.as_bits(t[:, 0]).any()


def test_input_wrapping_copies_and_guards_with_the_pattern():
    x = torch.arange(10, dtype=torch.float32)
    for pat in P.PATTERNS:
        p, v = P.wrap_input(x, 16, pat)
        assert P.bitwise_equal(v, x) and v.data_ptr() % 16 == 0
        assert (p.base[:p.off] == P.pattern_byte(pat)).all() and (p.base[p.off + 40:] == P.pattern_byte(pat)).all()
        p.check_guards()


# ------------------------------------------------------------------ coverage of the contract test
def test_header_names_the_writable_calls():
    found = writable_device_calls()
    assert len(found) == 20, sorted(found)
    for name in ('lp_net_forward', 'lp_maps_accumulate', 'lp_preprocess_batch_v', 'lp_final_preds_v', 'lp_net_tap'):
        assert name in found, name
    for name in ('lp_net_set_weight', 'lp_round16', 'lp_diag_read', 'lp_net_tap_offset', 'lp_stream_abort_capture'):
        assert name not in found, name


def test_every_writable_call_is_covered_or_excused():
    missing, stale, unknown, both = coverage_gaps(_calls(), EXCUSED)
    assert not missing, ('writable entry points neither in CALLS nor EXCUSED', missing)
    assert not stale, ('EXCUSED names functions the header no longer declares', stale)
    assert not unknown, ('CALLS names functions the header does not declare', unknown)
    assert not both, both
    for why in EXCUSED.values():
        assert len(why) >= 30


def test_calls_name_tests_that_exist():
    import test_gpu_buffer_contract as bc
    for name, tests in _calls().items():
        assert tests, name
        for t in tests:
            assert callable(getattr(bc, t, None)), (name, t)


@pytest.mark.parametrize('drop', ['key', 'fake_call', 'stale_excuse'])
def test_coverage_check_fails_when_coverage_is_lost(drop, tmp_path):
    calls = dict(_calls())
    if drop == 'key':
        del calls['lp_parse_dm']
        missing, _, _, _ = coverage_gaps(calls, EXCUSED)
        assert missing == ['lp_parse_dm'], missing
    elif drop == 'fake_call':
        with open(HEADER) as f:
            src = f.read()
        hdr = tmp_path / 'litepose_amd.h'
        hdr.write_text(src.replace('#ifdef __cplusplus\n}', 'int lp_fake(const float* d_in, int n,\n'
                                   '            float* d_out, void* stream);\n#ifdef __cplusplus\n}'))
        missing, _, _, _ = coverage_gaps(calls, EXCUSED, str(hdr))
        assert missing == ['lp_fake'], missing
    else:
        _, stale, _, _ = coverage_gaps(calls, dict(EXCUSED, lp_gone='an entry point that was removed long ago'))
        assert stale == ['lp_gone'], stale
