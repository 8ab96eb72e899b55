"""fp16 storage at the edges of the format, through every 16-bit kernel form (tests/_f16_range.py: the rows, the state
dicts, the derived bound).  Needs a real MI355X.

Per row, one profiled forward of a net whose weights push ONE tensor of ONE launch into the subnormal range (or past
65504), then the emulation walked to that launch on the device's own inputs:
  (a) the row's kernel form (tag) stored the row's op;
  (b) every element is within the derived bound;
  (c) 'sub': the device is nonzero wherever the emulation exceeds the bound -- a flush cannot hide in the tolerance;
      'top': the same infinity where the emulation overflows, finite where it does not (check_top);
  (d) printed: the worst |d| / bound, the shares of the target tensor that are nonzero and subnormal.
Nothing after the row's op is compared.  test_f16_range_form_again_in_bf16 runs every form's first subnormal row in bf16
storage with the same state dict under check_bf16: the rows lean on the dispatch both formats share."""
import pytest
import torch

import _f16_range as fr
from _net_check import _cfg, check_bf16, fused_inner, profiled_forward, set_options

pytestmark = pytest.mark.gpu


def _net(arch, sd, storage):
    from litepose_amd.models import pose_mobilenet
    m = pose_mobilenet.get_pose_net(_cfg(), is_train=False, cfg_arch=arch, storage=storage)
    m.load_state_dict(sd, strict=True)
    return m


def _forward(m, r, x):
    old = set_options(m, r[5])
    try:
        return profiled_forward(m, x.cuda(), 0)
    finally:
        set_options(m, old)


def _stored_name(launch):
    """The tensor a launch stores: its own name, or the last op of a fused launch."""
    fused = fused_inner([launch])
    return next(iter(fused)) if fused else launch


@pytest.mark.parametrize('rid', [r[0] for r in fr.ROWS])
def test_f16_range_row(rid):
    r = fr.row(rid)
    tag, op, edge = r[6], r[7], r[9]
    arch = fr.arch_of(r)
    sd, rc = fr.edge_state_dict(arch, r)
    x = fr.images(r)
    m = _net(arch, sd, 'f16')
    assert m.storage == 'f16'
    outs, launches = _forward(m, r, x)
    # (a)
    by_store = {_stored_name(n): (n, t) for n, t in launches}
    assert op in by_store, (op, sorted(by_store))
    assert by_store[op][1] == tag, (op, by_store[op])
    fused = fused_inner([n for n, _ in launches])
    assert fused.get(op, []) == fr.launch_inner(r), (fused.get(op), fr.launch_inner(r))
    inner = {t for v in fused.values() for t in v}

    def stored(name, shape):
        if name in inner:
            return None
        if name.startswith('final.') and name.endswith('.pw'):
            return outs[int(name.split('.')[1])].cpu().view(shape)
        return m.tap(name).cpu().view(shape)

    res = fr.evaluate(r, sd, arch, x, rc['target'], stored)
    if edge == 'sub':
        nz, sub = fr.shares(res['target'])
        live = float((res['exp'].abs() > res['bound']).float().mean())
        d = (res['got'] - res['exp']).abs() / res['bound']
        print('%s %s %s@%s: worst |d| / bound %.3f; %s: %.3f nonzero, %.3f subnormal; %.3f of the output beyond the bound, '
              'bound <= 2^%.1f' % (rid, tag, op, r[8], float(d.max()), rc['target'], nz, sub, live,
                                   float(torch.log2(res['bound'].max()))))
        assert nz > 0.1 and sub > 0.1, (rid, nz, sub)              # the preconditions, on the device's own inputs
        assert float(res['bound'].max()) < fr.SUB_BOUND_MAX
        fr.check_sub(res)                                           # (b), (c)
    else:
        big, ninf = fr.top_shares(res['exp'])
        got = res['got']
        print('%s %s %s: emulation %.3f finite >= 2^14, %d inf; device %d inf, largest finite %.6g'
              % (rid, tag, op, big, ninf, int(torch.isinf(got).sum()), float(got[torch.isfinite(got)].abs().max())))
        assert big >= 0.1 and ninf >= 100, (rid, big, ninf)
        worst, undecided = fr.check_top(res)
        print('%s: worst |d| / bound %.3f over the finite values, %d elements within the slack of the tie' % (rid, worst, undecided))


def _first_rows():
    seen, out = set(), []
    for r in fr.ROWS:
        if r[9] == 'sub' and r[6] not in seen:
            seen.add(r[6])
            out.append(r[0])
    return out


@pytest.mark.parametrize('rid', _first_rows())
def test_f16_range_form_again_in_bf16(rid):
    """The form's first subnormal row in bf16 storage, same state dict and options: the same tag, and check_bf16 on the
    whole forward (fp16-subnormal magnitudes are ordinary bf16 values)."""
    r = fr.row(rid)
    arch = fr.arch_of(r)
    sd, _ = fr.edge_state_dict(arch, r)
    x = fr.images(r)
    m = _net(arch, sd, 'bf16')
    outs, launches = _forward(m, r, x)
    assert {_stored_name(n): t for n, t in launches}.get(r[7]) == r[6], (r[7], launches)
    rows = check_bf16(m, arch, sd, x, 0, outs, [n for n, _ in launches])
    worst = max(rows.items(), key=lambda kv: kv[1][2])
    print('%s bf16 (%s): worst criterion %.3f of its bound at %s' % (rid, r[6], worst[1][2], worst[0]))
