"""tests/_ew_cases.py without a GPU: the case table reaches every launch form of csrc/elementwise.hip, and the bounds of
tests/_ew_ref.py are no tighter than correct float32 arithmetic allows -- the plain-C checker meets every k u B, with the same k,
and so does a float32 numpy restatement of every entry (which stands in for the one entry the checker lacks,
fourier_embedding_bwd).  The kernels are run on the same tables by tests/test_gpu_elementwise.py."""
import pytest

import _ew_cases as ec


def _of(entry, **want):
  def ok(c):
    p = ec.params(c)
    return all((getattr(c, k) if k in c._fields else p.get(k)) == v for k, v in want.items())
  return [c for c in ec.CASES if c.entry == entry and ok(c)]


def test_case_table_is_complete():
  for name, e in ec.ENTRIES.items():
    assert _of(name), name
    if e.kind in ('flat', 'row'):
      key = 'n' if e.kind == 'flat' else 'inner'
      assert _of(name, form='vec', where='aligned') and _of(name, form='scalar', where='aligned'), name
      assert any(ec.params(c)[key] % 4 == 0 for c in _of(name, form='scalar', where='entered-one-in')), name
      assert _of(name, form='vec', strided=True) and _of(name, form='scalar', strided=True), name
      if e.kind == 'flat':
        assert {ec.params(c)['n'] for c in _of(name)} >= set(ec.FLAT_N), name
        assert all(_of(name, n=n, where='entered-one-in') for n in ec.FLAT_N if n % 4 == 0), name
      else:
        assert {(ec.params(c)['N'], ec.params(c)['inner']) for c in _of(name)} >= set(ec.ROWS), name
      if name not in ('fill', 'dropout_mask'):           # several pointers: the output alone, one input alone
        assert _of(name, where='out-one-in') and _of(name, where='in-one-in'), name
    if e.accum:
      assert _of(name, beta=0.0), name                   # run() prefills NaN there
      assert name in ('concat_bwd', 'resample_naive') or {ec.params(c)['beta'] for c in _of(name)} >= set(ec.BETAS), name
    if e.null:
      assert any(ec.params(c).get('null') or ec.params(c).get('variant') == 'null' or ec.params(c).get('bias') is False
                 for c in _of(name)), name
    if name in ec.STRIDED_PLAIN:
      assert _of(name, strided=True), name
  assert {name for name, e in ec.ENTRIES.items() if e.base in ('act_fwd', 'act_bwd')} == \
      {f'act_{d}[{a}]' for d in ('fwd', 'bwd') for a in range(5)}
  assert len([n for n in ec.ENTRIES if n.startswith('sm_loss_bwd')]) == 8
  assert {(ec.params(c)['vp'], ec.params(c)['mode'], ec.params(c)['rm']) for c in _of('sm_loss_fwd', inner=257, N=6)} == set(ec.FLAGS)
  assert _of('fused_bias_act_f32', n=60, step_b=5, where='aligned', form='vec')      # a float4 spans two bias entries
  assert {(ec.params(c)['bias'], ec.params(c)['ref']) for c in _of('fused_bias_act_f32', n=1028)} == {(a, b) for a in (True, False) for b in (True, False)}
  assert {c.where for c in _of('resample_naive')} == {'aligned', 'entered-two-in'}
  # pointer hygiene: only the entries that choose between the 16-byte and the scalar form are entered one element in
  assert all(ec.ENTRIES[c.entry].kind in ('flat', 'row') for c in ec.CASES if 'one-in' in c.where)
  assert len(set(ec.CASES)) == len(ec.CASES)


@pytest.mark.parametrize('group', ec.GROUP_IDS)
def test_checker_and_float32_restatement_meet_the_bounds(ref_lib, group):
  entry, size = ec.GROUPS[ec.GROUP_IDS.index(group)]
  seen, worst = set(), {}
  for case in ec.group_cases(entry, size):
    if case.p not in seen:                               # the restatement has no placements
      seen.add(case.p)
      units, k = ec.check(case, ec.restatement(entry, case.p))
      worst['float32'] = max(worst.get('float32', (0.0, k)), (units, k))
    if entry == 'fourier_embedding_bwd' and not ref_lib.has_blocks:
      continue                                           # the checker lacks it: the restatement above stands in
    units, k = ec.check(case, ec.run(ref_lib, case))
    ec.check_null_matches_full(ref_lib, case)
    worst[case.form] = max(worst.get(case.form, (0.0, k)), (units, k))
  print(f'  {group}: ' + ', '.join(f'{f} {u:.2f} of {k}' for f, (u, k) in worst.items()))
