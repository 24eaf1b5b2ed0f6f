"""The case table, the reference, the bounds and the numpy model of the short-map attention tests, without a GPU
(tests/_attn_cases.py, tests/_attn_ref.py; the GPU half is tests/test_gpu_attention_forms.py).

  - the table reaches every kernel family, launch form, T, d and grid it names (REQUIRED);
  - the reference is _mh_ref.attention_with_grads and torch autograd in float64;
  - the numpy model of the arithmetic lands at or below HALF of every bound on every case: a derivation that forgot a
    rounding fails here, not on the device;
  - the floors hide nothing: outside the floor cases the floor is under 10 % of the bound on 90 % of the rows (columns) of
    every output, and in the floor cases the model's error reaches a quarter of the floor;
  - each mutant of the model lands at least 5 bounds out on the case named for it.
Ratios are printed per case with -s."""
import numpy as np
import pytest
import torch

import _attn_cases as ac
import _attn_ref as ar
import _mh_ref


def test_table_reaches_every_family_and_form():
  reached = set().union(*(ac.forms(c) for c in ac.CASES))
  missing = sorted(ac.REQUIRED - reached)
  assert not missing, f'the table does not reach: {missing}'
  for c in ac.CASES:
    d = c.C // c.heads
    assert c.C % c.heads == 0 and d % 32 == 0 and 32 <= d <= 256 and c.T % 4 == 0 and 4 <= c.T <= 256, c.name
    assert c.B * c.C * c.T <= 2 * 512 * 256, c.name
    assert c.entry == 'mh' or (c.heads == 1 and c.null is None), c.name
    bs, gs, _, _ = ac.strides(c)
    assert bs >= c.C * c.T and gs >= c.C * c.T and bs % 4 == 0 and gs % 4 == 0, c.name
  padded = [c for c in ac.CASES if c.place == 'padded']
  assert all(len({c.C * c.T, *ac.strides(c)[:2], 3 * c.C * c.T}) == 4 for c in padded)    # neither C T nor 3 C T, and not each other


def test_launch_rule_restated():
  assert ac.kernel(False, 256, 256) == ('sh full', 256, True) and ac.kernel(False, 224, 256)[0] == 'sh rolled 256'
  assert ac.kernel(False, 256, 128)[0] == 'sh rolled 128' and ac.kernel(False, 32, 132)[0] == 'sh rolled 256'
  assert [ac.kernel(True, d, 256)[0] for d in (32, 64, 96, 128, 160, 256)] == ['mh full', 'mh full', 'mh rolled 256', 'mh full',
                                                                              'mh rolled 256', 'mh full']
  assert ac.kernel(True, 64, 128)[0] == 'mh rolled 128' and ac.kernel(True, 64, 252)[0] == 'mh rolled 256'
  one = ac.BY_NAME['mh_B1C128h1T128_padded_triple_sd_randn']
  assert ac.uses_mh_kernels(one) == (False, False) and ac.family(one) == 'sh rolled 128'
  null = ac.BY_NAME['mh_B1C128h1T64_separate_zero_sd_null0_randn']
  assert ac.uses_mh_kernels(null) == (False, True) and ac.family(null) == 'mh rolled 128'


@pytest.mark.parametrize('name', ['mh_B3C96h3T28_stacked_triple_sd_negative', 'mh_B1C128h2T256_stacked_zero_sd_null0_decades',
                                  'sh_B2C224h1T64_mixed-b_zero_sd_apart'])
def test_reference_is_mh_ref_and_autograd(name):
  c, t = ac.BY_NAME[name], ac.inputs(name)
  scale = ac.scale_of(c)
  ref = ar.reference(t['q'], t['k'], t['v'], t['do'], c.heads, scale)
  tt = [torch.from_numpy(t[n]).double() for n in ('q', 'k', 'v', 'do')]
  other = _mh_ref.attention_with_grads(*tt, c.heads, scale)
  q, k, v = (x.clone().requires_grad_(True) for x in tt[:3])
  _mh_ref.attention(q, k, v, c.heads, scale).backward(tt[3])
  auto = {'dq': q.grad, 'dk': k.grad, 'dv': v.grad}
  for n in ar.OUTPUTS:
    for what, o in (('_mh_ref', other), ('autograd', auto)):
      if n in o:
        w = o[n].numpy()
        assert np.abs(ref[n] - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300) + (1e-12 if n == 'lse' else 0), (n, what)
  a = ref['aux']
  assert np.allclose(a['p'].sum(-1), 1.0, rtol=1e-12) and np.all(a['S_abs'] >= np.abs(scale * np.einsum(
      'bhct,bhcs->bhts', *(ar.heads_view(t[n].astype(np.float64), c.heads) for n in ('q', 'k')))) * (1 - 1e-12))


def rows(name, a):
  """An output's array as [rows or columns of one head, elements of it]: the position index last."""
  return a.reshape(-1, a.shape[-1]).T if name in ('o', 'dq', 'dk', 'dv') else a.reshape(-1, 1)


@pytest.mark.parametrize('name', ac.IDS)
def test_model_within_half_of_every_bound(name):
  c = ac.BY_NAME[name]
  want, bnd, ref = ac.reference(name)
  assert bnd['rel'] < 2.0 ** -5, f'{name}: a first-order relative error of {bnd["rel"]:.3g}: the second-order factor does not cover it'
  if c.fam == 'negative':
    assert ref['aux']['max_s'].max() <= -20.0, ref['aux']['max_s'].max()
  if c.fam == 'offset':
    assert 50.0 <= np.median(ref['aux']['max_s']) <= 70.0, np.median(ref['aux']['max_s'])
  got = ac.run_model(c)
  msg = []
  for n in ac.checked(c):
    r = ar.ratio(got[n], want[n], ar.bound_of(bnd, n))
    msg.append(f'{n} {r.max():.3f}')
    assert r.max() <= 0.5, f'{name} {n}: the model is {r.max():.3g} bounds out'
    ff = ar.floor_fraction(bnd, n)
    if c.fam in ac.FLOOR_CASES:
      if n in ac.FLOOR_CASES[c.fam]:
        err = np.abs(got[n].astype(np.float64) - want[n])
        assert (ff >= 0.5).any(), f'{name} {n}: the floor is the larger part of the bound nowhere'
        q = float((err / np.maximum(bnd[n][1], 1e-300))[ff >= 0.5].max())      # where the floor IS the bound
        msg.append(f'({n} err / floor {q:.2f})')
        assert q >= 0.25, f'{name} {n}: the model reaches {q:.3g} of the floor term: the floor is slack here'
    else:
      low = (rows(n, ff).max(1) < 0.1).mean()
      assert low >= 0.9, f'{name} {n}: the floor is under 10 % of the bound on {100 * low:.0f} % of the rows only'
  if c.null is not None:
    n = ('dq', 'dk', 'dv')[c.null]
    assert np.array_equal(got[n].view(np.int32), ac.inputs(name)['g0'][c.null].view(np.int32)), f'{name}: NULL {n} touched'
  print(f'  {name}: model err / bound', ', '.join(msg))


# mutant -> the case expected to catch it
MUTANTS = {
  'mask admits T': 'sh_B3C64h1T28_stacked_triple_s0.37_negative',
  'last 4 keys dropped': 'sh_B2C160h1T252_mixed-a_zero_sd_negative',
  'lse of the neighbouring head': 'mh_B2C192h3T256_mixed-a_triple_sd_randn',
  'delta of the neighbouring head': 'mh_B2C192h3T256_mixed-a_triple_sd_randn',
  'head offset with C': 'mh_B9C64h2T32_padded_zero_s0.37_decades',
  'scale of C': 'mh_B1C64h2T256_separate_zero_sd_randn',
  'hi lo dropped': 'mh_B2C64h2T64_separate_zero_sd_coherent',
  'ds scale of the image': 'mh_B1C64h2T128_separate_zero_sd_floor-unattended',
  'beta_k and beta_v exchanged': 'mh_B3C96h3T28_stacked_triple_sd_negative',
  'gradients at the qkv stride': 'sh_B2C256h1T68_padded_triple_sd_negative',
  'do at the gradient stride': 'sh_B2C96h1T32_padded_zero_sd_decades',
}


@pytest.mark.parametrize('mutant', list(MUTANTS))
def test_mutant_lands_five_bounds_out(mutant):
  name = MUTANTS[mutant]
  c = ac.BY_NAME[name]
  want, bnd, _ = ac.reference(name)
  got = ac.run_model(c, mutant)
  worst = {n: float(ar.ratio(got[n], want[n], ar.bound_of(bnd, n)).max()) for n in ac.checked(c)}
  n = max(worst, key=worst.get)
  print(f'  {mutant}: caught by {name}, {n} {worst[n]:.3g} bounds out')
  assert worst[n] >= 5.0, f'{mutant}: at most {worst[n]:.3g} bounds out ({n}) on {name}: the bounds would let it pass'
