"""The case table, the bounds and the numpy model of the streaming attention tests, without a GPU
(tests/_attn_long_cases.py, tests/_attn_long_ref.py; the GPU half is tests/test_gpu_attention_long_forms.py).

  - the table reaches every entry, T edge, width, grid and launch form it names (REQUIRED);
  - the launch rule restated there agrees with the constants of csrc/attention_long.hip, read as text;
  - the reference is test_gpu_attention_long.ref_attention, _mh_ref.attention_with_grads and torch autograd in float64;
  - the numpy model of the streaming arithmetic lands at or below HALF of every bound on every case, and every relative
    error of the derivation is under 2^-5;
  - the floors hide nothing: outside the floor cases the floor is under 10 % of the bound on 90 % of the rows (columns) of
    every output, and in the floor cases the model's error reaches a quarter of the floor where the floor is the bound;
  - each mutant of the model lands at least 5 bounds out on the case named for it.
Ratios are printed per case with -s."""
import os
import re

import numpy as np
import pytest
import torch

import _attn_long_cases as lc
import _attn_long_ref as al
import _attn_ref as ar
import _mh_ref
from test_attention_cases_cpu import rows

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'soft-truncation_amd', 'csrc', 'attention_long.hip')


def test_table_reaches_every_entry_edge_and_form():
  reached = set().union(*(lc.forms(c) for c in lc.CASES))
  missing = sorted(lc.REQUIRED - reached)
  assert not missing, f'the table does not reach: {missing}'
  for c in lc.CASES:
    d = c.C // c.heads
    assert c.C % c.heads == 0 and d % 32 == 0 and 32 <= d <= 256 and c.T % 4 == 0 and 4 <= c.T <= 516 and c.B <= 9, c.name
    assert lc.streaming(c) and (c.entry == 'mh' or c.heads == 1), c.name
    assert len(c.null) < 3 and (c.beta == 'zero' or c.fam not in lc.STREAM_FAMILIES), c.name
    bs, gs, _, _ = lc.ac.strides(c)
    assert bs >= c.C * c.T and gs >= c.C * c.T and bs % 4 == 0 and gs % 4 == 0, c.name
    if c.place == 'padded':
      assert len({c.C * c.T, bs, gs, 3 * c.C * c.T}) == 4 and (bs, gs) == (c.C * c.T + 28, c.C * c.T + 12), c.name
    if c.fam in lc.STREAM_FAMILIES and c.fam != 'tiny do':
      assert c.T <= 132 and al.n_chunks(c.T) >= 4, c.name


def test_launch_rule_restated():
  src = open(SRC).read()
  const = lambda name: int(re.search(r'constexpr int (?:\w+ = \d+, )*' + name + r' = (\d+)', src).group(1))
  assert (const('KC'), const('TPAD'), const('NW_FWD'), const('NW_DKV')) == (lc.KC, lc.TPAD, lc.NW_FWD, lc.NW_DKV) == (al.KC, 128, 8, 4)
  m = re.search(r'nw_dq\(\) \{ return C >= (\d+) \? (\d+) : (\d+); \}', src)
  assert tuple(int(x) for x in m.groups()) == (lc.DQ_4_WAVES_FROM, 4, 8)
  assert int(re.search(r'mh_short\(int T\) \{ return T <= (\d+); \}', src).group(1)) == lc.MH_SHORT_T
  assert 'constexpr int PR = C / 8, N = 2 * KC * PR' in src and 'constexpr int N = 2 * C * 4' in src      # N = 8 d pieces a chunk
  assert [lc.tpad(T) for T in (4, 128, 132, 256, 260, 516)] == [128, 128, 256, 256, 384, 640]
  r = lc.launch_rule(5, 1, 96, 132)
  assert r == {'fwd': (128, 10, True, False), 'dq': (128, 10, True, False), 'dkv': (64, 20, False, False)}
  r = lc.launch_rule(1, 2, 224, 260)
  assert r == {'fwd': (128, 6, True, False), 'dq': (64, 12, False, False), 'dkv': (64, 12, False, False)}
  assert lc.launch_rule(1, 1, 32, 4) == {'fwd': (128, 1, True, True), 'dq': (128, 1, True, True), 'dkv': (64, 2, False, False)}
  assert [d for d in lc.D_VALUES if lc.launch_rule(1, 1, d, 4)['fwd'][2]] == [32, 96, 160, 224]
  assert [d for d in lc.D_VALUES if lc.launch_rule(1, 1, d, 4)['dq'][2]] == [32, 96, 160]
  assert not any(lc.launch_rule(1, 1, d, 4)['dkv'][2] for d in lc.D_VALUES)
  lines = src.split('\n')                                                       # the lines the derivation of _attn_long_ref.py cites
  for no, text in ((45, 'constexpr int KC = 32'), (133, '__fmaf_rn(d_o['), (223, 'if (dmax >= 1.17549435e-38f)'), (227, 'sc / sig'),
                   (280, 'tk < T ? us * s'), (286, 'alpha = expf(m - mn)'), (290, 'expf(x[i] - mn)'), (291, 'ps += p[i]'),
                   (294, '__fmaf_rn(l, alpha, ps)'), (300, 'o[cb] *= alpha'), (304, '__shfl_xor(l, 16, 64)'),
                   (307, '1.f / (sv * P_SCALE * l)'), (312, 'inv * o[cb][e]'), (313, 'm + logf(l)'), (360, 'expf(us * s'),
                   (361, 'p * (ud * dp'), (374, '(a.scale / sk) / sig'), (381, 'f * acc[cb][e]'), (440, 'expf(us * s[u][e] - lsv[e])'),
                   (441, 'pv * (ud * dp[u][e] - dlv[e])'), (459, '(a.scale / sq) / sig')):
    assert text in lines[no - 1], (no, text, lines[no - 1])
  for m_ in (0.0, 1e-30, 2.0 ** -100, 0.7, 1.0, 8191.0, 3e38):
    assert float(al.pow2_scale_arr(np.float32(m_))) == ar.pow2_scale_of(m_), m_


@pytest.mark.parametrize('name', ['long_B5C96h1T132_padded_triple_sd_negative', 'mh_B2C96h3T260_stacked_triple_sd_randn',
                                  'long_B2C64h1T128_separate_zero_sd_tiny-do'])
def test_reference_is_ref_attention_mh_ref_and_autograd(name):
  from test_gpu_attention_long import ref_attention
  c, t = lc.BY_NAME[name], lc.inputs(name)
  scale = lc.scale_of(c)
  ref = ar.reference(t['q'], t['k'], t['v'], t['do'], c.heads, scale)
  tt = [torch.from_numpy(t[n]).double() for n in ('q', 'k', 'v', 'do')]
  others = [('_mh_ref', _mh_ref.attention_with_grads(*tt, c.heads, scale))]
  q, k, v = (x.clone().requires_grad_(True) for x in tt[:3])
  _mh_ref.attention(q, k, v, c.heads, scale).backward(tt[3])
  others.append(('autograd', {'dq': q.grad, 'dk': k.grad, 'dv': v.grad}))
  if c.heads == 1:
    others.append(('ref_attention', {n: (x[:, None] if n in ('lse', 'delta') else x) for n, x in
                                     ref_attention(*(x.float() for x in tt), scale, chunk=48).items()}))
  for n in ar.OUTPUTS:
    for what, o in others:
      if n in o:
        w = o[n].numpy()
        assert np.abs(ref[n] - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300) + (1e-12 if n == 'lse' else 0), (n, what)


# Outputs whose reference is (next to) zero by construction on most rows, so that their bound is all floor there; the first
# floor condition does not apply to them, and the case is held to its bounds like every other.
#   last / first chunk: the keys outside the three that carry the maximum have p = e^-30 < 2^-38 for every query: their dv
#     lies under the floor of the probabilities' split, the situation of 'floor unattended' (which shows that floor reached).
#   peaked: q is one-hot, so dk[c, t'] sums over the few queries that look along c, with p ~ e^-100 unless t' is their peak,
#     where ds cancels: most of dk is zero next to f_q sum |ds| and the column floor.  A key that is nobody's peak is
#     unattended: its dv as in last / first chunk.
FLOOR_BY_CONSTRUCTION = {'last chunk': ('dv',), 'first chunk': ('dv',), 'peaked': ('dk', 'dv')}


@pytest.mark.parametrize('name', lc.IDS)
def test_model_within_half_of_every_bound(name):
  c = lc.BY_NAME[name]
  want, bnd, ref = lc.reference(name)
  assert bnd['rel'] < 2.0 ** -5, f'{name}: a first-order relative error of {bnd["rel"]:.3g}: the second-order factor does not cover it'
  if c.fam == 'negative':
    assert ref['aux']['max_s'].max() <= -20.0, ref['aux']['max_s'].max()
  got = lc.run_model(c)
  msg = []
  for n in lc.checked(c):
    r = ar.ratio(got[n], want[n], ar.bound_of(bnd, n))
    msg.append(f'{n} {r.max():.3f}')
    assert r.max() <= 0.5, f'{name} {n}: the model is {r.max():.3g} bounds out'
    ff = ar.floor_fraction(bnd, n)
    if c.fam in lc.FLOOR_CASES:
      if n in lc.FLOOR_CASES[c.fam]:
        err = np.abs(got[n].astype(np.float64) - want[n])
        assert (ff >= 0.5).any(), f'{name} {n}: the floor is the larger part of the bound nowhere'
        q = float((err / np.maximum(bnd[n][1], 1e-300))[ff >= 0.5].max())      # where the floor IS the bound
        msg.append(f'({n} err / floor {q:.2f})')
        assert q >= 0.25, f'{name} {n}: the model reaches {q:.3g} of the floor term: the floor is slack here'
    elif n not in FLOOR_BY_CONSTRUCTION.get(c.fam, ()):
      low = (rows(n, ff).max(1) < 0.1).mean()
      msg.append(f'[{100 * low:.0f} %]')
      assert low >= 0.9, f'{name} {n}: the floor is under 10 % of the bound on {100 * low:.0f} % of the rows only'
  for i in c.null:
    assert np.array_equal(got[lc.GRAD[i]].view(np.int32), lc.inputs(name)['g0'][i].view(np.int32)), f'{name}: NULL {lc.GRAD[i]} touched'
  print(f'  {name}: model err / bound', ', '.join(msg))


# mutant -> the case expected to catch it
MUTANTS = {
  'mask admits T': 'long_B7C160h1T36_mixed-a_triple_sd_negative',
  'last chunk dropped': 'long_B2C64h1T124_separate_zero_sd_last-chunk',
  'alpha on o only': 'long_B2C64h1T128_separate_zero_sd_rising',
  'alpha on l only': 'long_B2C64h1T128_separate_zero_sd_rising',
  'no rescale when the ds scale drops': 'long_B2C64h1T128_separate_zero_sd_ds-up-keys',
  'ds scale of the first chunk': 'long_B2C64h1T128_separate_zero_sd_ds-up-queries',
  'ds scale of the image': 'long_B1C32h1T128_separate_zero_sd_floor-unattended',
  'delta of the neighbouring head': 'mh_B2C96h3T260_stacked_triple_sd_randn',
  'lse of the neighbouring head': 'mh_B2C96h3T260_stacked_triple_sd_randn',
  'head offset with C in CF': 'mh_B2C96h3T260_stacked_triple_sd_randn',
  'head offset with C in the output': 'mh_B2C96h3T260_stacked_triple_sd_randn',
  'hi lo dropped': 'long_B2C64h1T64_separate_zero_sd_coherent',
  'beta_k and beta_v exchanged': 'long_B3C64h1T28_stacked_triple_s0.37_negative',
  'gradients at the qkv stride': 'long_B5C96h1T132_padded_triple_sd_negative',
  'f of the overflowing product': 'long_B2C64h1T128_separate_zero_sd_tiny-do',
  'a subnormal maximum sets the scale': 'long_B2C32h1T128_separate_zero_sd_peaked',
}


def test_every_mutant_of_the_model_is_named():
  assert set(al.MUTANTS) | {'gradients at the qkv stride'} == set(MUTANTS)
  assert all(n in lc.BY_NAME for n in MUTANTS.values())


@pytest.mark.parametrize('mutant', list(MUTANTS))
def test_mutant_lands_five_bounds_out(mutant):
  name = MUTANTS[mutant]
  c = lc.BY_NAME[name]
  want, bnd, _ = lc.reference(name)
  got = lc.run_model(c, mutant)
  worst = {n: float(ar.ratio(got[n], want[n], ar.bound_of(bnd, n)).max()) for n in lc.checked(c)}
  n = max(worst, key=worst.get)
  print(f'  {mutant}: caught by {name}, {n} {worst[n]:.3g} bounds out')
  assert worst[n] >= 5.0, f'{mutant}: at most {worst[n]:.3g} bounds out ({n}) on {name}: the bounds would let it pass'
