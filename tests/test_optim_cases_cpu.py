"""The optimizer-side cases of tests/_optim_cases.py on the plain-C checker, and the float64 reference of tests/_optim_ref.py
against torch.optim.  No GPU: this half proves that the reference and the bounds are self-consistent -- an fp32
implementation of the same step (the checker, and torch.optim.Adam in fp32 for the drift) stays inside them."""
import numpy as np
import pytest
import torch

import _optim_cases as oc
import _optim_ref as R


def test_case_table_is_complete():
  """Every kernel form of the optimizer half of csrc/reduce_optim.hip, every grid rule of sumsq, every size on every entry
  and one misaligned tensor at a time for every entry appear in the table."""
  labels = {c['label'] for c in oc.CASES}
  assert {l.split(' ')[0] for l in labels} == oc.ALL_BRANCHES
  assert {l.split(' ')[1] for l in labels if l.startswith('sumsq')} == oc.ALL_GRIDS
  for op in ('adam', 'amsgrad', 'ema', 'sumsq'):
    assert {c['n'] for c in oc.CASES if c['op'] == op and c['mis'] is None} >= set(oc.SIZES), op
  mis = {(c['op'], c['mis']) for c in oc.CASES if c['mis']}
  assert mis >= {('adam', k) for k in 'pgmv'} | {('amsgrad', 'vmax'), ('ema', 's'), ('ema', 'p'), ('sumsq', 'x')}
  for op in ('adam', 'amsgrad'):
    assert {c['variant'] for c in oc.CASES if c['op'] == op} == {'plain', 'l2', 'adamw'}
    assert {c['step'] for c in oc.CASES if c['op'] == op} >= {1, 10 ** 6}
  assert {c['clip'] for c in oc.CASES if c['op'] == 'adam'} == {'null', 'neg', 'below', 'above3', 'zero'}


@pytest.mark.parametrize('variant', ['plain', 'l2', 'adamw', 'amsgrad', 'amsgrad_l2'])
def test_reference_matches_torch_float64(variant):
  """tests/_optim_ref.py against torch.optim.Adam / AdamW themselves in float64, three steps.  torch forms 1 - b^t from the
  betas it is given in float64; the reference is handed the same corrections, which it rounds to fp32 as the ABI does, so the
  two agree to a few fp32 roundings of the SCALARS (1e-6 of the step), far below any mistake in the formula."""
  n, gen = 257, torch.Generator().manual_seed(5)
  wd = 0.0 if variant in ('plain', 'amsgrad') else 0.01
  ams, adamw = variant.startswith('amsgrad'), variant == 'adamw'
  p0 = torch.randn(n, generator=gen, dtype=torch.float64)
  grads = [torch.randn(n, generator=gen, dtype=torch.float64) * 0.01 for _ in range(3)]
  p = torch.nn.Parameter(p0.clone())
  kw = dict(lr=R.f32(1e-3), betas=(R.f32(0.9), R.f32(0.999)), eps=R.f32(1e-8), weight_decay=R.f32(wd))
  opt = torch.optim.AdamW([p], **kw) if adamw else torch.optim.Adam([p], amsgrad=ams, **kw)
  q, m, v = p0.numpy().copy(), np.zeros(n), np.zeros(n)
  vmax = np.zeros(n) if ams else None
  for t, g in enumerate(grads, 1):
    p.grad = g.clone()
    opt.step()
    before = q
    r = R.adam_step(q, g.numpy(), m, v, R.Hyper(lr=1e-3, wd=wd, adamw=adamw, bc=(1 - R.f32(0.9) ** t, 1 - R.f32(0.999) ** t)),
                    vmax=vmax)
    q, m, v = r['p'], r['m'], r['v']
    vmax = r.get('vmax')
    step = np.abs(q - before).max()
    assert np.abs(q - p.detach().numpy()).max() <= 1e-6 * t * step, (variant, t)
  st = opt.state[p]                # (with L2 decay the 1e-6 of p feeds back into the moments: 1e-7 relative, not 1e-12)
  assert np.allclose(m, st['exp_avg'].numpy(), rtol=1e-7, atol=0) and np.allclose(v, st['exp_avg_sq'].numpy(), rtol=1e-7, atol=0)
  if ams:
    assert np.allclose(vmax, st['max_exp_avg_sq'].numpy(), rtol=1e-7, atol=0)


def test_clip_coefficient_matches_clip_grad_norm():
  g = torch.randn(1000, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
  for max_norm in (0.0, 1.0, 100.0):
    p = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
    p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p], max_norm)
    want = g.numpy() * R.clip_coef(R.sumsq_ref(g.numpy()), max_norm)
    assert np.allclose(p.grad.numpy(), want, rtol=1e-12, atol=0)
  assert np.isnan(R.clip_coef(float('nan'), 1.0))


def test_decimal_betas_would_be_flagged():
  """1 - 0.999f is 0.0009999871: a float64 reference given the decimal beta disagrees with the ABI's by 1.29e-5 relative in
  the weight of g^2 -- two hundred times the 4 u the drift check allows the mean of v."""
  assert 1.0 - R.f32(0.999) == float(np.float32(1) - np.float32(0.999))
  assert abs((1.0 - R.f32(0.999)) / 1e-3 - 1) > 200 * R.U
  assert abs((1.0 - R.f32(0.999)) / 1e-3 - 1 + 1.29e-5) < 1e-7


@pytest.mark.parametrize('name', oc.CASE_IDS)
def test_checker_meets_the_bounds(ref_lib, name):
  case = oc.CASES[oc.CASE_IDS.index(name)]
  fig, reached = oc.run_case(ref_lib, case)
  assert reached == case['label'], (name, reached)
  bad = oc.report(fig, f'checker {name} [{reached}]')
  assert not bad, (name, bad)


@pytest.mark.parametrize('op,mis', [('adam', None), ('adam', 'g'), ('amsgrad', None)])
def test_checker_nonfinite_gradient(ref_lib, op, mis):
  oc.nonfinite(ref_lib, op, mis)


def test_checker_trajectory_and_drift(ref_lib):
  worst, p0, pT, vT = oc.trajectory(ref_lib)
  bad = oc.report(worst, 'checker trajectory (worst of 50 steps)')
  e_lib, e_torch, v_bias = oc.drift(p0, pT, vT)
  print(f'  drift of p_T - p_0 against float64: checker {e_lib:.3g}, torch.optim.Adam fp32 {e_torch:.3g};'
        f' mean relative error of v {v_bias / R.U:+.3g} u')
  assert not bad, bad
  assert e_lib <= 2 * e_torch, (e_lib, e_torch)
  assert abs(v_bias) <= 4 * R.U, v_bias
