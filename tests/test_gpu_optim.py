"""The optimizer-side kernels of csrc/reduce_optim.hip on the MI355X: every case of tests/_optim_cases.py against the float64
reference and the per-element bounds of tests/_optim_ref.py (tests/test_optim_cases_cpu.py runs the same on the checker)."""
import pytest

import _optim_cases as oc
import _optim_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', oc.CASE_IDS)
def test_optimizer_against_float64(hip_lib, name):
  case = oc.CASES[oc.CASE_IDS.index(name)]
  fig, reached = oc.run_case(hip_lib, case)
  assert reached == case['label'], (name, reached)
  bad = oc.report(fig, f'{name} [{reached}]')
  assert not bad, (name, bad)


@pytest.mark.parametrize('op,mis', [('adam', None), ('adam', 'g'), ('amsgrad', None)])
def test_nonfinite_gradient_poisons_like_clip_grad_norm(hip_lib, op, mis):
  oc.nonfinite(hip_lib, op, mis)


def test_trajectory_and_drift(hip_lib):
  worst, p0, pT, vT = oc.trajectory(hip_lib)
  bad = oc.report(worst, 'trajectory (worst of 50 steps)')
  e_lib, e_torch, v_bias = oc.drift(p0, pT, vT)
  print(f'  drift of p_T - p_0 against float64: kernel {e_lib:.3g}, torch.optim.Adam fp32 {e_torch:.3g};'
        f' mean relative error of v {v_bias / R.U:+.3g} u')
  assert not bad, bad
  assert e_lib <= 2 * e_torch, (e_lib, e_torch)
  assert abs(v_bias) <= 4 * R.U, v_bias
