"""The bias-gradient family and the row softmax of csrc/reduce_optim.hip on the MI355X, on every branch of their kernels and
host wrappers (tests/_reduce_cases.py): the bias gradients against the checker's double-accumulating restatement, the
softmax against float64, both with per-element bounds."""
import pytest

import _reduce_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', rc.BIAS_IDS)
def test_bias_grad_branches(ref_lib, hip_lib, name):
  case = rc.BIAS_CASES[rc.BIAS_IDS.index(name)]
  inp = rc.bias_inputs(case)
  ref, _ = rc.bias_run(ref_lib, case, inp)
  got, reached = rc.bias_run(hip_lib, case, inp)
  assert reached == case[6], (name, reached)
  assert set(got) == set(ref)
  fig = rc.bias_figures(case, got, ref, rc.bias_float64(case, inp), reached)
  print(f'  {name} [{reached}]: ' + ', '.join(f'{k} {r:.3g}' for k, r in fig.items()))
  bad = [(k, r) for k, r in fig.items() if not r <= 1.0]
  assert not bad, (name, bad)


@pytest.mark.parametrize('cols,label', rc.SOFTMAX_CASES)
def test_softmax_against_float64(hip_lib, cols, label):
  assert rc.softmax_branch(cols) == label
  x, dy = rc.softmax_inputs(cols)
  y, dx = rc.softmax_run(hip_lib, x, dy)
  fig = rc.softmax_figures(x, dy, y, dx)
  print(f'  softmax cols={cols} [{label}]: ' + ', '.join(f'{k} {r:.3g}' for k, r in fig.items()))
  assert all(r <= 1.0 for r in fig.values()), fig
