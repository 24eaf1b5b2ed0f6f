"""tests/_reduce_cases.py on the plain-C checker: the oracle the GPU half compares with is itself held to float64 here, and
the case table is checked for every kernel form of the bias-gradient family and the softmax."""
import pytest
import torch

import _reduce_cases as rc


def test_case_table_is_complete():
  labels = [c[6] for c in rc.BIAS_CASES]
  for k in rc.BIAS_KERNELS:
    forms = {l for l in labels if k in l}
    assert forms, k
    if k.startswith('bias_grad_kernel') or k == 'rowsum_kernel':
      assert any(k + ':vec' in l for l in forms) and any(k + ':scalar' in l for l in forms), k
  for entry in ('plain', 'amax', 'res', 'dual'):
    assert {c[2] for c in rc.BIAS_CASES if c[1] == entry and c[4] < 4096} >= {1, 16, 17, 32, 33, 48, 128}, entry
    assert {c[4] for c in rc.BIAS_CASES if c[1] == entry} >= {25, 81}, entry
    assert any('mis_dy' in c[5] for c in rc.BIAS_CASES if c[1] == entry), entry
  assert any('mis_res' in c[5] for c in rc.BIAS_CASES)
  assert any(c[3] == 1 and 'colsum' in c[6] for c in rc.BIAS_CASES) and any(c[3] % 32 and 'colsum' in c[6] for c in rc.BIAS_CASES)
  assert any(c[4] >= 4096 and 'mis_dy' in c[5] and 'rowsum_kernel' in c[6] for c in rc.BIAS_CASES)
  assert [c[0] for c in rc.SOFTMAX_CASES] == [1, 63, 64, 65, 1024]


@pytest.mark.parametrize('name', rc.BIAS_IDS)
def test_checker_bias_grad_against_float64(ref_lib, name):
  case = rc.BIAS_CASES[rc.BIAS_IDS.index(name)]
  inp = rc.bias_inputs(case)
  got, reached = rc.bias_run(ref_lib, case, inp)
  assert reached == case[6], (name, reached)
  f64 = rc.bias_float64(case, inp)
  fig = rc.bias_figures(case, got, f64, f64, reached)
  bad = [(k, r) for k, r in fig.items() if not r <= 1.0]
  print(f'  checker {name} [{reached}]: ' + ', '.join(f'{k} {r:.3g}' for k, r in fig.items()))
  assert not bad, (name, bad)


@pytest.mark.parametrize('cols,label', rc.SOFTMAX_CASES)
def test_checker_softmax_against_float64(ref_lib, cols, label):
  assert rc.softmax_branch(cols) == label
  x, dy = rc.softmax_inputs(cols)
  y, dx = rc.softmax_run(ref_lib, x, dy)
  fig = rc.softmax_figures(x, dy, y, dx)
  print(f'  checker softmax cols={cols} [{label}]: ' + ', '.join(f'{k} {r:.3g}' for k, r in fig.items()))
  assert all(r <= 1.0 for r in fig.values()), fig
