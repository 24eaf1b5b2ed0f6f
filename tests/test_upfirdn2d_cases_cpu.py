"""tests/_ufd_cases.py without a GPU: the float64 definition against two independently written statements of the operator
(the checker's loops, oracle/ref_torch.py), the condition on the inputs (plain fp32 passes the bound), the coverage of
routes and parameter axes by the case list, and the output-extent rule on the checker."""
import pytest
import torch

import _ufd_cases as uc
import ref_torch
from _stream_util import U

CASES = {c.name: c for c in uc.CASES}


def test_case_table_reaches_every_route_and_axis():
  assert len(set(uc.IDS)) == len(uc.IDS)
  reached = set()
  for c in uc.CASES:
    r = uc.route(c.params, aligned=not c.one_in)
    assert r == c.route, (c.name, r)
    reached.add(r)
  assert reached == uc.ROUTES, (uc.ROUTES - reached, reached - uc.ROUTES)
  for name, pred in uc.AXES.items():
    assert any(pred(c) for c in uc.CASES), f'no case with: {name}'
  assert 8 <= len(uc.TYPE_IDS) <= 12
  # small: at most 70 rows, or one plane about 520 wide; 12 K elements at the most
  for c in uc.CASES:
    major, H, W, minor = c.params[:4]
    assert major * H * W * minor <= 12 * 1024 and H <= 70, c.name


@pytest.mark.parametrize('beta', uc.BETAS)
@pytest.mark.parametrize('name', uc.IDS)
def test_definition_agrees_with_checker_loops(ref_lib, name, beta):
  """Two statements of the operator: F.pad / F.conv2d in float64, and the checker's gather loops (double accumulation, one
  rounding to float, one more in beta * old + acc): 2 * 2^-24 B apart at the most.  Guards and NaN are checked as on the GPU."""
  case = CASES[name]
  got, want, mag = uc.run(ref_lib, case, beta)
  uc.check(got, want, 2 * U * mag, f'checker {name} beta={beta}', show=True)


@pytest.mark.parametrize('name', uc.TYPE_IDS)
@pytest.mark.parametrize('dtype', [torch.float16, torch.float64], ids=['f16', 'f64'])
def test_definition_agrees_with_checker_loops_other_types(ref_lib, name, dtype):
  case = CASES[name]
  got, want, mag = uc.run(ref_lib, case, 0.0, dtype)
  uc.check(got, want, uc.bound(want, mag, case.params, dtype), f'checker {name} {dtype}', show=True)


@pytest.mark.parametrize('name', [c.name for c in uc.CASES if c.params[6] == c.params[7] and c.params[8] == c.params[9]
                                  and c.params[10:12] == c.params[12:14]])
def test_definition_agrees_with_ref_torch(name):
  """oracle/ref_torch.py's restatement (one factor and one padding pair for both axes) in double, on the cases it can state."""
  case = CASES[name]
  major, H, W, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1 = case.params
  x, k, _ = uc.inputs(case)
  want, mag = uc.want_and_mag(x, k, None, 0.0, case.params)
  nchw = x.double().permute(0, 3, 1, 2)
  got = ref_torch.upfirdn2d_ref(nchw, k.double(), up=ux, down=dx, pad=(px0, px1)).permute(0, 2, 3, 1)
  uc.check(got, want, (kh * kw + 2) * 2.0 ** -53 * mag, f'ref_torch {name}')


@pytest.mark.parametrize('beta', uc.BETAS)
@pytest.mark.parametrize('name', uc.IDS)
def test_plain_fp32_passes_the_bound(name, beta):
  """The condition on the inputs: the definition in float32 torch on the CPU stays within the fp32 bound."""
  case = CASES[name]
  x, k, old = uc.inputs(case)
  got = uc.define(x, k, case.params, torch.float32)
  if beta != 0.0:
    got = torch.tensor(beta) * old + got
  want, mag = uc.want_and_mag(x, k, old, beta, case.params)
  uc.check(got, want, uc.bound(want, mag, case.params), f'fp32 {name} beta={beta}', show=True)


def test_inputs_tell_planes_apart():
  """Neighbouring planes differ by far more than the bound: the scales of one case span 10^+-2."""
  x, _, _ = uc.inputs(CASES['flat_13planes'])
  rms = x.double().pow(2).mean((1, 2, 3)).sqrt()
  assert float(rms.max() / rms.min()) > 1e3
  ratio = rms[1:] / rms[:-1]
  assert float(torch.minimum(ratio, 1 / ratio).max()) < 0.5


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.float64], ids=['f32', 'f16', 'f64'])
@pytest.mark.parametrize('axis,params', uc.EXTENT_CASES, ids=[e[0] for e in uc.EXTENT_CASES])
def test_checker_refuses_an_empty_extent(ref_lib, axis, params, dtype):
  rc, rc_acc, untouched = uc.extent_refused(ref_lib, params, dtype)
  assert rc == uc.STK_EINVAL and rc_acc in (None, uc.STK_EINVAL), (rc, rc_acc)
  assert untouched, 'the refused call wrote into its output buffer'
