"""GroupNorm statistics of the HIP library against float64 on ill-conditioned groups (cases, reference and metric:
tests/_gn_cases.py; their CPU proof: tests/test_groupnorm_conditioning_cpu.py).

Every family of inputs goes through every place of csrc/groupnorm.hip that computes mean / rstd -- the shapes are chosen by
the dispatch there and `kernel_reached` asserts, with the library's own predicates, that the intended kernel is the one
taken -- and through the backward kernels with the mean / rstd the forward has just written.  Each (sample, group) is
judged on its own scale at 2e-5 (dx: times the float64 condition number of that group's dx).

Measured on an MI355X with the statistic this file was written against (one-pass shifted sums, shift = the first element
of the group), worst error / bound over all sites: family 1 (leading outlier) rstd 612 (|rstd / rstd64 - 1| = 1.2e-2 at
L = 262144, 2.0e-3 at 16384 .. 32768, 3.1e-4 at 4096; within the bound only at L <= 256), y 430, dx 643, mean 1.09;
families 2-5 <= 0.14 on every figure.  With the corrected two-pass statistic every family is <= 0.15 on every figure
(rstd <= 4.3e-7 everywhere); the table is in profiles/gn_statistics_conditioning.txt."""
import pytest
import torch

import _gn_cases as gc

pytestmark = pytest.mark.gpu

_RESULTS = {}
_REACHED = {}


def _figures(lib, site, kind):
  key = (site[0], kind)
  if key not in _RESULTS:
    name, entry, N, C1, C2, HW, G, act = site[:8]
    stat, bwd = gc.kernel_reached(lib, site)
    assert (stat, bwd) == (site[9], site[10]), (name, stat, bwd)
    inp = gc.inputs(N, C1, C2, HW, G, act, kind)
    out = gc.run(lib, site, inp)
    _REACHED[name] = (stat, bwd)
    _RESULTS[key] = (inp, gc.evaluate(out, inp, site))
  return _RESULTS[key]


@pytest.mark.parametrize('family', gc.FAMILIES, ids=lambda f: f'family{f}')
@pytest.mark.parametrize('site', gc.SITES, ids=gc.SITE_IDS)
def test_groupnorm_per_group_against_float64(hip_lib, site, family):
  """mean, rstd, y, the planes, dx of stk_gn_bwd_f32 and of stk_gn_bwd_out_f32: every group of `family` within its bound."""
  inp, fig = _figures(hip_lib, site, 'scales' if family == 5 else 'mixed')
  mask = inp.family == family
  assert int(mask.sum()) >= 3
  for k in ('mean', 'rstd', 'y', 'dx'):
    assert k in fig
  if site[1] != 'fwd':
    assert 'planes' in fig
  bad = gc.report(fig, mask, f'{site[0]} family {family}')
  if bad:
    rs = fig['rstd'][0]
    worst = [(inp.tags[(n, g)], f'{float(rs[n, g]):.2e}') for n, g in mask.nonzero().tolist() if float(rs[n, g]) > gc.TOL]
    assert not bad, (site[0], family, bad, 'rstd misses:', worst[:8])


@pytest.mark.parametrize('kind', ['mixed', 'scales'])
@pytest.mark.parametrize('site', gc.SITES, ids=gc.SITE_IDS)
def test_groupnorm_parameter_gradients_against_float64(hip_lib, site, kind):
  """dgamma / dbeta per channel relative to the sum of absolute terms; the by-product sums of stk_gn_bwd_out_f32."""
  inp, fig = _figures(hip_lib, site, kind)
  for k in ('dgamma', 'dbeta') + (('dx_out_sum',) if 'dx_out_sum' in fig else ()):
    worst = float((fig[k][0] / fig[k][1]).max())
    print(f'  {site[0]} {kind} {k}: worst error / bound = {worst:.3g}')
    assert worst <= 1.0, (site[0], kind, k, worst)


def test_every_statistics_site_was_reached(hip_lib):
  """The count of dispatch sites: every form of every statistics kernel and every backward kernel ran (and was checked
  above: `_figures` refuses a site whose shape reaches another kernel than the one it names)."""
  for site in gc.SITES:
    for kind in ('mixed', 'scales'):
      _figures(hip_lib, site, kind)
  assert len(_REACHED) == len(gc.SITES) == 20
  assert {s for s, _ in _REACHED.values()} == gc.STAT_SITES and len(gc.STAT_SITES) == 14
  assert {b for _, b in _REACHED.values()} == gc.BWD_SITES
