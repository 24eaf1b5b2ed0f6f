"""CPU half of the GroupNorm conditioning tests (tests/_gn_cases.py): the cases, the float64 torch reference and the
per-group metric are proved here without a GPU -- the plain-C checker (oracle/stk_ref.c, two passes in double) runs every
case of every dispatch site and must meet the bounds the HIP library is held to -- and condition (c) of the inputs is
asserted: a plain fp32 two-pass GroupNorm stays within half the tolerance on every case, so the GPU tests never ask of a
kernel what fp32 cannot give."""
import pytest
import torch

import _gn_cases as gc

KINDS = ('mixed', 'scales')


def _inputs(site, kind):
  name, entry, N, C1, C2, HW, G, act = site[:8]
  return gc.inputs(N, C1, C2, HW, G, act, kind)


def test_case_table_is_complete():
  """Every family has variants, every statistics site and backward kernel is listed, two-source shapes put a leading
  outlier where the shift used to come from the second source and into a straddling group."""
  assert {v[0] for v in gc.VARIANTS} == {1, 2, 3, 4} and len(gc.VARIANTS) == 22
  assert {s[9] for s in gc.SITES} == gc.STAT_SITES and len(gc.STAT_SITES) == 14
  assert {s[10] for s in gc.SITES} == gc.BWD_SITES
  assert len(set(gc.SITE_IDS)) == len(gc.SITES) == 20
  seen_straddle = seen_x2 = 0
  for site in gc.SITES:
    name, entry, N, C1, C2, HW, G, act = site[:8]
    inp = _inputs(site, 'mixed')
    assert set(inp.family.unique().tolist()) == {1, 2, 3, 4}, name
    assert {t for t in inp.tags.values()} == {v[1] for v in gc.VARIANTS}, name
    cpg = (C1 + C2) // G
    for g in range(G):
      lead = any(int(inp.family[n, g]) == 1 for n in range(N))
      seen_straddle += lead and g * cpg < C1 < (g + 1) * cpg
      seen_x2 += lead and C2 > 0 and g * cpg >= C1
    sc = _inputs(site, 'scales')
    xg = (torch.cat([sc.x1, sc.x2], 1) if C2 else sc.x1).reshape(N, G, -1)
    std = xg.double().std(2)
    assert float(std.max() / std.min()) >= 1e6, name                    # >= 6 decades inside one tensor
  assert seen_straddle >= 2 and seen_x2 >= 6


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('site', gc.SITES, ids=gc.SITE_IDS)
def test_condition_c_fp32_two_pass_within_half_tolerance(site, kind):
  inp = _inputs(site, kind)
  G = site[6]
  e = gc.group_errors(gc.two_pass_fp32(inp), inp.ref, G)
  for k in ('mean', 'rstd', 'y'):
    for fam in gc.FAMILIES:
      m = inp.family == fam
      if m.any():
        worst = float(e[k][m].max())
        print(f'  fp32 two-pass {site[0]} {kind} family {fam} {k}: {worst:.3g}')
        assert worst <= 0.5 * gc.TOL, (site[0], kind, fam, k, worst)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('site', gc.SITES, ids=gc.SITE_IDS)
def test_checker_meets_the_bounds(ref_lib, site, kind):
  inp = _inputs(site, kind)
  fig = gc.evaluate(gc.run(ref_lib, site, inp), inp, site)
  bad = []
  for fam in gc.FAMILIES:
    m = inp.family == fam
    if m.any():
      bad += [(fam,) + b for b in gc.report(fig, m, f'checker {site[0]} {kind} family {fam}')]
  for k in ('dgamma', 'dbeta'):
    worst = float(fig[k][0].max())
    print(f'  checker {site[0]} {kind} {k}: {worst:.3g}')
    if not worst <= fig[k][1]:
      bad.append((k, worst))
  assert not bad, bad

