"""The entries of include/stk_adagn.h through ctypes against float64 (tests/_adagn_ref.py), on every route they dispatch
to: register-resident, looping (HW % 4 != 0, operands 4 bytes off their alignment) and split through the workspace.

Metric and bound are those of tests/_gn_cases.py, per (sample, group): TOL = 2e-5 for mean, rstd, y; dx at TOL * cond(group);
ds_nc relative to sum |dv xhat| |gamma_c| + sum |dv| |beta_c|; db_nc to sum |dv|; dgamma[c] to sum_n (sum |dv xhat| +
sum |dv|) |1 + s_nc|; dbeta[c] to sum_n sum |dv| |1 + s_nc|.  tests/test_adagn_cpu.py shows that plain fp32 arithmetic keeps
half of that on the same inputs.

`mod` and `dmod` are always column blocks of a wider matrix whose other columns hold a sentinel."""
import itertools

import pytest
import torch

import _adagn_ref as R
from _util import call

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SENTINEL = 123.0
COL, EXTRA = 3, 7                     # mod begins at column 3 of a matrix of 2 C + 7 columns
SEED, SEED_DEV = 0x1234567, 5


def _place(t, off4):
  """t on the device; off4: entered 4 bytes into a buffer (whose base torch aligns to 256 bytes)."""
  if t is None:
    return None
  if not off4:
    return t.to(DEV).contiguous()
  buf = torch.zeros(t.numel() + 4, device=DEV)
  buf[1:1 + t.numel()] = t.reshape(-1).to(DEV)
  v = buf[1:1 + t.numel()].view(t.shape)
  assert v.data_ptr() % 16 == 4 and v.is_contiguous()
  return v


def _wide(N, C, s=None, b=None):
  """[N, 2 C + EXTRA] of sentinels with (s, b) at columns COL .. COL + 2 C; returns the matrix and the view the entry takes."""
  w = torch.full((N, 2 * C + EXTRA), SENTINEL, device=DEV)
  if s is not None:
    w[:, COL:COL + C] = s.to(DEV)
    w[:, COL + C:COL + 2 * C] = b.to(DEV)
  return w, w.view(-1)[COL:]


def _outside(w, C):
  return torch.cat([w[:, :COL], w[:, COL + 2 * C:]], 1)


class Run:
  """One forward and one backward of a case.  Outputs and the workspace start as NaN."""

  def __init__(self, lib, case, drop_p=None, s=None, b=None, dx_beta=0.0, want=('dmod', 'dgamma', 'dbeta'), want_dx=True):
    _, N, C, HW, G, act, opt = case
    d = R.inputs(case)
    off4 = 'off4' in opt
    self.p = (0.1 if 'drop' in opt else 0.0) if drop_p is None else drop_p
    self.s, self.b = (d['s'] if s is None else s), (d['b'] if b is None else b)
    nan = lambda *sh: _place(torch.full(sh, float('nan')), off4)
    self.x, self.gamma, self.beta, self.dy = (_place(d[k], off4) for k in ('x', 'gamma', 'beta', 'dy'))
    self.modw, self.mod = _wide(N, C, self.s, self.b)
    self.y, self.mean, self.rstd = nan(N, C, HW), nan(N * G), nan(N * G)
    wsf = int(lib.gn_mod_ws_bytes(N, C, HW, G)) // 4
    self.ws = torch.full((wsf,), float('nan'), device=DEV)
    self.seed_dev = torch.tensor([SEED_DEV], dtype=torch.int64, device=DEV)
    self.dims = (N, C, HW, G)
    self.tail = (act, self.p, SEED, self.seed_dev)
    self.stride = 2 * C + EXTRA
    call(lib, 'gn_mod_fwd_f32', self.x, self.gamma, self.beta, self.mod, self.stride, self.y, self.mean, self.rstd, *self.dims,
         R.EPS, *self.tail, self.ws)
    self.dx = _place(d['dx0'], off4) if want_dx else None
    self.dmodw, self.dmod = _wide(N, C)
    self.dgamma, self.dbeta = _place(d['dgamma0'], off4), _place(d['dbeta0'], off4)
    self.ws.fill_(float('nan'))
    call(lib, 'gn_mod_bwd_f32', self.dy, self.x, self.gamma, self.beta, self.mod, self.stride, self.mean, self.rstd, self.dx,
         dx_beta, self.dmod if 'dmod' in want else None, self.dgamma if 'dgamma' in want else None,
         self.dbeta if 'dbeta' in want else None, self.ws, *self.dims, *self.tail)
    torch.cuda.synchronize()

  def mask(self, lib):
    if self.p == 0.0:
      return None
    N, C, HW, G = self.dims
    m = torch.empty(N * C * HW, device=DEV)
    call(lib, 'dropout_mask_f32', m, N * C * HW, self.p, SEED + SEED_DEV)
    return m.view(N, C, HW).cpu()

  def outputs(self):
    N, C, HW, G = self.dims
    return dict(y=self.y, mean=self.mean, rstd=self.rstd, dx=self.dx, ds=self.dmodw[:, COL:COL + C],
                db=self.dmodw[:, COL + C:COL + 2 * C], dgamma=self.dgamma, dbeta=self.dbeta)


def _assert_route(lib, case):
  """The route the shape rules of _adagn_ref.route name, cross-checked with the library's own predicates."""
  _, N, C, HW, G, act, opt = case
  fwd, bwd = R.route(case)
  cpg = C // G
  assert int(lib.gn_mod_ok(C, HW, G)) == 1
  split_shape = int(lib.gn_mod_ws_bytes(N, C, HW, G)) > 8 * N * C
  assert split_shape == (cpg * HW > 16384 and HW % 4096 == 0)
  flat_shape = bool(int(lib.gn_bwd_out_ok(C, 0, HW, G)))
  aligned = 'off4' not in opt
  assert (bwd == 'split') == (aligned and split_shape)
  assert (bwd == 'flat') == (aligned and flat_shape)
  assert (fwd == 'split') == (aligned and split_shape)
  assert (fwd == 'loop') == (not aligned or HW % 4 != 0 or (cpg * HW > 16384 and not split_shape))
  return fwd, bwd


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_against_float64(hip_lib, case):
  lib = hip_lib
  _, N, C, HW, G, act, opt = case
  fwd, bwd = _assert_route(lib, case)
  d = R.inputs(case)
  dx_beta = float(R.CASE_IDS.index(case[0]) % 2)                 # both 0 and 1 over the cases
  r = Run(lib, case, dx_beta=dx_beta)
  ref = R.closed_form(d['x'], d['gamma'], d['beta'], r.s, r.b, d['dy'], G, act, r.mask(lib))
  # dx = dx_beta dx0 + (the layer's gradient); gamma / beta accumulate onto what was there
  ref = dict(ref)
  ref['dx'] = dx_beta * d['dx0'].double() + ref['dx']
  ref['dx_terms'] = dx_beta * d['dx0'].double().abs() + ref['dx_terms']
  ref['dgamma'], ref['dgamma_cond'] = ref['dgamma'] + d['dgamma0'].double(), ref['dgamma_cond'] + d['dgamma0'].double().abs()
  ref['dbeta'], ref['dbeta_cond'] = ref['dbeta'] + d['dbeta0'].double(), ref['dbeta_cond'] + d['dbeta0'].double().abs()
  fig = R.figures(r.outputs(), ref, G)
  print(case[0], fwd, bwd, f'dx_beta={dx_beta}', {k: f'{v * R.TOL:.2e}' for k, v in fig.items()})
  assert len(fig) == 8
  for k, v in fig.items():
    assert v <= 1.0, f'{case[0]} ({fwd} / {bwd}): {k} at {v * R.TOL:.3e} > {R.TOL:.0e}'
  # the columns of the wider matrices that are not this layer's
  assert bool((_outside(r.modw, C) == SENTINEL).all()) and bool((_outside(r.dmodw, C) == SENTINEL).all())
  assert torch.equal(r.modw[:, COL:COL + C].cpu(), r.s) and torch.equal(r.modw[:, COL + C:COL + 2 * C].cpu(), r.b)
  # two launches, the same bits
  r2 = Run(lib, case, dx_beta=dx_beta)
  for (k, a), b in zip(r.outputs().items(), r2.outputs().values()):
    assert torch.equal(a, b), f'{case[0]}: {k} differs between two launches'


@pytest.mark.parametrize('drop_p', [0.0, 0.1])
@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_zero_modulation_is_the_plain_layer_bit_for_bit(hip_lib, case, drop_p):
  """s = b = 0: y, mean, rstd of stk_gn_fwd_f32 on the same operands (so the dropout mask is the same function of the seed
  and the index); any modulation: the same mean and rstd."""
  lib = hip_lib
  _, N, C, HW, G, act, opt = case
  zero = torch.zeros(N, C)
  r0 = Run(lib, case, drop_p=drop_p, s=zero, b=zero)
  r1 = Run(lib, case, drop_p=drop_p)
  y, mean, rstd = torch.full_like(r0.y, float('nan')), torch.full_like(r0.mean, float('nan')), torch.full_like(r0.rstd, float('nan'))
  if 'off4' in opt:
    y = _place(y.cpu(), True)
  call(lib, 'gn_fwd_f32', r0.x, C, None, 0, r0.gamma, r0.beta, y, mean, rstd, N, HW, G, R.EPS, act, drop_p, SEED, r0.seed_dev,
       r0.ws)
  torch.cuda.synchronize()
  assert torch.equal(r0.y, y) and torch.equal(r0.mean, mean) and torch.equal(r0.rstd, rstd)
  assert torch.equal(r1.mean, mean) and torch.equal(r1.rstd, rstd)
  assert not torch.equal(r1.y, y), 'the modulation does not reach the output'
  if drop_p and act != 2:                                         # (ReLU zeroes about half on its own)
    frac = (y == 0).float().mean().item()
    assert 0.05 < frac < 0.2, f'{frac:.3f} of the outputs dropped at p = 0.1'


@pytest.mark.parametrize('name', ['flat_small', 'loop_hw25'])
def test_null_outputs(hip_lib, name):
  """Every subset of (dmod, dgamma, dbeta) and dx = NULL: what is asked for has the bits of the full call, what is not is
  not written."""
  case = R.CASES[R.CASE_IDS.index(name)]
  d = R.inputs(case)
  full = Run(hip_lib, case).outputs()
  C = case[2]
  for k in range(3):
    for want in itertools.combinations(('dmod', 'dgamma', 'dbeta'), k):
      r = Run(hip_lib, case, want=want)
      o = r.outputs()
      assert torch.equal(o['dx'], full['dx']), want
      for key, names in (('dmod', ('ds', 'db')), ('dgamma', ('dgamma',)), ('dbeta', ('dbeta',))):
        for n in names:
          if key in want:
            assert torch.equal(o[n], full[n]), (want, n)
          elif key == 'dmod':
            assert bool((r.dmodw == SENTINEL).all()), want
          else:
            assert torch.equal(o[n].cpu(), d[n + '0']), (want, n)
  r = Run(hip_lib, case, want_dx=False)
  o = r.outputs()
  for n in ('ds', 'db', 'dgamma', 'dbeta'):
    assert torch.equal(o[n], full[n]), n


def test_invalid_arguments_are_refused(hip_lib):
  lib = hip_lib
  case = R.CASES[0]
  _, N, C, HW, G, act, opt = case
  r = Run(lib, case)
  P = lambda t: None if t is None else t.data_ptr()
  s = torch.cuda.current_stream().cuda_stream

  def fwd(**kw):
    a = dict(x=r.x, gamma=r.gamma, beta=r.beta, mod=r.mod, stride=r.stride, y=r.y, mean=r.mean, rstd=r.rstd, N=N, C=C, HW=HW,
             G=G, act=act, p=0.0)
    a.update(kw)
    return lib.gn_mod_fwd_f32.raw(P(a['x']), P(a['gamma']), P(a['beta']), P(a['mod']), a['stride'], P(a['y']), P(a['mean']),
                                  P(a['rstd']), a['N'], a['C'], a['HW'], a['G'], R.EPS, a['act'], a['p'], SEED, None, P(r.ws), s)

  def bwd(**kw):
    a = dict(dy=r.dy, x=r.x, gamma=r.gamma, beta=r.beta, mod=r.mod, stride=r.stride, mean=r.mean, rstd=r.rstd, ws=r.ws, N=N,
             C=C, HW=HW, G=G, act=act, p=0.0)
    a.update(kw)
    return lib.gn_mod_bwd_f32.raw(P(a['dy']), P(a['x']), P(a['gamma']), P(a['beta']), P(a['mod']), a['stride'], P(a['mean']),
                                  P(a['rstd']), P(r.dx), 0.0, P(r.dmod), P(r.dgamma), P(r.dbeta), P(a['ws']), a['N'], a['C'],
                                  a['HW'], a['G'], a['act'], a['p'], SEED, None, s)

  EINVAL = -1
  assert fwd() == 0 and bwd() == 0
  for k in ('x', 'gamma', 'beta', 'mod', 'y', 'mean', 'rstd'):
    assert fwd(**{k: None}) == EINVAL, k
  for k in ('dy', 'x', 'gamma', 'beta', 'mod', 'mean', 'rstd', 'ws'):
    assert bwd(**{k: None}) == EINVAL, k
  for f in (fwd, bwd):
    assert f(stride=2 * C - 1) == EINVAL and f(stride=2 * C) == 0
    assert f(G=3) == EINVAL and f(N=0) == EINVAL and f(C=0) == EINVAL and f(HW=0) == EINVAL and f(G=0) == EINVAL
    assert f(act=5) == EINVAL and f(act=-1) == EINVAL and f(p=1.0) == EINVAL and f(p=-0.1) == EINVAL
  torch.cuda.synchronize()
  assert int(lib.gn_mod_ws_bytes(N, C, HW, 3)) == 0 and int(lib.gn_mod_ok(C, HW, 3)) == 0
